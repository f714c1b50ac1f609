// bsps_count.hip -- the staged hits-and-positions family of the bit-sliced count kernels (DESIGN.md §4e "Hits
// from the jobs stage"): bs_count.inc's body with STAGED, HITS and POS on -- the early launch and device
// packing of ac_window_positions_jobs / _submit, which beside the counts and every window's hit word of each
// level 0..E stores the eight plane words of end positions that bsp_count.hip's plain kernels store.  One
// instantiation per k in AC_BS_K_LIST over three NFA rows (edit budgets 0..2) and over four (budget 3).  A
// translation unit of its own, like bsp_count.hip; wm_count.hip's dispatch (count_kernel) takes its kernels
// from bsps_kernel().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bs_nfa.h"
#include "bs_nfa_r.h"
#include "bs_pos.h"
#include "nrec.h"
#include "wm_count.h"

namespace acamd {
namespace {

constexpr int WAVES_PER_BLOCK = AC_WAVES_PER_BLOCK;
// (the diagnostic stamps of wm_count.hip's -DAC_STAMPS builds are taken by the E = 2 kernels only)
__device__ __forceinline__ void stamp(uint64_t, int) {}
__device__ __forceinline__ void stage_stamp(uint32_t, int) {}

// (the frame also holds what only the word-parallel kernel calls)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "stage_dev.inc"
#include "count_frame.inc"
#pragma clang diagnostic pop
#include "bs_count.inc"

}  // namespace

// k = K, equal windows, R NFA rows (3: E = 0..2, 4: E = 3), staged, counts, hits and positions.
// bsps_waves_per_simd waves per SIMD, capped by the LDS allocation like bs_count_kernel.
template <int K, int R>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, bsps_waves_per_simd(K, R == 4 ? 3 : 2)) void bsps_count_kernel(LaunchArgs a) {
    // (a kernel at one wave per SIMD takes the LDS of two: its registers cap the residency)
    constexpr int kBlocksPerCu = 4 * std::max(2, bsps_waves_per_simd(K, R == 4 ? 3 : 2)) / WAVES_PER_BLOCK;
    __shared__ BsLds<K> lds[(160 * 1024 / kBlocksPerCu) / sizeof(BsLds<K>)];
    bs_body<K, true, R, true, true>(a, lds[0]);
}

void (*bsps_kernel(uint32_t k, uint32_t max_errors))(LaunchArgs) {
    if (max_errors > 3u) return nullptr;
#define AC_BS_PICK(KK) \
    if (k == KK) return max_errors == 3u ? bsps_count_kernel<KK, 4> : bsps_count_kernel<KK, 3>;
    AC_BS_K_LIST(AC_BS_PICK)
#undef AC_BS_PICK
    return nullptr;
}

}  // namespace acamd
