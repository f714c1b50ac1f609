// bshs_count.hip -- the staged hits-writing family of the bit-sliced count kernels (DESIGN.md §4e "Hits from
// the jobs stage"): bs_count.inc's body with STAGED and HITS on -- the early launch and device packing of
// ac_window_hits_jobs / _submit, whose kernel stages its own inputs (count_frame.inc, stage_dev.inc) and,
// beside the counts, stores every window's hit word of each level 0..E as bsh_count.hip's plain kernels do.
// These are the first hits launches that reach the body's inline-N-record code (nrec.h): the jobs stage packs
// records, the samples route's images carry none.  One instantiation per k in AC_BS_K_LIST over three NFA
// rows (edit budgets 0..2) and over four (budget 3).  A translation unit of its own, like bsh_count.hip, so
// that the other kernels' device compiles stay what they were; wm_count.hip's dispatch (count_kernel) takes
// its kernels from bshs_kernel().
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

// k = K, equal windows, R NFA rows (3: E = 0..2, 4: E = 3), staged, counts and hits.  bshs_waves_per_simd
// waves per SIMD, capped by the LDS allocation like bs_count_kernel.
template <int K, int R>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, bshs_waves_per_simd(K, R == 4 ? 3 : 2)) void bshs_count_kernel(LaunchArgs a) {
    // (a kernel at one wave per SIMD takes the LDS of two: its registers cap the residency)
    constexpr int kBlocksPerCu = 4 * std::max(2, bshs_waves_per_simd(K, R == 4 ? 3 : 2)) / WAVES_PER_BLOCK;
    __shared__ BsLds<K> lds[(160 * 1024 / kBlocksPerCu) / sizeof(BsLds<K>)];
    bs_body<K, true, R, true>(a, lds[0]);
}

void (*bshs_kernel(uint32_t k, uint32_t max_errors))(LaunchArgs) {
    if (max_errors > 3u) return nullptr;
#define AC_BS_PICK(KK) \
    if (k == KK) return max_errors == 3u ? bshs_count_kernel<KK, 4> : bshs_count_kernel<KK, 3>;
    AC_BS_K_LIST(AC_BS_PICK)
#undef AC_BS_PICK
    return nullptr;
}

}  // namespace acamd
