// bs3_count.hip -- the bit-sliced count kernels for an edit budget of 3 (M1(3): a window adds
// max(0, 4 - d); DESIGN.md §4e "Edit budget"): bs_count.inc's body over four NFA rows (bs_nfa_r.h), one
// instantiation per k in AC_BS_K_LIST, plain and staged.  A translation unit of its own, so that
// wm_count.hip's device compile stays what it was and the two compile side by side; it shares the
// frame (stage_dev.inc, count_frame.inc) and the body by inclusion, and wm_count.hip's dispatch
// (count_kernel) takes its kernels from bs3_kernel().
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// k = K, equal windows, E = 3.  bs_waves_per_simd(K, 3) waves per SIMD, capped by the LDS allocation
// like bs_count_kernel.
template <int K, bool STAGED>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, bs_waves_per_simd(K, 3)) void bs3_count_kernel(LaunchArgs a) {
    constexpr int kBlocksPerCu = 4 * bs_waves_per_simd(K, 3) / WAVES_PER_BLOCK;
    __shared__ BsLds<K> lds[(160 * 1024 / kBlocksPerCu) / sizeof(BsLds<K>)];
    bs_body<K, STAGED, 4>(a, lds[0]);
}

void (*bs3_kernel(uint32_t k, bool staged))(LaunchArgs) {
#define AC_BS_PICK(KK) \
    if (k == KK) return staged ? bs3_count_kernel<KK, true> : bs3_count_kernel<KK, false>;
    AC_BS_K_LIST(AC_BS_PICK)
#undef AC_BS_PICK
    return nullptr;
}

}  // namespace acamd
