// bs3_count.hip -- the bit-sliced count kernels for an edit budget of 3 (M1(3): a window adds
// max(0, 4 - d); DESIGN.md §4e "Edit budget"): bs_count.inc's body over four NFA rows (bs_nfa_r.h), one
// instantiation per k in AC_BS_K_LIST, plain and staged.  A translation unit of its own, so that
// wm_count.hip's device compile stays what it was and the two compile side by side.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bs_nfa.h"
#include "bs_nfa_r.h"
#include "bs_pos.h"
#include "nrec.h"
#include "wm_count.h"

namespace acamd {
namespace {

#include "bs_family.inc"

constexpr BsFamily family(bool staged) { return BsFamily{staged, BsOut::Count, 4}; }

}  // namespace

// k = K, equal windows, E = 3, at its family's residency (launch bounds, and the LDS allocation that caps it).
template <int K, bool STAGED>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, bs_waves_per_simd(family(STAGED), K)) void bs3_count_kernel(LaunchArgs a) {
    __shared__ BsLds<K> lds[(160 * 1024 / bs_blocks_per_cu(family(STAGED), K)) / sizeof(BsLds<K>)];
    bs_body<K, STAGED, 4>(a, lds[0]);
}

CountKernel bs3_kernel(uint32_t k, BsFamily f) {
#define AC_BS_PICK(KK) \
    if (k == KK) return f.staged ? bs3_count_kernel<KK, true> : bs3_count_kernel<KK, false>;
    AC_BS_K_LIST(AC_BS_PICK)
#undef AC_BS_PICK
    return nullptr;
}

}  // namespace acamd
