// bsps_count.hip -- the staged hits-and-positions family of the bit-sliced count kernels (DESIGN.md §4e "Hits
// from the jobs stage"): bs_count.inc's body with STAGED, HITS and POS on -- the early launch and device
// packing of ac_window_positions_jobs / _submit, which beside the counts and every window's hit word of each
// level 0..E stores the eight plane words of end positions that bsp_count.hip's plain kernels store.  One
// instantiation per k in AC_BS_K_LIST over three NFA rows (edit budgets 0..2) and over four (budget 3).
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

constexpr BsFamily family(int rows) { return BsFamily{true, BsOut::Pos, rows}; }

}  // namespace

// k = K, equal windows, R NFA rows (3: E = 0..2, 4: E = 3), staged, counts, hits and positions, at its
// family's residency.
template <int K, int R>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, bs_waves_per_simd(family(R), K)) void bsps_count_kernel(LaunchArgs a) {
    __shared__ BsLds<K> lds[(160 * 1024 / bs_blocks_per_cu(family(R), K)) / sizeof(BsLds<K>)];
    bs_body<K, true, R, true, true>(a, lds[0]);
}

CountKernel bsps_kernel(uint32_t k, BsFamily f) {
#define AC_BS_PICK(KK) \
    if (k == KK) return f.rows == 4 ? bsps_count_kernel<KK, 4> : bsps_count_kernel<KK, 3>;
    AC_BS_K_LIST(AC_BS_PICK)
#undef AC_BS_PICK
    return nullptr;
}

}  // namespace acamd
