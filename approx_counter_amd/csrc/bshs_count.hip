// bshs_count.hip -- the staged hits-writing family of the bit-sliced count kernels (DESIGN.md §4e "Hits from
// the jobs stage"): bs_count.inc's body with STAGED and HITS on -- the early launch and device packing of
// ac_window_hits_jobs / _submit, whose kernel stages its own inputs (count_frame.inc, stage_dev.inc) and,
// beside the counts, stores every window's hit word of each level 0..E as bsh_count.hip's plain kernels do.
// These are the first hits launches that reach the body's inline-N-record code (nrec.h): the jobs stage packs
// records, the samples route's images carry none.  One instantiation per k in AC_BS_K_LIST over three NFA
// rows (edit budgets 0..2) and over four (budget 3).
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

constexpr BsFamily family(int rows) { return BsFamily{true, BsOut::Hits, rows}; }

}  // namespace

// k = K, equal windows, R NFA rows (3: E = 0..2, 4: E = 3), staged, counts and hits, at its family's residency.
template <int K, int R>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, bs_waves_per_simd(family(R), K)) void bshs_count_kernel(LaunchArgs a) {
    __shared__ BsLds<K> lds[(160 * 1024 / bs_blocks_per_cu(family(R), K)) / sizeof(BsLds<K>)];
    bs_body<K, true, R, true>(a, lds[0]);
}

CountKernel bshs_kernel(uint32_t k, BsFamily f) {
#define AC_BS_PICK(KK) \
    if (k == KK) return f.rows == 4 ? bshs_count_kernel<KK, 4> : bshs_count_kernel<KK, 3>;
    AC_BS_K_LIST(AC_BS_PICK)
#undef AC_BS_PICK
    return nullptr;
}

}  // namespace acamd
