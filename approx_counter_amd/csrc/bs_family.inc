// bs_family.inc -- what every family translation unit of the bit-sliced kernels (bs3_count.hip, bsh_count.hip,
// bsp_count.hip, bshs_count.hip, bsps_count.hip) puts before its kernels, included inside the unit's anonymous
// namespace after bs_nfa.h, bs_nfa_r.h, bs_pos.h, nrec.h and wm_count.h: the frame (stage_dev.inc,
// count_frame.inc) and the body (bs_count.inc).  wm_count.hip, whose -DAC_STAMPS builds stamp, has its own.
constexpr int WAVES_PER_BLOCK = AC_WAVES_PER_BLOCK;
// (the diagnostic stamps of wm_count.hip's -DAC_STAMPS builds are taken by its own kernels only)
__device__ __forceinline__ void stamp(uint64_t, int) {}
__device__ __forceinline__ void stage_stamp(uint32_t, int) {}

// (the frame also holds what only the word-parallel kernel calls)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "stage_dev.inc"
#include "count_frame.inc"
#pragma clang diagnostic pop
#include "bs_count.inc"
