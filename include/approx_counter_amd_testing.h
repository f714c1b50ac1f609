/*
 * approx_counter_amd_testing.h -- test-only entry point of libapprox_counter_amd.so.
 *
 * Not part of the drop-in boundary (include/approx_counter_amd.h): no product
 * caller sets these hooks, and the reference has no counterpart.  They let the
 * test suite drive failure and diagnostic paths of the early-launch stage
 * (ac_error_count_jobs, the replacement of errorCount, approx_counter.cpp:531-601)
 * that a well-behaved host never reaches.  Hooks are process-wide and apply to
 * calls made after the call that sets them; 0 clears them.
 */
#ifndef APPROX_COUNTER_AMD_TESTING_H
#define APPROX_COUNTER_AMD_TESTING_H

#include <stdint.h>

#include "approx_counter_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The last job of an early-launch call is never flagged complete: the kernel's
 * bounded waits run out (0.5 s without progress), it reports AC_DEVERR_STAGE, and
 * the synchronous call retries through the DMA path (ac_stage_mode() == 0 after). */
#define AC_TESTING_UNFLAG_LAST 1u
/* Every job is sent ahead of the staged launch by the copy kernel, so the staged
 * kernel runs on resident input (a measurement of its own cost). */
#define AC_TESTING_ALL_AHEAD 2u
/* The publishing thread sleeps 60 ms after each of a call's first 12 progress
 * records: a host slower in total than the kernel's 0.5 s timeout, whose every
 * gap is not (the waits restart their clock on progress). */
#define AC_TESTING_SLOW_HOST 4u
/* Device packing (ABI 7) for every eligible job, whatever the call's size: the
 * default policy leaves small calls to the host pool. */
#define AC_TESTING_DEVICE_PACK 8u
/* A DMA-path jobs call (AC_STAGE_EARLY=0, or the retry of a timed-out early launch) with work is
 * cut into two parts whatever its size; without the hook a call needs 2^17 windows for that
 * (DESIGN.md §4c).  The parts of ac_window_hits_jobs write disjoint row ranges of one matrix. */
#define AC_TESTING_TWO_PARTS 16u

/* Sets the hooks (an OR of the flags above); returns the previous value. */
uint32_t ac_testing_stage_hooks(uint32_t flags);

/* Which count kernel the context's last count launch ran: 0 the word-parallel kernel
 * (wm2_count_kernel), 1 the bit-sliced kernel (bs_count_kernel: k = 16 or 18..32, every live
 * segment with equal windows of 1..256 bases, unless AC_BITSLICE=0); -1 before the first launch.  On an ac_create_multi context:
 * shard 0's. */
int ac_testing_last_count_kernel(ac_ctx* ctx);

/* ac_hit_cooccurrence_device in steps, for measurement (tools/kernel_run.py --cooc): stages 1 = only the
 * planes' transposition into the context's scratch, 2 = only the product from the scratch an earlier call
 * with the same shape filled, 3 = both (the product call itself). */
ac_status ac_testing_hit_cooccurrence_stages(ac_ctx* ctx, const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows,
                                             uint32_t levels, uint32_t* cooc, uint32_t stages, void* hip_stream);

/* ac_hit_cross_cooccurrence_device in steps, likewise (tools/kernel_run.py --cross): stages 1 = only the two
 * matrices' transpositions, 2 = only the product from the scratch, 3 = both. */
ac_status ac_testing_hit_cross_stages(ac_ctx* ctx, const uint32_t* hits_a, uint32_t n_a, const uint32_t* hits_b, uint32_t n_b,
                                      uint32_t n_windows, uint32_t levels, uint32_t* cross, uint32_t stages,
                                      void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* APPROX_COUNTER_AMD_TESTING_H */
