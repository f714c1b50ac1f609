// wm_count.h -- launch descriptor shared by the kernel and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AC_MAX_SEGS 4    // segments fused into one launch (start + end ends, shards)
#define AC_QUEUE_LINE 32  // u32 per queue counter: one 128-B line each (no false sharing between counters)
#define AC_MAX_PACK 4    // candidates interleaved per 32-bit lane word (P = min(32/k, 4))
// Largest window image (bases, exclusive): the count kernel reads it through buffer descriptors whose
// byte offsets and sizes are 32-bit (2 bits per base: 2^34 bases = 4 GiB of code words).  4096 bases
// (1 KiB of code words) below 2^34: the bit-sliced kernel marks a lane without a window with the slot
// offset 0xffffff00 (bs_count.inc NO_WINDOW), which has to lie past every image's range check together
// with the 64 bytes a lane loads from there on -- in an image of more than 2^34 - 1024 bases it was the
// offset of a real window, which the kernel then took for none (not counted, its hit words not written).
#define AC_MAX_IMAGE_BASES ((1ull << 34) - 4096ull)
#ifndef AC_WAVES_PER_BLOCK
#define AC_WAVES_PER_BLOCK 4  // waves per workgroup, all on one candidate group (shared ~Eq table, counts summed in LDS)
#endif
// Lane words per wave (P candidates each) for pattern pack P: 2 = two NFAs per lane sharing each
// base's SALU work (LDS table read, M0 set-up) at 4 resident waves per SIMD, 1 = one NFA at 8.
// Two words for P = 2 (k = 11-16): cfg2 kernel 107-108 -> 102-103 us, cfg3 equal; one word for
// P = 1, where two were 0.8 % slower at cfg5 (profiles/r03_dual_ab.log).  P = 3-4 (k <= 10) are
// unmeasured and keep one.  -DAC_WORDS=1 / 2 forces one choice for every P (A/B builds).
// Round 5: the early launch's staged kernel takes two words for P = 1 as well -- with one word (8 resident
// waves, 78 SGPRs per wave) its staging state spilled 140+ SGPRs inside the count loop, with two (4
// waves, 106 SGPRs) 52: cfg5 stage 4.568-4.570 vs 4.669-4.687 ms, same box (profiles/r05_m12), while
// the plain P = 1 kernel stays at one word (4.248 vs 4.362 ms on resident input).
#ifndef AC_P1_STAGED_WORDS
#define AC_P1_STAGED_WORDS 2
#endif
constexpr int words_for(int P, bool staged = false) {
#ifdef AC_WORDS
    return (void)P, (void)staged, AC_WORDS;
#else
    return P == 2 ? 2 : (P == 1 && staged) ? AC_P1_STAGED_WORDS : 1;
#endif
}
// resident count-kernel waves per SIMD, set by the LDS allocation (<= 64 VGPRs with one word)
#ifndef AC_W2_WAVES
#define AC_W2_WAVES 4  // (A/B builds: resident waves per SIMD with two lane words)
#endif
constexpr int waves_per_simd(int W) { return W == 2 ? AC_W2_WAVES : 8; }

// Device error word bits (ac_check, include/approx_counter_amd.h): a window
// that is misaligned or reaches past the image was skipped; the kernel found
// its set-up broken (the ~Eq table not at LDS address 0) and skipped its work.
#define AC_DEVERR_WINDOW 1u
#define AC_DEVERR_SETUP 2u
#define AC_DEVERR_STAGE 4u  // a staged launch timed out waiting for its host inputs (its work was skipped)
#define AC_NO_ULEN 0xffffffffu

// Staged launches ("early launch"): the count kernel is launched
// before the host has packed its inputs and stages them itself.  Per segment,
// one header line of pinned host memory, read by the kernel with ONE 16-byte
// load (words 0-3):
#define AC_HDR_PGEN 0    // progress record, one 8-byte store {PGEN, READY}: valid when PGEN = the launch's generation
#define AC_HDR_READY 1   //   bytes of the segment's region packed and free of N (a prefix: k-mers, then codes)
#define AC_HDR_FLAG 2    // = generation once the segment is complete and INFO holds
#define AC_HDR_INFO 3    //   its final byte count (<= the launch's chunks x AC_STAGE_CHUNK, a multiple of 256)
                         //   | AC_HDR_INFO_HAS_N when it holds an N (its N bitmap sent), or AC_HDR_INFO_ABORT:
                         //   the host gave up on the call (the waves skip the segment)
#define AC_HDR_INFO_HAS_N 0x80000000u
#define AC_HDR_INFO_ABORT 0xffffffffu
#define AC_HDR_LINES AC_MAX_SEGS
#define AC_STAGE_CHUNK 4096u  // bytes one wave copies per claimed chunk (64 lanes x 16 B x 4)
#define AC_STAGE_REPL 32      // replicas of a segment's done counter (pollers spread over lines)
// Device words of a staged launch, one AC_QUEUE_LINE line each, after the
// launch's sub-queue counters in its queue bank (zeroed with them for the next
// launch on that bank; only word 0 of a line is ever used, as the next launch
// zeroes word 0 of each): error bits, then per segment: chunk
// claims, the segment's final header (verdict, bytes, final seen),
// AC_STAGE_REPL replicas of the N-free bytes available so far, AC_STAGE_REPL
// done replicas (every workgroup polls one replica of each: ~1000 waves
// polling one line slowed the chunk copies).
#define AC_STAGE_L_ERR 0
#define AC_STAGE_SEG_LINES (4 + 2 * AC_STAGE_REPL)
#define AC_STAGE_L_SEG(s) (1 + (s) * AC_STAGE_SEG_LINES)
#define AC_STAGE_LINES (1 + AC_MAX_SEGS * AC_STAGE_SEG_LINES)
// 0.5 s of s_memrealtime (100 MHz) WITHOUT PROGRESS: every wait is bounded, and its clock restarts
// whenever the words it waits on advance (a large call may take far longer than this to pack)
#define AC_STAGE_TIMEOUT_TICKS 50000000ull

namespace acamd {

struct SegDev {
    const uint64_t* kmers;
    const uint32_t* codes;
    const uint32_t* nmask;
    const uint64_t* start;
    const uint32_t* length;
    uint32_t* counts;
    uint64_t n_bases;     // image size (bases); windows outside it are skipped
    uint32_t n_kmers;
    uint32_t n_windows;
    uint32_t groups;      // candidate groups of the launch's group size (cands_per_wave(P), bit-sliced: BS_GROUP)
    uint32_t chunk;       // windows per work item of the dynamic queues
    uint32_t queue_begin; // index of this segment's first sub-queue (groups x subq of them)
    uint32_t subq;        // sub-queues per candidate group (proportional to n_windows; a multiple of AC_WAVES_PER_BLOCK)
    uint32_t acc_begin;   // this segment's first slot in LaunchArgs::acc (groups x group size slots)
    uint32_t group_begin;  // launch-wide index of this segment's first candidate group (LaunchArgs::grp_err)
    uint32_t has_n;       // 0: the image holds no N (its N bitmap is not read; every word reads as 0)
    uint32_t ulen;        // AC_NO_ULEN, or every window has this length and window w starts at base
                          // w * ceil32(ulen) (start / length are not read)
    uint32_t nrec;        // equal windows with inline N records (nrec.h): the record's bits R, else 0;
                          // has_n then says whether the N bitmap is there (some record overflowed)
    // staged launches: the segment's packed region (k-mers first) is copied from stage_src (the
    // pinned block, device-visible address) to stage_dst (device memory; kmers / codes / ... point
    // into it) in stage_chunks chunks of AC_STAGE_CHUNK bytes once the host flags it
    const uint8_t* stage_src;
    uint8_t* stage_dst;
    uint32_t stage_chunks;
    uint32_t stage_codes_off;  // bytes of the region before the codes (k-mers)
    uint32_t* stage_gen;       // per chunk, one line each: = the launch's generation once copied (early counting)
    // Device packing (staged launches, equal windows of 1..256 bases): the segment's
    // sample is read as Dna5 bytes straight from pinned host memory (ac_host_alloc) by the copier
    // workgroups, which pack each codes chunk themselves (stage_pack_chunk) instead of copying one the
    // host packed.  dp_src = NULL: the host packed the codes into the staging block.
    const uint8_t* dp_src;     // device-visible address the windows' offsets are relative to
    const uint64_t* dp_off;    // device-visible address of the segment's n_windows offsets
    uint32_t dp_src_bytes;     // bytes readable from dp_src (< 2^31); a window outside them is an error
};

struct LaunchArgs {
    SegDev seg[AC_MAX_SEGS];
    uint64_t total_waves;
    // Work queues: two banks of `qstride` sub-queue counters, one per
    // AC_QUEUE_LINE-u32 line.  This launch dequeues from bank `bank` (zeroed)
    // and zeroes the first `zero_count` counters of the other bank for the next
    // launch.
    uint32_t* queue;
    uint32_t qstride;
    uint32_t bank;
    uint32_t zero_count;
    uint32_t n_queues;  // sub-queues over all segments (a multiple of AC_WAVES_PER_BLOCK); wave w of
                        // workgroup b serves sub-queue (b % (n_queues / AC_WAVES_PER_BLOCK)) * AC_WAVES_PER_BLOCK + w
    // Count hand-off: each workgroup adds (1 << 32) + its sum into every `acc` slot of
    // its candidate group with one returning 64-bit atomic per slot; the workgroup whose add finds
    // every other workgroup's arrival in the high half is the slot's last, writes the slot's total
    // to the segment's counts (stored, or added when `add_counts`) and zeroes the slot for the next
    // launch, so a launch needs no memset of the counts and no ticket round trip.
    uint64_t* acc;
    uint32_t* err;      // AC_DEVERR_* bits, or-ed in by the kernel
    uint32_t add_counts;
    // Staged launch (nonzero): inputs copied in by the kernel once the host flags each segment in
    // host_hdr (pinned, AC_HDR_LINES lines of AC_QUEUE_LINE u32); counts stored to host memory at
    // system scope, the launch's completion written to host_hdr's result line.  `stage` = this
    // launch's AC_STAGE_LINES device lines.
    uint32_t staged;
    uint32_t gen;
    uint32_t* host_hdr;
    uint32_t* stage;
    uint32_t* err_out;  // staged, counts in device memory (submits): each group ors its error bits in here
    // staged, tagged completion (synchronous calls): counts are u64 host words (generation << 32 | count)
    // and each candidate group stores its error snapshot (generation << 32 | bits) at grp_err[ticket index]
    uint32_t tag;
    uint64_t* grp_err;
    // staged: workgroups 0 .. n-1 stage, every wave of them, every segment in order, then they count
    // like the rest (a workgroup's wave holding a ticket would hold its other waves until its chunk
    // is packed); a staged launch with chunks always has n > 0 (0 is reported as a staging error)
    uint32_t copier_wgs;
    uint32_t n_segs;
    uint32_t eq;  // every live segment has equal windows (ulen), checked on the host to fit its image
    uint32_t m;  // k-mer length
    uint32_t P;  // candidates per lane word
    uint32_t bs;  // the bit-sliced kernel (bs_count.inc) counts this launch: `chunk` is in rows of windows
    uint32_t max_errors;  // the edit budget E (0..3) of the counts: a window adds max(0, E + 1 - d); other
                          // than 2 on bit-sliced launches only (3: the bs3_count.hip kernels)
    // Hit levels (bsh_count.hip; DESIGN.md §4e "Hit levels"), appended so that no field above moves: per
    // segment the device matrix the launch's hits kernel writes -- level e, window w, word c / 32 at
    // hits[(e * n_windows + w) * ceil(n_kmers / 32) + c / 32] -- read by that kernel family only.
    uint32_t* hits[AC_MAX_SEGS];
    uint32_t want_hits;  // the launch runs a hits-writing kernel (bit-sliced launches only; staged: bshs_count.hip)
    // Match end positions (bsp_count.hip; DESIGN.md §4e "Match end positions"), appended again: per segment
    // the device matrix of eight bit planes -- bit c % 32 of pos[(b * n_windows + w) * ceil(n_kmers / 32) +
    // c / 32] is bit b of pos - 1, 0 where window w holds candidate c at no level -- written beside the hits.
    uint32_t* pos[AC_MAX_SEGS];
    uint32_t want_pos;  // the launch runs a hits-and-positions kernel (implies want_hits)
    // Hits from the jobs stage (DESIGN.md §4e "Hits from the jobs stage"), appended again: per segment the window
    // count of the MATRIX hits[i] / pos[i] point into -- the level planes (and position planes) lie mat_nw[i] *
    // ceil(n_kmers / 32) words apart.  A whole-segment launch: the segment's n_windows.  A launch that counts
    // windows [lo, hi) of a job (a part of a DMA-path call): the job's n_windows, and the host has folded the
    // first row, lo * ceil(n_kmers / 32) words, into the pointers.
    uint32_t mat_nw[AC_MAX_SEGS];
};

inline uint32_t pack_factor(uint32_t k) { return (32u / k) < AC_MAX_PACK ? (32u / k) : AC_MAX_PACK; }
// candidates per wave of the plain (staged = false) or the early launch's staged kernel
inline uint32_t cands_per_wave(uint32_t P, bool staged) { return 64u * P * (uint32_t)words_for((int)P, staged); }

// The bit-sliced kernel (bs_count.inc): a candidate group of n candidates (1 .. the
// group size BS_GROUP) takes 1 << bs_lane_shift(n) lanes per window -- one per block of 32
// candidates, rounded up to a power of two, at least 2 (a row's text is parked in LDS: 32 windows'
// worth per wave) -- and a wave counts a row of 64 >> bs_lane_shift(n) consecutive windows at once.
// Its candidate groups hold BS_GROUP candidates whatever k is: for k = 16 that is the word-parallel
// kernel's group (cands_per_wave(2, *)), for k >= 17 (P = 1) it is not -- the host sizes a launch's
// groups with launch_group_size (stage_plan.h).
constexpr uint32_t BS_GROUP = 64u * 2u * (uint32_t)words_for(2, false);
static_assert(words_for(2, false) == words_for(2, true), "one group size for plain and staged launches");
inline __host__ __device__ uint32_t bs_lane_shift(uint32_t n) {
    const uint32_t blocks = (n + 31u) / 32u;
    uint32_t s = 1;
    while ((1u << s) < blocks) ++s;
    return s;
}
// rows of a segment's group g (of `cpw` candidates, the last one fewer) over n_windows windows
inline uint64_t bs_rows(uint32_t n_kmers, uint32_t g, uint32_t cpw, uint32_t n_windows) {
    const uint32_t n = n_kmers - g * cpw < cpw ? n_kmers - g * cpw : cpw;
    const uint32_t wpr = 64u >> bs_lane_shift(n);
    return ((uint64_t)n_windows + wpr - 1u) / wpr;
}

// A family of bit-sliced kernels: what a launch asks of the body beyond k.  Everything that differs from
// one family to the next -- the kernel, its residency, its slot in the context's resident-wave cache -- is
// looked up by this key.
enum class BsOut { Count, Hits, Pos };  // what a window leaves: counts; and its hit words; and its end positions
struct BsFamily {
    bool staged;  // the early launch's kernel, which stages its own inputs
    BsOut out;
    int rows;  // NFA rows: 3 (edit budgets 0..2) or 4 (budget 3)
};
// The one place that names a family from a launch's four facts (positions come with hits).
constexpr BsFamily bs_family(bool staged, bool hits, bool pos, uint32_t max_errors) {
    return BsFamily{staged, pos ? BsOut::Pos : hits ? BsOut::Hits : BsOut::Count, max_errors == 3u ? 4 : 3};
}
constexpr int BS_FAMILIES = 12;
constexpr int bs_family_index(BsFamily f) { return ((int)f.out * 2 + (f.staged ? 1 : 0)) * 2 + (f.rows == 4 ? 1 : 0); }
constexpr bool bs_family_indices_distinct() {
    uint32_t seen = 0;
    for (int staged = 0; staged < 2; ++staged)
        for (int hits = 0; hits < 2; ++hits)
            for (int pos = 0; pos <= hits; ++pos)
                for (uint32_t e = 2; e <= 3; ++e) {
                    const int i = bs_family_index(bs_family(staged != 0, hits != 0, pos != 0, e));
                    if (i < 0 || i >= BS_FAMILIES || (seen >> i & 1u)) return false;
                    seen |= 1u << i;
                }
    return seen == (1u << BS_FAMILIES) - 1u;
}
static_assert(bs_family_indices_distinct(), "twelve families, twelve slots");

// Resident waves per SIMD of the bit-sliced kernel of family f for pattern length k: the NFA state is 3 k
// registers and a base's table rows 2 k more, so the wider instantiations run at the highest residency
// whose register budget holds them without scratch access inside the 4-base block.
// __launch_bounds__, the LDS allocation that caps residency (bs_blocks_per_cu) and the host's launch
// sizing all take it from here.  The -D knobs are for A/B builds.
#ifndef BS_WAVES_PER_SIMD
#define BS_WAVES_PER_SIMD 4  // counting, three rows: k = 16
#endif
#ifndef BS_WAVES_PER_SIMD_MID
#define BS_WAVES_PER_SIMD_MID 3  // ... k = 18..BS_K_MID, then 2
#endif
#ifndef BS_K_MID
#define BS_K_MID 23  // (k = 24: the staged kernel spills VGPRs inside the NFA block at 3 waves)
#endif
// An edit budget of 3 (bs3_count.hip) is a fourth row, 4 k registers of state: 3 waves up to BS3_K_MID, then 2;
// from BS3_ONE_BASE_K on the block holds one base's table rows at a time instead of two (bs_block4), which
// is what keeps k = 29..32 at 2 waves without scratch access inside the block (DESIGN.md 4e "Edit budget").
#ifndef BS3_K_MID
#define BS3_K_MID 19
#endif
#ifndef BS3_ONE_BASE_K
#define BS3_ONE_BASE_K 29
#endif
// The hits-and-positions family (bsp_count.hip): eight position planes and per-base hit accumulation more
// in registers, so its residency is re-derived per (K, rows) from the compiler's remarks
// (profiles/r14_bsp_codegen.txt).
#ifndef BSP_WAVES_PER_SIMD_16
#define BSP_WAVES_PER_SIMD_16 4  // three rows, k = 16
#endif
#ifndef BSP_K_MID
#define BSP_K_MID 23  // three rows: 3 waves for k = 18..BSP_K_MID, then 2
#endif
#ifndef BSP3_K_MID
#define BSP3_K_MID 18  // four rows: 3 waves up to here, then 2 ...
#endif
#ifndef BSP3_K_ONE
#define BSP3_K_ONE 31  // ... and from here on 1 (two waves spill inside the block even with one base's rows held)
#endif
#ifndef BSP3_ONE_BASE_K
#define BSP3_ONE_BASE_K 26  // four rows: one base's table rows at a time from here on (BS3_ONE_BASE_K's sibling)
#endif
// The staged hits-writing family (bshs_count.hip: the early launch and device packing of ac_window_hits_jobs)
// and the staged hits-and-positions family (bsps_count.hip), re-derived likewise
// (profiles/r15_bshs_codegen.txt): the staged frame's state costs registers the plain kernels do not hold.
#ifndef BSHS_WAVES_PER_SIMD_16
#define BSHS_WAVES_PER_SIMD_16 3  // three rows, k = 16: the staged counting kernel sits at exactly 128 VGPRs
#endif
#ifndef BSHS_K_MID
#define BSHS_K_MID 23  // three rows: 3 waves for k = 18..BSHS_K_MID, then 2
#endif
#ifndef BSHS3_K_MID
#define BSHS3_K_MID 19  // four rows: 3 waves up to here, then 2
#endif
#ifndef BSPS_WAVES_PER_SIMD_16
#define BSPS_WAVES_PER_SIMD_16 3
#endif
#ifndef BSPS_K_MID
#define BSPS_K_MID 23  // three rows: 3 waves for k = 18..BSPS_K_MID but BSPS_K_TWO, then 2
#endif
#ifndef BSPS_K_TWO
#define BSPS_K_TWO 22  // (k = 22 alone of 18..23 has scratch accesses inside the NFA block at 3 waves)
#endif
#ifndef BSPS3_K_MID
#define BSPS3_K_MID 16  // four rows: 3 waves up to here (k = 18 spills inside the block at 3), then 2 ...
#endif
#ifndef BSPS3_K_ONE
#define BSPS3_K_ONE 31  // ... and from here on 1, like the plain family
#endif
constexpr int bs_waves_per_simd(BsFamily f, int k) {
    const bool four = f.rows == 4;
    if (f.out == BsOut::Pos && f.staged)
        return four ? (k <= BSPS3_K_MID ? 3 : k < BSPS3_K_ONE ? 2 : 1)
                    : k <= 16 ? BSPS_WAVES_PER_SIMD_16 : (k <= BSPS_K_MID && k != BSPS_K_TWO) ? 3 : 2;
    if (f.out == BsOut::Pos)
        return four ? (k <= BSP3_K_MID ? 3 : k < BSP3_K_ONE ? 2 : 1)
                    : k <= 16 ? BSP_WAVES_PER_SIMD_16 : k <= BSP_K_MID ? 3 : 2;
    if (f.out == BsOut::Hits && f.staged)
        return four ? (k <= BSHS3_K_MID ? 3 : 2) : k <= 16 ? BSHS_WAVES_PER_SIMD_16 : k <= BSHS_K_MID ? 3 : 2;
    // counting, plain and staged, and the plain hits-writing family (bsh_count.hip): its stores sit outside
    // the 4-base block and the compiler's occupancy equals its counting twin's (profiles/r12_bsh_codegen.txt)
    return four ? (k <= BS3_K_MID ? 3 : 2) : k <= 16 ? BS_WAVES_PER_SIMD : k <= BS_K_MID ? BS_WAVES_PER_SIMD_MID : 2;
}
// Workgroups per CU that a kernel's LDS array leaves room for (each kernel sizes its array as 160 KB over
// this): its residency -- a kernel at one wave per SIMD takes the LDS of two, its registers cap it.
constexpr int bs_blocks_per_cu(BsFamily f, int k) {
    return 4 * (bs_waves_per_simd(f, k) > 2 ? bs_waves_per_simd(f, k) : 2) / AC_WAVES_PER_BLOCK;
}

typedef void (*CountKernel)(LaunchArgs);
// The family translation units' pickers: the kernel of family f for k (AC_BS_K_LIST), nullptr if there is
// none.  Each serves the families its unit holds: bs3_count.hip counting at four rows (plain and staged),
// bsh_count.hip / bsp_count.hip the plain hits and hits-and-positions kernels, bshs_count.hip /
// bsps_count.hip their staged forms (three rows and four).
typedef CountKernel BsPicker(uint32_t k, BsFamily f);
BsPicker bs3_kernel, bsh_kernel, bsp_kernel, bshs_kernel, bsps_kernel;
hipError_t resident_waves_bs(BsFamily f, uint32_t k, int cu_count, uint32_t* waves);
// bsh_count.hip: level_counts[e * n_kmers + c] = the windows of level plane e of a hit matrix that hold
// candidate c (a column popcount); level_counts is zeroed on the stream first
hipError_t launch_hit_level_counts(const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows, uint32_t levels,
                                   uint32_t* level_counts, hipStream_t stream);
// bsp_count.hip: profile[(d * n_kmers + c) * window_len + p - 1] = the windows that hold candidate c at
// distance exactly d with their best occurrence ending at base p (1..window_len), from a hit matrix of
// `levels` planes and its position matrix; profile is zeroed on the stream first
hipError_t launch_hit_position_profile(const uint32_t* hits, const uint32_t* pos, uint32_t n_kmers, uint32_t n_windows,
                                       uint32_t levels, uint32_t window_len, uint32_t* profile, hipStream_t stream);
// hit_cooc.hip: cooc[(e * n_kmers + a) * n_kmers + b] = the windows of level plane e of a hit matrix that hold
// candidates a and b both.  stages bit 0: the planes' transposition into `scratch`
// (hit_cooc_scratch_words u32); bit 1: the product from scratch into cooc, every word of which is then
// defined (zeroed on the stream first where the launch rule splits the window axis).  3 = the whole call.
uint64_t hit_cooc_scratch_words(uint32_t n_kmers, uint32_t n_windows, uint32_t levels);
hipError_t launch_hit_cooccurrence(const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows, uint32_t levels,
                                   uint32_t* scratch, uint32_t* cooc, uint32_t stages, hipStream_t stream);
// hit_cooc.hip: window_counts[e * n_windows + w] = the candidates < n_kmers that row w of plane e holds; every
// word stored once
hipError_t launch_hit_window_counts(const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows, uint32_t levels,
                                    uint32_t* window_counts, hipStream_t stream);
// hit_span.hip: the start matrix (hit_span.h: eight planes of the hit matrix's shape) of a hit matrix of
// `levels` planes and its position matrix over equal windows of window_len bases (1..256) at ceil32 strides
// of the image codes / nmask; every word of start stored once
hipError_t launch_hit_start_positions(uint32_t k, const uint64_t* kmers, uint32_t n_kmers, const uint32_t* codes,
                                      const uint32_t* nmask, uint32_t n_windows, uint32_t window_len, const uint32_t* hits,
                                      const uint32_t* pos, uint32_t levels, uint32_t* start, hipStream_t stream);
// hit_flank.hip: the flank profile (hit_flank.h: 2 x n_kmers x depth x 5 words) of one level plane `hit`, its
// position matrix and -- or NULL: the left half stays 0 -- its start matrix over equal windows of window_len
// bases (1..256) at ceil32 strides of the image codes / nmask; depth 1..32; flank is zeroed on the stream
// first (n_kmers = 0: no work; n_windows = 0: the zeroes alone)
hipError_t launch_hit_flank_profile(const uint32_t* codes, const uint32_t* nmask, uint32_t n_windows, uint32_t window_len,
                                    const uint32_t* hit, const uint32_t* pos, const uint32_t* start, uint32_t n_kmers,
                                    uint32_t depth, uint32_t* flank, hipStream_t stream);
// hit_edit.hip: the edit profile (hit_edit.h: n_kmers x k x 12 words) of one level plane `hit`, its position
// matrix and its start matrix over equal windows of window_len bases (1..256) at ceil32 strides of the image
// codes / nmask; k 2..32, kmers on the device; edit is zeroed on the stream first (n_kmers = 0: no work;
// n_windows = 0: the zeroes alone)
hipError_t launch_hit_edit_profile(uint32_t k, const uint64_t* kmers, uint32_t n_kmers, const uint32_t* codes,
                                   const uint32_t* nmask, uint32_t n_windows, uint32_t window_len, const uint32_t* hit,
                                   const uint32_t* pos, const uint32_t* start, uint32_t* edit, hipStream_t stream);

// Waves of the count kernel for pattern pack P that fit on the device at once.
hipError_t resident_waves(uint32_t P, bool staged, int cu_count, uint32_t* waves);

#ifdef AC_STAMPS
hipError_t debug_stamps(void* host, size_t bytes);
#endif

hipError_t launch_wm2_count(const LaunchArgs& args, hipStream_t stream);

}  // namespace acamd
