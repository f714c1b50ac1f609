// wm_count.hip -- the approximate-count kernel for MI355X (gfx950).
//
// Replaces the OpenMP/SeqAn search loop of errorCount
// (approx_counter.cpp:550-599): for every (candidate k-mer, sampled window)
// pair it decides, per error level e = 0,1,2, whether the k-mer occurs in the
// window with at most e edits -- the three per-read bitfields tcount[e] of
// approx_counter.cpp:553/563 -- and adds the number of levels hit to the
// candidate's counter (the vectorSum of 590-593).
//
// Algorithm: bit-parallel Wu-Manber NFA for edit distance <= 2 (Wu & Manber
// 1992) in its complemented "shift-or" form (Baeza-Yates & Gonnet 1992), free
// start in the text.  With R_d bit i = "pattern prefix of length i+1 ends at
// the current text position with <= d edits" and D_d = ~R_d:
//   D0' = (D0 >> P) | ~Eq
//   Dd' = ((Dd >> P) | ~Eq) & Dd-1 & (Dd-1 >> P) & (Dd-1' >> P)      d = 1, 2
// The shift brings in zeros, i.e. "R bit set": that is the free start of row
// 0 and the always-set prefix bits of rows 1 and 2, with no mask operation.
// A window hits level d iff the AND of D_d over its positions has the
// pattern's last bit clear; the count adds the three levels.
//
// MI355X mapping:
//  * lane = P candidates, window text wave-uniform.  P = floor(32/k) (<= 4)
//    patterns are INTERLEAVED in one 32-bit register: character i of pattern p
//    sits at bit 31 - (i*P + p), so one logical right shift by P advances every
//    pattern at once and the zero fill reaches every pattern's first character.
//  * W lane words per wave (words_for(P): 2 for P = 2, i.e. k = 11-16, else 1):
//    each lane carries W x P candidates, and the W NFAs share every base's
//    SALU work and text.
//  * ~Eq is a table lookup, as in the textbook algorithm: each WORKGROUP (4
//    waves, all on one candidate group) keeps one W x 5 x 64-word LDS table
//    (per lane word: the lane's ~Eq for A, C, G, T, and all ones for N), built
//    by its wave 0; every wave reads one word per lane, lane word and text base
//    with ds_read_addtid_b32, the address coming from M0 = 256 * character,
//    two SALU ops from the wave-uniform 2-bit text held in an SGPR.  No VALU op
//    per base for ~Eq.
//  * The NFA runs in generated inline-asm blocks (wm_tid_blocks.inc,
//    tools/gen_tid_blocks.py): 8 full-rate VALU ops per base (v_or, v_lshrrev,
//    v_bitop3 -- the forms that issue in 2 cycles per wave64 on gfx950,
//    profiles/r01_ubench_valu.txt) + 1.5 of hit accumulation (AND3 over two
//    bases) = 9.5 VALU ops per base and lane word (P candidates), scheduled
//    skewed (row 0 of base s, row 1 of base s-1, row 2 of base s-2 per step) so
//    a lane word has three independent dependency chains, with the LDS reads
//    three bases ahead.
//  * The table is the workgroup's first LDS object, at address 0, so M0 needs
//    no per-wave add: per base 2 SALU + W LDS + 9.5 W VALU.  The SALU is the
//    CU-shared resource the first table-driven version ran out of (5 SALU per
//    base: no faster than computing ~Eq with 2 VALU ops; profiles/r01_kernel_log.md).
//  * Integer-only VALU work: no MFMA.  Counts are uint32 atomics
//    (order-independent, bit-exact).
//
// One translation unit, in files (map: DESIGN.md §4): here the word-parallel body (count_body; loop in
// wm_window_loop.inc, NFA blocks in wm_tid_blocks.inc), the two __global__ kernels and their dispatch;
// stage_dev.inc the staged launch's device side; count_frame.inc what the bodies share (deal, gate,
// count hand-off); bs_count.inc the bit-sliced body (k in AC_BS_K_LIST, equal windows).
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
#ifdef AC_STAMPS
// Diagnostic build only (tools/variants.sh ... -DAC_STAMPS): per-wave
// s_memrealtime stamps (100 MHz) at entry, after the prologue, after the last
// window and at exit; read back with ac_debug_stamps().  No output value is
// computed from them.
}  // namespace
__device__ uint64_t g_stamps[1 << 21];
__device__ uint64_t g_stage_stamps[64];  // per segment s, at [s*8 + i]: 0 final header seen by the poller, 1 its first
                                         // progress record, 2 last chunk in, 3 first record past the k-mers, 4 first
                                         // codes chunk flagged
namespace {
__device__ __forceinline__ void stamp(uint64_t wave, int i) {
    if ((threadIdx.x & 63u) == 0 && wave < (1u << 18)) {
        g_stamps[wave * 8 + i] = __builtin_amdgcn_s_memrealtime();
        if (i == 0) {
            uint32_t hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            g_stamps[wave * 8 + 4] = hw;
            g_stamps[wave * 8 + 5] = xcc;
        }
    }
}
__device__ __forceinline__ void stamp_val(uint64_t wave, int i, uint64_t v) {
    if ((threadIdx.x & 63u) == 0 && wave < (1u << 18)) g_stamps[wave * 8 + i] = v;
}
__device__ __forceinline__ void stage_stamp(uint32_t si, int i) {
    if ((threadIdx.x & 63u) == 0) g_stage_stamps[si * 8 + i] = __builtin_amdgcn_s_memrealtime();
}
}  // namespace
__device__ uint64_t g_win_stamps[1 << 20];  // per wave w < 2^15: the end of its windows 0..31 at [w * 32 + i]
namespace {
__device__ __forceinline__ void stamp_win(uint64_t wave, uint32_t i) {
    if ((threadIdx.x & 63u) == 0 && wave < (1u << 15) && i < 32u) g_win_stamps[wave * 32 + i] = __builtin_amdgcn_s_memrealtime();
}
#else
__device__ __forceinline__ void stamp_win(uint64_t, uint32_t) {}
__device__ __forceinline__ void stamp(uint64_t, int) {}
__device__ __forceinline__ void stamp_val(uint64_t, int, uint64_t) {}
__device__ __forceinline__ void stage_stamp(uint32_t, int) {}
#endif
constexpr uint32_t SEG = 256;  // window bases fetched per pass (16 code words, 8 N-mask words)

// 32-bit outer unshuffle (Hacker's Delight 7-2): odd bits to the upper half,
// even bits to the lower half, order kept.
__device__ __forceinline__ uint32_t unshuffle32(uint32_t x) {
    uint32_t t;
    t = (x ^ (x >> 1)) & 0x22222222u; x ^= t ^ (t << 1);
    t = (x ^ (x >> 2)) & 0x0c0c0c0cu; x ^= t ^ (t << 2);
    t = (x ^ (x >> 4)) & 0x00f000f0u; x ^= t ^ (t << 4);
    t = (x ^ (x >> 8)) & 0x0000ff00u; x ^= t ^ (t << 8);
    return x;
}

// Lane masks of P k-mers (dna2int layout, approx_counter.cpp:55-62):
// character i of pattern p at bit 31 - (i*P + p); ph holds the high bit of
// each character's 2-bit code, pl the low bit.  No per-character loop for the
// two packs the baseline configurations use (P = 2: k = 11..16, P = 1: k > 16).
template <int P>
__device__ __forceinline__ void build_masks(const uint64_t (&km)[P], uint32_t m, uint32_t& ph, uint32_t& pl) {
    if constexpr (P == 2) {
        // Left-aligned 2-bit codes already interleave a pattern's high and low
        // bits; the second pattern slots in one bit lower.
        const uint32_t a = (uint32_t)km[0] << (32u - 2u * m), b = (uint32_t)km[1] << (32u - 2u * m);
        ph = (a & 0xaaaaaaaau) | ((b & 0xaaaaaaaau) >> 1);
        pl = ((a << 1) & 0xaaaaaaaau) | (b & 0x55555555u);
    } else if constexpr (P == 1) {
        const uint64_t x = km[0] << (64u - 2u * m);
        const uint32_t H = unshuffle32((uint32_t)(x >> 32)), L = unshuffle32((uint32_t)x);
        ph = (H & 0xffff0000u) | (L >> 16);
        pl = (H << 16) | (L & 0xffffu);
    } else {
        ph = 0;
        pl = 0;
#pragma unroll
        for (int p = 0; p < P; ++p)
            for (uint32_t i = 0; i < m; ++i) {
                const uint32_t b = (uint32_t)(km[p] >> (2u * (m - 1u - i))) & 3u;
                ph |= (b >> 1) << (31u - (i * P + p));
                pl |= (b & 1u) << (31u - (i * P + p));
            }
    }
}

#ifdef AC_TID_BLOCKS_INC  // A/B builds (tools/variants.sh) of another generator setting
#include AC_TID_BLOCKS_INC
#else
#include "wm_tid_blocks.inc"
#endif

// Window descriptor (start, length) of window w with scalar loads: the arrays
// do not change during a launch, so the constant address space is legal, and
// both loads are in flight together (as vector loads hipcc waited for the
// start before issuing the length: two round trips per window).
typedef const __attribute__((address_space(4))) uint64_t* cu64p;
typedef const __attribute__((address_space(4))) uint32_t* cu32p;
__device__ __forceinline__ void load_desc(const uint64_t* start, const uint32_t* length, uint32_t w, uint64_t& base,
                                          uint32_t& len) {
#if !defined(AC_VECTOR_DESC)
    base = ((cu64p)start)[w];
    len = ((cu32p)length)[w];
#else
    base = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(start[w] >> 32)) << 32) |
           __builtin_amdgcn_readfirstlane((uint32_t)start[w]);
    len = __builtin_amdgcn_readfirstlane(length[w]);
#endif
}

// The same with vector loads, for staged launches: their descriptors are copied
// in by the kernel itself, so they DO change during the launch, and a scalar
// (constant address space) load could be hoisted above the staging wait or hit
// a scalar-cache line filled before it.
typedef const __attribute__((address_space(1))) uint64_t* gu64p;
typedef const __attribute__((address_space(1))) uint32_t* gu32p;
__device__ __forceinline__ void load_desc_vec(const uint64_t* start, const uint32_t* length, uint32_t w, uint64_t& base,
                                              uint32_t& len) {
    const uint64_t b = ((gu64p)start)[w];
    const uint32_t l = ((gu32p)length)[w];
    base = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) << 32) |
           __builtin_amdgcn_readfirstlane((uint32_t)b);
    len = __builtin_amdgcn_readfirstlane(l);
}

// The workgroup's ~Eq table (shared by its waves): for lane word w, word w*320 + c*64 + lane =
// the lane's ~Eq mask for character c (A C G T, then N = all ones), read per base with
// ds_read_addtid_b32.
template <int W>
struct TidTable {
    uint32_t e[W * 5 * 64];  // lane word w's table at e[w * 320]
};

// A window fetch: bases [pos, pos + 256) -- 16 code words and 8 N-mask words -- through buffer
// descriptors of the segment's two arrays (SGPRs); the byte offset is the window's (an SGPR) plus a
// per-lane constant.  The descriptors' range check (num_records = the array's bytes, voffset
// included) returns 0 for a word past the image, so no clamp: words past the window are never read
// as text (the chunk loop stops at the window length).  The consumer (tid_word) takes lanes 0-15's
// code words and lanes 16-23's N-mask words.
struct Image {
    __amdgpu_buffer_rsrc_t codes, nmask;
};
struct Fetch {
    uint32_t c, n;
};
__device__ __forceinline__ void tid_fetch(Fetch& f, const Image& im, uint64_t pos, uint32_t lane, uint32_t lane_off) {
    // Every lane loads both words -- code word (lane & 15) and N-mask word (lane & 7) of the segment;
    // lanes past 16 / 8 repeat addresses of the same lines, which the load coalesces -- so both results
    // are whole registers.  (Round 4 loaded each half under its own exec mask: hipcc then merged the
    // halves with the previous window's values, copying them back after a wait for both loads
    // -- s_waitcnt vmcnt(0) right after every prefetch inside multi-window items -- and computed the
    // second offset into the first load's destination, another wait.)
    (void)lane;
    f.c = __builtin_amdgcn_raw_buffer_load_b32(im.codes, (uint32_t)(pos >> 2) + (lane_off & 63u), 0, 0);
    f.n = __builtin_amdgcn_raw_buffer_load_b32(im.nmask, (uint32_t)(pos >> 3) + (lane_off >> 8), 0, 0);
}
__device__ __forceinline__ uint32_t tid_word(const Fetch& f, uint32_t lane) { return lane < 16u ? f.c : f.n; }

// start % 32 == 0 && length <= n_bases && start <= n_bases - length, on the
// scalar unit (hipcc compares 64-bit values with VALU ops), written so that no
// sum wraps: a start near 2^64 must not pass.
template <bool RFL>
__device__ __forceinline__ uint32_t window_valid(uint64_t base, uint32_t len, uint64_t nb) {
    // (RFL, the staged kernel: its early-counting gate leaves hipcc holding some of these
    // wave-uniform values in VGPRs; readfirstlane puts them back in SGPRs for the asm)
    const uint32_t nbl = RFL ? __builtin_amdgcn_readfirstlane((uint32_t)nb) : (uint32_t)nb;
    const uint32_t nbh = RFL ? __builtin_amdgcn_readfirstlane((uint32_t)(nb >> 32)) : (uint32_t)(nb >> 32);
    const uint32_t ln = RFL ? __builtin_amdgcn_readfirstlane(len) : len;
    const uint32_t bl = RFL ? __builtin_amdgcn_readfirstlane((uint32_t)base) : (uint32_t)base;
    const uint32_t bh = RFL ? __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) : (uint32_t)(base >> 32);
    uint32_t bad, t0, t1;
    asm("s_sub_u32 %[t0], %[nbl], %[len]\n\t"
        "s_subb_u32 %[t1], %[nbh], 0\n\t"  // scc: n_bases < length
        "s_cselect_b32 %[bad], 1, 0\n\t"
        "s_sub_u32 %[t0], %[t0], %[bl]\n\t"
        "s_subb_u32 %[t1], %[t1], %[bh]\n\t"  // scc: n_bases - length < start
        "s_cselect_b32 %[bad], 1, %[bad]\n\t"
        "s_and_b32 %[t0], %[bl], 31\n\t"  // scc: misaligned start
        "s_cselect_b32 %[bad], 1, %[bad]"
        : [bad] "=&s"(bad), [t0] "=&s"(t0), [t1] "=&s"(t1)
        : [nbl] "s"(nbl), [nbh] "s"(nbh), [len] "s"(ln), [bl] "s"(bl), [bh] "s"(bh)
        : "scc");
    return bad ^ 1u;
}

// The workgroup's waves serve one candidate group and share one table, the
// first LDS object, at address 0, so M0 needs no per-base add (the eb0 form of
// tools/gen_tid_blocks.py).
constexpr bool TID_EB0 = true;

// Workgroup LDS: the ~Eq table, then the count vector the waves sum into,
// then the staged launch's verdict for the workgroup's segment.
template <int W>
struct BlockLds {
    TidTable<W> tab;
    uint32_t cnt[W * AC_MAX_PACK * 64];
    uint32_t stage_r;
};

#include "stage_dev.inc"    // the staged launch's device side: copier loops, device packer, readers' waits
#include "count_frame.inc"  // what count_body and bs_body (bs_count.inc) share around their NFAs

// The NFA blocks over the wave's W lane-word states (two words: the generated
// tid2_* blocks, one base's SALU work and text shared by both words).
#define AC_NFA(nb, s, ...)                                            \
    do {                                                              \
        if constexpr (W == 2)                                         \
            tid2_block##nb<P, TID_EB0>(s[0], s[W - 1], __VA_ARGS__); \
        else                                                          \
            tid_block##nb<P, TID_EB0>(s[0], __VA_ARGS__);            \
    } while (0)
#define AC_NFA_FIRST(s, ...)                                               \
    do {                                                                   \
        if constexpr (W == 2)                                              \
            tid2_block32_first<P, TID_EB0>(s[0], s[W - 1], __VA_ARGS__); \
        else                                                               \
            tid_block32_first<P, TID_EB0>(s[0], __VA_ARGS__);            \
    } while (0)

// The remainder (< 16 bases) of a segment: blocks of 8, 4, 2, 1 bases.
template <int P, int W>
__device__ __forceinline__ void tid_tail(TidNfa* s, uint32_t code, uint32_t nm, uint32_t rem, uint32_t eb) {
    if (rem & 8u) {
        AC_NFA(8, s, code, nm & 0xffu, eb);
        code >>= 16;
        nm >>= 8;
    }
    if (rem & 4u) {
        AC_NFA(4, s, code, nm & 0xfu, eb);
        code >>= 8;
        nm >>= 4;
    }
    if (rem & 2u) {
        AC_NFA(2, s, code, nm & 0x3u, eb);
        code >>= 4;
        nm >>= 2;
    }
    if (rem & 1u) AC_NFA(1, s, code, nm & 0x1u, eb);
}

// STAGED: the early-launch instantiation (staging wait, vector descriptor loads,
// system-scope count stores, tagged completion).  The plain launches get a kernel
// without any of it: in one kernel the extra live values cost SGPR spills inside
// the count loop (+2.5 % VALU, +3.4 % SALU instructions, ~5 % time at cfg2).
// EQ: every live segment holds equal windows back to back (ulen set; the host has checked that they
// fit the image): window places by arithmetic, no descriptor arrays or per-window range checks held
// in registers (the staged kernel spilled SGPRs inside the count loop without this).
template <int P, bool STAGED, bool EQ>
__device__ __forceinline__ void count_body(const LaunchArgs& a, BlockLds<words_for(P, STAGED)>& lds) {
    constexpr int W = words_for(P, STAGED);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wib;
    stamp(wave, 0);
    // this workgroup's block-queue, this wave's segment, candidate group g and sub-queue j (count_frame.inc)
    const Deal deal = deal_of(a);
    const Place pl = place_of(a, deal.bq, wib);
    const int si = pl.si;
    const SegDev& sg = a.seg[si];
    const uint32_t g = pl.g, j = pl.j, rank = deal.rank;
    // Staged launch: the segment's inputs are not there yet (staged_prologue), and equal windows are
    // counted as they arrive (Gate).
    Gate gt;
    gt.has_n = sg.has_n;
    bool skip = false;
    if (STAGED && sg.stage_chunks) {  // (a segment sent ahead of a staged launch has no chunks)
        gt.words = a.stage + AC_STAGE_L_SEG(si) * AC_QUEUE_LINE;
        // the k-mer section fills whole chunks and is in the pinned block before the launch
        const uint32_t pre_bytes = sg.stage_codes_off;
        if (blockIdx.x < a.copier_wgs) {
            // Copier workgroup: every wave serves every segment's tickets, starting
            // with segment (workgroup mod segments) -- the host packs a large call's jobs interleaved,
            // so all segments arrive together -- before the workgroup counts like the others.
            for (uint32_t i2 = 0; i2 < a.n_segs; ++i2) {
                const uint32_t s2 = (blockIdx.x + i2) % a.n_segs;
                const SegDev& c2 = a.seg[s2];
                if (!c2.stage_chunks) continue;
#ifndef AC_NO_DEVICE_PACK
                const bool ok = c2.dp_src
                                    ? stage_copy_dp(c2, a.stage + AC_STAGE_L_SEG(s2) * AC_QUEUE_LINE, a.gen, a.err)
                                    : stage_copy(c2.stage_src, c2.stage_dst, c2.stage_chunks,
                                                 c2.stage_codes_off / AC_STAGE_CHUNK, a.host_hdr + s2 * AC_QUEUE_LINE,
                                                 a.stage + AC_STAGE_L_SEG(s2) * AC_QUEUE_LINE, c2.stage_gen, a.gen, s2);
#else  // (A/B builds without the device packer: its code out of the staged kernel, the host never asks for it)
                const bool ok = stage_copy(c2.stage_src, c2.stage_dst, c2.stage_chunks, c2.stage_codes_off / AC_STAGE_CHUNK,
                                           a.host_hdr + s2 * AC_QUEUE_LINE, a.stage + AC_STAGE_L_SEG(s2) * AC_QUEUE_LINE,
                                           c2.stage_gen, a.gen, s2);
#endif
                if (!__builtin_amdgcn_readfirstlane((uint32_t)ok))
                    if (lane == 0) atomicOr(a.err, AC_DEVERR_STAGE);
            }
        }
        if (wib == 0) {
            uint32_t r = ~0u;
            const bool equal = sg.ulen != AC_NO_ULEN && sg.n_kmers;
            // (the copier workgroups stage every chunk: a launch with chunks has them, count_launch.cpp
            // stage_copiers; round 3's wave-0 tickets in every workgroup were removed in round 5)
            if (!a.copier_wgs) {
                if (lane == 0) atomicOr(a.err, AC_DEVERR_STAGE);
            } else if (equal) {
                // only the k-mers (the ~Eq table) are needed before counting starts
                r = (uint32_t)stage_gate(gt.words, sg.stage_gen, sg.stage_chunks, blockIdx.x % AC_STAGE_REPL, a.gen, 0u,
                                         8u * sg.n_kmers, a.err, pre_bytes);
            } else {
                r = stage_wait_all(gt.words, sg.stage_chunks, blockIdx.x % AC_STAGE_REPL, a.err);
            }
            if (lane == 0) lds.stage_r = r;
            stamp(wave, 7);  // diagnostic builds (staged): the staging wait is over
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        const uint32_t r = __builtin_amdgcn_readfirstlane(lds.stage_r);
        skip = gt.open(r);
    }
    // The segment's arrays, pinned in SGPRs for the whole launch: read through the `sg` reference hipcc reloaded them from
    // the kernel arguments in every window, each load waited for on the spot.  The image through buffer
    // descriptors (range-checked fetches, tid_fetch); images are < 2^34 bases (checked on the host), so
    // every byte offset fits 32 bits.
    // (inputs pinned in SGPRs by an asm operand: hipcc must see them wave-uniform, or it wraps every
    // fetch in a waterfall loop)
    const uint32_t* codes_p = sg.codes;
    const uint32_t* nmask_p = sg.nmask;
    // (an N-free image: a zero-sized N-bitmap descriptor, whose loads all return 0 without a memory access)
    // (a segment with inline N records never fetches bitmap words with its windows: only a window
    // whose record overflowed reads its own, through a descriptor made for it)
    uint32_t code_bytes = (uint32_t)(sg.n_bases >> 2),
             nmask_bytes = (gt.has_n && !sg.nrec) ? (uint32_t)(sg.n_bases >> 3) : 0u;
    asm volatile("" : "+s"(codes_p), "+s"(nmask_p), "+s"(code_bytes), "+s"(nmask_bytes));
    Image im;
    im.codes = __builtin_amdgcn_make_buffer_rsrc((void*)codes_p, 0, (int)code_bytes, 0x00020000);
    im.nmask = __builtin_amdgcn_make_buffer_rsrc((void*)nmask_p, 0, (int)nmask_bytes, 0x00020000);
    const uint64_t* g_start = sg.start;
    const uint32_t* g_length = sg.length;
    uint64_t g_nbases = sg.n_bases;
    uint32_t* g_queue = group_counters(a, sg, g);
    if constexpr (!EQ) asm volatile("" : "+s"(g_start), "+s"(g_length), "+s"(g_nbases));
    // Equal windows packed back to back (the host-buffer stage's image): descriptors by arithmetic.
    uint32_t ulen = sg.ulen;
    asm volatile("" : "+s"(ulen));
    const uint32_t ustride = ulen == AC_NO_ULEN ? 0u : (ulen + 31u) & ~31u;
    // The segment's fields read inside the window loop, pinned: under the staged kernel's SGPR
    // pressure hipcc otherwise reloaded them from the kernel arguments at every item and gate call --
    // scalar loads, which count in lgkmcnt, so the NFA blocks' LDS waits waited for them too (staged
    // kernel on resident input +4.7 % wave-cycles at cfg3, 11x the SMEM instructions,
    // profiles/r05_m22).  Spilled to VGPR lanes instead, a reload is one VALU op.
    uint32_t seg_nw = sg.n_windows, seg_chunk = sg.chunk, seg_qb = sg.queue_begin;
    asm volatile("" : "+s"(seg_nw), "+s"(seg_chunk), "+s"(seg_qb));
    if constexpr (STAGED) gt.pin(sg);
    // inline N records (nrec.h): the lane of the fetch holding a window's record word, ~0u: none
    uint32_t rec_lane = sg.nrec ? nrec_word(ulen) : ~0u;
    asm volatile("" : "+s"(rec_lane));
    auto desc = [&](uint32_t ww, uint64_t& base_out, uint32_t& len_out) __attribute__((always_inline)) {
        if (EQ || ulen != AC_NO_ULEN) {
            base_out = (uint64_t)ww * ustride;
            len_out = ulen;
        } else if (STAGED) {
            load_desc_vec(g_start, g_length, ww, base_out, len_out);
        } else {
            load_desc(g_start, g_length, ww, base_out, len_out);
        }
    };
    const uint32_t m = a.m;
    // An occurrence with <= 2 edits spans >= m - 2 bases: none ends in a window's
    // first m - 3 bases, whose hit accumulation the first block skips (12 of them).
    const bool skip_first = m >= 15u;

    // Q = W x P candidates per lane: slot q = w * P + p is pattern p of lane word w
    constexpr int Q = W * P;
    uint32_t cand[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) cand[q] = g * (64u * Q) + (uint32_t)q * 64u + lane;
    uint32_t first = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) first |= 1u << (31 - p);
    // Initial rows (empty text): R1 has character 0 set, R2 characters 0 and 1.
    const uint32_t d1_init = ~first, d2_init = ~(first | (first >> P));
    const TidInit ini = {~0u >> P, d1_init >> P, d2_init >> P, d1_init, d2_init};  // (loop-invariant registers)
    uint32_t cnt[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) cnt[q] = 0;  // (P <= 2: misses, until the loop's end)
    uint32_t n_counted = 0;                   // (wave-uniform) windows whose levels were counted
    const uint32_t eb = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)(&lds.tab.e[0]));
    // The eb0 blocks address the table from LDS 0.  Never expected otherwise;
    // if it were, the waves skip the work (no fault) and report it in the
    // device error word (ac_check) instead of returning short counts silently.
    const bool eb_ok = !TID_EB0 || eb == 0u;
    if (!eb_ok && lane == 0) atomicOr(a.err, AC_DEVERR_SETUP);

    zero_other_bank(a, wave, lane);

    // The group's work queues (SubQueues): items of `chunk` windows; a wave's first item is
    // assigned statically, further ones are claimed one at a time (wm_window_loop.inc).
    const uint32_t S = sg.subq;
    const uint32_t chunk = seg_chunk;
    const uint32_t n_items = (seg_nw + chunk - 1u) / chunk;
    uint32_t jc = j;  // sub-queue currently served
    auto counter = [&](uint32_t jj) {
        return g_queue + (uint64_t)jj * AC_QUEUE_LINE;
    };
    auto waves_in = [&](uint32_t jj) {  // waves dealt to sub-queue (g, jj): their first items are static
        const uint32_t qq = seg_qb + g * S + jj;
        const uint32_t qb = qq / WAVES_PER_BLOCK;  // one wave of every workgroup dealt to block-queue qb
        return deal.wgs_of(qb);
    };
    // Sub-queue jj holds items jj, jj + S, jj + 2S, ... (strided): the waves'
    // first items are the image's first windows, so a staged launch's waves
    // start on the windows that arrive first and move through the image as it
    // arrives.  Round 3 measured strided against contiguous ranges (sub-queue jj
    // = one slice of the image, so each XCD's L2 fetched a slice): cfg2 kernel
    // 104.8 -> 101.1 us, cfg3 equal, cfg5 -0.5 % (profiles/r03_strided_ab.log);
    // contiguous ranges had been worth 1.5-2 % at cfg5 before two lane words per
    // wave and the rotated workgroup deal.
    auto n_in = [&](uint32_t jj) { return jj < n_items ? (n_items - jj + S - 1u) / S : 0u; };
    // Per-sub-queue constants of the served sub-queue, recomputed only when a
    // steal changes it (their divisions are SALU sequences; with 1-window items
    // they ran once per window).
    uint32_t jc_waves = waves_in(jc), jc_items = n_in(jc);
    auto item_of = [&](uint32_t c) { return c < jc_items ? jc + c * S : n_items; };
    auto dequeue_issue = [&]() -> uint32_t {  // lane 0 holds the result; read with readfirstlane
        uint32_t v = 0;
        if (lane == 0) v = __hip_atomic_fetch_add(counter(jc), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return v;
    };
    // Next item from a sibling sub-queue, or n_items.  One wave-wide probe
    // reads up to 63 sibling counters at once (a sequential probe costs one
    // ~2 µs device-scope round trip per sibling, which used to stretch the
    // launch tail); the wave then claims from the first sibling that still had
    // items.  A failed claim means that sibling is dry for good (counters only
    // grow), so the loop ends after at most S - 1 failed claims, and a wave
    // exits only once every sub-queue of its group has been seen dry.
    auto steal = [&]() -> uint32_t {
        for (;;) {
            uint32_t found = S;
            for (uint32_t b = 1; b < S && found == S; b += 63u) {  // siblings j+b .. j+b+62
                bool have = false;
                if (lane < 63u && b + lane < S) {
                    const uint32_t jj = (j + b + lane) % S;
                    const uint32_t v = __hip_atomic_load(counter(jj), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    have = waves_in(jj) + v < n_in(jj);
                }
                const uint64_t mk = __ballot(have);
                if (mk) found = b + (uint32_t)__builtin_ctzll(mk);
            }
            if (found == S) return n_items;
            const uint32_t jj = (j + found) % S;
            jc = jj;
            jc_waves = waves_in(jj);
            jc_items = n_in(jj);
            const uint32_t c = jc_waves + __builtin_amdgcn_readfirstlane(dequeue_issue());
            if (c < jc_items) return item_of(c);
        }
    };
    uint32_t item = (j < n_items && eb_ok && !skip) ? item_of(rank) : n_items;
    uint32_t pending = 0;
    uint32_t w = item * chunk, item_end = min(seg_nw, w + chunk);

    // Window pipeline: the next window's first segment is fetched while the current one is counted.
    // (written so that no sum wraps: a start near 2^64 must not pass)
    auto valid = [&](uint64_t base, uint32_t len) { return EQ || window_valid<STAGED>(base, len, g_nbases) != 0u; };
    // an empty window reads no word (its start may be the image's end)
    auto fetchable = [&](uint64_t base, uint32_t len) { return len != 0u && valid(base, len); };
    // Staged early counting: before a window's first fetch, make sure every byte its fetches read
    // (256 bases per fetch from `base`, up to the image end) is in; false = skip the segment.
    uint32_t n_win = 0;  // (diagnostic builds: windows counted, for the per-window stamps)
    // The segment is complete or skipped (Gate::completed): its N bitmap's descriptor, if it has one.
    auto completed = [&](uint32_t r) __attribute__((always_inline)) {
        if (!gt.completed(r)) return false;
        nmask_bytes = (gt.has_n && rec_lane == ~0u) ? (uint32_t)(g_nbases >> 3) : 0u;
        im.nmask = __builtin_amdgcn_make_buffer_rsrc((void*)nmask_p, 0, (int)nmask_bytes, 0x00020000);
        return true;
    };
    auto gate = [&](uint64_t base, uint32_t len) __attribute__((always_inline)) {
        if constexpr (STAGED) {
            if (!gt.partial) return true;
            const uint64_t end = min(base + (((uint64_t)len + 255u) & ~255ull), g_nbases);
            const uint32_t r0 = gt.codes_off + (uint32_t)(base >> 2);
            const uint32_t r1 = gt.codes_off + (uint32_t)(end >> 2);
            return gt.pass(r0, r1, a.gen, a.err, completed);
        } else {
            (void)base;
            (void)len;
            return true;
        }
    };
    uint64_t nbase = 0;
    uint32_t nlen = 0;
    Fetch nf = {0u, 0u};
    // this lane's code word (bits 0-5) and N-mask word (bits 8+) of a segment, in bytes
    const uint32_t lane_off = ((lane & 15u) << 2) | ((lane & 7u) << 10);
    auto fetch_next = [&](uint64_t b) __attribute__((always_inline)) { tid_fetch(nf, im, b, lane, lane_off); };
    if (item < n_items) {
        desc(w, nbase, nlen);
        // (staged: after the table barrier -- a wave waiting for its first window must not hold
        // its workgroup's other waves at the barrier)
        if (!STAGED && fetchable(nbase, nlen)) fetch_next(nbase);
    }

    // ~Eq table, built by wave 0 of the workgroup (the waves share the
    // candidates) while the first windows' loads are in flight: ~Eq_c =
    // (ph ^ H_c) | (pl ^ L_c), H_c / L_c = all ones where character c's high /
    // low code bit is set; N matches nothing.  Only wave 0 loads the k-mers
    // (every wave of a group loading them at launch start queued for up to
    // 12 us, tools/stamps.py).  The barrier waits for LDS only, not for the
    // window prefetches.
    if (wib == 0) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            uint64_t km[P];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const uint32_t c = cand[w * P + p];
                km[p] = c < sg.n_kmers ? sg.kmers[c] : 0ull;
            }
            uint32_t ph, pl;
            build_masks<P>(km, a.m, ph, pl);
            uint32_t* tw = &lds.tab.e[w * 5 * 64];
#pragma unroll
            for (int c = 0; c < 4; ++c) tw[c * 64 + lane] = ((c & 2) ? ~ph : ph) | ((c & 1) ? ~pl : pl);
            tw[4 * 64 + lane] = ~0u;
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) lds.cnt[q * 64 + lane] = 0u;
    }
    if (!STAGED) stamp(wave, 7);  // diagnostic builds: the wave's own prologue done, before the barrier
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    stamp(wave, 1);
    bool stage_ok = true;
    if (STAGED && item < n_items && fetchable(nbase, nlen)) {
        stage_ok = gate(nbase, nlen);
        if (stage_ok) fetch_next(nbase);
    }
    if (!stage_ok) item = n_items;

    // Per window, the next window's three dependent global accesses (for an
    // item's last window: claim -> descriptor -> first words; otherwise
    // descriptor -> first words) are spread over the gaps between the window's
    // first 32-base blocks, so none of them stalls the wave between windows.
    // The window loop in two copies (staged kernel; GATED a constant in each): while the segment is not known complete (`partial`), a window's fetch first goes
    // through the gate; once it is, the loop without any staging state, so none of it stays live -- in
    // SGPRs or spilled to VGPR lanes -- through the rest of the launch.  The plain kernel runs only the
    // second.
    if constexpr (STAGED) {
#define AC_GATED 1
#include "wm_window_loop.inc"
#undef AC_GATED
    }
#define AC_GATED 0
#include "wm_window_loop.inc"
#undef AC_GATED

    stamp(wave, 2);
    stamp_val(wave, 6, ((uint64_t)si << 32) | ((uint64_t)g << 16) | j);
#ifdef AC_STAMPS
    if (STAGED) {  // (staged diagnostic builds: slots 4 / 5 hold the gate's time and calls, not the HW ids)
        stamp_val(wave, 4, gt.ticks);
        stamp_val(wave, 5, gt.calls);
    }
#endif
    // The workgroup's waves sum their counts in LDS, from where count_hand_off takes them.
#pragma unroll
    for (int q = 0; q < Q; ++q)
        if (P <= 2) cnt[q] = 3u * n_counted - cnt[q];
#pragma unroll
    for (int q = 0; q < Q; ++q)
        if (cnt[q]) __hip_atomic_fetch_add(&lds.cnt[q * 64 + lane], cnt[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    count_hand_off<Q, STAGED>(a, sg, deal, g, wib, lane, lds.cnt);
    stamp(wave, 3);
}

#include "bs_count.inc"

}  // namespace

// The bit-sliced kernel (bs_count.inc): k = K, equal windows, counting over three rows, at its family's
// residency (K = 16: four waves per SIMD, <= 128 VGPRs; wider patterns fewer), capped by the LDS allocation
// like the two-word kernel below.
template <int K, bool STAGED>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, bs_waves_per_simd(BsFamily{STAGED, BsOut::Count, 3}, K)) void bs_count_kernel(LaunchArgs a) {
    __shared__ BsLds<K> lds[(160 * 1024 / bs_blocks_per_cu(BsFamily{STAGED, BsOut::Count, 3}, K)) / sizeof(BsLds<K>)];
    bs_body<K, STAGED>(a, lds[0]);
}

template <int P, bool STAGED, bool EQ>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, waves_per_simd(words_for(P, STAGED))) void wm2_count_kernel(LaunchArgs a) {
    // The LDS allocation also caps residency at waves_per_simd waves per SIMD
    // (one word: 8, faster than 6 or 10, profiles/r01_kernel_log.md; two words: 4).
    constexpr int W = words_for(P, STAGED);
    constexpr int kBlocksPerCu = 4 * waves_per_simd(W) / WAVES_PER_BLOCK;
    __shared__ BlockLds<W> lds[(160 * 1024 / kBlocksPerCu) / sizeof(BlockLds<W>)];
    count_body<P, STAGED, EQ>(a, lds[0]);
}

namespace {
// The kernel that counts a launch; nullptr if there is none.  Bit-sliced, of family f for k (AC_BS_K_LIST):
// counting over three rows is this unit's, every other family has a unit and a picker of its own.
CountKernel bs_kernel(uint32_t k, BsFamily f) {
    switch (f.out) {
        case BsOut::Pos: return f.staged ? bsps_kernel(k, f) : bsp_kernel(k, f);
        case BsOut::Hits: return f.staged ? bshs_kernel(k, f) : bsh_kernel(k, f);
        case BsOut::Count: break;
    }
    if (f.rows == 4) return bs3_kernel(k, f);
#define AC_BS_PICK(KK) \
    if (k == KK) return f.staged ? bs_count_kernel<KK, true> : bs_count_kernel<KK, false>;
    AC_BS_K_LIST(AC_BS_PICK)
#undef AC_BS_PICK
    return nullptr;
}
// Word-parallel, for pattern pack P.
CountKernel wm_kernel(uint32_t P, bool staged, bool eq) {
#define AC_PICK(PP)                                                                                      \
    case PP:                                                                                             \
        return staged ? (eq ? wm2_count_kernel<PP, true, true> : wm2_count_kernel<PP, true, false>)      \
                      : (eq ? wm2_count_kernel<PP, false, true> : wm2_count_kernel<PP, false, false>);
    switch (P) {
        AC_PICK(1)
        AC_PICK(2)
        AC_PICK(3)
        AC_PICK(4)
        default: return nullptr;
    }
#undef AC_PICK
}

// Waves of `kernel` that fit on the device at once.
hipError_t occupancy(CountKernel kernel, int cu_count, uint32_t* waves) {
    if (!kernel) return hipErrorInvalidValue;
    int blocks = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, 64 * WAVES_PER_BLOCK, 0);
    if (e != hipSuccess) return e;
    if (blocks < 1) blocks = 1;
    *waves = (uint32_t)blocks * WAVES_PER_BLOCK * (uint32_t)cu_count;
    return hipSuccess;
}
}  // namespace

#ifdef AC_STAMPS
hipError_t debug_stamps(void* host, size_t bytes) {
    // g_stamps, then g_stage_stamps
    const size_t a = bytes < sizeof(g_stamps) ? bytes : sizeof(g_stamps);
    hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), a, 0, hipMemcpyDeviceToHost);
    if (e != hipSuccess || bytes < sizeof(g_stamps) + sizeof(g_stage_stamps)) return e;
    e = hipMemcpyFromSymbol((char*)host + sizeof(g_stamps), HIP_SYMBOL(g_stage_stamps), sizeof(g_stage_stamps), 0,
                            hipMemcpyDeviceToHost);
    // then the per-window stamps (g_win_stamps), if the buffer holds them
    if (e != hipSuccess || bytes < sizeof(g_stamps) + sizeof(g_stage_stamps) + sizeof(g_win_stamps)) return e;
    return hipMemcpyFromSymbol((char*)host + sizeof(g_stamps) + sizeof(g_stage_stamps), HIP_SYMBOL(g_win_stamps),
                               sizeof(g_win_stamps), 0, hipMemcpyDeviceToHost);
}
#endif

hipError_t resident_waves(uint32_t P, bool staged, int cu_count, uint32_t* waves) {
    // (queried on the equal-window kernel, the one the bench's kernel leg, the CLI and the stage launch:
    // the query loads the kernel's code, and that load then is not paid again at its first launch --
    // the instantiations of one word count have the same LDS allocation, so the same residency)
    return occupancy(wm_kernel(P, staged, true), cu_count, waves);
}

hipError_t resident_waves_bs(BsFamily f, uint32_t k, int cu_count, uint32_t* waves) {
    return occupancy(bs_kernel(k, f), cu_count, waves);
}

hipError_t launch_wm2_count(const LaunchArgs& args, hipStream_t stream) {
    if (args.total_waves == 0) return hipSuccess;
    const uint64_t blocks = (args.total_waves + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    const dim3 grid((uint32_t)blocks), block(64 * WAVES_PER_BLOCK);
    // (the bit-sliced kernel: the host routes only equal-window launches of a listed k to it)
    if (args.bs && !(args.eq && args.m)) return hipErrorInvalidValue;
    // (and only bit-sliced launches at another edit budget than 2)
    if (args.max_errors > 3u || (args.max_errors != 2u && !args.bs)) return hipErrorInvalidValue;
    // (hits: bit-sliced launches only -- there is no other kernel that writes them)
    if (args.want_hits && !args.bs) return hipErrorInvalidValue;
    if (args.want_pos && !args.want_hits) return hipErrorInvalidValue;
    const CountKernel kernel =
        args.bs ? bs_kernel(args.m, bs_family(args.staged != 0u, args.want_hits != 0u, args.want_pos != 0u, args.max_errors))
                : wm_kernel(args.P, args.staged != 0u, args.eq != 0u);
    if (!kernel) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, args);
    return hipGetLastError();
}

}  // namespace acamd
