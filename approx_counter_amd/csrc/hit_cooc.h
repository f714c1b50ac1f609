// hit_cooc.h -- the co-occurrence of a hit matrix's candidates (DESIGN.md §4e "Co-occurrence"): how many
// windows of one level plane hold candidates a and b both, a bit-matrix Gram product, and the other
// marginal, how many candidates a window holds.  Plain C++ that compiles for the device (hit_cooc.hip's
// kernels) and for the host (tools/hit_cooc_check.cpp, tests/test_cooc_cpu.py), so the code the kernels
// run is the code the CPU test checks: the masks, the 32 x 32 bit transposition, the tile's inner
// product, the tile-pair numbering and the launch rule.
//
// A level plane is n_windows rows of `words` u32, bit j of word x = candidate 32 x + j.  The product runs
// over its transpose T: one bit row per candidate, rows = 32 words of them, each co_t_words(n_windows) u32,
// bit w % 32 of word w / 32 = window w; rows of candidates >= n_kmers and bits of windows >= n_windows are
// 0, so the product needs no masks.  A row is padded to whole slabs of CO_SLAB words, the unit the product
// streams through LDS (and splits the window axis by).
#pragma once
#include <stdint.h>

#include "bs_nfa.h"

namespace acamd {
namespace bs {

constexpr uint32_t CO_TILE = 64u;   // candidates of a product tile: 16 x 16 threads of CO_ACC x CO_ACC sums
constexpr int CO_ACC = 4;
constexpr uint32_t CO_SLAB = 32u;   // window words of T a product workgroup holds in LDS at a time (1024 windows)
// The product kernel's waves per SIMD (__launch_bounds__; tests/test_cooc_kernel_asm.py holds the compiler's
// occupancy to it): workgroups of four waves, so also its resident workgroups per CU.
constexpr int CO_WAVES_PER_SIMD = 4;
// The launch rule (co_splits) cuts the window axis until a launch has this many workgroups: CO_ROUNDS rounds
// of the workgroups resident on 256 CUs, so that the idle tail of the last round stays below 1 / CO_ROUNDS.
constexpr uint32_t CO_ROUNDS = 4u;
constexpr uint32_t CO_BLOCKS = CO_ROUNDS * 256u * (uint32_t)CO_WAVES_PER_SIMD;
constexpr uint32_t CO_MIN_SLABS = 2u;  // slabs a workgroup of a split launch gets at least (its atomics' worth)
// The transposition's tile: CO_TC word columns x CO_TB blocks of 32 windows, one 32 x 32 block per thread.
constexpr uint32_t CO_TC = 16u, CO_TB = 16u;

// The bits of word column `col` that are candidates < n_kmers (col < ceil(n_kmers / 32)).
AC_BS_FN uint32_t co_col_mask(uint32_t col, uint32_t n_kmers) {
    const uint32_t left = n_kmers - 32u * col;
    return left >= 32u ? ~0u : (1u << left) - 1u;
}

// u32 words of one bit row of T, and T's rows.
AC_BS_FN uint64_t co_t_words(uint64_t n_windows) { return (n_windows + 32u * CO_SLAB - 1u) / (32u * CO_SLAB) * CO_SLAB; }
AC_BS_FN uint64_t co_t_rows(uint64_t n_kmers) { return (n_kmers + 31u) / 32u * 32u; }

// What the transposition reads for window w and word column col: the word without its stray bits, 0
// outside the plane.
AC_BS_FN uint32_t co_load_word(const uint32_t* plane, uint64_t words, uint32_t n_kmers, uint64_t n_windows, uint64_t w,
                               uint64_t col) {
    return w < n_windows && col < words ? plane[w * words + col] & co_col_mask((uint32_t)col, n_kmers) : 0u;
}

// A 32 x 32 bit block in place: bit i of a[j] becomes bit j of a[i].  In: a[i] = window i's word of one
// column; out: a[j] = the 32 windows' bits of candidate j.  Five rounds of masked swaps between the words
// k and k + s (s = 16 .. 1), all indices known at compile time.
AC_BS_FN void co_transpose32(uint32_t (&a)[32]) {
    AC_BS_UNROLL
    for (int r = 4; r >= 0; --r) {
        const int s = 1 << r;
        const uint32_t m = 0xFFFFFFFFu / ((1u << s) + 1u);  // the low s bits of every 2 s
        AC_BS_UNROLL
        for (int k = 0; k < 32; ++k)
            if (!(k & s)) {
                const uint32_t t = ((a[k] >> s) ^ a[k + s]) & m;
                a[k + s] ^= t;
                a[k] ^= t << s;
            }
    }
}

// One window word of a tile's inner product: acc[i][j] += the windows of this word that hold a[i] and b[j].
AC_BS_FN void co_dot(uint32_t (&acc)[CO_ACC][CO_ACC], const uint32_t (&a)[CO_ACC], const uint32_t (&b)[CO_ACC]) {
    AC_BS_UNROLL
    for (int i = 0; i < CO_ACC; ++i) {
        AC_BS_UNROLL
        for (int j = 0; j < CO_ACC; ++j) acc[i][j] += (uint32_t)__builtin_popcount(a[i] & b[j]);
    }
}

// Tile pairs of the upper triangle, numbered p = tb (tb + 1) / 2 + ta, ta <= tb.
AC_BS_FN uint64_t co_pairs(uint64_t tiles) { return tiles * (tiles + 1u) / 2u; }
AC_BS_FN void co_pair(uint32_t p, uint32_t& ta, uint32_t& tb) {
    uint64_t t = (uint64_t)((__builtin_sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
    while (t * (t + 1u) / 2u > p) --t;
    while ((t + 1u) * (t + 2u) / 2u <= p) ++t;
    tb = (uint32_t)t;
    ta = p - (uint32_t)(t * (t + 1u) / 2u);
}

// The launch rule of the product.  A workgroup takes one tile pair of one plane over `per` consecutive slabs;
// `splits` workgroups share a pair.  splits == 1: every word of the output is stored once.  splits > 1: the
// output is zeroed on the stream first and the workgroups add into it.  The window axis is cut only while
// the launch has fewer than CO_BLOCKS workgroups, and never below CO_MIN_SLABS slabs a workgroup.
struct CoSplit {
    uint32_t splits, per;
};
AC_BS_FN CoSplit co_splits(uint64_t n_kmers, uint64_t n_windows, uint32_t levels) {
    const uint64_t slabs = co_t_words(n_windows) / CO_SLAB;
    const uint64_t work = co_pairs((n_kmers + CO_TILE - 1u) / CO_TILE) * levels;
    CoSplit r = {1u, (uint32_t)(slabs ? slabs : 1u)};
    if (!work || work >= CO_BLOCKS || slabs < 2u) return r;
    const uint64_t want = (CO_BLOCKS + work - 1u) / work;
    uint64_t per = (slabs + want - 1u) / want;
    if (per < CO_MIN_SLABS) per = CO_MIN_SLABS;
    r.per = (uint32_t)per;
    r.splits = (uint32_t)((slabs + per - 1u) / per);
    return r;
}

// The window counts' share of one word: its candidates < n_kmers.
AC_BS_FN uint32_t co_word_count(uint32_t x, uint32_t col, uint32_t n_kmers) {
    return (uint32_t)__builtin_popcount(x & co_col_mask(col, n_kmers));
}

}  // namespace bs
}  // namespace acamd
