// hit_flank.h -- flank profiles (DESIGN.md §4e "Flank profiles"): per k-mer, a histogram of the D bases after
// the end and of the D bases before the start of its best occurrence, over the windows of one hit plane.
// Plain C++ that compiles for the device (hit_flank.hip's kernel) and for the host
// (tools/hit_flank_check.cpp, tests/test_flanks_cpu.py), so the code the kernel runs is the code the CPU test
// checks against the definition in numpy.
//
// The contract.  w is a window of L bases (1..256, at ceil32(L)-base strides of the image), c a k-mer, H a hit
// plane (n_windows x words words: one level plane of a hit matrix), pos(c, w) the exclusive end from the
// position matrix (bs_pos.h: the planes store pos - 1), start(c, w) the inclusive start from the start matrix
// (hit_span.h: stored as it is).  Symbols are A, C, G, T = 0..3 and N = 4, D = 1..32:
//     right[c][j][s] = #{ w : H(w, c), q = pos(c, w) + j       <  L, sym(w[q]) = s }     j = 0..D-1
//     left [c][j][s] = #{ w : H(w, c), q = start(c, w) - 1 - j >= 0, sym(w[q]) = s }
//     flank[((side * n_kmers + c) * D + j) * 5 + s]      side 0 = right, 1 = left
// A base outside [0, L) is not counted and slot padding is never read.  The planes may hold anything: a pair
// with pos past L or start >= pos counts on neither side (the stored pos - 1 decodes to pos >= 1), and bits of
// candidates >= n_kmers are dropped.  Without a start matrix only the right side is counted.
#pragma once
#include <stdint.h>

#include "bs_pos.h"

namespace acamd {
namespace bs {

constexpr uint32_t FL_MAX_DEPTH = 32u;
constexpr uint32_t FL_SYMS = 5u;  // A C G T N

// The words of a result: 2 sides x n_kmers x depth x 5.
AC_BS_FN uint64_t fl_words(uint32_t n_kmers, uint32_t depth) { return 2ull * n_kmers * depth * FL_SYMS; }

// Base q of the window whose first base is base `base` of the image (codes: 2 bits a base, nmask: the N
// bitmap): 0..3, or 4 where the N bit is set.
AC_BS_FN uint32_t fl_sym(const uint32_t* codes, const uint32_t* nmask, uint64_t base, uint32_t q) {
    const uint64_t g = base + q;
    if (nmask[g >> 5] >> (uint32_t)(g & 31u) & 1u) return 4u;
    return codes[g >> 4] >> (2u * (uint32_t)(g & 15u)) & 3u;
}

// The walk of one hit word: word column `col` of window w of the plane `hit` and of the position and start
// matrices (POS_PLANES planes of the plane's shape each; start may be NULL).  fl_word_mask: the bits to walk,
// candidates c = 32 col + j < n_kmers only.  fl_word: every bit j of that mask `m` calls add(j, pos, start),
// pos = the stored position + 1, start = the stored start (0 without a start matrix); the sixteen planes are
// read only where a bit exists.
AC_BS_FN uint32_t fl_word_mask(const uint32_t* hit, uint32_t n_kmers, uint64_t w, uint32_t col) {
    const uint64_t words = ((uint64_t)n_kmers + 31u) >> 5;
    const uint32_t left = n_kmers - 32u * col;
    const uint32_t keep = left >= 32u ? ~0u : (1u << left) - 1u;
    return hit[w * words + col] & keep;
}
template <class F>
AC_BS_FN void fl_word(const uint32_t* pos, const uint32_t* start, uint32_t n_kmers, uint64_t n_windows, uint64_t w,
                      uint32_t col, uint32_t m, F&& add) {
    if (!m) return;
    const uint64_t words = ((uint64_t)n_kmers + 31u) >> 5;
    const uint64_t plane = n_windows * words, at = w * words + col;
    uint32_t p[POS_PLANES], s[POS_PLANES];
    AC_BS_UNROLL
    for (int b = 0; b < POS_PLANES; ++b) {
        p[b] = pos[(uint64_t)b * plane + at];
        s[b] = start ? start[(uint64_t)b * plane + at] : 0u;
    }
    for (; m; m &= m - 1u) {
        const uint32_t j = (uint32_t)__builtin_ctz(m);
        add(j, pos_get(p, j) + 1u, pos_get(s, j));
    }
}

// The run of n bases q0 .. q0 + n - 1 of that window (1 <= n <= 32, all of them inside the window): base
// q0 + i's code in bits 2 i, 2 i + 1 of *code, its N bit in bit i of *isn.  The text of one side of a pair,
// fetched once: at most three code words and two bitmap words, the words that hold those bases and no other
// (a load per base would be two a column).
AC_BS_FN void fl_run(const uint32_t* codes, const uint32_t* nmask, uint64_t base, uint32_t q0, uint32_t n, uint64_t* code,
                     uint32_t* isn) {
    const uint64_t g = base + q0, last = g + n - 1u;
    const uint64_t cw = g >> 4, cl = last >> 4, nw = g >> 5, nl = last >> 5;
    const uint32_t csh = 2u * (uint32_t)(g & 15u), nsh = (uint32_t)(g & 31u);
    const uint32_t c0 = codes[cw], c1 = cl > cw ? codes[cw + 1u] : 0u, c2 = cl > cw + 1u ? codes[cw + 2u] : 0u;
    const uint64_t lo = (uint64_t)c1 << 32 | c0;
    *code = csh ? lo >> csh | (uint64_t)c2 << (64u - csh) : lo;
    const uint32_t n0 = nmask[nw], n1 = nl > nw ? nmask[nw + 1u] : 0u;
    *isn = (uint32_t)(((uint64_t)n1 << 32 | n0) >> nsh);
}
// Base i of a run: fl_sym's value.
AC_BS_FN uint32_t fl_run_sym(uint64_t code, uint32_t isn, uint32_t i) {
    return (isn >> i & 1u) ? 4u : (uint32_t)(code >> (2u * i)) & 3u;
}

// One pair: count(side, j, s) for every base it counts -- the bases pos .. pos + D - 1 below L on the right
// and, with a start matrix, start - 1 .. start - D down to 0 on the left.  Safe on any pos and start: nothing
// where pos is past L or start >= pos, and no base outside the window is read.
template <class F>
AC_BS_FN void fl_pair(const uint32_t* codes, const uint32_t* nmask, uint64_t base0, uint32_t L, uint32_t depth,
                      uint32_t pos, uint32_t start, bool with_start, F&& count) {
    if (pos < 1u || pos > L || (with_start && start >= pos)) return;
    uint64_t code;
    uint32_t isn;
    const uint32_t nr = L - pos < depth ? L - pos : depth;
    if (nr) {
        fl_run(codes, nmask, base0, pos, nr, &code, &isn);
        for (uint32_t j = 0; j < nr; ++j) count(0u, j, fl_run_sym(code, isn, j));
    }
    const uint32_t nl = !with_start ? 0u : start < depth ? start : depth;
    if (nl) {
        fl_run(codes, nmask, base0, start - nl, nl, &code, &isn);  // (column j is base start - 1 - j: the run's nl - 1 - j)
        for (uint32_t j = 0; j < nl; ++j) count(1u, j, fl_run_sym(code, isn, nl - 1u - j));
    }
}

}  // namespace bs
}  // namespace acamd
