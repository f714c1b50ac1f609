// hit_span.h -- match spans (DESIGN.md §4e "Match spans"): where each candidate's best occurrence STARTS,
// from the hit levels and the end positions a launch has already written.  Plain C++ that compiles for the
// device (hit_span.hip's kernel) and for the host (tools/hit_span_check.cpp, tests/test_spans_cpu.py), so
// the code the kernel runs is the code the CPU test checks against a plain DP.
//
// The contract.  w is a window of L bases, c a k-mer, E the budget, d = d(c, w) <= E, pos = pos(c, w) the
// exclusive end of the leftmost occurrence at distance d (bs_pos.h), ed the plain global edit distance, an
// N of the window matching nothing:
//     start(c, w) = max { s : ed(c, w[s, pos)) = d }        0 <= start <= pos - (k - d)
//     len(c, w)   = pos - start                             k - d <= len <= k + d
// the SHORTEST substring ending at pos at the best distance -- the left edge prefers the shorter occurrence
// as the end rule does at the right edge: a first base substituted in the text is left out of the span, not
// covered as a mismatch.  Such an s exists, because e(pos) = d says exactly that.
// A start matrix has the layout of a position matrix: eight bit planes of the hit matrix's shape,
//     start_m[(b * n_windows + w) * words + c / 32], bit c % 32 = bit b of start(c, w)   (stored as it is)
// 0 in every plane where d > E, for candidates >= n_kmers and in skipped windows; every word is written.
//
// The step.  With j = pos - s the rule asks for the least j in k - d .. min(pos, k + d) with
// ed(reversed k-mer, reversed w[pos - j, pos)) = d: a GLOBAL alignment of the reversed k-mer against the
// prefixes of the reversed text before pos.  One Myers column per text base in one 32-bit word (k <= 32):
// bit i of the vertical deltas Pv / Mv is row i + 1 of the reversed k-mer, the horizontal delta shifted into
// row 0 is +1 (the top row of a global alignment is 0, 1, 2, ..), and the bottom cell's value is carried
// as a score that starts at k.  The first column whose score is d is the answer; a column j < k - d
// cannot be (its score is at least k - j).  Bits above k never reach the bits below (carries and shifts only
// move up), so no mask is needed.  The text is fetched once, before the columns (up to seven loads, all in
// flight together): a load inside the loop would be issued at every column of a wave, whose lanes cross their
// word seams at different columns.  About 30 integer operations a column -- 17 of the recurrence, the rest
// taking the base and its N bit off two shift registers and building its match mask -- over at most
// k + d <= 35 columns, after about 60 to split the k-mer's code bits and align the text: at most some 1100 a
// pair.
#pragma once
#include <stdint.h>

#include "bs_pos.h"

namespace acamd {
namespace bs {

constexpr uint32_t SP_NONE = 0u;  // sp_span: no occurrence length qualifies (a length is >= 1)

// The even bits of v (bits 0, 2, .., 62) packed into 32.
AC_BS_FN uint32_t sp_even_bits(uint64_t v) {
    v &= 0x5555555555555555ull;
    v = (v | v >> 1) & 0x3333333333333333ull;
    v = (v | v >> 2) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | v >> 4) & 0x00FF00FF00FF00FFull;
    v = (v | v >> 8) & 0x0000FFFF0000FFFFull;
    v = (v | v >> 16) & 0x00000000FFFFFFFFull;
    return (uint32_t)v;
}

// The top 32 bits of hi : lo shifted left by sh (0..31): a funnel shift, one instruction on the device.
AC_BS_FN uint32_t sp_fshl(uint32_t hi, uint32_t lo, uint32_t sh) {
    return (uint32_t)((((uint64_t)hi << 32 | lo) << sh) >> 32);
}

// The occurrence's length pos - start, or SP_NONE.  `kmer`: 2 bits a base, the first base highest (base i of
// the reversed k-mer is bits 2 i, 2 i + 1).  `codes` / `nmask`: the image's 2-bit and N-bitmap words; the
// window's bases are base0 .. base0 + L - 1 of it (base0 a multiple of 32) and nothing outside them is read.
// Safe on any pos and d: SP_NONE when pos is 0 or past L, when d >= k, or when no length qualifies.
AC_BS_FN uint32_t sp_span(uint64_t kmer, uint32_t k, const uint32_t* codes, const uint32_t* nmask, uint64_t base0,
                          uint32_t L, uint32_t pos, uint32_t d) {
    if (pos < 1u || pos > L || d >= k || k > 32u) return SP_NONE;
    const uint32_t lo = sp_even_bits(kmer), hi = sp_even_bits(kmer >> 1);
    const uint32_t valid = k >= 32u ? ~0u : (1u << k) - 1u;
    // (lo, hi: bit i = the low / high code bit of the reversed k-mer's base i)
    const uint32_t top = 1u << (k - 1u);
    const uint32_t steps = pos < k + d ? pos : k + d;
    // The text, fetched once: the columns read the bases last, last - 1, .. (at most 35 of them), which lie in
    // at most four code words and three bitmap words ending at last's.  Words below the window's first one hold
    // no base a column reads (steps <= pos) and are not loaded.  Both runs are then shifted so that base `last`
    // sits at the top of the highest word, and every column takes the top and shifts on.
    const uint64_t last = base0 + pos - 1u;
    const uint64_t cw = last >> 4, cw_min = base0 >> 4, nw = last >> 5, nw_min = base0 >> 5;
    const uint32_t c2 = codes[cw];
    const uint32_t c1 = cw >= cw_min + 1u ? codes[cw - 1u] : 0u;
    const uint32_t c0 = cw >= cw_min + 2u ? codes[cw - 2u] : 0u;
    const uint32_t cx = cw >= cw_min + 3u ? codes[cw - 3u] : 0u;
    const uint32_t n1 = nmask[nw];
    const uint32_t n0 = nw >= nw_min + 1u ? nmask[nw - 1u] : 0u;
    const uint32_t nx = nw >= nw_min + 2u ? nmask[nw - 2u] : 0u;
    const uint32_t csh = 2u * (15u - (uint32_t)(last & 15u)), nsh = 31u - (uint32_t)(last & 31u);
    // two 64-bit shift registers: 32 bases of codes (refilled once, for the columns past 32: k + d > 32 only)
    // and 64 N bits, of which at most 35 are taken
    uint64_t ct = (uint64_t)sp_fshl(c2, c1, csh) << 32 | sp_fshl(c1, c0, csh);
    const uint64_t ct_more = (uint64_t)sp_fshl(c0, cx, csh) << 32;
    uint64_t nt = (uint64_t)sp_fshl(n1, n0, nsh) << 32 | sp_fshl(n0, nx, nsh);
    uint32_t pv = ~0u, mv = 0u, score = k;
    for (uint32_t j = 1u; j <= steps; ++j) {
        if (j == 33u) ct = ct_more;
        const uint32_t code = (uint32_t)(ct >> 62), is_n = (uint32_t)(nt >> 63);
        ct <<= 2;
        nt <<= 1;
        // the reversed k-mer's bases that match this one: both code bits agree, and it is no N
        const uint32_t same = ((code & 1u) ? lo : ~lo) & ((code & 2u) ? hi : ~hi) & valid;
        const uint32_t eq = is_n ? 0u : same;
        const uint32_t xv = eq | mv;
        const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
        uint32_t ph = mv | ~(xh | pv);
        uint32_t mh = pv & xh;
        score += (ph & top) ? 1u : 0u;
        score -= (mh & top) ? 1u : 0u;
        ph = ph << 1 | 1u;
        mh <<= 1;
        pv = mh | ~(xv | ph);
        mv = ph & xv;
        if (score == d) return j;
    }
    return SP_NONE;
}

// The walk of one hit word: word column `col` of window w of a hit matrix (`levels` planes of n_windows x
// words) and its position matrix (POS_PLANES planes of that shape).  sp_word_mask: the bits to walk -- the
// TOP level plane's, candidates c = 32 col + j < n_kmers only; bits of lower planes without the top one are
// not walked (planes that do not nest give nothing there).  sp_word: every bit j of that mask `m` calls
// add(j, pos, d), pos = the pair's stored position + 1, d = the first level plane that holds its bit; the
// other planes are read only where a bit exists.
AC_BS_FN uint32_t sp_word_mask(const uint32_t* hits, uint32_t n_kmers, uint64_t n_windows, uint32_t levels, uint64_t w,
                               uint32_t col) {
    const uint64_t words = ((uint64_t)n_kmers + 31u) >> 5;
    const uint32_t left = n_kmers - 32u * col;
    const uint32_t keep = left >= 32u ? ~0u : (1u << left) - 1u;
    return hits[((uint64_t)(levels - 1u) * n_windows + w) * words + col] & keep;
}
template <class F>
AC_BS_FN void sp_word(const uint32_t* hits, const uint32_t* pos, uint32_t n_kmers, uint64_t n_windows, uint32_t levels,
                      uint64_t w, uint32_t col, uint32_t m, F&& add) {
    if (!m) return;
    const uint64_t words = ((uint64_t)n_kmers + 31u) >> 5;
    const uint64_t plane = n_windows * words, at = w * words + col;
    uint32_t p[POS_PLANES];
    AC_BS_UNROLL
    for (int b = 0; b < POS_PLANES; ++b) p[b] = pos[(uint64_t)b * plane + at];
    uint32_t lv[3] = {0u, 0u, 0u};  // the planes below the top one
    for (uint32_t e = 0; e + 1u < levels && e < 3u; ++e) lv[e] = hits[(uint64_t)e * plane + at];
    for (; m; m &= m - 1u) {
        const uint32_t j = (uint32_t)__builtin_ctz(m);
        uint32_t d = levels - 1u;
        for (uint32_t e = levels - 1u; e-- > 0u;)
            if (e < 3u && (lv[e] >> j & 1u)) d = e;
        add(j, pos_get(p, j) + 1u, d);
    }
}

// The start's plane bits for candidate bit j: or_word(b, bit) for every plane b that holds one.
template <class F>
AC_BS_FN void sp_put(uint32_t start, uint32_t j, F&& or_word) {
    AC_BS_UNROLL
    for (uint32_t b = 0; b < (uint32_t)POS_PLANES; ++b)
        if (start >> b & 1u) or_word(b, 1u << j);
}

}  // namespace bs
}  // namespace acamd
