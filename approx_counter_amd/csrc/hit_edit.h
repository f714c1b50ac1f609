// hit_edit.h -- edit profiles (DESIGN.md §4e "Edit profiles"): per k-mer and per base of it, how the best
// occurrence differs from the k-mer -- matched, substituted by which base, missing from the read, or followed
// by which inserted base -- over the windows of one hit plane.  Plain C++ that compiles for the device
// (hit_edit.hip's kernel) and for the host (tools/hit_edit_check.cpp, tests/test_edits_cpu.py), so the code
// the kernel runs is the code the CPU test checks against a plain full-table DP.
//
// The contract.  w is a window of L bases (1..256, at ceil32(L)-base strides of the image), c a k-mer of k
// bases (2..32), H a hit plane (n_windows x words words: one level plane of a hit matrix), p = pos(c, w) the
// exclusive end from the position matrix (bs_pos.h: the planes store pos - 1), s = start(c, w) the inclusive
// start from the start matrix (hit_span.h), t = w[s, p), m = p - s; an N of the window matches nothing;
// D[i][j] the plain global edit-distance table of c[0, i) against t[0, j), D[i][0] = i, D[0][j] = j.
// A pair counts only if H(w, c), 1 <= p <= L, s < p, |m - k| <= 3 and D[k][m] <= 3 (3: the largest edit budget
// of the ABI, a constant of the pass).  Its alignment is the canonical traceback from (k, m) to (0, 0); at
// cell (i, j) the first rule that applies:
//   1. diagonal   i > 0, j > 0 and D[i-1][j-1] + (c[i-1] != t[j-1]) = D[i][j]: k-mer base i-1 is matched, or
//                 substituted by t[j-1] (A C G T N); i--, j--
//   2. deletion   i > 0 and D[i-1][j] + 1 = D[i][j]: k-mer base i-1 is deleted (missing from the read); i--
//   3. insertion  otherwise: t[j-1] is inserted after k-mer base i-1 (at i = 0 nothing is counted); j--
//     edit[(c * k + i) * 12 + op]     op 0 match, 1..5 substituted by A C G T N, 6 deleted,
//                                     7..11 inserted after: A C G T N
// The planes may hold anything: a pair that fails a condition counts nowhere, nothing outside [0, L) of the
// window is read, and bits of candidates >= n_kmers are dropped.
//
// The step.  Every cell on a path of cost <= 3 lies within 3 of the main diagonal, so the table is never
// built: the forward pass is the furthest-reaching one over the 7 diagonals j - i = -3..3 and the costs 0..3,
//     R[e][g] = the last row i with D[i][i + g] <= e
// (D does not decrease along a diagonal), R[e][g] = the farthest of R[e-1][g] + 1 (substitution), R[e-1][g+1] + 1
// (deletion) and R[e-1][g-1] (insertion), cut to the diagonal's last cell and run on over the matches that
// follow -- one count-trailing-zeros of the diagonal's mismatch mask (bit i: c[i] differs from t[i + g], or one
// of them does not exist).  D[k][m] is the least e with R[e][m - k] = k.  The traceback needs no table either:
// where the bases match, D[i][j] = D[i-1][j-1], so the diagonal rule holds over a whole run of matches, found
// with one count-leading-zeros; at a mismatch (or in column 0) with D[i][j] = v the diagonal rule holds iff
// D[i-1][j-1] <= v - 1 iff R[v-1][g] >= i - 1, the deletion rule iff R[v-1][g+1] >= i - 1, else it is an
// insertion: d + 1 steps, not k + m.  R's rows for e = 0..2 are packed 6 bits a diagonal in one 64-bit word
// each, so that the traceback indexes diagonals by shifts and costs by selects; the 7 masks are selected.  No
// array is indexed dynamically (no scratch on the device).  A match is not reported: every counted pair gives
// every base exactly one of the operations 0..6, so the caller counts the pair once and derives
// match = pairs - (operations 1..6).  The text (at most 35 bases: at most four code words and three bitmap
// words) is fetched once.  About 100 integer operations for the text, 100 for the masks, 300 for R and 40 a
// traceback step.
#pragma once
#include <stdint.h>

#include "hit_flank.h"
#include "hit_span.h"

namespace acamd {
namespace bs {

constexpr uint32_t EP_OPS = 12u;     // match, 5 substitutions, deletion, 5 insertions
constexpr uint32_t EP_BAND = 3u;     // the diagonals kept on either side of the main one; the cost bound
constexpr uint32_t EP_DIAGS = 2u * EP_BAND + 1u;
constexpr uint32_t EP_SAT = EP_BAND + 1u;
constexpr uint32_t EP_MIN_K = 2u, EP_MAX_K = 32u;
constexpr uint32_t EP_MATCH = 0u, EP_SUB = 1u, EP_DEL = 6u, EP_INS = 7u;

// The words of a result: n_kmers x k x 12.
AC_BS_FN uint64_t ep_words(uint32_t n_kmers, uint32_t k) { return (uint64_t)n_kmers * k * EP_OPS; }

// The text of a pair, fetched once: the m bases (1..35) from base g of the image, as bit planes -- bit j of
// lo / hi the low / high code bit of base j, bit j of isn its N bit; bits m and above are 0 in isn and
// undefined in lo / hi.  Reads the words that hold those bases and no other.
AC_BS_FN void ep_text(const uint32_t* codes, const uint32_t* nmask, uint64_t g, uint32_t m, uint64_t* lo, uint64_t* hi,
                      uint64_t* isn) {
    const uint64_t last = g + m - 1u;
    const uint64_t cw = g >> 4, cl = last >> 4, nw = g >> 5, nl = last >> 5;
    const uint32_t csh = 2u * (uint32_t)(g & 15u), nsh = (uint32_t)(g & 31u);
    const uint32_t c0 = codes[cw], c1 = cl > cw ? codes[cw + 1u] : 0u, c2 = cl > cw + 1u ? codes[cw + 2u] : 0u,
                   c3 = cl > cw + 2u ? codes[cw + 3u] : 0u;
    const uint64_t w01 = (uint64_t)c1 << 32 | c0, w23 = (uint64_t)c3 << 32 | c2;
    const uint64_t first = csh ? w01 >> csh | w23 << (64u - csh) : w01;  // bases 0..31
    const uint64_t more = w23 >> csh;                                    // bases 32.. (three of them at most)
    *lo = (uint64_t)sp_even_bits(more) << 32 | sp_even_bits(first);
    *hi = (uint64_t)sp_even_bits(more >> 1) << 32 | sp_even_bits(first >> 1);
    const uint32_t n0 = nmask[nw], n1 = nl > nw ? nmask[nw + 1u] : 0u, n2 = nl > nw + 1u ? nmask[nw + 2u] : 0u;
    const uint64_t n01 = (uint64_t)n1 << 32 | n0;
    *isn = (nsh ? n01 >> nsh | (uint64_t)n2 << (64u - nsh) : n01) & ((1ull << m) - 1ull);
}

// v's bits in reverse order (one instruction on the device).
AC_BS_FN uint32_t ep_rev32(uint32_t v) {
#if defined(__clang__)
    return __builtin_bitreverse32(v);
#else
    v = (v >> 1 & 0x55555555u) | (v & 0x55555555u) << 1;
    v = (v >> 2 & 0x33333333u) | (v & 0x33333333u) << 2;
    v = (v >> 4 & 0x0F0F0F0Fu) | (v & 0x0F0F0F0Fu) << 4;
    v = (v >> 8 & 0x00FF00FFu) | (v & 0x00FF00FFu) << 8;
    return v >> 16 | v << 16;
#endif
}

// Row r of diagonal g's run: r plus the matches that follow it on the mask `neq` (bit i: row i + 1's
// comparison c[i] against t[i + g] fails), at most `lim`.
AC_BS_FN int32_t ep_run(uint32_t neq, int32_t r, int32_t lim) {
    if (r >= lim) return r;  // (and r < 32)
    const uint32_t x = neq >> r;
    const int32_t to = r + (x ? (int32_t)__builtin_ctz(x) : 32 - r);
    return to < lim ? to : lim;
}

// One pair: true if it counts (see the contract), after count(i, op) for every EDIT of its alignment -- op
// 1..11 at k-mer base i; the matches are what is left: every base of a counted pair has exactly one of the
// operations 0..6.  `kmer`: 2 bits a base, the first base highest.  Safe on any pos and start: false where a
// condition fails, and no base outside the window is read.
template <class F>
AC_BS_FN bool ep_pair(uint64_t kmer, uint32_t k, const uint32_t* codes, const uint32_t* nmask, uint64_t base0, uint32_t L,
                      uint32_t pos, uint32_t start, F&& count) {
    if (k < EP_MIN_K || k > EP_MAX_K || pos < 1u || pos > L || start >= pos) return false;
    const uint32_t m = pos - start;
    if (m + EP_BAND < k || m > k + EP_BAND) return false;
    uint64_t lo, hi, isn;
    ep_text(codes, nmask, base0 + start, m, &lo, &hi, &isn);
    const uint64_t in_text = ~isn & ((1ull << m) - 1ull);  // the bases a k-mer base can match
    // the k-mer's code bits, bit i = base i (sp_even_bits: the reversed k-mer's)
    const uint32_t klo = ep_rev32(sp_even_bits(kmer)) >> (32u - k);
    const uint32_t khi = ep_rev32(sp_even_bits(kmer >> 1)) >> (32u - k);
    const uint32_t kvalid = k >= 32u ? ~0u : (1u << k) - 1u;
    // the diagonals' mismatch masks, index q = g + 3
    uint32_t neq[EP_DIAGS];
    AC_BS_UNROLL
    for (uint32_t q = 0; q < EP_DIAGS; ++q) {
        const uint32_t tl = q < EP_BAND ? (uint32_t)(lo << (EP_BAND - q)) : (uint32_t)(lo >> (q - EP_BAND));
        const uint32_t th = q < EP_BAND ? (uint32_t)(hi << (EP_BAND - q)) : (uint32_t)(hi >> (q - EP_BAND));
        const uint32_t tv = q < EP_BAND ? (uint32_t)(in_text << (EP_BAND - q)) : (uint32_t)(in_text >> (q - EP_BAND));
        neq[q] = ~(~(klo ^ tl) & ~(khi ^ th) & tv & kvalid);
    }
    // R, one cost after the other; NONE: no cell of the diagonal is within the cost
    constexpr int32_t NONE = -64;
    const int32_t ik = (int32_t)k, im = (int32_t)m;
    int32_t r[EP_DIAGS], prev[EP_DIAGS];
    uint64_t packed[EP_BAND] = {0u, 0u, 0u};  // R[e] for e = 0..2: 6 bits a diagonal, row + 1 (0: none)
    const uint32_t qe = m + EP_BAND - k;      // the diagonal of (k, m)
    uint32_t d = EP_SAT;
    AC_BS_UNROLL
    for (uint32_t e = 0; e <= EP_BAND; ++e) {
        AC_BS_UNROLL
        for (uint32_t q = 0; q < EP_DIAGS; ++q) prev[q] = e ? r[q] : NONE;
        AC_BS_UNROLL
        for (uint32_t q = 0; q < EP_DIAGS; ++q) {
            const int32_t g = (int32_t)q - (int32_t)EP_BAND, first = g < 0 ? -g : 0;
            const int32_t lim = ik < im - g ? ik : im - g;  // the diagonal's last row
            int32_t c = e ? prev[q] + 1 : (g == 0 ? 0 : NONE);
            if (e && q + 1u < EP_DIAGS && prev[q + 1u] + 1 > c) c = prev[q + 1u] + 1;
            if (e && q > 0u && prev[q - 1u] > c) c = prev[q - 1u];
            c = c < lim ? c : lim;
            r[q] = c >= first ? ep_run(neq[q], c, lim) : NONE;
            if (e < EP_BAND) packed[e] |= (uint64_t)(r[q] >= 0 ? r[q] + 1 : 0) << (6u * q);
            if (q == qe && r[q] == ik && d == EP_SAT) d = e;
        }
    }
    if (d > EP_BAND) return false;
    // the traceback: from (k, m) at cost d, an edit a step
    uint32_t i = k, j = m, q = qe;
    for (uint32_t v = d; i > 0u; --v) {
        uint32_t x = 0u;
        AC_BS_UNROLL
        for (uint32_t y = 0; y < EP_DIAGS; ++y) x = q == y ? neq[y] : x;
        // the run of matches below row i (a row left of column 0 is a mismatch in the mask)
        const uint32_t below = x & (i >= 32u ? ~0u : (1u << i) - 1u);
        const uint32_t run = below ? i - 32u + (uint32_t)__builtin_clz(below) : i;
        i -= run, j -= run;
        if (!i || !v) break;  // (v = 0 with i > 0 cannot be: a cell of cost 0 lies on a run down to row 0)
        const uint64_t rows = v == 1u ? packed[0] : v == 2u ? packed[1] : packed[2];
        const uint32_t tj = (j ? j : 1u) - 1u;
        const uint32_t sym = (isn >> tj & 1u) ? 4u : (uint32_t)(lo >> tj & 1u) | (uint32_t)(hi >> tj & 1u) << 1;
        if (j && (uint32_t)(rows >> (6u * q) & 63u) >= i) {
            count(i - 1u, EP_SUB + sym);
            --i, --j;
        } else if (q + 1u < EP_DIAGS && (uint32_t)(rows >> (6u * (q + 1u)) & 63u) >= i) {
            count(i - 1u, EP_DEL);
            --i, ++q;
        } else {
            if (!j || !q) break;  // (unreachable: in column 0 the deletion rule holds, and a path of cost <= 3 stays in the band)
            count(i - 1u, EP_INS + sym);
            --j, --q;
        }
    }
    return true;
}

}  // namespace bs
}  // namespace acamd
