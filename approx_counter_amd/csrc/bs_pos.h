// bs_pos.h -- match end positions beside the bit-sliced NFA's hits (DESIGN.md §4e "Match end positions"):
// where in its window each candidate's best occurrence ends.  Plain C++ that compiles for the device
// (bs_count.inc's POS switch, bsp_count.hip) and for the host (tools/bs_pos_check.cpp,
// tests/test_positions_cpu.py), so the code the kernels run is the code the CPU test checks against a
// Sellers DP.
//
// Level e's bit of the rows' last position is clear at base j iff e(j) <= e, e(j) the least edit distance
// of the whole pattern against a substring of the window that ends at j.  The first bases at which the
// levels E, E - 1, .., 0 get hit do not increase with the level, so whenever ANY level 0..E is hit for the
// first time the best level so far has just improved: the position is overwritten at every such base, and
// the last overwrite is pos = min { j : e(j) = min e }.
// Eight bit planes hold pos - 1 (0..255) of 32 candidates: plane b is bit b.  The base's index inside a
// block of 4 is a compile-time constant and its upper bits are wave-uniform over the block, so planes 0-1
// are written per base and planes 2-7 once per block from the OR of the block's four `new` masks (a later
// `new` base of one block overwrites an earlier one's planes 0-1; planes 2-7 are the same for both).
#pragma once
#include <stdint.h>

#include "bs_nfa.h"
#include "bs_nfa_r.h"

namespace acamd {
namespace bs {

constexpr int POS_PLANES = 8;
constexpr uint32_t TT_XOR_OR = 0xbe;   // (a ^ b) | c
constexpr uint32_t TT_XOR_AND = 0x28;  // (a ^ b) & c
constexpr uint32_t TT_OR3 = 0xfe;      // a | b | c
constexpr uint32_t TT_SEL = 0xb8;      // b ? c : a, bit by bit

struct PosPlanes {
    static constexpr bool ON = true;
    uint32_t p[POS_PLANES];
    uint32_t blk;  // the OR of the `new` masks of the block's bases so far
};
AC_BS_FN void pos_clear(PosPlanes& P) {
    AC_BS_UNROLL
    for (int b = 0; b < POS_PLANES; ++b) P.p[b] = 0u;
    P.blk = 0u;
}

// One base's hits (after advance), level by level, and the candidates for which some level 0..E was hit for
// the first time at this base.  Three rows: E = 0, 1 or 2, wave-uniform -- a level above E is accumulated
// (the caller drops it, vc_add_e) but must not move the position.  With a' = a & last, a & ~last = a ^ a'.
template <int K>
AC_BS_FN uint32_t hits_new(State<K>& s, uint32_t E) {
    const uint32_t k1 = E >= 1u ? ~0u : 0u, k2 = E >= 2u ? ~0u : 0u;
    const uint32_t b0 = s.a0 & s.d0[K - 1], b1 = s.a1 & s.d1[K - 1], b2 = s.a2 & s.d2[K - 1];
    const uint32_t nw = bitop3<TT_OR3>(s.a0 ^ b0, bitop3<TT_XOR_AND>(s.a1, b1, k1), bitop3<TT_XOR_AND>(s.a2, b2, k2));
    s.a0 = b0;
    s.a1 = b1;
    s.a2 = b2;
    return nw;
}
// R rows: E = R - 1, every level counts.
template <int K, int R>
AC_BS_FN uint32_t hits_new(StateR<K, R>& s, uint32_t) {
    uint32_t nw = 0u;
    AC_BS_UNROLL
    for (int r = 0; r < R; ++r) {
        const uint32_t b = s.a[r] & s.d[r][K - 1];
        nw = r == 0 ? s.a[r] ^ b : bitop3<TT_XOR_OR>(s.a[r], b, nw);
        s.a[r] = b;
    }
    return nw;
}

// Base number `b` (0..3, a constant where this is inlined) of a block: planes 0 and 1.
AC_BS_FN void pos_base(PosPlanes& P, uint32_t nw, uint32_t b) {
    P.p[0] = (b & 1u) ? P.p[0] | nw : P.p[0] & ~nw;
    P.p[1] = (b & 2u) ? P.p[1] | nw : P.p[1] & ~nw;
    P.blk = b == 0u ? nw : P.blk | nw;
}
// The end of block number q (its bases are 4 q .. 4 q + 3; wave-uniform): planes 2..7 take q's bits where
// one of the block's bases was new.
AC_BS_FN void pos_block(PosPlanes& P, uint32_t q) {
    AC_BS_UNROLL
    for (int b = 2; b < POS_PLANES; ++b) P.p[b] = bitop3<TT_SEL>(P.p[b], P.blk, 0u - (q >> (b - 2) & 1u));
}
// Candidate j's pos - 1 from the planes.
AC_BS_FN uint32_t pos_get(const uint32_t (&p)[POS_PLANES], uint32_t j) {
    uint32_t r = 0;
    AC_BS_UNROLL
    for (int b = 0; b < POS_PLANES; ++b) r |= (p[b] >> j & 1u) << b;
    return r;
}

// The position profile's walk (bsp_count.hip's hit_position_profile_kernel): word column `col` of a hit
// matrix (levels planes of n_windows x words) and its position matrix (POS_PLANES planes of the same shape)
// over the windows w0, w0 + step, .. below w1, for distance d: every candidate c = 32 col + j < n_kmers
// whose word has level d set and level d - 1 clear (the levels nest) calls add(j, pos - 1).  The position
// planes are read only where such a bit exists.
template <class F>
AC_BS_FN void pp_column(const uint32_t* hits, const uint32_t* pos, uint32_t n_kmers, uint64_t n_windows, uint32_t d,
                        uint32_t col, uint64_t w0, uint64_t w1, uint64_t step, F&& add) {
    const uint64_t words = ((uint64_t)n_kmers + 31u) >> 5;
    const uint64_t plane = n_windows * words;
    const uint32_t left = n_kmers - 32u * col;  // (>= 1) candidates of this column
    const uint32_t keep = left >= 32u ? ~0u : (1u << left) - 1u;
    for (uint64_t w = w0; w < w1; w += step) {
        const uint64_t at = w * words + col;
        uint32_t m = hits[(uint64_t)d * plane + at] & keep;
        if (d) m &= ~hits[(uint64_t)(d - 1u) * plane + at];
        if (!m) continue;
        uint32_t p[POS_PLANES];
        AC_BS_UNROLL
        for (int b = 0; b < POS_PLANES; ++b) p[b] = pos[(uint64_t)b * plane + at];
        for (; m; m &= m - 1u) {
            const uint32_t j = (uint32_t)__builtin_ctz(m);
            add(j, pos_get(p, j));
        }
    }
}

}  // namespace bs
}  // namespace acamd
