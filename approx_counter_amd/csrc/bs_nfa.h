// bs_nfa.h -- the bit-sliced ("candidate per bit") form of the count kernel's NFA, and the
// bit-plane counters its hits are summed in.  Plain C++ that compiles for the
// device (bs_count.inc) and for the host (tools/bs_nfa_check.cpp, tests/test_bs_nfa.py), so the
// code the kernel runs is the code the CPU test checks against the oracle.  Also here, and checked the
// same way (tools/bs_flush_check.cpp, tests/test_bs_flush_cpu.py): the plane adder and extraction of the
// flush, and the ~Eq table's masks.
//
// The recurrence is wm_count.hip's (Wu-Manber, complemented, free start in the text), transposed:
// bit j of a word is candidate j of a block of 32, register i is pattern position i.  The shift
// (D >> P)[i] = D[i-1] is then a register rename, and only position K-1 is accumulated for hits.
// With nE[i] = the 32 candidates' ~Eq at position i under the current text character:
//   D0'[0] = nE[0]                       D0'[i] = D0[i-1] | nE[i]
//   Dd'[i] = (Dd[i-1] | nE[i]) & Dd-1[i] & Dd-1[i-1] & Dd-1'[i-1]          d = 1, 2
// The zero fill of the shift makes D1[0], D2[0] and D2[1] zero for good (from the initial rows:
// R1 has position 0 set, R2 positions 0 and 1), so they are constants here: no register, no op.
// Per text base: K-1 ORs, 2(K-1) + 2(K-2) three-input ops, and 1.5 ops of hit accumulation when
// bases go in pairs (step2) -- 74.5 for K = 16, for 32 candidates.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AC_BS_FN __host__ __device__ __forceinline__
#else
#define AC_BS_FN inline
#endif
#if defined(__clang__)
#define AC_BS_UNROLL _Pragma("unroll")
#define AC_BS_NOUNROLL _Pragma("nounroll")
#else
#define AC_BS_UNROLL  // (the host build's compiler may not know the pragma)
#define AC_BS_NOUNROLL
#endif

namespace acamd {
namespace bs {

// The instantiated pattern lengths, in one place (the host's bs_launch routes by it, wm_count.hip
// instantiates by it, tools/bs_nfa_check.cpp runs by it): 16 and 18..32.  k = 15 and k = 17 stay on the
// word-parallel kernel (tests pin them there); below 16 that kernel packs 2-4 candidates per lane
// word and is not the slower one.
#define AC_BS_K_LIST(X) \
    X(16) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)
constexpr bool has_k(uint32_t k) {
#define AC_BS_K_EQ(KK) || k == KK
    return false AC_BS_K_LIST(AC_BS_K_EQ);
#undef AC_BS_K_EQ
}

// v_bitop3_b32 by its truth table: bit (a << 2 | b << 1 | c) of TT is the result for inputs a, b, c.
template <uint32_t TT>
AC_BS_FN uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
#else
    uint32_t r = 0;
    for (uint32_t i = 0; i < 8; ++i)
        if (TT >> i & 1u) r |= ((i & 4u) ? a : ~a) & ((i & 2u) ? b : ~b) & ((i & 1u) ? c : ~c);
    return r;
#endif
}
constexpr uint32_t TT_OR_AND = 0xa8;  // (a | b) & c
constexpr uint32_t TT_AND3 = 0x80;    // a & b & c
constexpr uint32_t TT_XOR3 = 0x96;    // a ^ b ^ c
constexpr uint32_t TT_MAJ = 0xe8;     // majority(a, b, c)

// The three rows of 32 candidates' NFAs and the AND of their last position over a window.
template <int K>
struct State {
    uint32_t d0[K], d1[K], d2[K];  // d1[0], d2[0], d2[1] stay 0
    uint32_t a0, a1, a2;           // bit clear: that level has hit somewhere in the window
};

template <int K>
AC_BS_FN void init(State<K>& s) {
    AC_BS_UNROLL
    for (int i = 0; i < K; ++i) {
        s.d0[i] = ~0u;
        s.d1[i] = i >= 1 ? ~0u : 0u;
        s.d2[i] = i >= 2 ? ~0u : 0u;
    }
    s.a0 = s.a1 = s.a2 = ~0u;
}

// One text base (no hit accumulation).
template <int K>
AC_BS_FN void advance(State<K>& s, const uint32_t (&nE)[K]) {
    static_assert(K >= 3, "pattern length");
    uint32_t n0[K], n1[K], n2[K];
    n0[0] = nE[0];
    n1[0] = 0u;
    n2[0] = 0u;
    n2[1] = 0u;
    AC_BS_UNROLL
    for (int i = 1; i < K; ++i) n0[i] = s.d0[i - 1] | nE[i];
    // (position 1 of row 1: D1[0] = 0, so the OR falls away)
    n1[1] = bitop3<TT_AND3>(nE[1] & s.d0[1], s.d0[0], n0[0]);
    AC_BS_UNROLL
    for (int i = 2; i < K; ++i)
        n1[i] = bitop3<TT_AND3>(bitop3<TT_OR_AND>(s.d1[i - 1], nE[i], s.d0[i]), s.d0[i - 1], n0[i - 1]);
    n2[2] = bitop3<TT_AND3>(nE[2] & s.d1[2], s.d1[1], n1[1]);
    AC_BS_UNROLL
    for (int i = 3; i < K; ++i)
        n2[i] = bitop3<TT_AND3>(bitop3<TT_OR_AND>(s.d2[i - 1], nE[i], s.d1[i]), s.d1[i - 1], n1[i - 1]);
    AC_BS_UNROLL
    for (int i = 0; i < K; ++i) {
        s.d0[i] = n0[i];
        s.d1[i] = n1[i];
        s.d2[i] = n2[i];
    }
}

// The last position of the three rows: what a base contributes to the window's hits.
struct Last {
    uint32_t x0, x1, x2;
};
template <int K>
AC_BS_FN Last last(const State<K>& s) {
    return Last{s.d0[K - 1], s.d1[K - 1], s.d2[K - 1]};
}
// The hits of two bases (the previous base's last positions in `x`) in one AND3 per level: 1.5 ops per base.
template <int K>
AC_BS_FN void hits2(State<K>& s, const Last& x) {
    s.a0 = bitop3<TT_AND3>(s.a0, x.x0, s.d0[K - 1]);
    s.a1 = bitop3<TT_AND3>(s.a1, x.x1, s.d1[K - 1]);
    s.a2 = bitop3<TT_AND3>(s.a2, x.x2, s.d2[K - 1]);
}

// One base with its hits: 3 ops.
template <int K>
AC_BS_FN void step(State<K>& s, const uint32_t (&nE)[K]) {
    advance(s, nE);
    s.a0 &= s.d0[K - 1];
    s.a1 &= s.d1[K - 1];
    s.a2 &= s.d2[K - 1];
}

// Two bases.
template <int K>
AC_BS_FN void step2(State<K>& s, const uint32_t (&nEa)[K], const uint32_t (&nEb)[K]) {
    advance(s, nEa);
    const Last x = last(s);
    advance(s, nEb);
    hits2(s, x);
}

// Bit-plane ("vertical") counters: plane b holds bit b of 32 candidates' counts.  A window adds
// its number of levels hit (0..3) to every candidate at once: the levels nest (a row-d match is one
// of row d+1), so with h_d = ~a_d the sum h0 + h1 + h2 has low bit h0 ^ h1 ^ h2 and high bit h1; the
// two bits ripple into the planes.  NPL planes hold counts up to 2^NPL - 1, i.e. VC_WINDOWS
// windows: the owner flushes (reads every candidate's count with get() and clears) before adding
// one more.
constexpr int VC_PLANES = 5;
constexpr uint32_t VC_WINDOWS = ((1u << VC_PLANES) - 1u) / 3u;  // 10 windows between flushes
struct VCount {
    uint32_t p[VC_PLANES];
    uint32_t n;  // windows added since the last flush (the same in every lane)
};
AC_BS_FN void vc_clear(VCount& v) {
    AC_BS_UNROLL
    for (int b = 0; b < VC_PLANES; ++b) v.p[b] = 0u;
    v.n = 0u;
}
AC_BS_FN bool vc_full(const VCount& v) { return v.n >= VC_WINDOWS; }
// `live`: the candidates' windows that count (a lane without a window adds nothing)
AC_BS_FN void vc_add(VCount& v, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t live) {
    const uint32_t lo = ~bitop3<TT_XOR3>(a0, a1, a2) & live;  // (~a0 ^ ~a1 ^ ~a2 = ~(a0 ^ a1 ^ a2))
    const uint32_t hi = ~a1 & live;
    const uint32_t c0 = v.p[0] & lo;
    v.p[0] ^= lo;
    uint32_t c = bitop3<TT_MAJ>(v.p[1], hi, c0);
    v.p[1] = bitop3<TT_XOR3>(v.p[1], hi, c0);
    AC_BS_UNROLL
    for (int b = 2; b < VC_PLANES; ++b) {
        const uint32_t t = v.p[b] & c;
        v.p[b] ^= c;
        c = t;
    }
    ++v.n;
}
AC_BS_FN uint32_t vc_get(const VCount& v, uint32_t j) {
    uint32_t r = 0;
    AC_BS_UNROLL
    for (int b = 0; b < VC_PLANES; ++b) r |= (v.p[b] >> j & 1u) << b;
    return r;
}

// The flush by plane merge (bs_count.inc): the lanes of a wave that hold the same 32 candidates -- one per
// window of the row -- add their plane counters to each other in registers before anything goes to LDS.
// One round of that sum is a bit-plane ripple adder: two numbers of N planes give one of N + 1, so
// VC_PLANES planes of at most 2^VC_PLANES - 1 merged over 32 lanes (five rounds) fill VC_MERGED_PLANES.
constexpr int VC_MERGED_PLANES = VC_PLANES + 5;
// sum[0..N] = a[0..N-1] + b[0..N-1]; `sum` may be `a`.
template <int N>
AC_BS_FN void planes_add(const uint32_t* a, const uint32_t* b, uint32_t* sum) {
    uint32_t c = a[0] & b[0];
    sum[0] = a[0] ^ b[0];
    AC_BS_UNROLL
    for (int i = 1; i < N; ++i) {
        const uint32_t x = a[i], y = b[i];
        sum[i] = bitop3<TT_XOR3>(x, y, c);
        c = bitop3<TT_MAJ>(x, y, c);
    }
    sum[N] = c;
}
// Candidate j's count from N planes.
template <int N>
AC_BS_FN uint32_t planes_get(const uint32_t (&p)[N], uint32_t j) {
    uint32_t r = 0;
    AC_BS_UNROLL
    for (int b = 0; b < N; ++b) r |= (p[b] >> j & 1u) << b;
    return r;
}
// After the merge every one of the 64 / LW lanes of a candidate block (LW = 1 << lwsh lanes per window)
// holds the block's sums; lane number wl of them (its window in the row) takes the 32 LW / 64 candidates
// from merged_first(lwsh, wl) on, so each (block, candidate) is added to LDS by one lane.
AC_BS_FN uint32_t merged_per_lane(uint32_t lwsh) { return 32u >> (6u - lwsh); }
AC_BS_FN uint32_t merged_first(uint32_t lwsh, uint32_t wl) { return wl * merged_per_lane(lwsh); }

// The workgroup's ~Eq table (bs_count.inc), one (position, character) of up to 64 candidates: bit j is set
// iff candidate j's base at pattern position i (0 = first base: the k-mer's highest two bits) differs from
// character c (0..3), or slot j is past the n candidates present -- `km` holds 64 slots, those past n are
// not looked at.
template <int K>
AC_BS_FN uint64_t neq_mask(const uint64_t* km, uint32_t n, uint32_t i, uint32_t c) {
    const uint32_t sh = 2u * ((uint32_t)K - 1u - i);
    uint32_t lo = 0u, hi = 0u;
    AC_BS_NOUNROLL  // (eight slots of each half at a time: unrolled whole, the 64 reads are all hoisted and spill)
    for (int j0 = 24; j0 >= 0; j0 -= 8) {
        AC_BS_UNROLL
        for (int j = j0 + 7; j >= j0; --j) {
            lo = lo << 1 | (((uint32_t)(km[j] >> sh) & 3u) != c ? 1u : 0u);
            hi = hi << 1 | (((uint32_t)(km[j + 32] >> sh) & 3u) != c ? 1u : 0u);
        }
    }
    const uint64_t m = (uint64_t)hi << 32 | lo;
    return n < 64u ? m | ~0ull << n : m;
}

}  // namespace bs
}  // namespace acamd
