// bs_nfa_r.h -- bs_nfa.h's NFA and bit-plane counters for a chosen number of rows R = E + 1, E the
// edit budget of the count (M1(E): a window adds max(0, E + 1 - d); DESIGN.md §4e "Edit budget").
// bs_nfa.h stays the R = 3 form the E = 2 kernels are built from; this header is what the E = 3
// kernels (bs3_count.hip) run, and -- through vc_add_e -- how the E = 2 kernels count at E = 0 and 1.
// Plain C++ for the device and the host (tools/bs_nfa_r_check.cpp, tests/test_bs_nfa_budget.py).
//
// Rows follow bs_nfa.h's one recurrence,
//   D0'[0] = nE[0]                       D0'[i] = D0[i-1] | nE[i]
//   Dd'[i] = (Dd[i-1] | nE[i]) & Dd-1[i] & Dd-1[i-1] & Dd-1'[i-1]          d = 1 .. R - 1
// with Dd[i] constant 0 for i < d.  Per text base: K - 1 ORs and 2 (K - d) three-input ops for each
// row d >= 1 -- 2 (3K - 6) at R = 4 -- plus R / 2 ops of hit accumulation when bases go in pairs.
#pragma once
#include "bs_nfa.h"

namespace acamd {
namespace bs {

template <int K, int R>
struct StateR {
    uint32_t d[R][K];  // d[r][i] stays 0 for i < r
    uint32_t a[R];     // bit clear: that level has hit somewhere in the window
};

template <int K, int R>
AC_BS_FN void init(StateR<K, R>& s) {
    AC_BS_UNROLL
    for (int r = 0; r < R; ++r) {
        AC_BS_UNROLL
        for (int i = 0; i < K; ++i) s.d[r][i] = i >= r ? ~0u : 0u;
        s.a[r] = ~0u;
    }
}

// One text base (no hit accumulation).
template <int K, int R>
AC_BS_FN void advance(StateR<K, R>& s, const uint32_t (&nE)[K]) {
    static_assert(R >= 1 && R <= 4 && K >= R, "rows and pattern length");
    uint32_t n[R][K];
    n[0][0] = nE[0];
    AC_BS_UNROLL
    for (int i = 1; i < K; ++i) n[0][i] = s.d[0][i - 1] | nE[i];
    AC_BS_UNROLL
    for (int r = 1; r < R; ++r) {
        AC_BS_UNROLL
        for (int i = 0; i < r; ++i) n[r][i] = 0u;
        // (position r of row r: Dr[r - 1] = 0, so the OR falls away)
        n[r][r] = bitop3<TT_AND3>(nE[r] & s.d[r - 1][r], s.d[r - 1][r - 1], n[r - 1][r - 1]);
        AC_BS_UNROLL
        for (int i = r + 1; i < K; ++i)
            n[r][i] = bitop3<TT_AND3>(bitop3<TT_OR_AND>(s.d[r][i - 1], nE[i], s.d[r - 1][i]), s.d[r - 1][i - 1],
                                      n[r - 1][i - 1]);
    }
    AC_BS_UNROLL
    for (int r = 0; r < R; ++r) {
        AC_BS_UNROLL
        for (int i = 0; i < K; ++i) s.d[r][i] = n[r][i];
    }
}

// The last position of the rows: what a base contributes to the window's hits.
template <int R>
struct LastR {
    uint32_t x[R];
};
template <int K, int R>
AC_BS_FN LastR<R> last(const StateR<K, R>& s) {
    LastR<R> x;
    AC_BS_UNROLL
    for (int r = 0; r < R; ++r) x.x[r] = s.d[r][K - 1];
    return x;
}
// The hits of two bases (the previous base's last positions in `x`) in one AND3 per level.
template <int K, int R>
AC_BS_FN void hits2(StateR<K, R>& s, const LastR<R>& x) {
    AC_BS_UNROLL
    for (int r = 0; r < R; ++r) s.a[r] = bitop3<TT_AND3>(s.a[r], x.x[r], s.d[r][K - 1]);
}

// One base with its hits.
template <int K, int R>
AC_BS_FN void step(StateR<K, R>& s, const uint32_t (&nE)[K]) {
    advance(s, nE);
    AC_BS_UNROLL
    for (int r = 0; r < R; ++r) s.a[r] &= s.d[r][K - 1];
}

// Two bases.
template <int K, int R>
AC_BS_FN void step2(StateR<K, R>& s, const uint32_t (&nEa)[K], const uint32_t (&nEb)[K]) {
    advance(s, nEa);
    const LastR<R> x = last(s);
    advance(s, nEb);
    hits2(s, x);
}

// The bit-plane counters for R levels: a window adds 0..R, so VC_PLANES planes hold
// (2^VC_PLANES - 1) / R windows between flushes -- 31, 15, 10, 7 for R = 1..4.
constexpr uint32_t vc_windows(int R) { return ((1u << VC_PLANES) - 1u) / (uint32_t)R; }
template <int R>
AC_BS_FN bool vc_full_r(const VCount& v) {
    return v.n >= vc_windows(R);
}

// The E = 2 kernels at a smaller budget: the rows of the unused levels are computed and dropped.  The
// triple handed to vc_add stays nested (a level never hit, then the levels in use), so its plane
// arithmetic holds: E = 1 adds h0 + h1, E = 0 adds h0.  E >= 2: the three levels as they are.
AC_BS_FN void vc_add_e(VCount& v, uint32_t E, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t live) {
    const uint32_t b2 = E >= 2u ? a2 : E == 1u ? a1 : a0;
    const uint32_t b1 = E >= 2u ? a1 : E == 1u ? a0 : ~0u;
    const uint32_t b0 = E >= 2u ? a0 : ~0u;
    vc_add(v, b0, b1, b2, live);  // (at most 2 per window: the owner's flush at VC_WINDOWS windows holds)
}

// Four nested levels: with h_d = ~a_d the sum h0 + h1 + h2 + h3 (0..4) is at least 2 iff h2 and 4 iff
// h0, so its bits are h0 ^ h1 ^ h2 ^ h3, h2 & ~h0 and h0; they ripple into the planes.
AC_BS_FN void vc_add4(VCount& v, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t live) {
    static_assert(VC_PLANES >= 4, "planes");
    const uint32_t b0 = (bitop3<TT_XOR3>(a0, a1, a2) ^ a3) & live;  // (an even number of complements cancels)
    const uint32_t b1 = ~a2 & a0 & live;
    const uint32_t b2 = ~a0 & live;
    uint32_t c = v.p[0] & b0;
    v.p[0] ^= b0;
    uint32_t t = bitop3<TT_MAJ>(v.p[1], b1, c);
    v.p[1] = bitop3<TT_XOR3>(v.p[1], b1, c);
    c = t;
    t = bitop3<TT_MAJ>(v.p[2], b2, c);
    v.p[2] = bitop3<TT_XOR3>(v.p[2], b2, c);
    c = t;
    AC_BS_UNROLL
    for (int b = 3; b < VC_PLANES; ++b) {
        t = v.p[b] & c;
        v.p[b] ^= c;
        c = t;
    }
    ++v.n;
}

// R levels' hits into the planes, R = 1..4 (R = 3 is bs_nfa.h's vc_add).
template <int R>
AC_BS_FN void vc_add_r(VCount& v, const uint32_t (&a)[R], uint32_t live) {
    if constexpr (R == 4)
        vc_add4(v, a[0], a[1], a[2], a[3], live);
    else if constexpr (R == 3)
        vc_add(v, a[0], a[1], a[2], live);
    else if constexpr (R == 2)
        vc_add(v, ~0u, a[0], a[1], live);
    else
        vc_add(v, ~0u, ~0u, a[0], live);
}

}  // namespace bs
}  // namespace acamd
