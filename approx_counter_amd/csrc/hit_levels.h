// hit_levels.h -- the column counter of a hit matrix (DESIGN.md §4e "Hit levels"): how many windows of
// one level plane hold each candidate.  Plain C++ that compiles for the device (bsh_count.hip's
// hit_level_counts_kernel) and for the host (tools/hit_levels_check.cpp, tests/test_hits_cpu.py), so the
// code the kernel runs is the code the CPU test checks.
//
// A level plane is n_windows rows of `words` u32, bit j of word x = candidate 32 x + j.  One word column
// is counted by adding its words, one window each, into bit-plane counters -- the one-bit-add sibling of
// bs_nfa.h's VCount: plane b holds bit b of 32 candidates' counts, an add ripples one carry through the
// planes -- which are flushed into 32 integer counters before they can overflow.
#pragma once
#include <stdint.h>

#include "bs_nfa.h"

namespace acamd {
namespace bs {

constexpr int HC_PLANES = 5;
constexpr uint32_t HC_WINDOWS = (1u << HC_PLANES) - 1u;  // 31 one-bit adds between flushes
struct HCount {
    uint32_t p[HC_PLANES];
    uint32_t n;  // words added since the last flush
};
AC_BS_FN void hc_clear(HCount& v) {
    AC_BS_UNROLL
    for (int b = 0; b < HC_PLANES; ++b) v.p[b] = 0u;
    v.n = 0u;
}
AC_BS_FN bool hc_full(const HCount& v) { return v.n >= HC_WINDOWS; }
AC_BS_FN void hc_add(HCount& v, uint32_t w) {
    uint32_t c = w;
    AC_BS_UNROLL
    for (int b = 0; b < HC_PLANES; ++b) {
        const uint32_t t = v.p[b] & c;
        v.p[b] ^= c;
        c = t;
    }
    ++v.n;
}
AC_BS_FN uint32_t hc_get(const HCount& v, uint32_t j) {
    uint32_t r = 0;
    AC_BS_UNROLL
    for (int b = 0; b < HC_PLANES; ++b) r |= (v.p[b] >> j & 1u) << b;
    return r;
}
// The planes into the 32 integer counters, and cleared.
AC_BS_FN void hc_flush(HCount& v, uint32_t (&cnt)[32]) {
    AC_BS_UNROLL
    for (uint32_t j = 0; j < 32u; ++j) cnt[j] += hc_get(v, j);
    hc_clear(v);
}

// N more words (N <= HC_WINDOWS), flushing first if the planes could not hold them: the form the kernel
// adds a batch of loads in.
template <int N>
AC_BS_FN void hc_add_n(HCount& v, const uint32_t (&x)[N], uint32_t (&cnt)[32]) {
    static_assert(N >= 1 && (uint32_t)N <= HC_WINDOWS, "a batch fits the planes");
    if (v.n + (uint32_t)N > HC_WINDOWS) hc_flush(v, cnt);
    AC_BS_UNROLL
    for (int i = 0; i < N; ++i) hc_add(v, x[i]);
}

constexpr int HC_BATCH = 8;  // words a thread loads before it adds them (loads in flight per lane)

// Column `col` of one level plane over the windows w0, w0 + step, .. below w1: cnt[j] += the windows whose
// word has bit j set.  Batches of HC_BATCH words, then one by one.
AC_BS_FN void hc_column(const uint32_t* plane, uint32_t words, uint32_t col, uint64_t w0, uint64_t w1, uint64_t step,
                        uint32_t (&cnt)[32]) {
    HCount v;
    hc_clear(v);
    uint64_t w = w0;
    for (; w + (uint64_t)(HC_BATCH - 1) * step < w1; w += (uint64_t)HC_BATCH * step) {
        uint32_t x[HC_BATCH];
        AC_BS_UNROLL
        for (int i = 0; i < HC_BATCH; ++i) x[i] = plane[(w + (uint64_t)i * step) * words + col];
        hc_add_n<HC_BATCH>(v, x, cnt);
    }
    for (; w < w1; w += step) {
        const uint32_t x[1] = {plane[w * words + col]};
        hc_add_n<1>(v, x, cnt);
    }
    hc_flush(v, cnt);
}

}  // namespace bs
}  // namespace acamd
