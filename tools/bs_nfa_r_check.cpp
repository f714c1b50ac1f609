// bs_nfa_r_check -- runs the host build of the bit-sliced NFA at an edit budget E = 0..3
// (approx_counter_amd/csrc/bs_nfa_r.h over bs_nfa.h: the code the bit-sliced count kernels run per base
// and per window) on a case read from a file, for tests/test_bs_nfa_budget.py (host-only; built there
// with the sanitizers on).  File formats as tools/bs_nfa_check.cpp's.
//   bs_nfa_r_check count FORM E IN OUT
//     IN : u32 k, n_kmers, n_windows; n_kmers u64 k-mers (2 bits per base, first base highest);
//          per window u32 length, then its bases as bytes (0-3 = A C G T, 4 = N)
//     OUT: n_kmers u32 counts (sum over the windows of the levels 0..E hit), then u32 flushes
//     FORM kernel: what the kernels run -- E <= 2 the three rows of bs_nfa.h with the levels chosen
//          where the hit masks become counts (vc_add_e, flushed at VC_WINDOWS), E = 3 four rows
//          (StateR<K, 4>, vc_add_r<4>, flushed at vc_windows(4)).
//     FORM rows: E + 1 rows of the generic recurrence for every E (StateR<K, E + 1>, vc_add_r, vc_full_r).
//   The candidates go in blocks of 32, every window through step2 (pairs of bases) and step (an odd
//   last base); a block's hits are summed in a VCount flushed when full and at the end.
//   bs_nfa_r_check vc R IN OUT
//     IN : u32 n, then n x (u32 a0, a1, a2, a3, live): the windows added to one VCount (levels a0 ..
//          a[R-1]; the others ignored), without a flush
//     OUT: u32 VC_PLANES, vc_windows(R); per add u32 vc_full_r<R> after it; then the 32 counts (vc_get)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bs_nfa.h"
#include "bs_nfa_r.h"

namespace {

using namespace acamd;

std::vector<unsigned char> slurp(const char* path) {
    std::vector<unsigned char> buf;
    if (FILE* f = std::fopen(path, "rb")) {
        unsigned char tmp[4096];
        for (size_t n; (n = std::fread(tmp, 1, sizeof tmp, f)) > 0;) buf.insert(buf.end(), tmp, tmp + n);
        std::fclose(f);
    }
    return buf;
}

struct Reader {
    std::vector<unsigned char> buf;
    size_t at = 0;
    bool bad = false;
    template <class T>
    T get() {
        T v{};
        if (at + sizeof v <= buf.size()) std::memcpy(&v, buf.data() + at, sizeof v);
        else bad = true;
        at += sizeof v;
        return v;
    }
};

typedef std::vector<std::vector<unsigned char>> Windows;

// The block's ~Eq table: nE[c][i] bit j = candidate j's base i differs from c; N matches nothing;
// candidate slots past the end are all ones.
template <int K>
void eq_table(const std::vector<uint64_t>& kmers, size_t b0, uint32_t (&nE)[5][K]) {
    for (int c = 0; c < 5; ++c)
        for (int i = 0; i < K; ++i) {
            uint32_t w = ~0u;
            for (size_t j = 0; j < 32 && b0 + j < kmers.size(); ++j)
                if (c < 4 && ((kmers[b0 + j] >> (2 * (K - 1 - i))) & 3u) == (uint32_t)c) w &= ~(1u << j);
            nE[c][i] = w;
        }
}

template <int K, class S>
void run_window(S& s, const uint32_t (&nE)[5][K], const std::vector<unsigned char>& w) {
    bs::init<K>(s);
    size_t p = 0;
    for (; p + 2 <= w.size(); p += 2) bs::step2<K>(s, nE[w[p]], nE[w[p + 1]]);
    if (p < w.size()) bs::step<K>(s, nE[w[p]]);
}

// R rows of the generic recurrence.
template <int K, int R>
void count_rows(const std::vector<uint64_t>& kmers, const Windows& wins, std::vector<uint32_t>& counts, uint32_t& flushes) {
    for (size_t b0 = 0; b0 < kmers.size(); b0 += 32) {
        uint32_t nE[5][K];
        eq_table<K>(kmers, b0, nE);
        bs::VCount vc;
        bs::vc_clear(vc);
        auto flush = [&] {
            for (uint32_t j = 0; j < 32 && b0 + j < kmers.size(); ++j) counts[b0 + j] += bs::vc_get(vc, j);
            bs::vc_clear(vc);
            ++flushes;
        };
        for (const auto& w : wins) {
            bs::StateR<K, R> s;
            run_window<K>(s, nE, w);
            if (bs::vc_full_r<R>(vc)) flush();
            bs::vc_add_r<R>(vc, s.a, ~0u);
        }
        if (vc.n) flush();
    }
}

// The E = 0..2 kernels' form: three rows, the levels chosen at vc_add_e.
template <int K>
void count_e(uint32_t E, const std::vector<uint64_t>& kmers, const Windows& wins, std::vector<uint32_t>& counts,
             uint32_t& flushes) {
    for (size_t b0 = 0; b0 < kmers.size(); b0 += 32) {
        uint32_t nE[5][K];
        eq_table<K>(kmers, b0, nE);
        bs::VCount vc;
        bs::vc_clear(vc);
        auto flush = [&] {
            for (uint32_t j = 0; j < 32 && b0 + j < kmers.size(); ++j) counts[b0 + j] += bs::vc_get(vc, j);
            bs::vc_clear(vc);
            ++flushes;
        };
        for (const auto& w : wins) {
            bs::State<K> s;
            run_window<K>(s, nE, w);
            if (bs::vc_full(vc)) flush();
            bs::vc_add_e(vc, E, s.a0, s.a1, s.a2, ~0u);
        }
        if (vc.n) flush();
    }
}

template <int K>
void count_k(bool rows, uint32_t E, const std::vector<uint64_t>& kmers, const Windows& wins, std::vector<uint32_t>& counts,
             uint32_t& flushes) {
    if (E == 3u) return count_rows<K, 4>(kmers, wins, counts, flushes);
    if (!rows) return count_e<K>(E, kmers, wins, counts, flushes);
    if (E == 2u) return count_rows<K, 3>(kmers, wins, counts, flushes);
    if (E == 1u) return count_rows<K, 2>(kmers, wins, counts, flushes);
    return count_rows<K, 1>(kmers, wins, counts, flushes);
}

int run_count(bool rows, uint32_t E, Reader& in, FILE* out) {
    const uint32_t k = in.get<uint32_t>(), nk = in.get<uint32_t>(), nw = in.get<uint32_t>();
    if (in.bad || nk > in.buf.size() || nw > in.buf.size()) return 2;
    std::vector<uint64_t> kmers(nk);
    for (auto& v : kmers) v = in.get<uint64_t>();
    Windows wins(nw);
    for (auto& w : wins) {
        const uint32_t len = in.get<uint32_t>();
        if (in.bad || len > in.buf.size() - in.at) return 2;
        w.assign(in.buf.begin() + in.at, in.buf.begin() + in.at + len);
        in.at += len;
        for (unsigned char c : w)
            if (c > 4) return 2;
    }
    if (in.bad || in.at != in.buf.size()) return 2;
    std::vector<uint32_t> counts(nk, 0u);
    uint32_t flushes = 0;
    bool done = false;
#define AC_BS_RUN(KK)                                      \
    if (k == KK) {                                         \
        count_k<KK>(rows, E, kmers, wins, counts, flushes); \
        done = true;                                       \
    }
    AC_BS_K_LIST(AC_BS_RUN)
#undef AC_BS_RUN
    if (!done) return 3;  // not an instantiated pattern length
    std::fwrite(counts.data(), sizeof(uint32_t), counts.size(), out);
    std::fwrite(&flushes, sizeof flushes, 1, out);
    return 0;
}

template <int R>
int run_vc(Reader& in, FILE* out) {
    const uint32_t n = in.get<uint32_t>();
    if (in.bad || n > in.buf.size()) return 2;
    const uint32_t consts[2] = {(uint32_t)bs::VC_PLANES, bs::vc_windows(R)};
    std::fwrite(consts, sizeof(uint32_t), 2, out);
    bs::VCount vc;
    bs::vc_clear(vc);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t a[4], lv[R];
        for (uint32_t& x : a) x = in.get<uint32_t>();
        const uint32_t live = in.get<uint32_t>();
        if (in.bad) return 2;
        for (int r = 0; r < R; ++r) lv[r] = a[r];
        bs::vc_add_r<R>(vc, lv, live);
        const uint32_t full = bs::vc_full_r<R>(vc) ? 1u : 0u;
        std::fwrite(&full, sizeof full, 1, out);
    }
    for (uint32_t j = 0; j < 32; ++j) {
        const uint32_t v = bs::vc_get(vc, j);
        std::fwrite(&v, sizeof v, 1, out);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const bool count = argc == 6 && !std::strcmp(argv[1], "count");
    const bool vc = argc == 5 && !std::strcmp(argv[1], "vc");
    if (!count && !vc) {
        std::fprintf(stderr, "usage: bs_nfa_r_check count kernel|rows E IN OUT | vc R IN OUT\n");
        return 2;
    }
    const unsigned long num = std::strtoul(argv[count ? 3 : 2], nullptr, 10);
    if (count ? num > 3 || (std::strcmp(argv[2], "kernel") && std::strcmp(argv[2], "rows")) : num < 1 || num > 4) return 2;
    Reader in;
    in.buf = slurp(argv[argc - 2]);
    FILE* out = std::fopen(argv[argc - 1], "wb");
    if (!out) return 2;
    int rc;
    if (count) rc = run_count(!std::strcmp(argv[2], "rows"), (uint32_t)num, in, out);
    else rc = num == 4 ? run_vc<4>(in, out) : num == 3 ? run_vc<3>(in, out) : num == 2 ? run_vc<2>(in, out) : run_vc<1>(in, out);
    std::fclose(out);
    return rc;
}
