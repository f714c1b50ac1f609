// bs_nfa_check -- runs the host build of the bit-sliced NFA and its bit-plane counters
// (approx_counter_amd/csrc/bs_nfa.h, the code the bit-sliced count kernel runs per base) on a case read
// from a file, for tests/test_bs_nfa.py (host-only; built there with the sanitizers on).
//   bs_nfa_check count IN OUT
//     IN : u32 k, n_kmers, n_windows; n_kmers u64 k-mers (2 bits per base, first base highest);
//          per window u32 length, then its bases as bytes (0-3 = A C G T, 4 = N)
//     OUT: n_kmers u32 counts (levels 0, 1, 2 hit, summed over the windows), then u32 flushes
//   The candidates go in blocks of 32 (bit j of a word = candidate j of the block), every window
//   through step2 (pairs of bases) and step (an odd last base); a block's hits are summed in a VCount
//   that is flushed into the counts when vc_full says so and at the end, as the kernel does.
//   bs_nfa_check vc IN OUT
//     IN : u32 n, then n x (u32 a0, a1, a2, live): the windows added to one VCount, without a flush
//     OUT: u32 VC_PLANES, VC_WINDOWS; per add u32 vc_full after it; then the 32 counts (vc_get)
#include <cstdio>
#include <cstring>
#include <vector>

#include "bs_nfa.h"

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

template <int K>
void count_k(const std::vector<uint64_t>& kmers, const std::vector<std::vector<unsigned char>>& wins,
             std::vector<uint32_t>& counts, uint32_t& flushes) {
    for (size_t b0 = 0; b0 < kmers.size(); b0 += 32) {
        // the block's ~Eq table: nE[c][i] bit j = candidate j's base i differs from c; N matches nothing;
        // candidate slots past the end are all ones
        uint32_t nE[5][K];
        for (int c = 0; c < 5; ++c)
            for (int i = 0; i < K; ++i) {
                uint32_t w = ~0u;
                for (size_t j = 0; j < 32 && b0 + j < kmers.size(); ++j)
                    if (c < 4 && ((kmers[b0 + j] >> (2 * (K - 1 - i))) & 3u) == (uint32_t)c) w &= ~(1u << j);
                nE[c][i] = w;
            }
        bs::VCount vc;
        bs::vc_clear(vc);
        auto flush = [&] {
            for (uint32_t j = 0; j < 32 && b0 + j < kmers.size(); ++j) counts[b0 + j] += bs::vc_get(vc, j);
            bs::vc_clear(vc);
            ++flushes;
        };
        for (const auto& w : wins) {
            bs::State<K> s;
            bs::init<K>(s);
            size_t p = 0;
            for (; p + 2 <= w.size(); p += 2) bs::step2<K>(s, nE[w[p]], nE[w[p + 1]]);
            if (p < w.size()) bs::step<K>(s, nE[w[p]]);
            if (bs::vc_full(vc)) flush();
            bs::vc_add(vc, s.a0, s.a1, s.a2, ~0u);
        }
        if (vc.n) flush();
    }
}

int run_count(Reader& in, FILE* out) {
    const uint32_t k = in.get<uint32_t>(), nk = in.get<uint32_t>(), nw = in.get<uint32_t>();
    if (in.bad || nk > in.buf.size() || nw > in.buf.size()) return 2;
    std::vector<uint64_t> kmers(nk);
    for (auto& v : kmers) v = in.get<uint64_t>();
    std::vector<std::vector<unsigned char>> wins(nw);
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
#define AC_BS_RUN(KK)                           \
    if (k == KK) {                              \
        count_k<KK>(kmers, wins, counts, flushes); \
        done = true;                            \
    }
    AC_BS_K_LIST(AC_BS_RUN)
#undef AC_BS_RUN
    if (!done) return 3;  // not an instantiated pattern length
    std::fwrite(counts.data(), sizeof(uint32_t), counts.size(), out);
    std::fwrite(&flushes, sizeof flushes, 1, out);
    return 0;
}

int run_vc(Reader& in, FILE* out) {
    const uint32_t n = in.get<uint32_t>();
    if (in.bad || n > in.buf.size()) return 2;
    const uint32_t consts[2] = {(uint32_t)bs::VC_PLANES, bs::VC_WINDOWS};
    std::fwrite(consts, sizeof(uint32_t), 2, out);
    bs::VCount vc;
    bs::vc_clear(vc);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t a0 = in.get<uint32_t>(), a1 = in.get<uint32_t>(), a2 = in.get<uint32_t>(), live = in.get<uint32_t>();
        if (in.bad) return 2;
        bs::vc_add(vc, a0, a1, a2, live);
        const uint32_t full = bs::vc_full(vc) ? 1u : 0u;
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
    if (argc != 4) {
        std::fprintf(stderr, "usage: bs_nfa_check count|vc IN OUT\n");
        return 2;
    }
    Reader in;
    in.buf = slurp(argv[2]);
    FILE* out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    const int rc = !std::strcmp(argv[1], "count") ? run_count(in, out) : !std::strcmp(argv[1], "vc") ? run_vc(in, out) : 2;
    std::fclose(out);
    return rc;
}
