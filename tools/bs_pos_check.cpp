// bs_pos_check -- runs the host build of the match-end-position code (approx_counter_amd/csrc/bs_pos.h over
// bs_nfa.h / bs_nfa_r.h: what the hits-and-positions kernels run per base, per block and per window, and the
// profile kernel's column walk) on a case read from a file, for tests/test_positions_cpu.py (host-only;
// built there with the sanitizers on).
//   bs_pos_check pos E IN OUT
//     IN : u32 k, n_kmers, n_windows; n_kmers u64 k-mers (2 bits per base, first base highest);
//          per window u32 length (1..256), then its bases as bytes (0-3 = A C G T, 4 = N)
//     OUT: per window, per k-mer: i32 distance (the lowest level 0..E hit, -1: none), i32 pos (1..length,
//          0 where the distance is -1) -- the stored word's form: planes masked with ~a_E
//     The kernel's form: the candidates in blocks of 32, a window in blocks of 4 bases, its last block
//     filled up with N; per base advance, hits_new, pos_base, per block pos_block.  E <= 2: the three rows
//     of bs_nfa.h with the wave-uniform budget; E = 3: StateR<K, 4>.
//   bs_pos_check profile IN OUT
//     IN : u32 n_kmers, n_windows, levels, window_len, walks; the hit matrix (levels x n_windows x words
//          u32), the position matrix (8 x n_windows x words u32)
//     OUT: levels x n_kmers x window_len u32, every column walked in `walks` interleaved walks (pp_column);
//          positions past window_len dropped, as the kernel drops them
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bs_pos.h"

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

// The accumulated hit word of level e (bit clear: hit).
template <int K>
uint32_t level(const bs::State<K>& s, int e) {
    return e == 0 ? s.a0 : e == 1 ? s.a1 : s.a2;
}
template <int K, int R>
uint32_t level(const bs::StateR<K, R>& s, int e) {
    return s.a[e];
}

template <int K, class S>
void run(uint32_t E, const std::vector<uint64_t>& kmers, const Windows& wins, std::vector<int32_t>& out) {
    for (size_t b0 = 0; b0 < kmers.size(); b0 += 32) {
        uint32_t nE[5][K];
        eq_table<K>(kmers, b0, nE);
        for (size_t wi = 0; wi < wins.size(); ++wi) {
            const auto& w = wins[wi];
            S s;
            bs::init<K>(s);
            bs::PosPlanes ps;
            bs::pos_clear(ps);
            const uint32_t nq = ((uint32_t)w.size() + 3u) >> 2;
            for (uint32_t q = 0; q < nq; ++q) {
                for (uint32_t b = 0; b < 4u; ++b) {
                    const size_t j = 4u * q + b;
                    bs::advance<K>(s, nE[j < w.size() ? w[j] : 4]);
                    bs::pos_base(ps, bs::hits_new(s, E), b);
                }
                bs::pos_block(ps, q);
            }
            const uint32_t hit = ~level(s, (int)E);
            uint32_t stored[bs::POS_PLANES];
            for (int b = 0; b < bs::POS_PLANES; ++b) stored[b] = ps.p[b] & hit;
            for (uint32_t j = 0; j < 32 && b0 + j < kmers.size(); ++j) {
                int32_t d = -1;
                for (int e = (int)E; e >= 0; --e)
                    if (!(level(s, e) >> j & 1u)) d = e;
                int32_t* o = &out[2 * (wi * kmers.size() + b0 + j)];
                o[0] = d;
                o[1] = (hit >> j & 1u) ? (int32_t)bs::pos_get(stored, j) + 1 : (bs::pos_get(stored, j) ? -2 : 0);
            }
        }
    }
}

int run_pos(uint32_t E, Reader& in, FILE* out) {
    const uint32_t k = in.get<uint32_t>(), nk = in.get<uint32_t>(), nw = in.get<uint32_t>();
    if (in.bad || nk > in.buf.size() || nw > in.buf.size()) return 2;
    std::vector<uint64_t> kmers(nk);
    for (auto& v : kmers) v = in.get<uint64_t>();
    Windows wins(nw);
    for (auto& w : wins) {
        const uint32_t len = in.get<uint32_t>();
        if (in.bad || len < 1 || len > 256 || len > in.buf.size() - in.at) return 2;
        w.assign(in.buf.begin() + in.at, in.buf.begin() + in.at + len);
        in.at += len;
        for (unsigned char c : w)
            if (c > 4) return 2;
    }
    if (in.bad || in.at != in.buf.size()) return 2;
    std::vector<int32_t> res(2 * (size_t)nk * nw, 0);
    bool done = false;
#define AC_BS_RUN(KK)                                                   \
    if (k == KK) {                                                      \
        if (E == 3u) run<KK, bs::StateR<KK, 4>>(E, kmers, wins, res);   \
        else run<KK, bs::State<KK>>(E, kmers, wins, res);               \
        done = true;                                                    \
    }
    AC_BS_K_LIST(AC_BS_RUN)
#undef AC_BS_RUN
    if (!done) return 3;  // not an instantiated pattern length
    std::fwrite(res.data(), sizeof(int32_t), res.size(), out);
    return 0;
}

int run_profile(Reader& in, FILE* out) {
    const uint32_t nk = in.get<uint32_t>(), nw = in.get<uint32_t>(), lv = in.get<uint32_t>(), L = in.get<uint32_t>(),
                   walks = in.get<uint32_t>();
    if (in.bad || !nk || lv < 1 || lv > 4 || L < 1 || L > 256 || !walks) return 2;
    const size_t words = ((size_t)nk + 31) / 32;
    if ((in.buf.size() - in.at) != sizeof(uint32_t) * (lv + (size_t)bs::POS_PLANES) * nw * words) return 2;
    std::vector<uint32_t> hits((size_t)lv * nw * words), pos((size_t)bs::POS_PLANES * nw * words);
    for (auto& v : hits) v = in.get<uint32_t>();
    for (auto& v : pos) v = in.get<uint32_t>();
    std::vector<uint32_t> prof((size_t)lv * nk * L, 0u);
    for (uint32_t d = 0; d < lv; ++d)
        for (uint32_t col = 0; col < words; ++col)
            for (uint32_t t = 0; t < walks; ++t)
                bs::pp_column(hits.data(), pos.data(), nk, nw, d, col, t, nw, walks, [&](uint32_t j, uint32_t p) {
                    if (p < L) ++prof[((size_t)d * nk + 32u * col + j) * L + p];
                });
    std::fwrite(prof.data(), sizeof(uint32_t), prof.size(), out);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const bool pos = argc == 5 && !std::strcmp(argv[1], "pos");
    const bool profile = argc == 4 && !std::strcmp(argv[1], "profile");
    if (!pos && !profile) {
        std::fprintf(stderr, "usage: bs_pos_check pos E IN OUT | profile IN OUT\n");
        return 2;
    }
    const unsigned long E = pos ? std::strtoul(argv[2], nullptr, 10) : 0;
    if (E > 3) return 2;
    Reader in;
    in.buf = slurp(argv[argc - 2]);
    FILE* out = std::fopen(argv[argc - 1], "wb");
    if (!out) return 2;
    const int rc = pos ? run_pos((uint32_t)E, in, out) : run_profile(in, out);
    std::fclose(out);
    return rc;
}
