// hit_cross_check -- runs the cross co-occurrence arithmetic (approx_counter_amd/csrc/hit_cross.h over
// hit_cooc.h: the code of hit_cross.hip's kernel) on the host, for tests/test_cross_cpu.py (built there with
// the sanitizers on).
//   hit_cross_check cross IN OUT
//     IN:  u32 n_a, n_b, n_windows, levels, then A: levels x n_windows x ceil(n_a / 32) u32, then B: levels x
//          n_windows x ceil(n_b / 32) u32 (the matrices as ac_window_hits_* lay them out; stray bits allowed)
//     OUT: cross[levels][n_a][n_b]: both matrices transposed as the transposition kernel stores them
//          (co_load_word, co_transpose32), then the product kernel's walk: the tiles of the full grid by
//          cx_tile, slabs in cx_splits' chunks, cx_thread_sums per thread's 4 x 4 block, stores guarded by
//          a < n_a && b < n_b -- stored once when the rule does not split, added into zeros when it does
//   hit_cross_check rule N_A N_B N_WINDOWS LEVELS
//     prints "<splits> <slabs per workgroup> <slabs> <tiles>" of the product's launch rule
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hit_cross.h"

using namespace acamd::bs;

static std::vector<uint32_t> transposed(const std::vector<uint32_t>& m, uint32_t n, uint32_t nw, uint32_t levels) {
    const uint32_t words = (n + 31u) / 32u;
    const uint64_t rows = co_t_rows(n), tw = co_t_words(nw);
    std::vector<uint32_t> T((size_t)(levels * rows * tw), 0xFFFFFFFFu);
    for (uint32_t e = 0; e < levels; ++e) {
        const uint32_t* plane = m.data() + (size_t)e * nw * words;
        for (uint32_t c = 0; c < words; ++c)
            for (uint64_t b = 0; b < tw; ++b) {
                uint32_t a[32];
                for (uint32_t i = 0; i < 32u; ++i) a[i] = co_load_word(plane, words, n, nw, 32u * b + i, c);
                co_transpose32(a);
                for (uint32_t j = 0; j < 32u; ++j) T[(size_t)((e * rows + 32u * c + j) * tw + b)] = a[j];
            }
    }
    return T;
}

int main(int argc, char** argv) {
    if (argc == 6 && !std::strcmp(argv[1], "rule")) {
        const uint64_t na = std::strtoull(argv[2], nullptr, 10), nb = std::strtoull(argv[3], nullptr, 10);
        const uint64_t nw = std::strtoull(argv[4], nullptr, 10);
        const uint32_t lv = (uint32_t)std::strtoul(argv[5], nullptr, 10);
        const CoSplit sp = cx_splits(na, nb, nw, lv);
        std::printf("%u %u %llu %llu\n", sp.splits, sp.per, (unsigned long long)(co_t_words(nw) / CO_SLAB),
                    (unsigned long long)(cx_tiles(na) * cx_tiles(nb)));
        return 0;
    }
    if (argc != 4 || std::strcmp(argv[1], "cross")) {
        std::fprintf(stderr, "usage: hit_cross_check cross IN OUT | rule N_A N_B N_WINDOWS LEVELS\n");
        return 2;
    }
    FILE* in = std::fopen(argv[2], "rb");
    uint32_t h[4];
    if (!in || std::fread(h, 4, 4, in) != 4) return 2;
    const uint32_t na = h[0], nb = h[1], nw = h[2], levels = h[3];
    std::vector<uint32_t> ma((size_t)levels * nw * ((na + 31u) / 32u)), mb((size_t)levels * nw * ((nb + 31u) / 32u));
    if (std::fread(ma.data(), 4, ma.size(), in) != ma.size() || std::fread(mb.data(), 4, mb.size(), in) != mb.size()) return 2;
    std::fclose(in);
    const uint64_t rows_a = co_t_rows(na), rows_b = co_t_rows(nb), tw = co_t_words(nw);
    const std::vector<uint32_t> Ta = transposed(ma, na, nw, levels), Tb = transposed(mb, nb, nw, levels);
    std::vector<uint32_t> cross((size_t)levels * na * nb, 0xFFFFFFFFu);
    const CoSplit sp = cx_splits(na, nb, nw, levels);
    const uint32_t tiles_a = (uint32_t)cx_tiles(na), tiles_b = (uint32_t)cx_tiles(nb), slabs = (uint32_t)(tw / CO_SLAB);
    if (sp.splits > 1u) std::fill(cross.begin(), cross.end(), 0u);
    for (uint32_t e = 0; e < levels; ++e)
        for (uint32_t p = 0; p < tiles_a * tiles_b; ++p)
            for (uint32_t y = 0; y < sp.splits; ++y) {
                uint32_t ta, tb;
                cx_tile(p, tiles_a, ta, tb);
                if (ta >= tiles_a || tb >= tiles_b) return 3;
                const uint32_t s0 = y * sp.per, s1 = s0 + sp.per < slabs ? s0 + sp.per : slabs;
                for (uint32_t ty = 0; ty < 16u; ++ty)
                    for (uint32_t tx = 0; tx < 16u; ++tx) {
                        uint32_t acc[CO_ACC][CO_ACC] = {};
                        cx_thread_sums(acc, Ta.data() + (size_t)(e * rows_a * tw), rows_a, Tb.data() + (size_t)(e * rows_b * tw),
                                       rows_b, tw, ta, tb, ty, tx, (uint64_t)s0 * CO_SLAB, (uint64_t)s1 * CO_SLAB);
                        for (int i = 0; i < CO_ACC; ++i)
                            for (int j = 0; j < CO_ACC; ++j) {
                                const uint64_t a = (uint64_t)ta * CO_TILE + ty + 16u * i, b = (uint64_t)tb * CO_TILE + tx + 16u * j;
                                if (a >= na || b >= nb) continue;
                                uint32_t& out = cross[(size_t)(((uint64_t)e * na + a) * nb + b)];
                                if (sp.splits > 1u) out += acc[i][j];
                                else out = acc[i][j];
                            }
                    }
            }
    FILE* o = std::fopen(argv[3], "wb");
    bool ok = o && std::fwrite(cross.data(), 4, cross.size(), o) == cross.size();
    if (!ok || std::fclose(o)) return 2;
    return 0;
}
