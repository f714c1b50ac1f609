// hit_cooc_check -- runs the co-occurrence arithmetic (approx_counter_amd/csrc/hit_cooc.h: the code of
// hit_cooc.hip's kernels) on the host, for tests/test_cooc_cpu.py (built there with the sanitizers on).
//   hit_cooc_check cooc IN OUT
//     IN:  u32 n_kmers, n_windows, levels, then levels x n_windows x ceil(n_kmers / 32) u32 (the matrix as
//          ac_window_hits_* lay it out; stray bits past n_kmers allowed)
//     OUT: u32 rows, t_words, then T[levels][rows][t_words] (the transposed planes, as the transposition
//          kernel stores them: co_load_word, co_transpose32), then cooc[levels][n_kmers][n_kmers] (the
//          product kernel's walk: tile pairs by co_pair, slabs in co_splits' chunks, co_dot per thread's
//          4 x 4 block, the mirror image of an off-diagonal tile), then window_counts[levels][n_windows]
//          (co_word_count)
//   hit_cooc_check rule N_KMERS N_WINDOWS LEVELS
//     prints "<splits> <slabs per workgroup> <slabs> <tile pairs>" of the product's launch rule
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hit_cooc.h"

using namespace acamd::bs;

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "rule")) {
        const uint64_t nk = std::strtoull(argv[2], nullptr, 10), nw = std::strtoull(argv[3], nullptr, 10);
        const uint32_t lv = (uint32_t)std::strtoul(argv[4], nullptr, 10);
        const CoSplit sp = co_splits(nk, nw, lv);
        std::printf("%u %u %llu %llu\n", sp.splits, sp.per, (unsigned long long)(co_t_words(nw) / CO_SLAB),
                    (unsigned long long)co_pairs((nk + CO_TILE - 1u) / CO_TILE));
        return 0;
    }
    if (argc != 4 || std::strcmp(argv[1], "cooc")) {
        std::fprintf(stderr, "usage: hit_cooc_check cooc IN OUT | rule N_KMERS N_WINDOWS LEVELS\n");
        return 2;
    }
    FILE* in = std::fopen(argv[2], "rb");
    uint32_t h[3];
    if (!in || std::fread(h, 4, 3, in) != 3) return 2;
    const uint32_t n = h[0], nw = h[1], levels = h[2], words = (n + 31u) / 32u;
    std::vector<uint32_t> m((size_t)levels * nw * words);
    if (std::fread(m.data(), 4, m.size(), in) != m.size()) return 2;
    std::fclose(in);
    const uint64_t rows = co_t_rows(n), tw = co_t_words(nw);
    std::vector<uint32_t> T((size_t)(levels * rows * tw), 0xFFFFFFFFu);
    std::vector<uint32_t> cooc((size_t)levels * n * n, 0xFFFFFFFFu), wc((size_t)levels * nw, 0xFFFFFFFFu);
    // the transposition: one 32 x 32 block per (word column, block of 32 windows), every word of T once
    for (uint32_t e = 0; e < levels; ++e) {
        const uint32_t* plane = m.data() + (size_t)e * nw * words;
        for (uint32_t c = 0; c < words; ++c)
            for (uint64_t b = 0; b < tw; ++b) {
                uint32_t a[32];
                for (uint32_t i = 0; i < 32u; ++i) a[i] = co_load_word(plane, words, n, nw, 32u * b + i, c);
                co_transpose32(a);
                for (uint32_t j = 0; j < 32u; ++j) T[(size_t)((e * rows + 32u * c + j) * tw + b)] = a[j];
            }
        for (uint32_t w = 0; w < nw; ++w) {
            uint32_t s = 0;
            for (uint32_t c = 0; c < words; ++c) s += co_word_count(plane[(size_t)w * words + c], c, n);
            wc[(size_t)e * nw + w] = s;
        }
    }
    // the product: the workgroups' walk, split or not as the launch rule says
    const CoSplit sp = co_splits(n, nw, levels);
    const uint32_t tiles = (n + CO_TILE - 1u) / CO_TILE, slabs = (uint32_t)(tw / CO_SLAB);
    if (sp.splits > 1u) std::fill(cooc.begin(), cooc.end(), 0u);
    auto put = [&](uint64_t at, uint32_t v) {
        if (sp.splits > 1u) cooc[(size_t)at] += v;
        else cooc[(size_t)at] = v;
    };
    for (uint32_t e = 0; e < levels; ++e)
        for (uint32_t p = 0; p < (uint32_t)co_pairs(tiles); ++p)
            for (uint32_t y = 0; y < sp.splits; ++y) {
                uint32_t ta, tb;
                co_pair(p, ta, tb);
                if (ta > tb || tb >= tiles) return 3;
                const uint32_t s0 = y * sp.per, s1 = s0 + sp.per < slabs ? s0 + sp.per : slabs;
                for (uint32_t ty = 0; ty < 16u; ++ty)
                    for (uint32_t tx = 0; tx < 16u; ++tx) {
                        uint32_t acc[CO_ACC][CO_ACC] = {};
                        for (uint64_t x = (uint64_t)s0 * CO_SLAB; x < (uint64_t)s1 * CO_SLAB; ++x) {
                            uint32_t a[CO_ACC], b[CO_ACC];
                            for (int i = 0; i < CO_ACC; ++i) {
                                const uint64_t ra = (uint64_t)ta * CO_TILE + ty + 16u * i, rb = (uint64_t)tb * CO_TILE + tx + 16u * i;
                                a[i] = ra < rows ? T[(size_t)((e * rows + ra) * tw + x)] : 0u;
                                b[i] = rb < rows ? T[(size_t)((e * rows + rb) * tw + x)] : 0u;
                            }
                            co_dot(acc, a, b);
                        }
                        for (int i = 0; i < CO_ACC; ++i)
                            for (int j = 0; j < CO_ACC; ++j) {
                                const uint64_t a = (uint64_t)ta * CO_TILE + ty + 16u * i, b = (uint64_t)tb * CO_TILE + tx + 16u * j;
                                if (a >= n || b >= n) continue;
                                put(((uint64_t)e * n + a) * n + b, acc[i][j]);
                                if (ta != tb) put(((uint64_t)e * n + b) * n + a, acc[i][j]);
                            }
                    }
            }
    FILE* o = std::fopen(argv[3], "wb");
    const uint32_t head[2] = {(uint32_t)rows, (uint32_t)tw};
    bool ok = o && std::fwrite(head, 4, 2, o) == 2;
    ok = ok && std::fwrite(T.data(), 4, T.size(), o) == T.size();
    ok = ok && std::fwrite(cooc.data(), 4, cooc.size(), o) == cooc.size();
    ok = ok && std::fwrite(wc.data(), 4, wc.size(), o) == wc.size();
    if (!ok || std::fclose(o)) return 2;
    return 0;
}
