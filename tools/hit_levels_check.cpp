// hit_levels_check -- runs the hit matrix's column counter (approx_counter_amd/csrc/hit_levels.h: the code of
// bsh_count.hip's hit_level_counts_kernel) on the host, for tests/test_hits_cpu.py (built there with the
// sanitizers on).
//   hit_levels_check count IN OUT
//     IN:  u32 n_kmers, n_windows, levels, slab, then levels x n_windows x ceil(n_kmers / 32) u32 (the
//          matrix as ac_window_hits_* lay it out)
//     OUT: u32 HC_PLANES, HC_WINDOWS, then level_counts[levels][n_kmers]; every column is counted in `slab`
//          interleaved walks of stride `slab`, as the kernel's waves walk theirs
//   hit_levels_check raw N WORD
//     N adds of WORD (hex) into one HCount WITHOUT a flush; prints "<hc_full> <count of bit 0> <count of bit 31>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hit_levels.h"

using namespace acamd::bs;

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "raw")) {
        HCount v;
        hc_clear(v);
        const uint32_t n = (uint32_t)std::strtoul(argv[2], nullptr, 10), w = (uint32_t)std::strtoul(argv[3], nullptr, 16);
        for (uint32_t i = 0; i < n; ++i) hc_add(v, w);
        std::printf("%d %u %u\n", hc_full(v) ? 1 : 0, hc_get(v, 0), hc_get(v, 31));
        return 0;
    }
    if (argc != 4 || std::strcmp(argv[1], "count")) {
        std::fprintf(stderr, "usage: hit_levels_check count IN OUT | raw N WORD\n");
        return 2;
    }
    FILE* in = std::fopen(argv[2], "rb");
    uint32_t h[4];
    if (!in || std::fread(h, 4, 4, in) != 4 || !h[3]) return 2;
    const uint32_t n_kmers = h[0], n_windows = h[1], levels = h[2], slab = h[3], words = (n_kmers + 31u) / 32u;
    std::vector<uint32_t> m((size_t)levels * n_windows * words);
    if (std::fread(m.data(), 4, m.size(), in) != m.size()) return 2;
    std::fclose(in);
    std::vector<uint32_t> out{(uint32_t)HC_PLANES, HC_WINDOWS};
    out.resize(2 + (size_t)levels * n_kmers, 0u);
    for (uint32_t e = 0; e < levels; ++e)
        for (uint32_t col = 0; col < words; ++col) {
            uint32_t cnt[32] = {};
            // `slab` interleaved walks of the column (windows s, s + slab, ..), as the kernel's waves walk theirs
            for (uint32_t s0 = 0; s0 < slab && s0 < n_windows; ++s0)
                hc_column(m.data() + (size_t)e * n_windows * words, words, col, s0, n_windows, slab, cnt);
            for (uint32_t j = 0; j < 32u && 32u * col + j < n_kmers; ++j) out[2 + (size_t)e * n_kmers + 32u * col + j] = cnt[j];
        }
    FILE* o = std::fopen(argv[3], "wb");
    if (!o || std::fwrite(out.data(), 4, out.size(), o) != out.size()) return 2;
    std::fclose(o);
    return 0;
}
