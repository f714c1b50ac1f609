// hit_flank_check -- runs the host build of the flank-profile code (approx_counter_amd/csrc/hit_flank.h: the
// hit word's walk fl_word_mask / fl_word and the per-pair step fl_pair over fl_run, what hit_flank.hip's kernel
// runs, and the per-base fl_sym) on a case read from a file, for tests/test_flanks_cpu.py (host-only; built
// there with the sanitizers on).
//   hit_flank_check IN OUT
//     IN : u32 n_kmers, n_windows, window_len (1..256), depth (1..32), with_start (0 / 1); n_windows x
//          window_len bases as bytes (0-3 = A C G T, 4 = N); the hit plane (n_windows x words u32); the
//          position matrix (8 x n_windows x words u32); with_start: the start matrix (the same shape).  The
//          planes may hold anything.
//     OUT: the flank profile, 2 x n_kmers x depth x 5 u32
// Every pair is computed three times: by fl_pair over the whole image (windows at ceil32(window_len)-base
// strides, the padding between them all N with code 3), by fl_pair over a copy of the window alone in buffers
// of exactly its own words, so that the sanitizer sees a read past the window's last word, and base by base
// with fl_sym over that copy.  The three must agree (exit status 4).  All buffers the walk reads or writes have
// exactly their size.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hit_flank.h"

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

void pack(const unsigned char* bases, uint32_t L, uint32_t* codes, uint32_t* nmask) {
    for (uint32_t b = 0; b < L; ++b) {
        if (bases[b] < 4) codes[b >> 4] |= (uint32_t)bases[b] << (2 * (b & 15));
        else nmask[b >> 5] |= 1u << (b & 31);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: hit_flank_check IN OUT\n");
        return 2;
    }
    const std::vector<unsigned char> buf = slurp(argv[1]);
    uint32_t hd[5];
    if (buf.size() < sizeof hd) return 2;
    std::memcpy(hd, buf.data(), sizeof hd);
    const uint32_t nk = hd[0], nw = hd[1], L = hd[2], D = hd[3], with_start = hd[4];
    if (!nk || !nw || L < 1 || L > 256 || D < 1 || D > bs::FL_MAX_DEPTH || with_start > 1) return 2;
    const size_t words = ((size_t)nk + 31) / 32, plane = (size_t)nw * words;
    const size_t mats = (size_t)bs::POS_PLANES * (1 + with_start);
    const size_t need = sizeof hd + (size_t)nw * L + 4 * (1 + mats) * plane;
    if (buf.size() != need) return 2;
    size_t at = sizeof hd;
    const unsigned char* bases = buf.data() + at;
    at += (size_t)nw * L;
    for (size_t i = 0; i < (size_t)nw * L; ++i)
        if (bases[i] > 4) return 2;
    std::vector<uint32_t> hit(plane), pos((size_t)bs::POS_PLANES * plane), start(with_start ? pos.size() : 0);
    std::memcpy(hit.data(), buf.data() + at, 4 * hit.size());
    at += 4 * hit.size();
    std::memcpy(pos.data(), buf.data() + at, 4 * pos.size());
    at += 4 * pos.size();
    if (with_start) std::memcpy(start.data(), buf.data() + at, 4 * start.size());

    // the image: padding bases are N with code 3, so a step that read one would count what it should not
    const uint64_t stride = ((uint64_t)L + 31u) & ~31ull;
    std::vector<uint32_t> codes((size_t)(nw * stride / 16), ~0u), nmask((size_t)(nw * stride / 32), ~0u);
    for (uint32_t w = 0; w < nw; ++w) {
        for (uint32_t b = 0; b < L; ++b) {
            const uint64_t g = w * stride + b;
            codes[g >> 4] &= ~(3u << (2 * (g & 15)));
            nmask[g >> 5] &= ~(1u << (g & 31));
        }
        pack(bases + (size_t)w * L, L, codes.data() + w * stride / 16, nmask.data() + w * stride / 32);
    }
    std::vector<uint32_t> out((size_t)bs::fl_words(nk, D), 0u), own(out.size(), 0u), plain(out.size(), 0u);
    const uint32_t* sp = with_start ? start.data() : nullptr;
    for (uint32_t w = 0; w < nw; ++w) {
        std::vector<uint32_t> own_c((L + 15) / 16, 0u), own_n((L + 31) / 32, 0u);
        pack(bases + (size_t)w * L, L, own_c.data(), own_n.data());
        for (uint32_t col = 0; col < words; ++col) {
            const uint32_t m = bs::fl_word_mask(hit.data(), nk, w, col);
            bs::fl_word(pos.data(), sp, nk, nw, w, col, m, [&](uint32_t j, uint32_t p, uint32_t s) {
                const size_t c = 32u * (size_t)col + j;
                bs::fl_pair(codes.data(), nmask.data(), w * stride, L, D, p, s, with_start != 0,
                            [&](uint32_t side, uint32_t jj, uint32_t sym) { ++out.at(((side * (size_t)nk + c) * D + jj) * 5 + sym); });
                bs::fl_pair(own_c.data(), own_n.data(), 0, L, D, p, s, with_start != 0,
                            [&](uint32_t side, uint32_t jj, uint32_t sym) { ++own.at(((side * (size_t)nk + c) * D + jj) * 5 + sym); });
                if (p > L || (with_start && s >= p)) return;
                for (uint32_t jj = 0; jj < D; ++jj) {
                    if (p + jj < L) ++plain.at(((0 * (size_t)nk + c) * D + jj) * 5 + bs::fl_sym(own_c.data(), own_n.data(), 0, p + jj));
                    if (with_start && s >= jj + 1u)
                        ++plain.at(((1 * (size_t)nk + c) * D + jj) * 5 + bs::fl_sym(own_c.data(), own_n.data(), 0, s - 1u - jj));
                }
            });
        }
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), sizeof(uint32_t), out.size(), f);
    std::fclose(f);
    return out == own && out == plain ? 0 : 4;
}
