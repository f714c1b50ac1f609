// hit_span_check -- runs the host build of the match-span code (approx_counter_amd/csrc/hit_span.h: the
// per-pair step sp_span and the hit word's walk sp_word_mask / sp_word / sp_put, what hit_span.hip's kernel
// runs) on a case read from a file, for tests/test_spans_cpu.py (host-only; built there with the sanitizers
// on).
//   hit_span_check IN OUT
//     IN : u32 k, n_kmers, n_windows, levels (1..4), window_len (1..256); n_kmers u64 k-mers (2 bits per
//          base, first base highest); n_windows x window_len bases as bytes (0-3 = A C G T, 4 = N); the hit
//          matrix (levels x n_windows x words u32); the position matrix (8 x n_windows x words u32).  The
//          planes may hold anything.
//     OUT: the start matrix, 8 x n_windows x words u32
// Every pair is computed twice: over the whole image (windows at ceil32(window_len)-base strides, the padding
// between them all N with code 3) and over a copy of the window alone in buffers of exactly its own words, so
// that the sanitizer sees a read past the window's last word.  The two must agree (exit status 4).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hit_span.h"

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
        std::fprintf(stderr, "usage: hit_span_check IN OUT\n");
        return 2;
    }
    const std::vector<unsigned char> buf = slurp(argv[1]);
    uint32_t hd[5];
    if (buf.size() < sizeof hd) return 2;
    std::memcpy(hd, buf.data(), sizeof hd);
    const uint32_t k = hd[0], nk = hd[1], nw = hd[2], levels = hd[3], L = hd[4];
    if (k < 2 || k > 32 || !nk || !nw || levels < 1 || levels > 4 || levels >= k || L < 1 || L > 256) return 2;
    const size_t words = ((size_t)nk + 31) / 32, plane = (size_t)nw * words;
    const size_t need = sizeof hd + 8 * (size_t)nk + (size_t)nw * L + 4 * (levels + (size_t)bs::POS_PLANES) * plane;
    if (buf.size() != need) return 2;
    size_t at = sizeof hd;
    std::vector<uint64_t> kmers(nk);
    std::memcpy(kmers.data(), buf.data() + at, 8 * (size_t)nk);
    at += 8 * (size_t)nk;
    const unsigned char* bases = buf.data() + at;
    at += (size_t)nw * L;
    for (size_t i = 0; i < (size_t)nw * L; ++i)
        if (bases[i] > 4) return 2;
    std::vector<uint32_t> hits((size_t)levels * plane), pos((size_t)bs::POS_PLANES * plane);
    std::memcpy(hits.data(), buf.data() + at, 4 * hits.size());
    at += 4 * hits.size();
    std::memcpy(pos.data(), buf.data() + at, 4 * pos.size());

    // the image: padding bases are N with code 3, so a step that read one would not match what it should
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
    std::vector<uint32_t> out((size_t)bs::POS_PLANES * plane, 0u);
    int rc = 0;
    for (uint32_t w = 0; w < nw; ++w) {
        std::vector<uint32_t> own_c((L + 15) / 16, 0u), own_n((L + 31) / 32, 0u);
        pack(bases + (size_t)w * L, L, own_c.data(), own_n.data());
        for (uint32_t col = 0; col < words; ++col) {
            const uint32_t m = bs::sp_word_mask(hits.data(), nk, nw, levels, w, col);
            bs::sp_word(hits.data(), pos.data(), nk, nw, levels, w, col, m, [&](uint32_t j, uint32_t p, uint32_t d) {
                const uint64_t km = kmers[32u * col + j];
                const uint32_t len = bs::sp_span(km, k, codes.data(), nmask.data(), w * stride, L, p, d);
                if (len != bs::sp_span(km, k, own_c.data(), own_n.data(), 0, L, p, d)) rc = 4;
                if (len != bs::SP_NONE)
                    bs::sp_put(p - len, j, [&](uint32_t b, uint32_t bit) { out[(size_t)b * plane + w * words + col] |= bit; });
            });
        }
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), sizeof(uint32_t), out.size(), f);
    std::fclose(f);
    return rc;
}
