// hit_edit_check -- runs the host build of the edit-profile code (approx_counter_amd/csrc/hit_edit.h: the
// per-pair furthest-reaching alignment and traceback ep_pair over ep_text, behind hit_flank.h's walk of the hit
// word, what hit_edit.hip's kernel runs) on a case read from a file, for tests/test_edits_cpu.py (host-only; built
// there with the sanitizers on).
//   hit_edit_check IN OUT
//     IN : u32 n_kmers, n_windows, window_len (1..256), k (2..32); n_kmers u64 k-mers (2 bits a base, the first
//          base highest); n_windows x window_len bases as bytes (0-3 = A C G T, 4 = N); the hit plane
//          (n_windows x words u32); the position matrix (8 x n_windows x words u32); the start matrix (the
//          same shape).  The planes may hold anything.
//     OUT: the edit profile, n_kmers x k x 12 u32
// Every pair is computed twice: by ep_pair over the whole image (windows at ceil32(window_len)-base strides,
// the padding between them all N with code 3) and by ep_pair over a copy of the window alone in buffers of
// exactly its own words, so that the sanitizer sees a read past the window's last word.  The two must agree
// (exit status 4).  ep_pair reports a pair's edits; the tool adds a match at every base of a counted pair that
// has none of the operations 1..6, as the kernel's flush does, and a base with two of them is an error (exit
// status 5).  All buffers the walk reads or writes have exactly their size.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hit_edit.h"

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
        std::fprintf(stderr, "usage: hit_edit_check IN OUT\n");
        return 2;
    }
    const std::vector<unsigned char> buf = slurp(argv[1]);
    uint32_t hd[4];
    if (buf.size() < sizeof hd) return 2;
    std::memcpy(hd, buf.data(), sizeof hd);
    const uint32_t nk = hd[0], nw = hd[1], L = hd[2], k = hd[3];
    if (!nk || !nw || L < 1 || L > 256 || k < bs::EP_MIN_K || k > bs::EP_MAX_K) return 2;
    const size_t words = ((size_t)nk + 31) / 32, plane = (size_t)nw * words;
    const size_t need = sizeof hd + 8 * (size_t)nk + (size_t)nw * L + 4 * (1 + 2 * (size_t)bs::POS_PLANES) * plane;
    if (buf.size() != need) return 2;
    size_t at = sizeof hd;
    std::vector<uint64_t> kmers(nk);
    std::memcpy(kmers.data(), buf.data() + at, 8 * (size_t)nk);
    at += 8 * (size_t)nk;
    const unsigned char* bases = buf.data() + at;
    at += (size_t)nw * L;
    for (size_t i = 0; i < (size_t)nw * L; ++i)
        if (bases[i] > 4) return 2;
    std::vector<uint32_t> hit(plane), pos((size_t)bs::POS_PLANES * plane), start(pos.size());
    std::memcpy(hit.data(), buf.data() + at, 4 * hit.size());
    at += 4 * hit.size();
    std::memcpy(pos.data(), buf.data() + at, 4 * pos.size());
    at += 4 * pos.size();
    std::memcpy(start.data(), buf.data() + at, 4 * start.size());

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
    std::vector<uint32_t> out((size_t)bs::ep_words(nk, k), 0u), own(out.size(), 0u);
    for (uint32_t w = 0; w < nw; ++w) {
        std::vector<uint32_t> own_c((L + 15) / 16, 0u), own_n((L + 31) / 32, 0u);
        pack(bases + (size_t)w * L, L, own_c.data(), own_n.data());
        for (uint32_t col = 0; col < words; ++col) {
            const uint32_t m = bs::fl_word_mask(hit.data(), nk, w, col);
            bs::fl_word(pos.data(), start.data(), nk, nw, w, col, m, [&](uint32_t j, uint32_t p, uint32_t s) {
                const size_t c = 32u * (size_t)col + j;
                // (ep_pair reports the edits; a counted pair's matches are what is left of its bases)
                auto run = [&](const uint32_t* cd, const uint32_t* nm, uint64_t base, std::vector<uint32_t>& into) {
                    std::vector<uint32_t> touched(k, 0u);
                    const bool counted = bs::ep_pair(kmers.at(c), k, cd, nm, base, L, p, s, [&](uint32_t i, uint32_t op) {
                        ++into.at((c * k + i) * bs::EP_OPS + op);
                        if (op <= bs::EP_DEL) ++touched.at(i);
                    });
                    for (uint32_t i = 0; i < k; ++i) {
                        if (touched[i] > (counted ? 1u : 0u)) std::exit(5);  // two of the operations 0..6 at one base
                        if (counted && !touched[i]) ++into.at((c * k + i) * bs::EP_OPS + bs::EP_MATCH);
                    }
                };
                run(codes.data(), nmask.data(), w * stride, out);
                run(own_c.data(), own_n.data(), 0, own);
            });
        }
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), sizeof(uint32_t), out.size(), f);
    std::fclose(f);
    return out == own ? 0 : 4;
}
