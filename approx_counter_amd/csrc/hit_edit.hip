// hit_edit.hip -- edit profiles (DESIGN.md §4e "Edit profiles"): per k-mer and base the histogram of what the
// best occurrence holds there -- the base, another base, nothing, or an inserted base after it -- hit_edit.h's
// furthest-reaching alignment and traceback over the hit pairs of one level plane.  A reduction over resident
// matrices like the span and flank passes; a translation unit of its own: the count kernels' device compiles
// stay what they were.
//
// The mapping is the flank pass's (hit_flank.hip).  The output is keyed by k-mer, so a workgroup owns one word
// column (32 k-mers) and a strip of windows, and keeps the column's histogram -- 32 k-mers x k x 12 u32, a
// k-mer's row padded to an odd number of words, sized by the launch for its k (dynamic LDS) -- in LDS.  The
// strip is walked in chunks of EP_CHUNK windows: one lane per hit word of the chunk reads it, claims popcount
// entries of an LDS work list with one LDS atomic add and appends its set bits there (fl_word: word, bit,
// pos - 1 and start from the sixteen planes); all lanes then take list entries densely and run ep_pair, which
// reports the pair's edits: every edit one LDS atomic add, and one more a counted pair into the row's pad word,
// the k-mer's pairs.  A match is never added: every counted pair gives every base exactly one of the
// operations 0..6, so the flush writes match = pairs - (operations 1..6).  No global atomic per observation:
// the histogram is flushed once per workgroup, its non-zero cells added onto the output, which the launch zeroes
// on the stream first.  The sums do not depend on the claims' order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hit_edit.h"
#include "wm_count.h"

namespace acamd {

using namespace bs;

constexpr uint32_t EP_CHUNK = 128u;   // windows of a chunk: one scanning lane each; also the entry's word field
constexpr uint32_t EP_THREADS = 256u;
constexpr uint32_t EP_BLOCKS = 1024u;       // workgroups a launch aims at: the strips are cut to give about these
constexpr uint32_t EP_MAX_STRIPS = 65535u;  // (grid y)
// A k-mer's row of the LDS histogram: k x 12 words and one more, the k-mer's counted pairs, which also makes the
// row odd, so that the lanes of one LDS add -- the same base and operation of different k-mers -- fall into
// different banks.
constexpr uint32_t ep_row(uint32_t k) { return (k * EP_OPS) | 1u; }
constexpr uint32_t ep_hist_bytes(uint32_t k) { return 4u * 32u * ep_row(k); }
static_assert(EP_CHUNK <= EP_THREADS && EP_CHUNK <= 1u << 9, "one scanning lane per word; 9 bits of an entry");
static_assert(4u * 32u * EP_CHUNK + ep_hist_bytes(EP_MAX_K) + 16u <= 80u * 1024u,
              "the work list and the largest histogram: half a CU's LDS");

__global__ __launch_bounds__(EP_THREADS) void hit_edit_profile_kernel(uint32_t k, const uint64_t* kmers, uint32_t n_kmers,
                                                                     const uint32_t* codes, const uint32_t* nmask,
                                                                     uint32_t n_windows, uint32_t window_len,
                                                                     const uint32_t* hit, const uint32_t* pos,
                                                                     const uint32_t* start, uint64_t strip, uint32_t* edit) {
    extern __shared__ uint32_t hist[];          // c * ep_row(k) + i * 12 + op (op 0 unused); + k * 12: the pairs
    __shared__ uint32_t list[EP_CHUNK * 32u];   // lane | bit << 9 | (pos - 1) << 14 | start << 22
    __shared__ uint32_t n_list;
    const uint32_t tid = threadIdx.x;
    const uint64_t stride = ((uint64_t)window_len + 31u) & ~31ull;
    const uint32_t col = blockIdx.x;
    const uint64_t w_lo = blockIdx.y * strip, w_hi = std::min<uint64_t>(n_windows, w_lo + strip);
    const uint32_t row = k * EP_OPS, lrow = ep_row(k), cells = 32u * lrow;
    for (uint32_t i = tid; i < cells; i += EP_THREADS) hist[i] = 0u;
    for (uint64_t wc = w_lo; wc < w_hi; wc += EP_CHUNK) {
        if (tid == 0u) n_list = 0u;
        __syncthreads();  // (and the histogram's zeroes)
        if (tid < EP_CHUNK && wc + tid < w_hi) {
            const uint64_t w = wc + tid;
            const uint32_t m = fl_word_mask(hit, n_kmers, w, col);
            if (m) {
                uint32_t at = atomicAdd(&n_list, (uint32_t)__builtin_popcount(m));
                fl_word(pos, start, n_kmers, n_windows, w, col, m,
                        [&](uint32_t j, uint32_t p, uint32_t s) { list[at++] = tid | j << 9 | (p - 1u) << 14 | s << 22; });
            }
        }
        __syncthreads();
        const uint32_t n = n_list;  // (<= 32 EP_CHUNK: every claim is a word's popcount)
        for (uint32_t i = tid; i < n; i += EP_THREADS) {
            const uint32_t e = list[i], lane = e & 511u, j = e >> 9 & 31u, p = (e >> 14 & 255u) + 1u, s = e >> 22 & 255u;
            // (32 col + j < n_kmers: fl_word_mask dropped the others)
            if (ep_pair(kmers[32ull * col + j], k, codes, nmask, (wc + lane) * stride, window_len, p, s,
                        [&](uint32_t base, uint32_t op) { atomicAdd(&hist[j * lrow + base * EP_OPS + op], 1u); }))
                atomicAdd(&hist[j * lrow + row], 1u);
        }
        __syncthreads();  // (the next chunk clears the count these lanes read; the flush reads every lane's adds)
    }
    for (uint32_t i = tid; i < cells; i += EP_THREADS) {
        const uint32_t c = i / lrow, r = i % lrow;
        if (r == row) continue;  // (the pairs: no cell of the output)
        uint32_t v = hist[i];
        if (r % EP_OPS == EP_MATCH) {  // the pairs that neither substituted nor deleted this base
            v = hist[c * lrow + row];
            for (uint32_t op = EP_SUB; op <= EP_DEL; ++op) v -= hist[i + op];
        }
        // (32 col + c < n_kmers: fl_word_mask dropped the others, their cells stayed 0)
        if (v) atomicAdd(&edit[(32ull * col + c) * row + r], v);
    }
}

hipError_t launch_hit_edit_profile(uint32_t k, const uint64_t* kmers, uint32_t n_kmers, const uint32_t* codes,
                                   const uint32_t* nmask, uint32_t n_windows, uint32_t window_len, const uint32_t* hit,
                                   const uint32_t* pos, const uint32_t* start, uint32_t* edit, hipStream_t stream) {
    if (!n_kmers) return hipSuccess;
    if (hipError_t e = hipMemsetAsync(edit, 0, sizeof(uint32_t) * ep_words(n_kmers, k), stream)) return e;
    if (!n_windows) return hipSuccess;
    const uint64_t words = ((uint64_t)n_kmers + 31u) >> 5;  // (<= 2^27: grid x)
    const uint64_t chunks = ((uint64_t)n_windows + EP_CHUNK - 1u) / EP_CHUNK;
    // about EP_BLOCKS workgroups: whole chunks to a strip, at most EP_MAX_STRIPS strips
    const uint64_t want = std::min<uint64_t>(std::min<uint64_t>(chunks, std::max<uint64_t>(EP_BLOCKS / words, 1u)), EP_MAX_STRIPS);
    const uint64_t strip = (chunks + want - 1u) / want * EP_CHUNK;
    const uint64_t strips = ((uint64_t)n_windows + strip - 1u) / strip;
    // (at most 49,280 bytes of dynamic LDS beside the 16 KiB list: a workgroup may hold up to a CU's 160 KiB)
    hipLaunchKernelGGL(hit_edit_profile_kernel, dim3((uint32_t)words, (uint32_t)strips), dim3(EP_THREADS), ep_hist_bytes(k), stream,
                       k, kmers, n_kmers, codes, nmask, n_windows, window_len, hit, pos, start, strip, edit);
    return hipGetLastError();
}

}  // namespace acamd
