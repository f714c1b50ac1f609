// hit_span.hip -- match spans (DESIGN.md §4e "Match spans"): the start matrix of a hit matrix and its
// position matrix, hit_span.h's step over the hit pairs only.  A reduction over resident matrices like the
// level counts and the co-occurrence products; a translation unit of its own: the count kernels' device
// compiles stay what they were.
//
// The work follows the hits, not the pairs.  A workgroup takes a slab of SP_SLAB consecutive hit words of the
// top level plane (whole and partial windows alike: the planes are n_windows x words words, flat).  One lane
// per word reads it, claims popcount entries of an LDS work list with one LDS atomic add, and appends its set
// bits there (sp_word: word, bit, pos - 1 from the eight planes, d from the first level plane set).  All 256
// lanes then take list entries densely and run sp_span; each ORs its start bits into an LDS copy of the
// slab's output words, zeroed first, and the slab is stored plane by plane, consecutive lanes consecutive
// words: every word of the start matrix is written exactly once, with no global atomic.  The list's order
// depends on the claims' order; the OR does not.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hit_span.h"
#include "wm_count.h"

namespace acamd {

using namespace bs;

constexpr uint32_t SP_SLAB = 128u;     // hit words of a slab (7 bits of a list entry)
constexpr uint32_t SP_THREADS = 256u;
constexpr uint32_t SP_MAX_BLOCKS = 8192u;  // workgroups of a launch; the slabs past them by a grid stride
static_assert(SP_SLAB <= SP_THREADS && SP_SLAB == 1u << 7, "one scanning lane per word; the entry's word field");

__global__ __launch_bounds__(SP_THREADS) void hit_start_positions_kernel(uint32_t k, const uint64_t* kmers, uint32_t n_kmers,
                                                                        const uint32_t* codes, const uint32_t* nmask,
                                                                        uint32_t n_windows, uint32_t window_len,
                                                                        const uint32_t* hits, const uint32_t* pos,
                                                                        uint32_t levels, uint32_t* start) {
    __shared__ uint32_t list[SP_SLAB * 32u];           // word | bit << 7 | (pos - 1) << 12 | d << 20
    __shared__ uint32_t out[POS_PLANES * SP_SLAB];
    __shared__ uint32_t win[SP_SLAB];                  // the window of the slab's word
    __shared__ uint32_t n_list;
    const uint32_t tid = threadIdx.x;
    const uint64_t words = ((uint64_t)n_kmers + 31u) >> 5;
    const uint64_t plane = (uint64_t)n_windows * words;
    const uint64_t stride = ((uint64_t)window_len + 31u) & ~31ull;
    const uint64_t slabs = (plane + SP_SLAB - 1u) / SP_SLAB;
    for (uint64_t s = blockIdx.x; s < slabs; s += gridDim.x) {
        const uint64_t f0 = s * SP_SLAB;
        const uint32_t nf = (uint32_t)std::min<uint64_t>(SP_SLAB, plane - f0);
        if (tid == 0u) n_list = 0u;
        for (uint32_t i = tid; i < POS_PLANES * SP_SLAB; i += SP_THREADS) out[i] = 0u;
        __syncthreads();
        if (tid < nf) {
            const uint64_t w = (f0 + tid) / words;
            const uint32_t col = (uint32_t)(f0 + tid - w * words);
            win[tid] = (uint32_t)w;
            const uint32_t m = sp_word_mask(hits, n_kmers, n_windows, levels, w, col);
            if (m) {
                uint32_t at = atomicAdd(&n_list, (uint32_t)__builtin_popcount(m));
                sp_word(hits, pos, n_kmers, n_windows, levels, w, col, m,
                        [&](uint32_t j, uint32_t p, uint32_t d) { list[at++] = tid | j << 7 | (p - 1u) << 12 | d << 20; });
            }
        }
        __syncthreads();
        const uint32_t n = n_list;  // (<= 32 nf: every claim is a word's popcount)
        for (uint32_t i = tid; i < n; i += SP_THREADS) {
            const uint32_t e = list[i], lw = e & (SP_SLAB - 1u), j = e >> 7 & 31u, p = (e >> 12 & 255u) + 1u, d = e >> 20 & 3u;
            const uint64_t w = win[lw];
            const uint64_t c = 32u * (f0 + lw - w * words) + j;  // (< n_kmers: sp_word_mask dropped the others)
            const uint32_t len = sp_span(kmers[c], k, codes, nmask, w * stride, window_len, p, d);
            if (len != SP_NONE) sp_put(p - len, j, [&](uint32_t b, uint32_t bit) { atomicOr(&out[b * SP_SLAB + lw], bit); });
        }
        __syncthreads();
        for (uint32_t i = tid; i < POS_PLANES * SP_SLAB; i += SP_THREADS) {
            const uint32_t b = i / SP_SLAB, lw = i % SP_SLAB;
            if (lw < nf) start[(uint64_t)b * plane + f0 + lw] = out[i];
        }
        __syncthreads();  // (the next slab zeroes what these stores read)
    }
}

hipError_t launch_hit_start_positions(uint32_t k, const uint64_t* kmers, uint32_t n_kmers, const uint32_t* codes,
                                      const uint32_t* nmask, uint32_t n_windows, uint32_t window_len, const uint32_t* hits,
                                      const uint32_t* pos, uint32_t levels, uint32_t* start, hipStream_t stream) {
    if (!n_kmers || !n_windows) return hipSuccess;
    const uint64_t plane = (uint64_t)n_windows * (((uint64_t)n_kmers + 31u) >> 5);
    const uint64_t slabs = (plane + SP_SLAB - 1u) / SP_SLAB;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(slabs, SP_MAX_BLOCKS);
    hipLaunchKernelGGL(hit_start_positions_kernel, dim3(blocks), dim3(SP_THREADS), 0, stream, k, kmers, n_kmers, codes, nmask,
                       n_windows, window_len, hits, pos, levels, start);
    return hipGetLastError();
}

}  // namespace acamd
