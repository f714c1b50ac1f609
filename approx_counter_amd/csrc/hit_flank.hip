// hit_flank.hip -- flank profiles (DESIGN.md §4e "Flank profiles"): per k-mer the histogram of the D bases
// after the end and before the start of its best occurrence, hit_flank.h's step over the hit pairs of one
// level plane.  A reduction over resident matrices like the span pass and the co-occurrence products; a
// translation unit of its own: the count kernels' device compiles stay what they were.
//
// The output is keyed by k-mer, so a workgroup owns a tile of FL_TILE word columns (32 FL_TILE k-mers) and a
// strip of windows, and keeps the tile's histogram -- 2 sides x 32 FL_TILE k-mers x D x 5 u32, a k-mer's row
// padded to an odd number of words, sized by the launch for its depth (dynamic LDS) -- in LDS.  The
// strip is walked in chunks of FL_CHUNK windows.  The work follows the hits: one lane per hit word of the
// chunk reads it, claims popcount entries of an LDS work list with one LDS atomic add and appends its set
// bits there (fl_word: word, bit, pos - 1 and start from the sixteen planes) -- a word's bits side by side,
// so the lanes of one LDS add hold different k-mers, not the many windows of one adapter k-mer.  All lanes
// then take list entries densely and run fl_pair (each side's text fetched once), every counted base one LDS
// atomic add.  No global atomic
// per observation: the histogram is flushed once per workgroup, its non-zero cells added onto the output,
// which the launch zeroes on the stream first.  The sums do not depend on the claims' order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hit_flank.h"
#include "wm_count.h"

namespace acamd {

using namespace bs;

constexpr uint32_t FL_TILE = 1u;      // word columns of a tile (2 and 4 measured, not kept)
constexpr uint32_t FL_CHUNK = 128u;   // windows of a chunk: FL_TILE FL_CHUNK hit words, one scanning lane each
constexpr uint32_t FL_THREADS = 256u;
constexpr uint32_t FL_BLOCKS = 1024u;      // workgroups a launch aims at: the strips are cut to give about these
constexpr uint32_t FL_MAX_STRIPS = 65535u;  // (grid y)
constexpr uint32_t FL_TILE_KMERS = 32u * FL_TILE;
constexpr uint32_t FL_LANES = FL_TILE * FL_CHUNK;  // scanning lanes; also the entry's word field
// A k-mer's row of the LDS histogram: D x 5 words made odd, so that the lanes of one LDS add -- the same
// column of different k-mers -- fall into different banks.
constexpr uint32_t fl_row(uint32_t depth) { return (depth * FL_SYMS) | 1u; }
constexpr uint32_t fl_hist_bytes(uint32_t depth) { return 4u * 2u * FL_TILE_KMERS * fl_row(depth); }
static_assert(FL_LANES <= 1u << 9, "9 bits of an entry");
static_assert(4u * 32u * FL_LANES + fl_hist_bytes(FL_MAX_DEPTH) + 16u <= 80u * 1024u,
              "the work list and the largest histogram: half a CU's LDS");

__global__ __launch_bounds__(FL_THREADS) void hit_flank_profile_kernel(const uint32_t* codes, const uint32_t* nmask,
                                                                      uint32_t n_windows, uint32_t window_len,
                                                                      const uint32_t* hit, const uint32_t* pos,
                                                                      const uint32_t* start, uint32_t n_kmers, uint32_t depth,
                                                                      uint64_t strip, uint32_t* flank) {
    extern __shared__ uint32_t hist[];  // (side * tile k-mers + c) * fl_row(D) + j * 5 + s
    __shared__ uint32_t list[FL_LANES * 32u];                               // lane | bit << 9 | (pos - 1) << 14 | start << 22
    __shared__ uint32_t n_list;
    const uint32_t tid = threadIdx.x;
    const uint64_t words = ((uint64_t)n_kmers + 31u) >> 5;
    const uint64_t stride = ((uint64_t)window_len + 31u) & ~31ull;
    const uint64_t col0 = (uint64_t)blockIdx.x * FL_TILE;
    const uint64_t w_lo = blockIdx.y * strip, w_hi = std::min<uint64_t>(n_windows, w_lo + strip);
    const uint32_t row = depth * FL_SYMS, lrow = fl_row(depth), cells = 2u * FL_TILE_KMERS * lrow;
    const bool with_start = start != nullptr;
    for (uint32_t i = tid; i < cells; i += FL_THREADS) hist[i] = 0u;
    for (uint64_t wc = w_lo; wc < w_hi; wc += FL_CHUNK) {
        if (tid == 0u) n_list = 0u;
        __syncthreads();  // (and the histogram's zeroes)
        for (uint32_t lane = tid; lane < FL_LANES; lane += FL_THREADS) {
            const uint64_t w = wc + lane / FL_TILE, col = col0 + lane % FL_TILE;
            if (w >= w_hi || col >= words) continue;
            const uint32_t m = fl_word_mask(hit, n_kmers, w, (uint32_t)col);
            if (m) {
                uint32_t at = atomicAdd(&n_list, (uint32_t)__builtin_popcount(m));
                fl_word(pos, start, n_kmers, n_windows, w, (uint32_t)col, m,
                        [&](uint32_t j, uint32_t p, uint32_t s) { list[at++] = lane | j << 9 | (p - 1u) << 14 | s << 22; });
            }
        }
        __syncthreads();
        const uint32_t n = n_list;  // (<= 32 FL_LANES: every claim is a word's popcount)
        for (uint32_t i = tid; i < n; i += FL_THREADS) {
            const uint32_t e = list[i], lane = e & 511u, j = e >> 9 & 31u, p = (e >> 14 & 255u) + 1u, s = e >> 22 & 255u;
            const uint32_t c = 32u * (lane % FL_TILE) + j;  // the k-mer inside the tile
            fl_pair(codes, nmask, (wc + lane / FL_TILE) * stride, window_len, depth, p, s, with_start,
                    [&](uint32_t side, uint32_t jj, uint32_t sym) {
                        atomicAdd(&hist[(side * FL_TILE_KMERS + c) * lrow + jj * FL_SYMS + sym], 1u);
                    });
        }
        __syncthreads();  // (the next chunk clears the count these lanes read; the flush reads every lane's adds)
    }
    for (uint32_t i = tid; i < cells; i += FL_THREADS) {
        const uint32_t v = hist[i];
        if (!v) continue;
        const uint32_t side = i / (FL_TILE_KMERS * lrow), c = i / lrow % FL_TILE_KMERS, r = i % lrow;  // (r < row: the pad is 0)
        // (32 col0 + c < n_kmers: fl_word_mask dropped the others, their cells stayed 0)
        atomicAdd(&flank[((uint64_t)side * n_kmers + 32u * col0 + c) * row + r], v);
    }
}

hipError_t launch_hit_flank_profile(const uint32_t* codes, const uint32_t* nmask, uint32_t n_windows, uint32_t window_len,
                                    const uint32_t* hit, const uint32_t* pos, const uint32_t* start, uint32_t n_kmers,
                                    uint32_t depth, uint32_t* flank, hipStream_t stream) {
    if (!n_kmers) return hipSuccess;
    if (hipError_t e = hipMemsetAsync(flank, 0, sizeof(uint32_t) * fl_words(n_kmers, depth), stream)) return e;
    if (!n_windows) return hipSuccess;
    const uint64_t words = ((uint64_t)n_kmers + 31u) >> 5;
    const uint64_t tiles = (words + FL_TILE - 1u) / FL_TILE;  // (<= 2^27: grid x)
    const uint64_t chunks = ((uint64_t)n_windows + FL_CHUNK - 1u) / FL_CHUNK;
    // about FL_BLOCKS workgroups: whole chunks to a strip, at most FL_MAX_STRIPS strips
    const uint64_t want = std::min<uint64_t>(std::min<uint64_t>(chunks, std::max<uint64_t>(FL_BLOCKS / tiles, 1u)), FL_MAX_STRIPS);
    const uint64_t strip = (chunks + want - 1u) / want * FL_CHUNK;
    const uint64_t strips = ((uint64_t)n_windows + strip - 1u) / strip;
    const uint32_t lds = fl_hist_bytes(depth);
    hipLaunchKernelGGL(hit_flank_profile_kernel, dim3((uint32_t)tiles, (uint32_t)strips), dim3(FL_THREADS), lds, stream, codes,
                       nmask, n_windows, window_len, hit, pos, start, n_kmers, depth, strip, flank);
    return hipGetLastError();
}

}  // namespace acamd
