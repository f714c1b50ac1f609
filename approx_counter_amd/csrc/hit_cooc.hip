// hit_cooc.hip -- co-occurrence over a hit matrix (DESIGN.md §4e "Co-occurrence"): for every pair of
// candidates the windows of a level plane that hold both -- what two of the reference's per-read bitfields
// tcount[errors][read] (approx_counter.cpp:553-565) say together, which vectorSum's collapse (580-596) loses
// -- and the windows' own counts.  Three kernels over hit_cooc.h's arithmetic:
//   hit_cooc_transpose_kernel  a level plane [n_windows][words] into candidate-major bit rows T
//   hit_cooc_product_kernel    the Gram product T T^t by tiles of 64 x 64 candidates, popcounts of ANDs
//   hit_window_counts_kernel   row popcounts
// A translation unit of its own: the count kernels' device compiles stay what they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hit_cooc.h"
#include "wm_count.h"

namespace acamd {

using namespace bs;

// ---- transposition ---------------------------------------------------------------------------------------
// A workgroup takes CO_TC word columns x CO_TB blocks of 32 windows of one plane.  It reads the tile row by
// row -- consecutive lanes consecutive words of a row, the whole tile one contiguous run when the plane has
// no more than CO_TC columns -- into LDS, column-major with one pad word per 32 windows, so that the 16
// threads that then each gather one column's 32 windows of a block (lanes = consecutive blocks) hit 16
// banks.  Each thread transposes its 32 x 32 bits in registers (co_transpose32) and stores 32 words of T;
// 16 lanes store 16 consecutive words of a candidate's row.  Every word of T is stored exactly once.
constexpr uint32_t CO_T_WIN = 32u * CO_TB;                // windows of a tile
constexpr uint32_t CO_T_LDS = CO_T_WIN + CO_TB + 1u;      // LDS words of a column (529: odd)
static_assert(CO_TC * CO_TB == 256u, "one 32 x 32 block per thread");
static_assert(CO_SLAB % CO_TB == 0u, "a row of T is whole tiles");

__global__ __launch_bounds__(256) void hit_cooc_transpose_kernel(const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows,
                                                                 uint32_t tw, uint32_t col_tiles, uint32_t* T) {
    __shared__ uint32_t tile[CO_TC * CO_T_LDS];
    const uint32_t words = (n_kmers + 31u) >> 5;
    const uint32_t ct = blockIdx.x % col_tiles, bt = blockIdx.x / col_tiles, e = blockIdx.z;
    const uint32_t c0 = ct * CO_TC, cw = min(CO_TC, words - c0);
    const uint64_t w0 = (uint64_t)bt * CO_T_WIN;
    const uint32_t* plane = hits + (uint64_t)e * n_windows * words;
    for (uint32_t i = threadIdx.x; i < CO_T_WIN * cw; i += 256u) {
        const uint32_t r = i / cw, c = i - r * cw;
        tile[c * CO_T_LDS + r + (r >> 5)] = co_load_word(plane, words, n_kmers, n_windows, w0 + r, c0 + c);
    }
    __syncthreads();
    const uint32_t b = threadIdx.x % CO_TB, c = threadIdx.x / CO_TB;
    if (c >= cw) return;
    uint32_t a[32];
#pragma unroll
    for (uint32_t i = 0; i < 32u; ++i) a[i] = tile[c * CO_T_LDS + 33u * b + i];
    co_transpose32(a);
    uint32_t* row = T + ((uint64_t)e * (32ull * words) + 32ull * (c0 + c)) * tw + (uint64_t)bt * CO_TB + b;
#pragma unroll
    for (uint32_t j = 0; j < 32u; ++j) row[(uint64_t)j * tw] = a[j];
}

// ---- product ---------------------------------------------------------------------------------------------
// A workgroup takes tile pair blockIdx.x (ta <= tb, co_pair) of plane blockIdx.z over the slabs
// [blockIdx.y * per, + per).  A slab of both tiles' bit rows -- 2 x 64 rows of CO_SLAB words, 16-byte loads,
// rows past T read as 0 -- goes into LDS, rows CO_LDS_ROW words apart (36 = 4 x 9: the 16 lanes of a 16-byte
// read that differ in their row hit different banks).  Thread (ty, tx) of 16 x 16 owns the candidates
// ty + 16 i of tile ta against tx + 16 j of tile tb.  It stores its sums (split == 0: every word of the
// output exactly once) or adds them into the zeroed output (split != 0), and for ta != tb the mirror image
// too, turned through LDS so that its lanes also write consecutive words.
constexpr uint32_t CO_LDS_ROW = CO_SLAB + 4u;
constexpr uint32_t CO_C_ROW = CO_TILE + 1u;
static_assert(2u * CO_TILE * CO_LDS_ROW >= CO_TILE * CO_C_ROW, "the mirror tile fits the slabs' LDS");
static_assert(CO_TILE == 16u * CO_ACC && (CO_LDS_ROW / 4u) % 2u == 1u, "thread grid and bank spread");

__device__ __forceinline__ void co_put(uint32_t* p, uint32_t v, bool split) {
    if (!split) *p = v;
    else if (v) atomicAdd(p, v);
}

__global__ __launch_bounds__(256, CO_WAVES_PER_SIMD) void hit_cooc_product_kernel(const uint32_t* T, uint32_t n_kmers,
                                                                                  uint32_t rows, uint32_t tw, uint32_t per,
                                                                                  uint32_t split, uint32_t* cooc) {
    __shared__ __align__(16) uint32_t lds[2u * CO_TILE * CO_LDS_ROW];
    uint32_t ta, tb;
    co_pair(blockIdx.x, ta, tb);
    const uint32_t e = blockIdx.z, tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint32_t* Tp = T + (uint64_t)e * rows * tw;
    const uint32_t slabs = tw / CO_SLAB, s0 = blockIdx.y * per, s1 = min(s0 + per, slabs);
    uint32_t acc[CO_ACC][CO_ACC];
#pragma unroll
    for (int i = 0; i < CO_ACC; ++i)
#pragma unroll
        for (int j = 0; j < CO_ACC; ++j) acc[i][j] = 0u;
    // A slab is 2 tiles x 64 rows x 8 quads, four 16-byte loads a thread: quad lq of the rows lr + 32 n of
    // the two tiles stacked (n < 2: tile ta).  The next slab's are in flight while this one is multiplied.
    constexpr uint32_t LOADS = 2u * CO_TILE * (CO_SLAB / 4u) / 256u;
    const uint32_t lq = threadIdx.x % (CO_SLAB / 4u), lr = threadIdx.x / (CO_SLAB / 4u);
    uint4 pre[LOADS];
    auto fetch = [&](uint32_t s) {
#pragma unroll
        for (uint32_t n = 0; n < LOADS; ++n) {
            const uint32_t r = lr + n * (256u / (CO_SLAB / 4u));
            const uint32_t row = (r < CO_TILE ? ta : tb) * CO_TILE + (r & (CO_TILE - 1u));
            pre[n] = make_uint4(0u, 0u, 0u, 0u);
            if (row < rows) pre[n] = *reinterpret_cast<const uint4*>(Tp + (uint64_t)row * tw + (uint64_t)s * CO_SLAB + 4u * lq);
        }
    };
    if (s0 < s1) fetch(s0);
    for (uint32_t s = s0; s < s1; ++s) {
#pragma unroll
        for (uint32_t n = 0; n < LOADS; ++n)
            *reinterpret_cast<uint4*>(lds + (lr + n * (256u / (CO_SLAB / 4u))) * CO_LDS_ROW + 4u * lq) = pre[n];
        __syncthreads();
        if (s + 1u < s1) fetch(s + 1u);
#pragma unroll 1
        for (uint32_t q = 0; q < CO_SLAB / 4u; ++q) {
            uint4 a4[CO_ACC], b4[CO_ACC];
#pragma unroll
            for (int i = 0; i < CO_ACC; ++i) {
                a4[i] = *reinterpret_cast<const uint4*>(lds + (ty + 16u * i) * CO_LDS_ROW + 4u * q);
                b4[i] = *reinterpret_cast<const uint4*>(lds + (CO_TILE + tx + 16u * i) * CO_LDS_ROW + 4u * q);
            }
            {
                const uint32_t a[CO_ACC] = {a4[0].x, a4[1].x, a4[2].x, a4[3].x}, b[CO_ACC] = {b4[0].x, b4[1].x, b4[2].x, b4[3].x};
                co_dot(acc, a, b);
            }
            {
                const uint32_t a[CO_ACC] = {a4[0].y, a4[1].y, a4[2].y, a4[3].y}, b[CO_ACC] = {b4[0].y, b4[1].y, b4[2].y, b4[3].y};
                co_dot(acc, a, b);
            }
            {
                const uint32_t a[CO_ACC] = {a4[0].z, a4[1].z, a4[2].z, a4[3].z}, b[CO_ACC] = {b4[0].z, b4[1].z, b4[2].z, b4[3].z};
                co_dot(acc, a, b);
            }
            {
                const uint32_t a[CO_ACC] = {a4[0].w, a4[1].w, a4[2].w, a4[3].w}, b[CO_ACC] = {b4[0].w, b4[1].w, b4[2].w, b4[3].w};
                co_dot(acc, a, b);
            }
        }
        __syncthreads();
    }
    uint32_t* out = cooc + (uint64_t)e * n_kmers * n_kmers;
#pragma unroll
    for (int i = 0; i < CO_ACC; ++i) {
        const uint64_t a = (uint64_t)ta * CO_TILE + ty + 16u * i;
#pragma unroll
        for (int j = 0; j < CO_ACC; ++j) {
            const uint64_t b = (uint64_t)tb * CO_TILE + tx + 16u * j;
            if (a < n_kmers && b < n_kmers) co_put(out + a * n_kmers + b, acc[i][j], split != 0u);
        }
    }
    if (ta == tb) return;
    // (the loop's last barrier has every thread past its reads of the slabs)
#pragma unroll
    for (int i = 0; i < CO_ACC; ++i)
#pragma unroll
        for (int j = 0; j < CO_ACC; ++j) lds[(ty + 16u * i) * CO_C_ROW + tx + 16u * j] = acc[i][j];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < CO_ACC; ++i) {
        const uint64_t b = (uint64_t)tb * CO_TILE + ty + 16u * i;
#pragma unroll
        for (int j = 0; j < CO_ACC; ++j) {
            const uint64_t a = (uint64_t)ta * CO_TILE + tx + 16u * j;
            if (a < n_kmers && b < n_kmers)
                co_put(out + b * n_kmers + a, lds[(tx + 16u * j) * CO_C_ROW + ty + 16u * i], split != 0u);
        }
    }
}

// ---- window counts ---------------------------------------------------------------------------------------
// A wave reads 64 consecutive words of a level plane at a time, like the level counter: with wpad =
// min(64, next_pow2(words)) its lane l adds the words l % wpad, + wpad, .. of row 64 / wpad * unit + l / wpad,
// the wpad lanes of a row sum by shuffles, and the first of them stores the row's count: every word of the
// output once.  blockIdx.y = the plane.
__global__ __launch_bounds__(256) void hit_window_counts_kernel(const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows,
                                                                uint32_t wpad_shift, uint32_t* window_counts) {
    const uint32_t words = (n_kmers + 31u) >> 5;
    const uint32_t wpad = 1u << wpad_shift, rpw = 64u >> wpad_shift;
    const uint32_t lane = threadIdx.x & 63u, cx = lane & (wpad - 1u), sub = lane >> wpad_shift;
    const uint32_t* plane = hits + (uint64_t)blockIdx.y * n_windows * words;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
    const uint64_t units = ((uint64_t)n_windows + rpw - 1u) / rpw;
    for (uint64_t u = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); u < units; u += n_waves) {
        const uint64_t w = u * rpw + sub;
        uint32_t n = 0u;
        if (w < n_windows)
            for (uint32_t c = cx; c < words; c += wpad) n += co_word_count(plane[w * words + c], c, n_kmers);
        for (uint32_t d = wpad >> 1; d; d >>= 1) n += __shfl_xor(n, d, 64);
        if (cx == 0u && w < n_windows) window_counts[(uint64_t)blockIdx.y * n_windows + w] = n;
    }
}

// ---- launches --------------------------------------------------------------------------------------------

uint64_t hit_cooc_scratch_words(uint32_t n_kmers, uint32_t n_windows, uint32_t levels) {
    return (uint64_t)levels * co_t_rows(n_kmers) * co_t_words(n_windows);
}

hipError_t launch_hit_cooccurrence(const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows, uint32_t levels,
                                   uint32_t* scratch, uint32_t* cooc, uint32_t stages, hipStream_t stream) {
    if (!n_kmers || !levels) return hipSuccess;
    const size_t out_bytes = sizeof(uint32_t) * (size_t)levels * n_kmers * n_kmers;
    if (!n_windows) return (stages & 2u) ? hipMemsetAsync(cooc, 0, out_bytes, stream) : hipSuccess;
    const uint32_t words = (n_kmers + 31u) >> 5;
    const uint64_t tw = co_t_words(n_windows), rows = co_t_rows(n_kmers);
    const uint64_t col_tiles = (words + CO_TC - 1u) / CO_TC, t_tiles = col_tiles * (tw / CO_TB);
    const uint64_t pairs = co_pairs(((uint64_t)n_kmers + CO_TILE - 1u) / CO_TILE);
    // (a matrix whose tiles outnumber a grid's x range has no scratch to begin with)
    if (t_tiles > 0x7FFFFFFFull || pairs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (stages & 1u) {
        hipLaunchKernelGGL(hit_cooc_transpose_kernel, dim3((uint32_t)t_tiles, 1u, levels), dim3(256), 0, stream, hits,
                           n_kmers, n_windows, (uint32_t)tw, (uint32_t)col_tiles, scratch);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (stages & 2u) {
        const CoSplit sp = co_splits(n_kmers, n_windows, levels);
        if (sp.splits > 1u)
            if (hipError_t e = hipMemsetAsync(cooc, 0, out_bytes, stream)) return e;
        hipLaunchKernelGGL(hit_cooc_product_kernel, dim3((uint32_t)pairs, sp.splits, levels), dim3(256), 0, stream, scratch,
                           n_kmers, (uint32_t)rows, (uint32_t)tw, sp.per, sp.splits > 1u ? 1u : 0u, cooc);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t launch_hit_window_counts(const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows, uint32_t levels,
                                    uint32_t* window_counts, hipStream_t stream) {
    if (!n_kmers || !levels || !n_windows) return hipSuccess;
    const uint32_t words = (n_kmers + 31u) >> 5;
    uint32_t shift = 0;
    while (shift < 6u && (1u << shift) < words) ++shift;
    const uint32_t rpw = 64u >> shift;
    const uint64_t units = ((uint64_t)n_windows + rpw - 1u) / rpw;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((units + 3u) / 4u, 1u << 16);
    hipLaunchKernelGGL(hit_window_counts_kernel, dim3(blocks, levels), dim3(256), 0, stream, hits, n_kmers, n_windows, shift,
                       window_counts);
    return hipGetLastError();
}

}  // namespace acamd
