// hit_cross.hip -- cross co-occurrence of two hit matrices over the same windows (DESIGN.md §4e "Cross
// co-occurrence"): for every candidate a of A and b of B the windows of a level plane that hold both -- the
// rectangular product T_A T_B^t of the transposed planes.  The transposition is hit_cooc.hip's, called once a
// matrix; the product kernel is this file's:
//   hit_cross_product_kernel   T_A T_B^t by tiles of 64 x 64 candidates over the full tiles_a x tiles_b grid
// A translation unit of its own: hit_cooc.hip's device compile stays what it was.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wm_count.h"
#include "hit_cross.h"

namespace acamd {

using namespace bs;

// ---- product ---------------------------------------------------------------------------------------------
// A workgroup takes tile blockIdx.x (cx_tile: ta of A, tb of B) of plane blockIdx.z over the slabs
// [blockIdx.y * per, + per).  The LDS layout, the prefetch and the occupancy are the Gram kernel's: a slab of
// tile ta's bit rows of T_A and tile tb's of T_B -- 2 x 64 rows of CO_SLAB words, 16-byte loads, rows past a
// matrix read as 0 -- goes into LDS, rows CX_LDS_ROW words apart (36 = 4 x 9: the 16 lanes of a 16-byte read
// that differ in their row hit different banks), the next slab's loads in flight while this one is
// multiplied.  Thread (ty, tx) of 16 x 16 owns the candidates ty + 16 i of tile ta against tx + 16 j of tile
// tb.  It stores its sums (split == 0: every word of the output exactly once) or adds the non-zero ones into
// the zeroed output (split != 0).  No triangle, no mirror: the loop's LDS is the kernel's only LDS.
constexpr uint32_t CX_LDS_ROW = CO_SLAB + 4u;
static_assert(CO_TILE == 16u * CO_ACC && (CX_LDS_ROW / 4u) % 2u == 1u, "thread grid and bank spread");
static_assert(2u * CO_TILE * (CO_SLAB / 4u) % 256u == 0u && 256u / (CO_SLAB / 4u) <= CO_TILE && CO_TILE % (256u / (CO_SLAB / 4u)) == 0u,
              "a thread's loads of a slab are whole and each stays in one tile");

__global__ __launch_bounds__(256, CX_WAVES_PER_SIMD) void hit_cross_product_kernel(
    const uint32_t* Ta, const uint32_t* Tb, uint32_t n_a, uint32_t n_b, uint32_t rows_a, uint32_t rows_b, uint32_t tiles_a,
    uint32_t tw, uint32_t per, uint32_t split, uint32_t* cross) {
    __shared__ __align__(16) uint32_t lds[2u * CO_TILE * CX_LDS_ROW];
    uint32_t ta, tb;
    cx_tile(blockIdx.x, tiles_a, ta, tb);
    const uint32_t e = blockIdx.z, tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint32_t* Ap = Ta + (uint64_t)e * rows_a * tw;
    const uint32_t* Bp = Tb + (uint64_t)e * rows_b * tw;
    const uint32_t slabs = tw / CO_SLAB, s0 = blockIdx.y * per, s1 = min(s0 + per, slabs);
    uint32_t acc[CO_ACC][CO_ACC];
#pragma unroll
    for (int i = 0; i < CO_ACC; ++i)
#pragma unroll
        for (int j = 0; j < CO_ACC; ++j) acc[i][j] = 0u;
    // A slab is 2 tiles x 64 rows x 8 quads, four 16-byte loads a thread: quad lq of the rows lr + 32 n of
    // the two tiles stacked (n < 2: tile ta of T_A, then tile tb of T_B).
    constexpr uint32_t LOADS = 2u * CO_TILE * (CO_SLAB / 4u) / 256u, STEP = 256u / (CO_SLAB / 4u);
    const uint32_t lq = threadIdx.x % (CO_SLAB / 4u), lr = threadIdx.x / (CO_SLAB / 4u);
    uint4 pre[LOADS];
    auto fetch = [&](uint32_t s) {
#pragma unroll
        for (uint32_t n = 0; n < LOADS; ++n) {
            const uint32_t r = lr + n * STEP;
            const bool is_a = r < CO_TILE;  // (known at compile time: STEP divides CO_TILE)
            const uint32_t row = (is_a ? ta : tb) * CO_TILE + (r & (CO_TILE - 1u));
            pre[n] = make_uint4(0u, 0u, 0u, 0u);
            if (row < (is_a ? rows_a : rows_b))
                pre[n] = *reinterpret_cast<const uint4*>((is_a ? Ap : Bp) + (uint64_t)row * tw + (uint64_t)s * CO_SLAB + 4u * lq);
        }
    };
    if (s0 < s1) fetch(s0);
    for (uint32_t s = s0; s < s1; ++s) {
#pragma unroll
        for (uint32_t n = 0; n < LOADS; ++n) *reinterpret_cast<uint4*>(lds + (lr + n * STEP) * CX_LDS_ROW + 4u * lq) = pre[n];
        __syncthreads();
        if (s + 1u < s1) fetch(s + 1u);
#pragma unroll 1
        for (uint32_t q = 0; q < CO_SLAB / 4u; ++q) {
            uint4 a4[CO_ACC], b4[CO_ACC];
#pragma unroll
            for (int i = 0; i < CO_ACC; ++i) {
                a4[i] = *reinterpret_cast<const uint4*>(lds + (ty + 16u * i) * CX_LDS_ROW + 4u * q);
                b4[i] = *reinterpret_cast<const uint4*>(lds + (CO_TILE + tx + 16u * i) * CX_LDS_ROW + 4u * q);
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
    uint32_t* out = cross + (uint64_t)e * n_a * n_b;
#pragma unroll
    for (int i = 0; i < CO_ACC; ++i) {
        const uint64_t a = (uint64_t)ta * CO_TILE + ty + 16u * i;
#pragma unroll
        for (int j = 0; j < CO_ACC; ++j) {
            const uint64_t b = (uint64_t)tb * CO_TILE + tx + 16u * j;
            if (a < n_a && b < n_b) {
                uint32_t* p = out + a * n_b + b;
                if (!split) *p = acc[i][j];
                else if (acc[i][j]) atomicAdd(p, acc[i][j]);
            }
        }
    }
}

// ---- launches --------------------------------------------------------------------------------------------

uint64_t hit_cross_scratch_words(uint32_t n_a, uint32_t n_b, uint32_t n_windows, uint32_t levels) {
    return (uint64_t)levels * (co_t_rows(n_a) + co_t_rows(n_b)) * co_t_words(n_windows);
}

hipError_t launch_hit_cross(const uint32_t* hits_a, uint32_t n_a, const uint32_t* hits_b, uint32_t n_b, uint32_t n_windows,
                            uint32_t levels, uint32_t* scratch, uint32_t* cross, uint32_t stages, hipStream_t stream) {
    if (!n_a || !n_b || !levels) return hipSuccess;
    const size_t out_bytes = sizeof(uint32_t) * (size_t)levels * n_a * n_b;
    if (!n_windows) return (stages & 2u) ? hipMemsetAsync(cross, 0, out_bytes, stream) : hipSuccess;
    const uint64_t tw = co_t_words(n_windows), rows_a = co_t_rows(n_a), rows_b = co_t_rows(n_b);
    const uint64_t tiles_a = cx_tiles(n_a), tiles_b = cx_tiles(n_b);
    if (tiles_a * tiles_b > 0x7FFFFFFFull) return hipErrorInvalidValue;
    uint32_t* t_a = scratch;
    uint32_t* t_b = scratch + (uint64_t)levels * rows_a * tw;
    if (stages & 1u) {
        // (the transposition alone: its product argument is not read; it checks its own tile counts)
        if (hipError_t e = launch_hit_cooccurrence(hits_a, n_a, n_windows, levels, t_a, nullptr, 1u, stream)) return e;
        if (hipError_t e = launch_hit_cooccurrence(hits_b, n_b, n_windows, levels, t_b, nullptr, 1u, stream)) return e;
    }
    if (stages & 2u) {
        const CoSplit sp = cx_splits(n_a, n_b, n_windows, levels);
        if (sp.splits > 1u)
            if (hipError_t e = hipMemsetAsync(cross, 0, out_bytes, stream)) return e;
        hipLaunchKernelGGL(hit_cross_product_kernel, dim3((uint32_t)(tiles_a * tiles_b), sp.splits, levels), dim3(256), 0, stream,
                           t_a, t_b, n_a, n_b, (uint32_t)rows_a, (uint32_t)rows_b, (uint32_t)tiles_a, (uint32_t)tw, sp.per,
                           sp.splits > 1u ? 1u : 0u, cross);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace acamd
