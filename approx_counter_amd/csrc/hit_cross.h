// hit_cross.h -- cross co-occurrence (DESIGN.md §4e "Cross co-occurrence"): for two hit matrices A and B over
// the same windows, how many windows of level plane e hold candidate a of A and candidate b of B -- the
// rectangular bit-matrix product T_A T_B^t where hit_cooc.h's is the Gram product T T^t.  It reuses that
// file's transposed layout, slab, tile and inner product (co_t_words, co_t_rows, CO_SLAB, CO_TILE, co_dot)
// and adds what a rectangle needs: the numbering of the full tiles_a x tiles_b grid and the launch rule
// over it.  Plain C++ for the device (hit_cross.hip) and the host (tools/hit_cross_check.cpp,
// tests/test_cross_cpu.py).
#pragma once
#include <stdint.h>
#ifdef __HIP_PLATFORM_AMD__  // (the library's builds; the host check compiles the arithmetic alone)
#include <hip/hip_runtime_api.h>
#endif

#include "hit_cooc.h"

namespace acamd {
namespace bs {

// The product kernel's waves per SIMD (__launch_bounds__; tests/test_cross_kernel_asm.py holds the
// compiler's occupancy to it).  The Gram kernel's: the inner loop and the LDS footprint are the same.
constexpr int CX_WAVES_PER_SIMD = CO_WAVES_PER_SIMD;

// Tiles of 64 candidates along one side.
AC_BS_FN uint64_t cx_tiles(uint64_t n) { return (n + CO_TILE - 1u) / CO_TILE; }

// Tile p of the tiles_a x tiles_b grid: ta fastest, so that the workgroups resident together share tile
// tb's rows of T_B and walk T_A.
AC_BS_FN void cx_tile(uint32_t p, uint32_t tiles_a, uint32_t& ta, uint32_t& tb) {
    tb = p / tiles_a;
    ta = p - tb * tiles_a;
}

// The launch rule: co_splits' over work = tiles_a * tiles_b * levels workgroups.  splits == 1: every word of
// the output is stored once; splits > 1: the output is zeroed on the stream and the workgroups add into it.
AC_BS_FN CoSplit cx_splits(uint64_t n_a, uint64_t n_b, uint64_t n_windows, uint32_t levels) {
    const uint64_t slabs = co_t_words(n_windows) / CO_SLAB;
    const uint64_t work = cx_tiles(n_a) * cx_tiles(n_b) * levels;
    CoSplit r = {1u, (uint32_t)(slabs ? slabs : 1u)};
    if (!work || work >= CO_BLOCKS || slabs < 2u) return r;
    const uint64_t want = (CO_BLOCKS + work - 1u) / work;
    uint64_t per = (slabs + want - 1u) / want;
    if (per < CO_MIN_SLABS) per = CO_MIN_SLABS;
    r.per = (uint32_t)per;
    r.splits = (uint32_t)((slabs + per - 1u) / per);
    return r;
}

// What thread (ty, tx) of the workgroup of tile (ta, tb) adds over the window words [x0, x1) of the two
// transposed planes (rows_a x tw and rows_b x tw words; rows past them read as 0): the kernel's sums, word
// by word.  The host's form of the kernel's walk; the kernel reads the same words through LDS.
AC_BS_FN void cx_thread_sums(uint32_t (&acc)[CO_ACC][CO_ACC], const uint32_t* Ta, uint64_t rows_a, const uint32_t* Tb,
                             uint64_t rows_b, uint64_t tw, uint32_t ta, uint32_t tb, uint32_t ty, uint32_t tx, uint64_t x0,
                             uint64_t x1) {
    for (uint64_t x = x0; x < x1; ++x) {
        uint32_t a[CO_ACC], b[CO_ACC];
        for (int i = 0; i < CO_ACC; ++i) {
            const uint64_t ra = (uint64_t)ta * CO_TILE + ty + 16u * i, rb = (uint64_t)tb * CO_TILE + tx + 16u * i;
            a[i] = ra < rows_a ? Ta[ra * tw + x] : 0u;
            b[i] = rb < rows_b ? Tb[rb * tw + x] : 0u;
        }
        co_dot(acc, a, b);
    }
}

}  // namespace bs

#ifdef __HIP_PLATFORM_AMD__
// hit_cross.hip: cross[(e * n_a + a) * n_b + b] = the windows of level plane e that hold candidate a of hits_a
// and candidate b of hits_b, two matrices over the same n_windows.  stages bit 0: both matrices' planes
// transposed into `scratch` (hit_cross_scratch_words u32: A's planes, then B's); bit 1: the product from
// scratch into cross, every word of which is then defined.  3 = the whole call.
uint64_t hit_cross_scratch_words(uint32_t n_a, uint32_t n_b, uint32_t n_windows, uint32_t levels);
hipError_t launch_hit_cross(const uint32_t* hits_a, uint32_t n_a, const uint32_t* hits_b, uint32_t n_b, uint32_t n_windows,
                            uint32_t levels, uint32_t* scratch, uint32_t* cross, uint32_t stages, hipStream_t stream);
#endif

}  // namespace acamd
