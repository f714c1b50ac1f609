// bsp_count.hip -- the hits-and-positions family of the bit-sliced count kernels (DESIGN.md §4e "Match end
// positions"): bs_count.inc's body with HITS and POS on, which beside the counts and every window's hit word
// of each level 0..E stores eight plane words of end positions -- where in the window each candidate's
// leftmost occurrence at its best distance ends, the one dimension of the reference's search delegate
// (approx_counter.cpp:553-565) that neither the counts nor the hit levels keep.  One instantiation per k in
// AC_BS_K_LIST over three NFA rows (edit budgets 0..2) and over four (budget 3), plain only.
// With it: the kernel that turns a hit matrix and its position matrix into the position profile (bs_pos.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bs_nfa.h"
#include "bs_nfa_r.h"
#include "bs_pos.h"
#include "nrec.h"
#include "wm_count.h"

namespace acamd {
namespace {

#include "bs_family.inc"

constexpr BsFamily family(int rows) { return BsFamily{false, BsOut::Pos, rows}; }

}  // namespace

// k = K, equal windows, R NFA rows (3: E = 0..2, 4: E = 3), counts, hits and positions, at its family's
// residency.
template <int K, int R>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, bs_waves_per_simd(family(R), K)) void bsp_count_kernel(LaunchArgs a) {
    __shared__ BsLds<K> lds[(160 * 1024 / bs_blocks_per_cu(family(R), K)) / sizeof(BsLds<K>)];
    bs_body<K, false, R, true, true>(a, lds[0]);
}

CountKernel bsp_kernel(uint32_t k, BsFamily f) {
#define AC_BS_PICK(KK) \
    if (k == KK) return f.rows == 4 ? bsp_count_kernel<KK, 4> : bsp_count_kernel<KK, 3>;
    AC_BS_K_LIST(AC_BS_PICK)
#undef AC_BS_PICK
    return nullptr;
}

// The position profile.  One workgroup per (word column, slab of PP_SLAB windows, distance d): thread t
// walks the slab's windows t, t + 256, .. (bs::pp_column), one LDS atomic per set bit into the workgroup's
// histogram of 32 candidates x window_len bins, then one global atomic per non-zero bin.  A position past
// window_len (no kernel of this library writes one) is dropped.
constexpr uint32_t PP_SLAB = 4096u;
constexpr uint32_t PP_MAX_LEN = 256u;
__global__ __launch_bounds__(256) void hit_position_profile_kernel(const uint32_t* hits, const uint32_t* pos, uint32_t n_kmers,
                                                                   uint32_t n_windows, uint32_t window_len, uint32_t* profile) {
    __shared__ uint32_t bins[32u * PP_MAX_LEN];
    const uint32_t col = blockIdx.x, d = blockIdx.z, L = window_len;
    const uint32_t slabs = (n_windows + PP_SLAB - 1u) / PP_SLAB;
    for (uint32_t slab = blockIdx.y; slab < slabs; slab += gridDim.y) {
        for (uint32_t i = threadIdx.x; i < 32u * L; i += 256u) bins[i] = 0u;
        __syncthreads();
        const uint64_t w0 = (uint64_t)slab * PP_SLAB, w1 = w0 + PP_SLAB < n_windows ? w0 + PP_SLAB : (uint64_t)n_windows;
        bs::pp_column(hits, pos, n_kmers, n_windows, d, col, w0 + threadIdx.x, w1, 256u, [&](uint32_t j, uint32_t p) {
            if (p < L) __hip_atomic_fetch_add(&bins[j * L + p], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        });
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < 32u * L; i += 256u) {
            const uint64_t c = 32ull * col + i / L;
            if (bins[i] && c < n_kmers) atomicAdd(&profile[((uint64_t)d * n_kmers + c) * L + i % L], bins[i]);
        }
        __syncthreads();
    }
}

hipError_t launch_hit_position_profile(const uint32_t* hits, const uint32_t* pos, uint32_t n_kmers, uint32_t n_windows,
                                       uint32_t levels, uint32_t window_len, uint32_t* profile, hipStream_t stream) {
    if (!n_kmers || !levels || !window_len) return hipSuccess;
    if (window_len > PP_MAX_LEN || levels > 4u) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(profile, 0, sizeof(uint32_t) * (size_t)levels * n_kmers * window_len, stream);
    if (e != hipSuccess || !n_windows) return e;
    const uint32_t words = (n_kmers + 31u) >> 5;
    const uint32_t slabs = (n_windows + PP_SLAB - 1u) / PP_SLAB;
    const dim3 grid(words, std::min<uint32_t>(slabs, 65535u), levels), block(256);
    hipLaunchKernelGGL(hit_position_profile_kernel, grid, block, 0, stream, hits, pos, n_kmers, n_windows, window_len, profile);
    return hipGetLastError();
}

}  // namespace acamd
