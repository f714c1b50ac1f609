// bsh_count.hip -- the hits-writing family of the bit-sliced count kernels (DESIGN.md §4e "Hit levels"):
// bs_count.inc's body with HITS on, which beside the counts stores every window's hit word of each level
// 0..E -- what the reference keeps per read in tcount[errors][read] (approx_counter.cpp:553-565) before
// vectorSum collapses it (580-596).  One instantiation per k in AC_BS_K_LIST over three NFA rows (edit
// budgets 0..2) and over four (budget 3), plain only: the staged forms are bshs_count.hip's.
// With it: the kernel that turns a hit matrix into per-level counts (hit_levels.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bs_nfa.h"
#include "bs_nfa_r.h"
#include "bs_pos.h"
#include "hit_levels.h"
#include "nrec.h"
#include "wm_count.h"

namespace acamd {
namespace {

#include "bs_family.inc"

constexpr BsFamily family(int rows) { return BsFamily{false, BsOut::Hits, rows}; }

}  // namespace

// k = K, equal windows, R NFA rows (3: E = 0..2, 4: E = 3), counts and hits, at its family's residency.
template <int K, int R>
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, bs_waves_per_simd(family(R), K)) void bsh_count_kernel(LaunchArgs a) {
    __shared__ BsLds<K> lds[(160 * 1024 / bs_blocks_per_cu(family(R), K)) / sizeof(BsLds<K>)];
    bs_body<K, false, R, true>(a, lds[0]);
}

CountKernel bsh_kernel(uint32_t k, BsFamily f) {
#define AC_BS_PICK(KK) \
    if (k == KK) return f.rows == 4 ? bsh_count_kernel<KK, 4> : bsh_count_kernel<KK, 3>;
    AC_BS_K_LIST(AC_BS_PICK)
#undef AC_BS_PICK
    return nullptr;
}

// Level counts of a hit matrix.  A wave reads 64 consecutive words of a level plane at a time: with
// wpad = min(64, next_pow2(words)) its lane l counts word column 64 blockIdx.x + l % wpad over the windows
// u * (64 / wpad) + l / wpad of the units u the wave takes (wave 4 blockIdx.y + threadIdx.x / 64, then grid
// strides) -- whole rows of the plane when words is a power of two or a multiple of 64, so the reads are
// coalesced along the word axis -- HC_BATCH loads in flight per lane (hit_levels.h).  A workgroup sums its
// threads' 32 counters per column in LDS and adds them to level_counts with one atomic per candidate.
constexpr uint32_t HC_BLOCKS = 1024u;     // workgroups of a call, about (4 per CU)
constexpr uint32_t HC_WAVE_UNITS = 16u;   // units a wave gets at least, when there are that many
__global__ __launch_bounds__(256) void hit_level_counts_kernel(const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows,
                                                               uint32_t wpad_shift, uint32_t* level_counts) {
    __shared__ uint32_t sums[64u * 32u];
    const uint32_t words = (n_kmers + 31u) >> 5;
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.y * 4u + (threadIdx.x >> 6), n_waves = gridDim.y * 4u;
    const uint32_t cx = lane & ((1u << wpad_shift) - 1u), sub = lane >> wpad_shift, rpw = 64u >> wpad_shift;
    const uint32_t col = blockIdx.x * 64u + cx;
    const uint32_t e = blockIdx.z;
    const uint32_t* plane = hits + (uint64_t)e * n_windows * words;
    for (uint32_t i = threadIdx.x; i < 64u * 32u; i += 256u) sums[i] = 0u;
    __syncthreads();
    if (col < words) {
        uint32_t cnt[32];
#pragma unroll
        for (uint32_t j = 0; j < 32u; ++j) cnt[j] = 0u;
        // this lane's windows: wave * rpw + sub, then every n_waves * rpw further
        bs::hc_column(plane, words, col, (uint64_t)wave * rpw + sub, n_windows, (uint64_t)n_waves * rpw, cnt);
#pragma unroll
        for (uint32_t j = 0; j < 32u; ++j)
            if (cnt[j]) __hip_atomic_fetch_add(&sums[cx * 32u + j], cnt[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 64u * 32u; i += 256u) {
        const uint64_t c = 32ull * (blockIdx.x * 64u) + i;  // (i = 32 cx + j)
        if (sums[i] && c < n_kmers) atomicAdd(&level_counts[(uint64_t)e * n_kmers + c], sums[i]);
    }
}

hipError_t launch_hit_level_counts(const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows, uint32_t levels,
                                   uint32_t* level_counts, hipStream_t stream) {
    if (!n_kmers || !levels) return hipSuccess;
    hipError_t e = hipMemsetAsync(level_counts, 0, sizeof(uint32_t) * (size_t)levels * n_kmers, stream);
    if (e != hipSuccess || !n_windows) return e;
    const uint32_t words = (n_kmers + 31u) >> 5;
    uint32_t shift = 0;
    while (shift < 6u && (1u << shift) < words) ++shift;
    const uint32_t tiles = (words + 63u) / 64u, rpw = 64u >> shift;
    const uint32_t units = (n_windows + rpw - 1u) / rpw;
    const uint32_t want = (units + 4u * HC_WAVE_UNITS - 1u) / (4u * HC_WAVE_UNITS);
    const uint32_t cap = std::max<uint32_t>(1u, HC_BLOCKS / std::min<uint32_t>(HC_BLOCKS, tiles * levels));
    const dim3 grid(tiles, std::min<uint32_t>(want, cap), levels), block(256);
    hipLaunchKernelGGL(hit_level_counts_kernel, grid, block, 0, stream, hits, n_kmers, n_windows, shift, level_counts);
    return hipGetLastError();
}

}  // namespace acamd
