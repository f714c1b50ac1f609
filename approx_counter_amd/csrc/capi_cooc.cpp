// capi_cooc.cpp -- the co-occurrence calls of the C ABI (include/approx_counter_amd.h "Co-occurrence";
// DESIGN.md §4e): reductions of a hit matrix that need two candidates at once, which the reference's
// collapse of its per-read bitfields (approx_counter.cpp:553-565, vectorSum at 580-596) cannot give.  The
// kernels are hit_cooc.hip's; this file checks the arguments, owns the scratch and enqueues.
#include <cstring>

#include "approx_counter_amd_testing.h"
#include "ctx.h"

using namespace ac_detail;

namespace {

// The refusals the co-occurrence entry points share; `out` is the call's result buffer.
ac_status cooc_check(ac_ctx* ctx, const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows, uint32_t levels,
                     const void* out) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (levels < 1u || levels > 4u) return fail(ctx, AC_ERR_INVALID, "co-occurrence: levels must be 1..4");
    if (n_kmers && !out) return fail(ctx, AC_ERR_INVALID, "co-occurrence: the output is NULL");
    if (n_kmers && n_windows && !hits) return fail(ctx, AC_ERR_INVALID, "co-occurrence: hits is NULL");
    return AC_OK;
}

ac_status cooc_device(ac_ctx* ctx, const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows, uint32_t levels,
                      uint32_t* cooc, uint32_t stages, hipStream_t stream) {
    AC_HIP(ctx, hipSetDevice(ctx->device));
    if (n_kmers && n_windows)
        if (ac_status st = grow(ctx, &ctx->d_cooc, &ctx->d_cooc_cap,
                                sizeof(uint32_t) * (size_t)acamd::hit_cooc_scratch_words(n_kmers, n_windows, levels)))
            return st;
    AC_HIP(ctx, acamd::launch_hit_cooccurrence(hits, n_kmers, n_windows, levels, (uint32_t*)ctx->d_cooc, cooc, stages, stream));
    return AC_OK;
}

}  // namespace

extern "C" {

uint64_t ac_hit_cooccurrence_words(uint32_t n_kmers, uint32_t levels) { return (uint64_t)levels * n_kmers * n_kmers; }

ac_status ac_hit_cooccurrence_device(ac_ctx* ctx, const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows,
                                     uint32_t levels, uint32_t* cooc, void* hip_stream) {
    if (ac_status st = cooc_check(ctx, hits, n_kmers, n_windows, levels, cooc)) return st;
    return cooc_device(ctx, hits, n_kmers, n_windows, levels, cooc, 3u, (hipStream_t)hip_stream);
}

ac_status ac_testing_hit_cooccurrence_stages(ac_ctx* ctx, const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows,
                                             uint32_t levels, uint32_t* cooc, uint32_t stages, void* hip_stream) {
    if (ac_status st = cooc_check(ctx, hits, n_kmers, n_windows, levels, cooc)) return st;
    if (stages < 1u || stages > 3u) return fail(ctx, AC_ERR_INVALID, "co-occurrence: stages must be 1..3");
    return cooc_device(ctx, hits, n_kmers, n_windows, levels, cooc, stages, (hipStream_t)hip_stream);
}

ac_status ac_hit_cooccurrence(ac_ctx* ctx, const uint32_t* hits_host, uint32_t n_kmers, uint32_t n_windows,
                              uint32_t levels, uint32_t* cooc_host) {
    if (ac_status st = cooc_check(ctx, hits_host, n_kmers, n_windows, levels, cooc_host)) return st;
    if (!n_kmers) return AC_OK;
    const size_t in_bytes = sizeof(uint32_t) * (size_t)levels * n_windows * (((size_t)n_kmers + 31u) / 32u);
    const size_t out_bytes = sizeof(uint32_t) * (size_t)ac_hit_cooccurrence_words(n_kmers, levels);
    if (!n_windows) {
        std::memset(cooc_host, 0, out_bytes);
        return AC_OK;
    }
    AC_HIP(ctx, hipSetDevice(ctx->device));
    if (ac_status st = grow(ctx, &ctx->d_cooc_io, &ctx->d_cooc_io_cap, align256(in_bytes) + out_bytes)) return st;
    uint32_t* d_hits = (uint32_t*)ctx->d_cooc_io;
    uint32_t* d_out = (uint32_t*)((char*)ctx->d_cooc_io + align256(in_bytes));
    AC_HIP(ctx, hipMemcpyAsync(d_hits, hits_host, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (ac_status st = cooc_device(ctx, d_hits, n_kmers, n_windows, levels, d_out, 3u, ctx->stream)) return st;
    AC_HIP(ctx, hipMemcpyAsync(cooc_host, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    AC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return AC_OK;
}

ac_status ac_hit_window_counts_device(ac_ctx* ctx, const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows,
                                      uint32_t levels, uint32_t* window_counts, void* hip_stream) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (levels < 1u || levels > 4u) return fail(ctx, AC_ERR_INVALID, "window counts: levels must be 1..4");
    if (n_kmers && !window_counts) return fail(ctx, AC_ERR_INVALID, "window counts: the output is NULL");
    if (n_kmers && n_windows && !hits) return fail(ctx, AC_ERR_INVALID, "window counts: hits is NULL");
    AC_HIP(ctx, hipSetDevice(ctx->device));
    AC_HIP(ctx, acamd::launch_hit_window_counts(hits, n_kmers, n_windows, levels, window_counts, (hipStream_t)hip_stream));
    return AC_OK;
}

}  // extern "C"
