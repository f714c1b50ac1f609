// capi_cross.cpp -- the cross co-occurrence calls of the C ABI (include/approx_counter_amd.h "Co-occurrence";
// DESIGN.md §4e "Cross co-occurrence"): two hit matrices over the same windows reduced over pairs (a of A, b
// of B).  The kernels are hit_cooc.hip's transposition and hit_cross.hip's product; this file checks the
// arguments, owns the scratch (the Gram call's, d_cooc and d_cooc_io) and enqueues.
#include <cstring>

#include "approx_counter_amd_testing.h"
#include "ctx.h"
#include "hit_cross.h"

using namespace ac_detail;

namespace {

ac_status cross_check(ac_ctx* ctx, const uint32_t* hits_a, uint32_t n_a, const uint32_t* hits_b, uint32_t n_b,
                      uint32_t n_windows, uint32_t levels, const void* out) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (levels < 1u || levels > 4u) return fail(ctx, AC_ERR_INVALID, "cross co-occurrence: levels must be 1..4");
    if (n_a && n_b && !out) return fail(ctx, AC_ERR_INVALID, "cross co-occurrence: the output is NULL");
    if (n_a && n_b && n_windows && !hits_a) return fail(ctx, AC_ERR_INVALID, "cross co-occurrence: hits_a is NULL");
    if (n_a && n_b && n_windows && !hits_b) return fail(ctx, AC_ERR_INVALID, "cross co-occurrence: hits_b is NULL");
    return AC_OK;
}

ac_status cross_device(ac_ctx* ctx, const uint32_t* hits_a, uint32_t n_a, const uint32_t* hits_b, uint32_t n_b,
                       uint32_t n_windows, uint32_t levels, uint32_t* cross, uint32_t stages, hipStream_t stream) {
    AC_HIP(ctx, hipSetDevice(ctx->device));
    if (n_a && n_b && n_windows)
        if (ac_status st = grow(ctx, &ctx->d_cooc, &ctx->d_cooc_cap,
                                sizeof(uint32_t) * (size_t)acamd::hit_cross_scratch_words(n_a, n_b, n_windows, levels)))
            return st;
    AC_HIP(ctx, acamd::launch_hit_cross(hits_a, n_a, hits_b, n_b, n_windows, levels, (uint32_t*)ctx->d_cooc, cross, stages,
                                        stream));
    return AC_OK;
}

size_t matrix_bytes(uint32_t n, uint32_t n_windows, uint32_t levels) {
    return sizeof(uint32_t) * (size_t)levels * n_windows * (((size_t)n + 31u) / 32u);
}

}  // namespace

extern "C" {

uint64_t ac_hit_cross_cooccurrence_words(uint32_t n_a, uint32_t n_b, uint32_t levels) { return (uint64_t)levels * n_a * n_b; }

ac_status ac_hit_cross_cooccurrence_device(ac_ctx* ctx, const uint32_t* hits_a, uint32_t n_a, const uint32_t* hits_b,
                                           uint32_t n_b, uint32_t n_windows, uint32_t levels, uint32_t* cross,
                                           void* hip_stream) {
    if (ac_status st = cross_check(ctx, hits_a, n_a, hits_b, n_b, n_windows, levels, cross)) return st;
    return cross_device(ctx, hits_a, n_a, hits_b, n_b, n_windows, levels, cross, 3u, (hipStream_t)hip_stream);
}

ac_status ac_testing_hit_cross_stages(ac_ctx* ctx, const uint32_t* hits_a, uint32_t n_a, const uint32_t* hits_b, uint32_t n_b,
                                      uint32_t n_windows, uint32_t levels, uint32_t* cross, uint32_t stages,
                                      void* hip_stream) {
    if (ac_status st = cross_check(ctx, hits_a, n_a, hits_b, n_b, n_windows, levels, cross)) return st;
    if (stages < 1u || stages > 3u) return fail(ctx, AC_ERR_INVALID, "cross co-occurrence: stages must be 1..3");
    return cross_device(ctx, hits_a, n_a, hits_b, n_b, n_windows, levels, cross, stages, (hipStream_t)hip_stream);
}

ac_status ac_hit_cross_cooccurrence(ac_ctx* ctx, const uint32_t* hits_a_host, uint32_t n_a, const uint32_t* hits_b_host,
                                    uint32_t n_b, uint32_t n_windows, uint32_t levels, uint32_t* cross_host) {
    if (ac_status st = cross_check(ctx, hits_a_host, n_a, hits_b_host, n_b, n_windows, levels, cross_host)) return st;
    if (!n_a || !n_b) return AC_OK;
    const size_t a_bytes = matrix_bytes(n_a, n_windows, levels), b_bytes = matrix_bytes(n_b, n_windows, levels);
    const size_t out_bytes = sizeof(uint32_t) * (size_t)ac_hit_cross_cooccurrence_words(n_a, n_b, levels);
    if (!n_windows) {
        std::memset(cross_host, 0, out_bytes);
        return AC_OK;
    }
    AC_HIP(ctx, hipSetDevice(ctx->device));
    if (ac_status st = grow(ctx, &ctx->d_cooc_io, &ctx->d_cooc_io_cap, align256(a_bytes) + align256(b_bytes) + out_bytes))
        return st;
    uint32_t* d_a = (uint32_t*)ctx->d_cooc_io;
    uint32_t* d_b = (uint32_t*)((char*)ctx->d_cooc_io + align256(a_bytes));
    uint32_t* d_out = (uint32_t*)((char*)ctx->d_cooc_io + align256(a_bytes) + align256(b_bytes));
    AC_HIP(ctx, hipMemcpyAsync(d_a, hits_a_host, a_bytes, hipMemcpyHostToDevice, ctx->stream));
    AC_HIP(ctx, hipMemcpyAsync(d_b, hits_b_host, b_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (ac_status st = cross_device(ctx, d_a, n_a, d_b, n_b, n_windows, levels, d_out, 3u, ctx->stream)) return st;
    AC_HIP(ctx, hipMemcpyAsync(cross_host, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    AC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return AC_OK;
}

}  // extern "C"
