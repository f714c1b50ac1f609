// capi_span.cpp -- the match-span calls of the C ABI (include/approx_counter_amd.h "Match spans"; DESIGN.md
// §4e): where each k-mer's best occurrence starts, a pass over the hit pairs of matrices a launch has
// written.  The kernel is hit_span.hip's; this file checks the arguments and enqueues.  (The samples route,
// ac_window_spans_samples, is capi.cpp's count_samples with a start matrix per job: it ends in span_device.)
#include "ctx.h"

using namespace ac_detail;

namespace ac_detail {

ac_status span_device(ac_ctx* ctx, uint32_t k, const uint64_t* kmers, uint32_t n_kmers, const ac_windows* sample,
                      uint32_t window_len, const uint32_t* hits, const uint32_t* pos, uint32_t levels, uint32_t* start_out,
                      hipStream_t stream) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (k < 2u || k > 32u) return fail(ctx, AC_ERR_INVALID, "match spans: k must be 2..32");
    if (levels < 1u || levels > 4u) return fail(ctx, AC_ERR_INVALID, "match spans: levels must be 1..4");
    if (levels >= k) return fail(ctx, AC_ERR_INVALID, "match spans: levels must be below k (an occurrence could be empty)");
    if (window_len < 1u || window_len > 256u) return fail(ctx, AC_ERR_INVALID, "match spans: window_len must be 1..256");
    if (!sample) return fail(ctx, AC_ERR_INVALID, "match spans: sample is NULL");
    const uint64_t stride = ((uint64_t)window_len + 31u) & ~31ull;
    if ((uint64_t)sample->n_windows * stride > sample->n_bases)
        return fail(ctx, AC_ERR_INVALID, "match spans: n_windows windows of ceil32(window_len) bases do not fit n_bases");
    if (!n_kmers || !sample->n_windows) return AC_OK;
    if (!hits || !pos) return fail(ctx, AC_ERR_INVALID, "match spans: hits or pos is NULL");
    if (!sample->codes || !sample->nmask) return fail(ctx, AC_ERR_INVALID, "match spans: the sample's codes or nmask is NULL");
    if (!kmers) return fail(ctx, AC_ERR_INVALID, "match spans: kmers is NULL");
    if (!start_out) return fail(ctx, AC_ERR_INVALID, "match spans: the output is NULL");
    AC_HIP(ctx, hipSetDevice(ctx->device));
    AC_HIP(ctx, acamd::launch_hit_start_positions(k, kmers, n_kmers, sample->codes, sample->nmask, sample->n_windows,
                                                  window_len, hits, pos, levels, start_out, stream));
    return AC_OK;
}

}  // namespace ac_detail

extern "C" {

ac_status ac_hit_start_positions_device(ac_ctx* ctx, uint32_t k, const uint64_t* kmers, uint32_t n_kmers,
                                        const ac_windows* sample, uint32_t window_len, const uint32_t* hits,
                                        const uint32_t* pos, uint32_t levels, uint32_t* start_out, void* hip_stream) {
    return span_device(ctx, k, kmers, n_kmers, sample, window_len, hits, pos, levels, start_out, (hipStream_t)hip_stream);
}

}  // extern "C"
