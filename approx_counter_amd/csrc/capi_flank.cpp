// capi_flank.cpp -- the flank-profile calls of the C ABI (include/approx_counter_amd.h "Flank profiles";
// DESIGN.md §4e): per k-mer the histogram of the bases after the end and before the start of its best
// occurrence, a pass over the hit pairs of matrices a launch and the span pass have written.  The kernel is
// hit_flank.hip's; this file checks the arguments and enqueues.  (The samples route, ac_window_flanks_samples,
// is capi.cpp's count_samples with a flank buffer per job: it ends in flank_device.)
#include "ctx.h"
#include "hit_flank.h"

using namespace ac_detail;

namespace ac_detail {

ac_status flank_device(ac_ctx* ctx, const ac_windows* sample, uint32_t window_len, const uint32_t* hit_plane,
                       const uint32_t* pos, const uint32_t* start, uint32_t n_kmers, uint32_t depth, uint32_t* flank_out,
                       hipStream_t stream) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (depth < 1u || depth > acamd::bs::FL_MAX_DEPTH) return fail(ctx, AC_ERR_INVALID, "flank profile: depth must be 1..32");
    if (window_len < 1u || window_len > 256u) return fail(ctx, AC_ERR_INVALID, "flank profile: window_len must be 1..256");
    if (!sample) return fail(ctx, AC_ERR_INVALID, "flank profile: sample is NULL");
    const uint64_t stride = ((uint64_t)window_len + 31u) & ~31ull;
    if ((uint64_t)sample->n_windows * stride > sample->n_bases)
        return fail(ctx, AC_ERR_INVALID, "flank profile: n_windows windows of ceil32(window_len) bases do not fit n_bases");
    if (!n_kmers) return AC_OK;
    if (!flank_out) return fail(ctx, AC_ERR_INVALID, "flank profile: the output is NULL");
    if (sample->n_windows) {
        if (!sample->codes || !sample->nmask) return fail(ctx, AC_ERR_INVALID, "flank profile: the sample's codes or nmask is NULL");
        if (!hit_plane || !pos) return fail(ctx, AC_ERR_INVALID, "flank profile: hit_plane or pos is NULL");
    }
    AC_HIP(ctx, hipSetDevice(ctx->device));
    AC_HIP(ctx, acamd::launch_hit_flank_profile(sample->codes, sample->nmask, sample->n_windows, window_len, hit_plane, pos,
                                                start, n_kmers, depth, flank_out, stream));
    return AC_OK;
}

}  // namespace ac_detail

extern "C" {

uint64_t ac_hit_flank_words(uint32_t n_kmers, uint32_t depth) { return acamd::bs::fl_words(n_kmers, depth); }

ac_status ac_hit_flank_profile_device(ac_ctx* ctx, const ac_windows* sample, uint32_t window_len, const uint32_t* hit_plane,
                                      const uint32_t* pos, const uint32_t* start, uint32_t n_kmers, uint32_t depth,
                                      uint32_t* flank_out, void* hip_stream) {
    return flank_device(ctx, sample, window_len, hit_plane, pos, start, n_kmers, depth, flank_out, (hipStream_t)hip_stream);
}

ac_status ac_window_flanks_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs, uint32_t depth,
                                   uint32_t* const* hits_host, uint32_t* const* pos_host, uint32_t* const* start_host,
                                   uint32_t* const* flank_host) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (depth < 1u || depth > acamd::bs::FL_MAX_DEPTH) return fail(ctx, AC_ERR_INVALID, "flank profile: depth must be 1..32");
    if (n_jobs && !hits_host) return fail(ctx, AC_ERR_INVALID, "window hits: hits_host is NULL");
    if (n_jobs && !pos_host) return fail(ctx, AC_ERR_INVALID, "window positions: pos_host is NULL");
    if (n_jobs && !start_host) return fail(ctx, AC_ERR_INVALID, "match spans: start_host is NULL");
    if (n_jobs && !flank_host) return fail(ctx, AC_ERR_INVALID, "flank profile: flank_host is NULL");
    static uint32_t* const none[AC_MAX_JOBS] = {};
    return count_samples(ctx, k, jobs, n_jobs, hits_host ? hits_host : none, pos_host ? pos_host : none,
                         start_host ? start_host : none, flank_host ? flank_host : none, depth);
}

}  // extern "C"
