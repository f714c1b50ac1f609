// capi_edit.cpp -- the edit-profile calls of the C ABI (include/approx_counter_amd.h "Edit profiles";
// DESIGN.md §4e): per k-mer and base how its best occurrence differs from it, a pass over the hit pairs of
// matrices a launch and the span pass have written.  The kernel is hit_edit.hip's; this file checks the
// arguments and enqueues.  (The samples route, ac_window_edits_samples, is capi.cpp's count_samples with an
// edit buffer per job: it ends in edit_device.)
#include "ctx.h"
#include "hit_edit.h"

using namespace ac_detail;

namespace ac_detail {

ac_status edit_device(ac_ctx* ctx, uint32_t k, const uint64_t* kmers, uint32_t n_kmers, const ac_windows* sample,
                      uint32_t window_len, const uint32_t* hit_plane, const uint32_t* pos, const uint32_t* start,
                      uint32_t* edit_out, hipStream_t stream) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (k < acamd::bs::EP_MIN_K || k > acamd::bs::EP_MAX_K) return fail(ctx, AC_ERR_INVALID, "edit profile: k must be 2..32");
    if (window_len < 1u || window_len > 256u) return fail(ctx, AC_ERR_INVALID, "edit profile: window_len must be 1..256");
    if (!sample) return fail(ctx, AC_ERR_INVALID, "edit profile: sample is NULL");
    const uint64_t stride = ((uint64_t)window_len + 31u) & ~31ull;
    if ((uint64_t)sample->n_windows * stride > sample->n_bases)
        return fail(ctx, AC_ERR_INVALID, "edit profile: n_windows windows of ceil32(window_len) bases do not fit n_bases");
    if (!sample->codes || !sample->nmask) return fail(ctx, AC_ERR_INVALID, "edit profile: the sample's codes or nmask is NULL");
    if (!n_kmers) return AC_OK;
    if (!edit_out) return fail(ctx, AC_ERR_INVALID, "edit profile: the output is NULL");
    if (sample->n_windows) {
        if (!kmers) return fail(ctx, AC_ERR_INVALID, "edit profile: kmers is NULL");
        if (!hit_plane || !pos || !start) return fail(ctx, AC_ERR_INVALID, "edit profile: hit_plane, pos or start is NULL");
    }
    AC_HIP(ctx, hipSetDevice(ctx->device));
    AC_HIP(ctx, acamd::launch_hit_edit_profile(k, kmers, n_kmers, sample->codes, sample->nmask, sample->n_windows, window_len,
                                               hit_plane, pos, start, edit_out, stream));
    return AC_OK;
}

}  // namespace ac_detail

extern "C" {

uint64_t ac_hit_edit_words(uint32_t n_kmers, uint32_t k) { return acamd::bs::ep_words(n_kmers, k); }

ac_status ac_hit_edit_profile_device(ac_ctx* ctx, uint32_t k, const uint64_t* kmers, uint32_t n_kmers, const ac_windows* sample,
                                     uint32_t window_len, const uint32_t* hit_plane, const uint32_t* pos, const uint32_t* start,
                                     uint32_t* edit_out, void* hip_stream) {
    return edit_device(ctx, k, kmers, n_kmers, sample, window_len, hit_plane, pos, start, edit_out, (hipStream_t)hip_stream);
}

ac_status ac_window_edits_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs, uint32_t flank_depth,
                                  uint32_t* const* hits_host, uint32_t* const* pos_host, uint32_t* const* start_host,
                                  uint32_t* const* flank_host, uint32_t* const* edit_host) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (flank_depth > acamd::bs::FL_MAX_DEPTH) return fail(ctx, AC_ERR_INVALID, "flank profile: depth must be 0 (no flanks) or 1..32");
    if (n_jobs && !hits_host) return fail(ctx, AC_ERR_INVALID, "window hits: hits_host is NULL");
    if (n_jobs && !pos_host) return fail(ctx, AC_ERR_INVALID, "window positions: pos_host is NULL");
    if (n_jobs && !start_host) return fail(ctx, AC_ERR_INVALID, "match spans: start_host is NULL");
    if (n_jobs && flank_depth && !flank_host) return fail(ctx, AC_ERR_INVALID, "flank profile: flank_host is NULL");
    if (n_jobs && !edit_host) return fail(ctx, AC_ERR_INVALID, "edit profile: edit_host is NULL");
    static uint32_t* const none[AC_MAX_JOBS] = {};
    // (a depth of 0: no flank pass, whatever flank_host is)
    return count_samples(ctx, k, jobs, n_jobs, hits_host ? hits_host : none, pos_host ? pos_host : none,
                         start_host ? start_host : none, flank_depth ? (flank_host ? flank_host : none) : nullptr, flank_depth,
                         edit_host ? edit_host : none);
}

}  // extern "C"
