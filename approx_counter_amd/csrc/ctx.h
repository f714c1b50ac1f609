// ctx.h -- the context and the helpers shared by the C-ABI translation units (capi.cpp,
// count_launch.cpp, capi_exact.cpp, capi_comm.cpp, capi_cooc.cpp, capi_cross.cpp, capi_span.cpp, capi_flank.cpp, capi_edit.cpp, jobs_stage.cpp).  Private to the library:
// nothing declared here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: RCCL is resolved at run time (capi_comm.cpp)

#include <string>
#include <thread>
#include <vector>

#include "approx_counter_amd.h"
#include "wm_count.h"

// A synchronous jobs call is cut into up to this many parts (window ranges of
// every job), each packed, sent and counted on its own stream, so a part's
// packing and DMA overlap the previous part's kernel.
#define AC_STAGE_MAX_PARTS 4

#pragma GCC visibility push(hidden)

struct ac_ctx {
    int device = 0;
    int cu_count = 256;
    hipStream_t stream = nullptr;
    std::string err;
    // grow-only device buffers of the samples entry points: every job's k-mers, and their uint32 counts
    void* d_kmers = nullptr;
    void* d_counts = nullptr;
    size_t d_kmers_cap = 0, d_counts_cap = 0;
    std::vector<uint32_t> h_counts;
    // ac_window_hits_samples / ac_window_hits_jobs: the jobs' device hit matrices, one block (grow-only)
    void* d_hits = nullptr;
    size_t d_hits_cap = 0;
    // ac_window_positions_samples / ac_window_positions_jobs: the jobs' device position matrices, likewise
    void* d_pos = nullptr;
    size_t d_pos_cap = 0;
    // ac_window_spans_samples: the jobs' device start matrices, likewise
    void* d_start = nullptr;
    size_t d_start_cap = 0;
    // ac_window_flanks_samples: the jobs' device flank profiles, likewise
    void* d_flank = nullptr;
    size_t d_flank_cap = 0;
    // ac_window_edits_samples: the jobs' device edit profiles, likewise
    void* d_edit = nullptr;
    size_t d_edit_cap = 0;
    // ac_hit_cooccurrence*: the transposed planes the product reads (grow-only; stream-ordered like the
    // count scratch), and the host-buffer call's device matrix and result, back to back
    void* d_cooc = nullptr;
    size_t d_cooc_cap = 0;
    void* d_cooc_io = nullptr;
    size_t d_cooc_io_cap = 0;
    // ac_error_count staging: the inputs packed back to back in pinned host
    // memory, one H2D copy into d_stage, counts copied back into the same
    // pinned block (grow-only)
    void* h_stage = nullptr;
    void* d_stage = nullptr;
    size_t h_stage_cap = 0, d_stage_cap = 0;
    // ac_sample_upload buffers (codes, nmask, start, length) and the exact-count
    // working set (table keys, table counts, small scalars + histogram, forbidden, gather out)
    void* s_buf[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t s_cap[4] = {0, 0, 0, 0};
    // what the upload found about each slot's image: equal windows back to back (their length,
    // else AC_NO_ULEN) and no N anywhere, so the count launch can take the EQ kernel and skip the
    // N bitmap; keyed by the device image it describes
    const uint32_t* s_codes[4] = {nullptr, nullptr, nullptr, nullptr};
    const uint64_t* s_start[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t s_ulen[4] = {AC_NO_ULEN, AC_NO_ULEN, AC_NO_ULEN, AC_NO_ULEN};
    bool s_no_n[4] = {false, false, false, false};
    uint64_t s_windows[4] = {0, 0, 0, 0}, s_bases[4] = {0, 0, 0, 0};
    // (+ the partitioned path's keys, parts, tmp, h1/h2/stot, bstart, phist: e_buf[6..11]; the forbidden
    // set by bucket and its bucket starts: e_buf[12..13])
    void* e_buf[14] = {};
    size_t e_cap[14] = {};
    // the exact count's readbacks (the small block, the list count, the gathered entries): pinned, so each
    // is one DMA into place instead of a copy through HIP's staging buffer (32 KB + 16 MB, at the first call)
    char* e_pin = nullptr;
    size_t e_pin_cap = 0;
    // Count-kernel scratch, one set per stream a launch may run on at the same
    // time as another: the parts of a synchronous jobs call (0 .. MAX_PARTS-1),
    // the parts of a submit (MAX_PARTS ..), so a synchronous call never shares
    // queues / sums / tickets with a submit still in flight on another stream.
    struct Scratch {
        // work-queue counters: two banks of qcap u32; dirty[b] =
        // counters of bank b used by the last launch on it (zeroed by the next launch)
        uint32_t* queue = nullptr;
        uint32_t qcap = 0, bank = 0, dirty[2] = {0, 0};
        // count hand-off scratch: per-slot arrivals and sums, (workgroups << 32) + sum (zero between launches)
        uint64_t* acc = nullptr;
        uint32_t acc_cap = 0;
        // staged launches: per-chunk "copied" flags (= the launch's generation once in device memory)
        uint32_t* stage_gen = nullptr;
        uint32_t stage_gen_cap = 0;
    } sc[2 * AC_STAGE_MAX_PARTS];
    // streams of parts 1.. of a synchronous jobs call (part 0 runs on `stream`)
    // and of a submit (part 0 runs on the caller's stream), with the events that
    // order a submit's parts around the caller's stream
    hipStream_t part_stream[AC_STAGE_MAX_PARTS] = {};
    hipStream_t sub_stream[AC_STAGE_MAX_PARTS] = {};
    hipEvent_t sub_ev[AC_STAGE_MAX_PARTS] = {};
    hipEvent_t sub_zero_ev = nullptr;
    // resident waves of the count kernel per pattern pack P (0 = not queried yet)
    uint32_t resident[2][AC_MAX_PACK + 1] = {};  // [staged][P]
    // ... and of the bit-sliced kernels: [bs_family_index(family)][k] (wm_count.h).  The warm-up queries
    // the counting kernels for k = 16, plain and staged; every other one is queried at its first launch.
    uint32_t resident_bs[acamd::BS_FAMILIES][33] = {};
    // The edit budget E of the approximate counts (ac_set_max_errors; M1(E): a window adds
    // max(0, E + 1 - d)): 2 = the reference's.  Another one counts on bit-sliced launches only
    // (stage_plan.h budget_refusal); on an ac_create_multi context every shard holds the same value.
    uint32_t max_errors = 2;
    int last_kernel = -1;  // the count kernel of the context's last launch: 0 word-parallel, 1 bit-sliced
    // last launch geometry
    uint64_t last_waves = 0;
    uint32_t last_wpw = 0, last_groups = 0;
    // ac_create_multi: contexts of shards 1..n-1 (this context is shard 0)
    std::vector<ac_ctx*> peers;
    // RCCL communicator of a multi-process job (ac_comm_init), or null
    ncclComm_t comm = nullptr;
    // device error word of the asynchronous entry points (ac_check), and a
    // pinned word to read it back through
    uint32_t* d_err = nullptr;
    uint32_t* h_err = nullptr;
    // ac_error_count_jobs staging: two slots used alternately, so a submit
    // packs into one while the previous launch still reads the other.  Each is
    // a pinned host block, a device block (same layout) and an event recorded
    // after the last stream work that reads either.
    struct Slot {
        void* h = nullptr;
        void* d = nullptr;
        void* hd = nullptr;  // device address of the pinned block (staging reads, counts written back)
        size_t h_cap = 0, d_cap = 0;
        hipEvent_t ev = nullptr;
        bool pending = false;
        // the early launch's header (flags, completion): coherent (fine-grained) pinned memory, so
        // the kernel's polls of it reach host memory every time instead of an L2 line
        uint32_t* hdr = nullptr;
        uint32_t* hdr_d = nullptr;
    } slot[3 * AC_STAGE_MAX_PARTS];  // synchronous parts, then two sets of submit parts
    uint32_t next_slot = 0;          // the submit set the next submit uses
    uint32_t gen = 0;                // generation of the last early-launch call (never 0 once used)
    uint32_t early_flip = 0;         // early-launch calls alternate between staging slots 0 and 1
    int exact_path = -1;             // the last exact count's path: 1 partitioned, 0 hash table
    int last_mode = -1;  // ac_stage_mode: 2 the last jobs call was an early launch, 0 the DMA path
    // Warm-up started by ac_create on a thread of its own (ensure_warm joins it before the first count
    // launch): the count kernels' code object is loaded by the occupancy queries, so the first launch
    // -- the CLI's one approximate count per run -- does not pay for it; it overlaps the caller's FASTA
    // parsing and exact count instead.
    std::thread warm;
    uint32_t warm_resident[2][AC_MAX_PACK + 1] = {};
    uint32_t warm_resident_bs[acamd::BS_FAMILIES][33] = {};
};

namespace ac_detail {

// --- capi.cpp: errors, checks, grow-only buffers, the pinned staging copy, pinned host blocks
ac_status fail(ac_ctx* ctx, ac_status st, const std::string& msg);
ac_status hip_fail(ac_ctx* ctx, hipError_t e, const char* what);

#define AC_HIP(ctx, expr)                                  \
    do {                                                   \
        hipError_t e_ = (expr);                            \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #expr); \
    } while (0)

ac_status check_k(ac_ctx* ctx, uint32_t k);
ac_status check_sample(ac_ctx* ctx, const ac_windows* s);
ac_status check_layout(ac_ctx* ctx, const ac_windows& s);
ac_status grow(ac_ctx* ctx, void** buf, size_t* cap, size_t bytes);
inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }
size_t staged_bytes(int n, const size_t* sz);
ac_status h2d_staged(ac_ctx* ctx, int n, const void* const* src, const size_t* sz, void* dst, size_t extra = 0);
// Status for a device error word read back after a launch (wm_count.h).
ac_status device_error(ac_ctx* ctx, uint32_t word);
int env_int(const char* name, int dflt);

struct HostBlock {
    char* h = nullptr;
    size_t n = 0;
    char* d = nullptr;  // device-visible address of h
};
// The block of ac_host_alloc holding [p, p + bytes) (bytes >= 1), if any.
bool find_block(const void* p, size_t bytes, HostBlock* out);

// --- count_launch.cpp: the fused count launch
struct StageLaunch {
    uint32_t gen = 0;
    uint32_t* host_hdr = nullptr;
    const uint8_t* src[AC_MAX_SEGS] = {};
    uint8_t* dst[AC_MAX_SEGS] = {};
    uint32_t chunks[AC_MAX_SEGS] = {};
    uint32_t codes_off[AC_MAX_SEGS] = {};  // bytes of the region before its codes (the k-mers section)
    uint32_t* err_out = nullptr;  // device word the launch's error bits are also or-ed into (submits: ac_check)
    uint32_t tag = 0;              // tagged completion (wm_count.h LaunchArgs::tag)
    uint64_t* grp_err = nullptr;   // its per-group error words (device-visible pinned address)
    uint32_t copiers = 0;          // copier workgroups (wm_count.h LaunchArgs::copier_wgs; 0: nothing to stage)
    // device packing (wm_count.h SegDev::dp_*): the segment's Dna5 bytes and window offsets in
    // pinned host memory, device-visible addresses; dp_src = NULL: the host packed the segment
    const uint8_t* dp_src[AC_MAX_SEGS] = {};
    const uint64_t* dp_off[AC_MAX_SEGS] = {};
    uint32_t dp_bytes[AC_MAX_SEGS] = {};
};
uint32_t stage_copiers(uint64_t tickets);
// Joins ac_create's warm-up thread (once) and takes the resident-wave counts it queried.
void ensure_warm(ac_ctx* ctx);
// One fused count launch over `n` device segments `segs` of k-mer length k, enqueued on `stream`.
struct CountLaunch {
    CountLaunch(uint32_t k_, const ac_segment* segs_, uint32_t n_, hipStream_t stream_)
        : k(k_), segs(segs_), n(n_), stream(stream_) {}
    uint32_t k;
    const ac_segment* segs;
    uint32_t n;
    hipStream_t stream;
    // what a call may set beside them:
    bool zero = true;         // the counts are stored; false: added to what the segments' count vectors hold
    uint32_t* err = nullptr;  // the device word the kernel reports skipped windows in (NULL: the context's, for ac_check)
    int scratch = 0;          // the scratch set (ac_ctx::sc: one per concurrently running stream)
    // (0, 1 = none) limits the launch to 1 / wave_div of its kernel's resident waves, so another launch's
    // waves can be resident beside it
    uint32_t wave_div = 0;
    const bool* no_n = nullptr;  // (optional, per segment) the segment's image is known to hold no N
    // (optional, per segment) AC_NO_ULEN, or all windows have this length and sit back to back at
    // ceil32(ulen)-base strides (start / length unread)
    const uint32_t* ulen = nullptr;
    // A staged launch (the early-launch stage): the kernel copies each segment's region from
    // src (the pinned block) to dst once the host flags it in host_hdr, and reports its completion there.
    const StageLaunch* stage = nullptr;
    const bool* nrec = nullptr;  // (optional, per equal-window segment) its windows carry inline N records (nrec.h)
    // (optional) per segment the device matrix the launch also writes its windows' hit words to (DESIGN.md §4e
    // "Hit levels"); refused -- hits_refusal -- unless the launch is bit-sliced.  A staged launch takes the
    // staged hits kernels (the jobs stage, DESIGN.md §4e "Hits from the jobs stage").
    uint32_t* const* hits = nullptr;
    // (optional, with `hits`) per segment the device matrix of end-position planes the launch writes as well
    // (DESIGN.md §4e "Match end positions"), by the hits-and-positions kernels
    uint32_t* const* pos = nullptr;
    // (optional, with `hits`) per segment the window count of the matrix hits[i] / pos[i] point into, when the
    // segment is a window sub-range [lo, hi) of it (the caller has folded row lo into the pointers); NULL:
    // every segment fills its whole matrix
    const uint32_t* mat_windows = nullptr;
};
ac_status launch(ac_ctx* ctx, const CountLaunch& rq);

// --- capi_span.cpp: ac_hit_start_positions_device's checks and launch (the samples route ends here too)
ac_status span_device(ac_ctx* ctx, uint32_t k, const uint64_t* kmers, uint32_t n_kmers, const ac_windows* sample,
                      uint32_t window_len, const uint32_t* hits, const uint32_t* pos, uint32_t levels, uint32_t* start_out,
                      hipStream_t stream);

// --- capi.cpp: the samples entry points' one body -- the count, and per job the host matrices asked for
// (hits; hits and positions; those and starts; those and the flank profile of `depth` bases; the first three
// and the edit profile, with or without the flank profile)
ac_status count_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs, uint32_t* const* hits_host,
                        uint32_t* const* pos_host = nullptr, uint32_t* const* start_host = nullptr,
                        uint32_t* const* flank_host = nullptr, uint32_t depth = 0, uint32_t* const* edit_host = nullptr);

// --- capi_flank.cpp: ac_hit_flank_profile_device's checks and launch (the samples route ends here too)
ac_status flank_device(ac_ctx* ctx, const ac_windows* sample, uint32_t window_len, const uint32_t* hit_plane,
                       const uint32_t* pos, const uint32_t* start, uint32_t n_kmers, uint32_t depth, uint32_t* flank_out,
                       hipStream_t stream);

// --- capi_edit.cpp: ac_hit_edit_profile_device's checks and launch (the samples route ends here too)
ac_status edit_device(ac_ctx* ctx, uint32_t k, const uint64_t* kmers, uint32_t n_kmers, const ac_windows* sample,
                      uint32_t window_len, const uint32_t* hit_plane, const uint32_t* pos, const uint32_t* start,
                      uint32_t* edit_out, hipStream_t stream);

// --- capi_comm.cpp
void comm_destroy(ac_ctx* ctx);  // the context's communicator, if it has one (ac_destroy)

}  // namespace ac_detail

#pragma GCC visibility pop
