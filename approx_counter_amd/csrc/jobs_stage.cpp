// jobs_stage.cpp -- ac_error_count_jobs / _submit: the whole errorCount stage from Dna5 host buffers
// (DESIGN.md §4c, §4d).  One launch of the stage is a sequence of steps (stage_and_launch): plan
// (stage_plan.cpp), choose device packing, acquire the staging slot, then either the early launch
// with its publishing loop or the DMA path.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "approx_counter_amd_testing.h"
#include "ctx.h"
#include "host_pack.h"
#include "stage_plan.h"

using namespace ac_detail;
using acamd::JobPlan;
using acamd::Task;

namespace {

// Test-only hooks (ac_testing_stage_hooks, include/approx_counter_amd_testing.h; never set by the
// product): AC_TESTING_UNFLAG_LAST leaves a call's last job unflagged, so the kernel's bounded wait
// runs out (the synchronous call then retries through the DMA path); AC_TESTING_ALL_AHEAD sends every
// job ahead of the staged launch (the staged kernel on resident input, a diagnostic of its own cost).
std::atomic<uint32_t> g_test_hooks{0};

// Device packing of jobs whose samples lie in ac_host_alloc blocks: 2 = auto (default),
// 1 = every eligible job (AC_DEVICE_PACK=1, or the test hook AC_TESTING_DEVICE_PACK), 0 = never
// (AC_DEVICE_PACK=0: the host pool packs).
int device_pack_mode() {
#ifdef AC_NO_DEVICE_PACK
    return 0;  // (A/B builds: the kernel has no device packer)
#endif
    if (g_test_hooks.load(std::memory_order_relaxed) & AC_TESTING_DEVICE_PACK) return 1;
    static const int v = [] {
        const char* e = std::getenv("AC_DEVICE_PACK");
        return (e && *e) ? (std::atoi(e) ? 1 : 0) : 2;
    }();
    return v;
}
// Auto: the kernel packs a call of at least this many windows.  Below it the host pool, which packs a
// cfg2 call in a few microseconds, is ahead: cfg2 stage 0.1145-0.1149 ms host-packed against
// 0.1262-0.1292 device-packed (the image crosses PCIe as 1 B/base instead of 0.25, 2 MB per call;
// profiles/r06_m4/abdev_*), and still with an 8-rank node's 1-participant pool: 0.1150 / 0.1158
// against 0.1270 / 0.1302 (profiles/r06_m10/rank8_*; round 6 first device-packed every call of a pool
// of <= 2 participants, which cost a cfg2 rank at N = 8 those 12 us).  At cfg3-cfg5 the two are within
// 1-3 % and the device-packed steps have no host-side tail (profiles/r06_m3/stall*, abbig_*).
uint64_t device_pack_min_windows() {
    static const uint64_t v = (uint64_t)std::max(0, env_int("AC_DEVICE_PACK_MIN_WINDOWS", 1 << 16));
    return v;
}

// The smallest packing task, in windows (stage_plan.cpp cut_tasks; AC_TASK_WINDOWS overrides, A/B runs).
uint64_t task_windows() {
    static const uint64_t v = (uint64_t)std::max(1, env_int("AC_TASK_WINDOWS", 1280));
    return v;
}

// The early-launch stage for calls on one device, synchronous calls and submits alike (default:
// AC_STAGE_EARLY=1).  0 = the pack -> copy kernel / copy engine -> launch order of round 2; 2 = the
// first job sent ahead of the launch by the copy kernel, the others staged by the count kernel.
// Same box, interleaved (profiles/r03_m2/summary.log): cfg2 step 0.141-0.143 vs 0.148-0.149 ms.
int stage_early() {
    static const int v = [] {
        const char* e = std::getenv("AC_STAGE_EARLY");
        return e ? std::max(0, std::min(2, std::atoi(e))) : 1;
    }();
    return v;
}

// AC_STAGE_TRACE=1: per-phase host timings of the jobs stage, summed over the
// calls and printed to stderr at exit (a measurement aid; no effect otherwise).
enum Phase { PH_SPAN, PH_LAYOUT, PH_PACK, PH_H2D_ENQ, PH_LAUNCH_ENQ, PH_D2H_ENQ, PH_SYNC, PH_WIDEN, PH_COUNT };
struct StageTrace {
    bool on = std::getenv("AC_STAGE_TRACE") != nullptr;
    double sum[PH_COUNT] = {};
    double cur[PH_COUNT] = {};
    uint64_t calls = 0;
    std::vector<std::vector<double>> per_call;  // AC_STAGE_TRACE=2: every call's phases
    void add(Phase i, double us) {
        sum[i] += us;
        cur[i] += us;
    }
    void end_call() {
        if (std::getenv("AC_STAGE_TRACE")[0] == '2') per_call.emplace_back(cur, cur + PH_COUNT);
        for (double& x : cur) x = 0.0;
    }
    void skip_warmup() {  // the first calls allocate: leave them out of the means
        if (calls == 5) {
            for (double& x : sum) x = 0.0;
        }
    }
    ~StageTrace() {
        if (!on || !calls) return;
        static const char* names[PH_COUNT] = {"span", "layout", "pack", "h2d_enq", "launch_enq", "d2h_enq", "sync", "widen"};
        const double n = calls > 5 ? double(calls - 5) : double(calls);
        const char* lr = std::getenv("LOCAL_RANK");
        std::fprintf(stderr, "[ac stage trace] local rank %s, %llu calls (first 5 left out), mean us:", lr ? lr : "-",
                     (unsigned long long)calls);
        for (int i = 0; i < PH_COUNT; ++i) std::fprintf(stderr, " %s %.1f", names[i], sum[i] / n);
        std::fprintf(stderr, "\n");
        for (size_t c = 0; c < per_call.size(); ++c) {
            std::fprintf(stderr, "[ac stage call %zu]", c);
            for (int i = 0; i < PH_COUNT; ++i) std::fprintf(stderr, " %s %.1f", names[i], per_call[c][i]);
            std::fprintf(stderr, "\n");
        }
    }
};
StageTrace g_trace;
inline double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// The time since the last mark goes to the phase that ends here.
struct PhaseClock {
    double tt = g_trace.on ? now_us() : 0.0;
    void mark(Phase i) {
        if (!g_trace.on) return;
        const double t = now_us();
        g_trace.add(i, t - tt);
        tt = t;
    }
};

// DMA-mode transfer of a one-part call: a copy kernel on the compute queue reads the pinned
// block once over PCIe and writes the device block, so the count kernel follows it on the
// same queue, rather than hipMemcpyAsync (the copy engine, whose completion -> kernel start
// costs ~9 us at cfg2); job by job, so job j's inputs travel while job j + 1 is packed; equal
// windows counted with arithmetic descriptors.  Each won its A/B (profiles/r02_stage_pipe_blit_ab.log:
// sync 114-118 vs 130-132 us; r02_stage_ulen_ab.log), and the switches are gone.
// Shape (A/B builds: tools/variants.sh).  64-thread workgroups with 4 loads in flight per
// thread measured faster on one box -- cfg2 stage p50 0.146-0.147 ms vs 0.150-0.159 for
// 256 x 2 (profiles/r02_blit_shape_ab.log) -- but no GPU box was free to run the test
// suite on it before round 2 ended, so the tested 256 x 2 stays the default.
#ifndef AC_BLIT_THREADS
#define AC_BLIT_THREADS 256
#endif
#ifndef AC_BLIT_UNROLL
#define AC_BLIT_UNROLL 2
#endif
constexpr uint32_t BLIT_THREADS = AC_BLIT_THREADS, BLIT_UNROLL = AC_BLIT_UNROLL;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(BLIT_THREADS) stage_blit_kernel(const u32x4* __restrict__ src,
                                                                  u32x4* __restrict__ dst, uint32_t n16) {
    const uint32_t i0 = blockIdx.x * (BLIT_THREADS * BLIT_UNROLL) + threadIdx.x;
    u32x4 v[BLIT_UNROLL];
#pragma unroll
    for (uint32_t u = 0; u < BLIT_UNROLL; ++u)
        if (i0 + u * BLIT_THREADS < n16) v[u] = __builtin_nontemporal_load(src + i0 + u * BLIT_THREADS);
#pragma unroll
    for (uint32_t u = 0; u < BLIT_UNROLL; ++u)
        if (i0 + u * BLIT_THREADS < n16) dst[i0 + u * BLIT_THREADS] = v[u];
}
// bytes: a multiple of 16 (the stage's offsets are 256-aligned)
hipError_t stage_blit_launch(const void* src_dev, void* dst, size_t bytes, hipStream_t stream) {
    const size_t n16 = bytes / 16;
    if (n16 == 0) return hipSuccess;
    if (n16 >= (1ull << 32)) return hipErrorInvalidValue;
    const uint32_t per = BLIT_THREADS * BLIT_UNROLL;
    const uint32_t blocks = (uint32_t)((n16 + per - 1) / per);
    stage_blit_kernel<<<blocks, BLIT_THREADS, 0, stream>>>((const u32x4*)src_dev, (u32x4*)dst, (uint32_t)n16);
    return hipGetLastError();
}

// Some job has candidates and windows (a launch with work, so tagged counts to wait for).
bool live_work(const ac_job* jobs, uint32_t n_jobs) {
    for (uint32_t j = 0; j < n_jobs; ++j)
        if (jobs[j].n_kmers && jobs[j].sample.n_windows) return true;
    return false;
}

// Spin until every count of the live jobs and every group error word of a tagged early launch
// carries the launch's generation (high half); hipStreamQuery every 1024 spins catches a launch that
// failed or finished without writing them.
ac_status wait_tagged(ac_ctx* ctx, const ac_job* jobs, uint32_t n_jobs, const JobPlan& p, const char* h,
                      hipStream_t stream) {
    uint32_t spins = 0;
    auto await = [&](const uint64_t* w) -> ac_status {
        while ((uint32_t)(__atomic_load_n(w, __ATOMIC_ACQUIRE) >> 32) != p.gen) {
            __builtin_ia32_pause();
            if ((++spins & 1023u) == 0u) {
                const hipError_t q = hipStreamQuery(stream);
                if (q == hipErrorNotReady) continue;
                if (q != hipSuccess) return hip_fail(ctx, q, "early launch");
                if ((uint32_t)(__atomic_load_n(w, __ATOMIC_ACQUIRE) >> 32) == p.gen) break;
                return fail(ctx, AC_ERR_INTERNAL, "early launch finished without writing its counts");
            }
        }
        return AC_OK;
    };
    // the group error words first (one per candidate group: each arrives with its group's counts)
    const uint64_t* ge = (const uint64_t*)(h + p.off_gerr);
    for (uint32_t i = 0; i < p.n_gerr; ++i)
        if (ac_status st = await(ge + i)) return st;
    for (uint32_t j = 0; j < n_jobs && j < p.n; ++j) {
        if (!jobs[j].n_kmers || p.hi[j] <= p.lo[j]) continue;
        const uint64_t* hc = (const uint64_t*)(h + p.off_counts[j]);
        for (uint32_t i = 0; i < jobs[j].n_kmers; ++i)
            if (ac_status st = await(hc + i)) return st;
    }
    return AC_OK;
}

ac_status check_jobs(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (ac_status st = check_k(ctx, k)) return st;
    if (n_jobs > AC_MAX_JOBS) return fail(ctx, AC_ERR_INVALID, "too many jobs in one call (max 4)");
    if (n_jobs && !jobs) return fail(ctx, AC_ERR_INVALID, "jobs is NULL");
    for (uint32_t j = 0; j < n_jobs; ++j) {
        const ac_job& b = jobs[j];
        if (b.n_kmers && !b.kmers) return fail(ctx, AC_ERR_INVALID, "job kmers is NULL");
        if (b.sample.n_windows && (!b.sample.bases || !b.sample.offset || !b.sample.length))
            return fail(ctx, AC_ERR_INVALID, "job sample has a NULL array");
    }
    // An edit budget other than 2 (ac_set_max_errors) counts on bit-sliced launches only.  A call may
    // become several launches (parts, shards), each of which asks budget_refusal of its own plan; the
    // whole call is asked first, over every job's whole sample -- whose parts are equal windows when
    // it is -- so that a call that is refused has launched nothing.
    if (ctx->max_errors != 2u) {
        bool live[AC_MAX_JOBS];
        uint32_t ulen[AC_MAX_JOBS];
        for (uint32_t j = 0; j < n_jobs; ++j) {
            const ac_dna5_windows& s = jobs[j].sample;
            live[j] = jobs[j].n_kmers && s.n_windows;
            ulen[j] = s.n_windows ? s.length[0] : AC_NO_ULEN;
            for (uint32_t i = 1; i < s.n_windows && ulen[j] != AC_NO_ULEN; ++i)
                if (s.length[i] != ulen[j]) ulen[j] = AC_NO_ULEN;
        }
        if (const char* why = acamd::budget_refusal(ctx->max_errors, k, n_jobs, live, ulen))
            return fail(ctx, AC_ERR_INVALID, why);
    }
    return AC_OK;
}

// ---------------------------------------------------------------------------
// The steps of one launch of the stage.

// What stage_and_launch was asked to do (its arguments), for the steps that run the launch.
struct StageCall {
    ac_ctx* ctx;
    uint32_t k;
    const ac_job* jobs;
    JobPlan& p;
    hipStream_t stream;
    uint32_t* d_counts;
    int part;
    uint32_t wave_div;
    bool zero;
    // hits from the jobs stage: the jobs' whole device matrices (NULL: a plain count), of which this launch
    // writes the rows of its window ranges (JobPlan::mat_row_off)
    uint32_t* const* hits;
    uint32_t* const* pos;
};

// The launch's rows of the jobs' matrices: the first row of the launch's window range folded into the
// pointers (a job without work here keeps none), for launch()'s hits / pos / mat_windows.
struct PartMats {
    uint32_t* hits[AC_MAX_JOBS] = {};
    uint32_t* pos[AC_MAX_JOBS] = {};
    PartMats(const StageCall& c) {
        for (uint32_t j = 0; j < c.p.n; ++j) {
            const bool work = c.jobs[j].n_kmers && c.p.hi[j] > c.p.lo[j];
            if (work && c.hits && c.hits[j]) hits[j] = c.hits[j] + c.p.mat_row_off[j];
            if (work && c.pos && c.pos[j]) pos[j] = c.pos[j] + c.p.mat_row_off[j];
        }
    }
};

// What the stage's two launches (the early one and the DMA path's) ask of launch() alike.
CountLaunch count_request(const StageCall& c, const ac_segment* segs, const PartMats& mats, const bool* no_n) {
    CountLaunch rq(c.k, segs, c.p.n, c.stream);
    rq.zero = c.zero;
    rq.scratch = c.p.scratch;
    rq.no_n = no_n;
    rq.ulen = c.p.ulen;
    rq.nrec = c.p.nrec;
    rq.hits = c.hits ? mats.hits : nullptr;
    rq.pos = c.hits && c.pos ? mats.pos : nullptr;
    rq.mat_windows = c.p.mat_windows;
    return rq;
}

// Device packing: device-visible addresses of the device-packed jobs' Dna5 bytes and
// window offsets, and the bytes readable from the former.
struct DevicePack {
    const uint8_t* src[AC_MAX_JOBS] = {};
    const uint64_t* off[AC_MAX_JOBS] = {};
    uint32_t bytes[AC_MAX_JOBS] = {};
};

// A job of equal windows (1..256 bases) whose Dna5 bytes and window
// offsets lie in ac_host_alloc blocks is packed by the kernel's copier workgroups straight from them;
// the host packs nothing of it (its region in the staging block stays unwritten): its tasks are
// dropped.  Not with jobs sent ahead of the launch (p.pre: those are host-packed and copied by the
// copy kernel).  Fills p.dp / p.dp_any and dp.
void choose_device_pack(const ac_job* jobs, JobPlan& p, std::vector<Task>& tasks, DevicePack& dp) {
    p.dp_any = false;
    const int dpm = device_pack_mode();
    if (!(p.early && p.pre == 0 && (dpm == 1 || (dpm == 2 && p.total_w >= device_pack_min_windows())))) return;
    for (uint32_t j = 0; j < p.n; ++j) {
        p.dp[j] = false;
        const ac_dna5_windows& w = jobs[j].sample;
        const uint32_t nw = p.hi[j] - p.lo[j];
        if (!jobs[j].n_kmers || !nw || p.ulen[j] == AC_NO_ULEN || p.ulen[j] == 0 || p.ulen[j] > 256 || !p.chunks[j])
            continue;
        HostBlock bb, bo;
        if (!find_block(w.bases, 1, &bb) || !find_block(w.offset + p.lo[j], sizeof(uint64_t) * nw, &bo)) continue;
        const size_t extent = (size_t)(bb.h + bb.n - (const char*)w.bases);  // bytes readable from `bases`
        if (extent < p.ulen[j] || extent >= (size_t(1) << 31)) continue;
        p.dp[j] = p.dp_any = true;
        dp.src[j] = (const uint8_t*)(bb.d + ((const char*)w.bases - bb.h));
        dp.off[j] = (const uint64_t*)(bo.d + ((const char*)(w.offset + p.lo[j]) - bo.h));
        dp.bytes[j] = (uint32_t)extent;
    }
    if (p.dp_any)  // the host packs only the other jobs' windows
        tasks.erase(std::remove_if(tasks.begin(), tasks.end(), [&](const Task& x) { return p.dp[x.job]; }), tasks.end());
}

// The call's staging slot, ready to be packed into: the pinned block, the device block, the
// device-visible address of the pinned block (the kernel writes the error word and the counts
// straight into it, so no copy comes back; profiles/r02_stage_dma_back_ab.log) and the early
// launch's header.
struct SlotMem {
    ac_ctx::Slot* sl = nullptr;
    char *h = nullptr, *d = nullptr, *hd = nullptr;
    uint32_t* hdr = nullptr;
};

// Waits until the launch that last read the slot has finished, grows its blocks to the plan, copies
// the k-mers in and zeroes what the kernel must not find stale: the error word, the tagged area,
// the header.
ac_status acquire_slot(ac_ctx* ctx, const ac_job* jobs, const JobPlan& p, SlotMem* out) {
    ac_ctx::Slot& sl = ctx->slot[p.slot];
    if (sl.pending) {
        AC_HIP(ctx, hipEventSynchronize(sl.ev));
        sl.pending = false;
    }
    if (!sl.ev) AC_HIP(ctx, hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    if (sl.h_cap < p.total) {
        if (sl.h) (void)hipHostFree(sl.h);
        sl.h = nullptr;
        sl.hd = nullptr;
        sl.h_cap = 0;
        const size_t cap = p.total + p.total / 4;
        AC_HIP(ctx, hipHostMalloc(&sl.h, cap, hipHostMallocDefault));
        sl.h_cap = cap;
        AC_HIP(ctx, hipHostGetDevicePointer(&sl.hd, sl.h, 0));
    }
    if (ac_status st = grow(ctx, &sl.d, &sl.d_cap, p.total)) return st;
    char* h = (char*)sl.h;
    for (uint32_t j = 0; j < p.n; ++j) {
        if (jobs[j].n_kmers) std::memcpy(h + p.off_kmers[j], jobs[j].kmers, sizeof(uint64_t) * jobs[j].n_kmers);
        if (p.no_bases[j]) {  // no window bases: the one 32-base block is zero
            std::memset(h + p.off_codes[j], 0, 2 * sizeof(uint32_t));
            std::memset(h + p.off_nmask[j], 0, sizeof(uint32_t));
        }
    }
    *(uint32_t*)(h + p.off_err) = 0u;
    // tagged completion: no count or error word may carry this call's generation before the kernel
    // writes it (the slot last held other data)
    if (p.tag) std::memset(h + p.off_counts[0], 0, p.total - p.off_counts[0]);
    // early launch: flags cleared before the launch (the slot's last
    // launch has finished: its event was waited for above)
    const size_t hdr_bytes = sizeof(uint32_t) * AC_QUEUE_LINE * AC_HDR_LINES;
    if (p.early && !sl.hdr) {
        AC_HIP(ctx, hipHostMalloc((void**)&sl.hdr, hdr_bytes, hipHostMallocCoherent | hipHostMallocMapped));
        AC_HIP(ctx, hipHostGetDevicePointer((void**)&sl.hdr_d, sl.hdr, 0));
    }
    if (p.early) std::memset(sl.hdr, 0, hdr_bytes);
    out->sl = &sl;
    out->h = h;
    out->d = (char*)sl.d;
    out->hd = (char*)sl.hd;
    out->hdr = sl.hdr;
    return AC_OK;
}

// Packs task t of the plan into the pinned block, and notes per task whether the job needs its N
// bitmap for these windows (an N, or with records an overflowed record).
struct Packer {
    const ac_job* jobs;
    const JobPlan& p;
    const std::vector<Task>& tasks;
    char* h;
    std::vector<uint8_t> task_n;
    Packer(const ac_job* jobs_, const JobPlan& p_, const std::vector<Task>& tasks_, char* h_)
        : jobs(jobs_), p(p_), tasks(tasks_), h(h_), task_n(tasks_.size(), 0) {}
    void operator()(uint32_t t) {
        const Task& x = tasks[t];
        const ac_dna5_windows& w = jobs[x.job].sample;
        const uint32_t j = x.job, r = x.w0 - p.lo[j];
        const uint32_t f = acamd::pack_dna5_range(w.bases, w.offset, w.length, x.w0, x.w1, x.first,
                                                  (uint32_t*)(h + p.off_codes[j]), (uint32_t*)(h + p.off_nmask[j]),
                                                  (uint64_t*)(h + p.off_start[j]) + r,
                                                  (uint32_t*)(h + p.off_len[j]) + r, p.nrec[j]);
        task_n[t] = (f & (p.nrec[j] ? acamd::PACK_OVERFLOW : acamd::PACK_HAS_N)) != 0u;
    }
    bool job_no_n(uint32_t j) const {
        for (size_t t = 0; t < tasks.size(); ++t)
            if (tasks[t].job == j && task_n[t]) return false;
        return true;
    }
};

// The launch's segments: job j's arrays in the device block, its counts in d_counts (job j at
// d_counts + sum of the earlier n_kmers) or, when NULL, in the slot's pinned counts area.
void make_segs(const ac_job* jobs, const JobPlan& p, const SlotMem& m, uint32_t* d_counts, ac_segment* segs) {
    uint64_t cbase = 0;
    for (uint32_t j = 0; j < p.n; ++j) {
        ac_segment& g = segs[j];
        const uint32_t nw = jobs[j].n_kmers ? p.hi[j] - p.lo[j] : 0;
        g.kmers = (const uint64_t*)(m.d + p.off_kmers[j]);
        g.n_kmers = jobs[j].n_kmers;
        g.sample = ac_windows{(const uint32_t*)(m.d + p.off_codes[j]), (const uint32_t*)(m.d + p.off_nmask[j]),
                              (const uint64_t*)(m.d + p.off_start[j]), (const uint32_t*)(m.d + p.off_len[j]), nw,
                              p.n_bases[j]};
        g.counts = d_counts ? d_counts + cbase : (uint32_t*)(m.hd + p.off_counts[j]);
        cbase += jobs[j].n_kmers;
    }
}

#ifndef AC_PUBLISH_STEP
#define AC_PUBLISH_STEP 16384
#endif
constexpr uint64_t PUBLISH_STEP = AC_PUBLISH_STEP;  // bytes of new prefix worth a header store

struct alignas(64) Done {
    std::atomic<uint32_t> v;
};

// The early launch's publishing loop.
// Progress records: the packed N-free prefix of each job's region (its k-mers, then the
// codes of its first tasks up to the first task holding an N), so the kernel moves chunks
// over PCIe -- and counts their windows -- while the rest of the job is packed.  Tasks are
// claimed in order but finish out of order; this thread alone publishes (a plain 8-byte
// store, read whole by the kernel's 16-byte header load): between the tasks it packs
// itself, it advances over the tasks the workers have finished.  (Publishing from the
// workers -- CAS on the one header line the GPU polls -- cost ~7 us of packing per call.)
struct EarlyRun {
    const StageCall& c;
    JobPlan& p;
    const std::vector<Task>& tasks;
    const SlotMem& m;
    Packer& pack;
    const StageLaunch& stg;
    PhaseClock& clk;
    const uint32_t hooks;
    acamd::WorkPool& pool;

    std::unique_ptr<Done[]> t_done;      // per task: packed
    std::vector<uint32_t> jt[AC_MAX_JOBS];  // per job: its tasks in claim order
    uint64_t ready[AC_MAX_JOBS] = {}, published[AC_MAX_JOBS] = {};
    uint32_t nt[AC_MAX_JOBS] = {};  // jt[j][0, nt[j]) seen finished
    bool n_seen[AC_MAX_JOBS] = {}, flagged[AC_MAX_JOBS] = {}, no_n[AC_MAX_JOBS] = {};
    uint32_t helped = 0, left_jobs = 0;
    uint32_t slow_left;  // (test-only hook AC_TESTING_SLOW_HOST: sleeps left)
    bool launched = false, first_flag = true;

    EarlyRun(const StageCall& c_, const std::vector<Task>& tasks_, const SlotMem& m_, Packer& pack_,
             const StageLaunch& stg_, PhaseClock& clk_, uint32_t hooks_)
        : c(c_), p(c_.p), tasks(tasks_), m(m_), pack(pack_), stg(stg_), clk(clk_), hooks(hooks_),
          pool(acamd::host_pool()), t_done(new Done[tasks_.size() + 1]),
          slow_left((hooks_ & AC_TESTING_SLOW_HOST) ? 12u : 0u) {
        for (size_t t = 0; t < tasks.size(); ++t) t_done[t].v.store(0, std::memory_order_relaxed);
    }

    void publish(uint32_t j, uint64_t bytes) {
        __atomic_store_n((uint64_t*)(m.hdr + j * AC_QUEUE_LINE + AC_HDR_PGEN), (bytes << 32) | p.gen, __ATOMIC_RELEASE);
        if (launched && slow_left) {
            --slow_left;
            std::this_thread::sleep_for(std::chrono::milliseconds(60));
        }
    }

    // The staged launch.  (The slot's event is recorded after the publishing loop, not right after
    // the launch: the caller's first progress records went out 1.2 us later with it there.)
    ac_status go() {
        ac_segment segs[AC_MAX_JOBS];
        make_segs(c.jobs, p, m, c.d_counts, segs);
        const PartMats mats(c);
        CountLaunch rq = count_request(c, segs, mats, no_n);
        rq.stage = &stg;
        if (ac_status st = launch(c.ctx, rq)) return st;
        clk.mark(PH_LAUNCH_ENQ);
        launched = true;
        return AC_OK;
    }
    ac_status record_slot() {
        if (!launched) return AC_OK;
        launched = false;
        AC_HIP(c.ctx, hipEventRecord(m.sl->ev, c.stream));
        m.sl->pending = true;
        return AC_OK;
    }

    // Job j is finished: its final byte count and N verdict, then its flag (or, jobs below
    // `pre`, the copy kernel sends it ahead of the launch; those finish in job order).
    ac_status finalize(uint32_t j) {
        const bool nn = pack.job_no_n(j);
        const size_t bytes = nn && p.ulen[j] != AC_NO_ULEN ? p.off_nmask[j] - p.off_kmers[j] : p.region[j];
        if (j < p.pre) {  // sent ahead of the launch, which follows it on the stream
            no_n[j] = nn;
            hipError_t e = stage_blit_launch(m.hd + p.off_kmers[j], m.d + p.off_kmers[j], bytes, c.stream);
            ac_status st = e == hipSuccess ? AC_OK : hip_fail(c.ctx, e, "stage transfer");
            if (st == AC_OK && j + 1 == p.pre) st = go();
            return st;
        }
        uint32_t* line = m.hdr + j * AC_QUEUE_LINE;
        // no N: the whole region is N-free (never below a prefix: the codes end inside the
        // bytes sent); with N the published prefix stays where the first N stopped it
        if (nn) publish(j, bytes);
        line[AC_HDR_INFO] = (uint32_t)bytes | (nn ? 0u : AC_HDR_INFO_HAS_N);
        // (test-only hook: the last job left unflagged, tests/test_gpu_jobs.py)
        if (!((hooks & AC_TESTING_UNFLAG_LAST) && j + 1 == p.n))
            __atomic_store_n(&line[AC_HDR_FLAG], p.gen, __ATOMIC_RELEASE);  // the kernel's waves may go
        if (first_flag) clk.mark(PH_H2D_ENQ);  // (AC_STAGE_TRACE: launch -> first job flagged, in "h2d_enq")
        first_flag = false;
        return AC_OK;
    }

    // Job j: takes in the tasks finished since the last look, publishes the new prefix when it is
    // worth a record, and finalizes the job once all of it is published.
    ac_status advance(uint32_t j) {
        const uint64_t base_off = p.off_codes[j] - p.off_kmers[j];
        const uint32_t nj = (uint32_t)jt[j].size();
        while (nt[j] < nj && t_done[jt[j][nt[j]]].v.load(std::memory_order_acquire)) {
            const Task& x = tasks[jt[j][nt[j]]];
            // (with records the kernel counts any packed window; one that overflowed its
            // record waits for the job's N bitmap by itself)
            n_seen[j] = n_seen[j] || (pack.task_n[jt[j][nt[j]]] && !p.nrec[j]);
            if (!n_seen[j]) ready[j] = base_off + (x.first + x.span) / 4;
            ++nt[j];
        }
        // (the first codes at once, however few: the kernel may be waiting for them)
        if (ready[j] >= published[j] + PUBLISH_STEP || (nt[j] == nj && ready[j] > published[j]) ||
            (published[j] == base_off && ready[j] > published[j])) {
            // (test-only slow host: one step per record while its sleeps last)
            const uint64_t r = slow_left ? std::min(ready[j], published[j] + PUBLISH_STEP) : ready[j];
            publish(j, r);
            published[j] = r;
        }
        if (nt[j] == nj && published[j] == ready[j]) {
            if (ac_status st = finalize(j)) return st;
            flagged[j] = true;
            --left_jobs;
        }
        return AC_OK;
    }

    ac_status run() {
        const std::function<void(uint32_t)> pack_counted = [this](uint32_t t) {
            pack(t);
            t_done[t].v.store(1, std::memory_order_release);
        };
        // the k-mers are in place already (copied with the layout)
        for (uint32_t j = 0; j < p.n; ++j) publish(j, p.off_codes[j] - p.off_kmers[j]);
        // the workers start packing job 0 while this thread launches the kernel
        pool.begin((uint32_t)tasks.size(), pack_counted);
        if (p.pre == 0)
            if (ac_status st = go()) {
                pool.finish();
                return st;
            }
        for (uint32_t t = 0; t < (uint32_t)tasks.size(); ++t) jt[tasks[t].job].push_back(t);
        left_jobs = p.n;
        for (uint32_t j = 0; j < p.n; ++j) {
            ready[j] = published[j] = p.off_codes[j] - p.off_kmers[j];
            if (p.dp[j]) {  // the kernel publishes a device-packed job's words itself: nothing to flag
                flagged[j] = true;
                --left_jobs;
            }
        }
        // With workers, this thread only publishes: packing a task of its own (~8 us at cfg2's
        // 312-window tasks) held every progress record back until it was done.  It still packs when
        // no worker has finished a task for 20 us (workers asleep or descheduled).
        const bool serial = pool.serial();
        // ... except when packing, not publishing, is the bottleneck: a pool of <= 4 participants (a
        // rank's share of the host) or a large call (the kernel counts faster than a few threads
        // pack), where a task of its own delays the records by one task but adds a packer.
        const bool caller_packs = !serial && (pool.size() <= 4 || p.total_w >= (1u << 16));
        uint32_t seen_done = 0, idle_polls = 0;
        auto last_seen = std::chrono::steady_clock::now();
        while (left_jobs) {
            bool help_now = false;
            if (!serial && (++idle_polls & 63u) == 0u) {
                uint32_t d = 0;
                for (uint32_t j = 0; j < p.n; ++j) d += nt[j];
                const auto now = std::chrono::steady_clock::now();
                if (d != seen_done) {
                    seen_done = d;
                    last_seen = now;
                } else if (now - last_seen > std::chrono::microseconds(20)) {
                    help_now = true;
                    last_seen = now;
                }
            }
            if (serial && helped < (uint32_t)tasks.size()) pool.help(++helped);  // packs task helped - 1
            else if (help_now || caller_packs) pool.help_one();
            for (uint32_t j = 0; j < p.n; ++j) {
                if (flagged[j] || (j > 0 && j <= p.pre && !flagged[j - 1])) continue;  // (pre: in job order)
                if (ac_status st = advance(j)) {
                    pool.finish();
                    (void)record_slot();
                    return st;
                }
            }
            if (!(serial && helped < (uint32_t)tasks.size()) && left_jobs) __builtin_ia32_pause();
        }
        pool.finish();
        clk.mark(PH_PACK);
        return record_slot();
    }
};

// Early launch: the count kernel is launched before the later jobs are
// packed; the pool packs job by job and the host flags each job in the header as soon
// as it is complete; the kernel copies a flagged job's region into device memory itself
// and counts it while the next job is still being packed.  The region of job j: k-mers,
// codes, then the N bitmap unless the job holds no N, and the window descriptors unless
// its windows have one length.  The first `pre` jobs (AC_STAGE_EARLY=2: the first; the test hook
// AC_TESTING_ALL_AHEAD: all) are sent before the launch by the copy kernel instead, stream-ordered
// ahead of it.
// (Packing the jobs' tasks interleaved, so both ends arrive together, was slower:
// 0.144 vs 0.134 ms per cfg2 step -- each end's last chunk waits for its final header,
// which then came ~27 us into the kernel for both; profiles/r03_stage/r03_early12_step3.log.)
ac_status run_early(const StageCall& c, std::vector<Task>& tasks, const DevicePack& dp, const SlotMem& m, Packer& pack,
                    PhaseClock& clk, uint32_t hooks) {
    JobPlan& p = c.p;
    StageLaunch stg;
    if (++c.ctx->gen == 0) ++c.ctx->gen;
    p.gen = stg.gen = c.ctx->gen;
    stg.host_hdr = m.sl->hdr_d;
    stg.err_out = c.d_counts ? c.ctx->d_err : nullptr;  // a submit reports through ac_check
    stg.tag = p.tag ? 1u : 0u;
    stg.grp_err = p.tag ? (uint64_t*)(m.hd + p.off_gerr) : nullptr;
    for (uint32_t j = 0; j < p.n; ++j) {
        stg.src[j] = (const uint8_t*)(m.hd + p.off_kmers[j]);
        stg.dst[j] = (uint8_t*)(m.d + p.off_kmers[j]);
        stg.chunks[j] = p.chunks[j];
        stg.codes_off[j] = p.codes_off[j];
        stg.dp_src[j] = dp.src[j];
        stg.dp_off[j] = dp.off[j];
        stg.dp_bytes[j] = dp.bytes[j];
    }
    stg.copiers = p.copiers;
    // A large call (copier workgroups) packs its jobs' tasks interleaved, so every segment's
    // windows arrive from the start and no segment's waves sit idle while the jobs before it are
    // packed (each copier workgroup starts on its own segment, wm_count.hip).  Small calls keep
    // job order (see above).
    if (stg.copiers && p.n > 1 && p.pre == 0) {
        std::vector<Task> by_job[AC_MAX_JOBS];
        for (const Task& x : tasks) by_job[x.job].push_back(x);
        const size_t n_tasks = tasks.size();
        tasks.clear();
        for (size_t i = 0; tasks.size() < n_tasks; ++i)
            for (uint32_t j = 0; j < p.n; ++j)
                if (i < by_job[j].size()) tasks.push_back(by_job[j][i]);
    }
    EarlyRun run(c, tasks, m, pack, stg, clk, hooks);
    return run.run();
}

// DMA mode sends the inputs [r0, r1) of the slot: the copy kernel for a one-part call, the copy
// engine for the parts of a multi-part one.
hipError_t stage_transfer(const StageCall& c, const SlotMem& m, size_t r0, size_t r1) {
    if (r1 <= r0) return hipSuccess;
    if (c.part == 0 && c.wave_div == 0) return stage_blit_launch(m.hd + r0, m.d + r0, r1 - r0, c.stream);
    return hipMemcpyAsync(m.d + r0, m.h + r0, r1 - r0, hipMemcpyHostToDevice, c.stream);
}

// The DMA path: pack, send, launch.
ac_status run_dma(const StageCall& c, const std::vector<Task>& tasks, const SlotMem& m, Packer& pack, PhaseClock& clk) {
    JobPlan& p = c.p;
    ac_ctx* ctx = c.ctx;
    acamd::WorkPool& pool = acamd::host_pool();
    bool no_n[AC_MAX_JOBS] = {};
    if (p.n > 1) {
        // job by job: job j's inputs travel while job j + 1 is packed.  One pool job for all
        // tasks (they are in job order); the caller packs job j's share, waits for its last
        // task, sends it, then helps with job j + 1 while the workers carry on.
        std::atomic<uint32_t> left[AC_MAX_JOBS];
        for (uint32_t j = 0; j < AC_MAX_JOBS; ++j) left[j].store(0, std::memory_order_relaxed);
        for (const Task& x : tasks) left[x.job].fetch_add(1, std::memory_order_relaxed);
        const std::function<void(uint32_t)> pack_counted = [&](uint32_t t) {
            pack(t);
            left[tasks[t].job].fetch_sub(1, std::memory_order_release);
        };
        pool.begin((uint32_t)tasks.size(), pack_counted);
        uint32_t t0 = 0;
        for (uint32_t j = 0; j < p.n; ++j) {
            uint32_t t1 = t0;
            while (t1 < (uint32_t)tasks.size() && tasks[t1].job == j) ++t1;
            pool.help(t1);
            while (left[j].load(std::memory_order_acquire) != 0u) __builtin_ia32_pause();
            no_n[j] = pack.job_no_n(j);
            hipError_t e = stage_transfer(c, m, p.off_kmers[j], no_n[j] ? p.off_nmask[j] : p.off_start[j]);
            if (e == hipSuccess && p.ulen[j] == AC_NO_ULEN)
                e = stage_transfer(c, m, p.off_start[j], j + 1 < p.n ? p.off_kmers[j + 1] : p.off_err);
            if (e != hipSuccess) {
                pool.finish();
                return hip_fail(ctx, e, "stage transfer");
            }
            t0 = t1;
        }
        pool.finish();
        clk.mark(PH_PACK);
    } else {
        const std::function<void(uint32_t)> pack_fn = [&pack](uint32_t t) { pack(t); };
        pool.run((uint32_t)tasks.size(), pack_fn);
        for (uint32_t j = 0; j < p.n; ++j) no_n[j] = pack.job_no_n(j);
        clk.mark(PH_PACK);
        AC_HIP(ctx, stage_transfer(c, m, 0, p.off_err));
    }
    clk.mark(PH_H2D_ENQ);
    ac_segment segs[AC_MAX_JOBS];
    make_segs(c.jobs, p, m, c.d_counts, segs);
    // the synchronous path reads the error word back with the counts; a
    // submit reports through the context's word (ac_check)
    const PartMats mats(c);
    CountLaunch rq = count_request(c, segs, mats, no_n);
    rq.err = c.d_counts ? nullptr : (uint32_t*)(m.hd + p.off_err);
    rq.wave_div = c.wave_div;
    if (ac_status st = launch(ctx, rq)) return st;
    clk.mark(PH_LAUNCH_ENQ);
    clk.mark(PH_D2H_ENQ);
    AC_HIP(ctx, hipEventRecord(m.sl->ev, c.stream));
    m.sl->pending = true;
    return AC_OK;
}

void run_on_pool(uint32_t n, const std::function<void(uint32_t)>& fn) { acamd::host_pool().run(n, fn); }

// Packs the jobs' window ranges p.lo/p.hi into a staging slot of ctx (the
// host worker pool writes the 2-bit codes, N bitmap and window descriptors
// straight into pinned memory), moves each job's region into device memory
// (p.early: the count kernel copies it itself once the host flags the job;
// otherwise the copy kernel on `stream`, or the copy engine for multi-part
// calls) and launches the fused count kernel, whose counts go to d_counts
// (job j at d_counts + sum of the earlier n_kmers) or, when NULL, to the
// slot's pinned counts area.  Records the slot's event after the launch.
// Staging slots: a synchronous call's part q uses slot q (a one-part early
// launch alternates between slots 0 and 1); submits alternate between two
// sets of slots of their own.
// `hits` / `pos` (optional): the jobs' whole device matrices; the launch also writes the hit levels (and the
// end positions) of its window ranges into their rows (DESIGN.md §4e "Hits from the jobs stage").
ac_status stage_and_launch(ac_ctx* ctx, uint32_t k, const ac_job* jobs, JobPlan& p, hipStream_t stream,
                           uint32_t* d_counts, int part = 0, uint32_t wave_div = 0, bool zero = true,
                           uint32_t* const* hits = nullptr, uint32_t* const* pos = nullptr) {
    PhaseClock clk;
    const uint32_t hooks = g_test_hooks.load(std::memory_order_relaxed);
    p.max_errors = ctx->max_errors;
    p.want_hits = hits != nullptr;
    p.want_pos = hits && pos;
    p.multi_device = !ctx->peers.empty();
    for (uint32_t j = 0; j < p.n; ++j) p.has_pos[j] = pos && pos[j];
    std::vector<Task> tasks = acamd::plan_stage(k, jobs, p, d_counts != nullptr, acamd::host_pool().size(), task_windows(),
                                                stage_early(), hooks, run_on_pool);
    clk.mark(PH_SPAN);
    if (p.refusal) return fail(ctx, AC_ERR_INVALID, p.refusal);
    if (p.early) {  // the copier workgroups of the launch
        ensure_warm(ctx);
        const uint32_t P = acamd::pack_factor(k);
        if (!ctx->resident[1][P]) AC_HIP(ctx, acamd::resident_waves(P, true, ctx->cu_count, &ctx->resident[1][P]));
        p.copiers = stage_copiers(p.tickets);
    }
    DevicePack dp;
    choose_device_pack(jobs, p, tasks, dp);
    SlotMem m;
    if (ac_status st = acquire_slot(ctx, jobs, p, &m)) return st;
    clk.mark(PH_LAYOUT);
    Packer pack(jobs, p, tasks, m.h);
    const StageCall c{ctx, k, jobs, p, stream, d_counts, part, wave_div, zero, hits, pos};
    return p.early ? run_early(c, tasks, dp, m, pack, clk, hooks) : run_dma(c, tasks, m, pack, clk);
}

// ---------------------------------------------------------------------------
// What the synchronous call and the submit share.

// A call on one device: the early launch takes every size in one part (large ones through copier
// workgroups); the copy-engine parts remain for AC_STAGE_EARLY=0 -- part q + 1 is packed and sent
// while part q counts.  (A region of 2^31 bytes or more falls back to one DMA part inside plan_stage.)
struct CallShape {
    bool early;
    int parts;
    std::vector<std::vector<uint32_t>> cuts;  // per job, its parts' window boundaries
};
CallShape call_shape(const ac_job* jobs, uint32_t n_jobs, bool allow_early) {
    uint64_t total_w = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) total_w += jobs[j].sample.n_windows;
    CallShape s;
    s.early = allow_early && stage_early() && live_work(jobs, n_jobs);
    s.parts = (!s.early && total_w >= 2048) ? acamd::stage_parts(total_w) : 1;
    // (test-only hook: two parts whatever the size)
    if (!s.early && live_work(jobs, n_jobs))
        s.parts = std::max(s.parts, acamd::stage_parts(0, g_test_hooks.load(std::memory_order_relaxed)));
    s.cuts = acamd::part_cuts(jobs, n_jobs, s.parts);
    return s;
}

// Unit q (a part, or a device's shard) of every job: windows [cuts[j][q], cuts[j][q + 1]).
void set_ranges(JobPlan& p, const std::vector<std::vector<uint32_t>>& cuts, uint32_t n_jobs, size_t q) {
    p.n = n_jobs;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        p.lo[j] = cuts[j][q];
        p.hi[j] = cuts[j][q + 1];
    }
}

// ac_stage_mode of a call, from its first unit's plan.
int stage_mode_of(const JobPlan& p) { return p.dp_any ? 3 : p.early ? 2 : 0; }

// One unit of a synchronous call: on an ac_create_multi context one per device (shard g of
// every job's windows on context g); on one device up to AC_STAGE_MAX_PARTS
// parts on their own streams, the first launched with half the resident
// waves so the second part's waves run beside it as soon as its DMA lands.
struct Unit {
    ac_ctx* c;
    int part;
    hipStream_t stream;
    uint32_t wave_div;
    JobPlan plan;
};

ac_status make_units(ac_ctx* ctx, const ac_job* jobs, uint32_t n_jobs, bool allow_early, std::vector<Unit>& units) {
    if (!ctx->peers.empty()) {
        const size_t G = ctx->peers.size() + 1;
        std::vector<std::vector<uint32_t>> cuts;
        for (uint32_t j = 0; j < n_jobs; ++j)
            cuts.push_back(acamd::shard_cuts(jobs[j].sample.length, jobs[j].sample.n_windows, G));
        for (size_t g = 0; g < G; ++g) {
            Unit u{g == 0 ? ctx : ctx->peers[g - 1], 0, nullptr, 0, JobPlan()};
            u.stream = u.c->stream;
            u.plan.slot = 0;
            u.plan.scratch = 0;
            set_ranges(u.plan, cuts, n_jobs, g);
            units.push_back(u);
        }
        return AC_OK;
    }
    const CallShape s = call_shape(jobs, n_jobs, allow_early);
    for (int q = 0; q < s.parts; ++q) {
        if (q > 0 && !ctx->part_stream[q])
            AC_HIP(ctx, hipStreamCreateWithFlags(&ctx->part_stream[q], hipStreamNonBlocking));
        Unit u{ctx, q, q == 0 ? ctx->stream : ctx->part_stream[q], (s.parts > 1 && q == 0) ? 2u : 0u, JobPlan()};
        u.plan.slot = q;
        u.plan.scratch = q;
        if (s.early) {
            // one part: the early-launch stage (alternating slots 0 / 1, so a call never waits for
            // the previous call's launch to retire before it packs)
            u.plan.early = true;
            u.plan.slot = (int)ctx->early_flip;
            ctx->early_flip ^= 1u;
        }
        set_ranges(u.plan, s.cuts, n_jobs, (size_t)q);
        units.push_back(u);
    }
    return AC_OK;
}

// Waits for unit u's launch and adds its counts into the jobs' (zeroed by the caller).  *err_word:
// the launch's device error bits.
ac_status collect_unit(Unit& u, const ac_job* jobs, uint32_t n_jobs, uint32_t* err_word) {
    ac_ctx::Slot& sl = u.c->slot[u.plan.slot];
    const char* h = (const char*)sl.h;
    if (u.plan.tag) {
        // every count and every group's error word is tagged with the launch's generation: poll
        // them instead of the stream (the launch's event is waited for when the slot is next used)
        if (ac_status st = wait_tagged(u.c, jobs, n_jobs, u.plan, h, u.stream)) return st;
        *err_word = 0;
        const uint64_t* ge = (const uint64_t*)(h + u.plan.off_gerr);
        for (uint32_t i = 0; i < u.plan.n_gerr; ++i) *err_word |= (uint32_t)ge[i];
    } else {
        AC_HIP(u.c, hipStreamSynchronize(u.stream));
        sl.pending = false;
        *err_word = *(const uint32_t*)(h + u.plan.off_err);
    }
    return AC_OK;
}

void add_counts(const Unit& u, const ac_job* jobs, uint32_t n_jobs) {
    const char* h = (const char*)u.c->slot[u.plan.slot].h;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        if (u.plan.tag) {
            const uint64_t* hc = (const uint64_t*)(h + u.plan.off_counts[j]);
            if (u.plan.hi[j] > u.plan.lo[j])  // (a job without windows here: its counts are 0)
                for (uint32_t i = 0; i < jobs[j].n_kmers; ++i) jobs[j].counts[i] += (uint32_t)hc[i];
            continue;
        }
        const uint32_t* hc = (const uint32_t*)(h + u.plan.off_counts[j]);
        for (uint32_t i = 0; i < jobs[j].n_kmers; ++i) jobs[j].counts[i] += hc[i];
    }
}

// The synchronous jobs stage (ac_error_count_jobs).  allow_early = false: the DMA path whatever
// AC_STAGE_EARLY says.  *stage_timeout: the early launch gave up waiting for the host's inputs.
// `mats` (optional): the call also returns hit levels (and end positions) -- every unit's launch writes its
// rows of the context's device matrices, which the last unit's stream copies to the caller's host matrices
// once every unit has been collected; the call returns when those copies have landed.
struct HostMats {
    uint32_t* const* hits_host;
    uint32_t* const* pos_host;  // NULL: hit levels only
    uint32_t* d_hits[AC_MAX_JOBS] = {};
    uint32_t* d_pos[AC_MAX_JOBS] = {};
    size_t hits_bytes[AC_MAX_JOBS] = {}, pos_bytes[AC_MAX_JOBS] = {};
};

ac_status count_jobs_sync(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs, bool allow_early,
                          bool* stage_timeout, const HostMats* mats = nullptr) {
    *stage_timeout = false;
    std::vector<Unit> units;
    if (ac_status st = make_units(ctx, jobs, n_jobs, allow_early, units)) return st;
    // Units are staged one after another on the host pool; a unit's DMA and
    // kernel run while the next one is packed.
    for (size_t g = 0; g < units.size(); ++g) {
        Unit& u = units[g];
        AC_HIP(u.c, hipSetDevice(u.c->device));
        if (ac_status st = stage_and_launch(u.c, k, jobs, u.plan, u.stream, nullptr, u.part, u.wave_div, true,
                                            mats ? mats->d_hits : nullptr, mats && mats->pos_host ? mats->d_pos : nullptr))
            return u.c != ctx ? fail(ctx, st, "shard " + std::to_string(g) + ": " + u.c->err) : st;
    }
    for (uint32_t j = 0; j < n_jobs; ++j)
        for (uint32_t i = 0; i < jobs[j].n_kmers; ++i) jobs[j].counts[i] = 0;
    ac_status first_err = AC_OK;
    PhaseClock clk;
    for (size_t g = 0; g < units.size(); ++g) {
        Unit& u = units[g];
        AC_HIP(u.c, hipSetDevice(u.c->device));
        uint32_t err_word = 0;
        if (ac_status st = collect_unit(u, jobs, n_jobs, &err_word)) return st;
        if (g + 1 == units.size()) clk.mark(PH_SYNC);
        if (u.plan.early && (err_word & AC_DEVERR_STAGE)) *stage_timeout = true;
        if (ac_status st = device_error(u.c, err_word)) {
            if (first_err == AC_OK)
                first_err = u.c != ctx ? fail(ctx, st, "shard " + std::to_string(g) + ": " + u.c->err) : st;
            continue;
        }
        add_counts(u, jobs, n_jobs);
    }
    if (first_err == AC_OK) units[0].c->last_mode = stage_mode_of(units[0].plan);
    if (first_err == AC_OK && mats) {
        // Every unit's counts are in, so every DMA-path unit's stream has been waited for; a tagged early
        // launch's counts may arrive before its kernel has retired, and the copies follow it on its stream.
        hipStream_t st = units.back().stream;
        for (uint32_t j = 0; j < n_jobs; ++j) {
            if (!jobs[j].n_kmers || !jobs[j].sample.n_windows) continue;
            AC_HIP(ctx, hipMemcpyAsync(mats->hits_host[j], mats->d_hits[j], mats->hits_bytes[j], hipMemcpyDeviceToHost, st));
            if (mats->pos_host)
                AC_HIP(ctx, hipMemcpyAsync(mats->pos_host[j], mats->d_pos[j], mats->pos_bytes[j], hipMemcpyDeviceToHost, st));
        }
        AC_HIP(ctx, hipStreamSynchronize(st));
    }
    if (g_trace.on) {
        clk.mark(PH_WIDEN);
        ++g_trace.calls;
        g_trace.skip_warmup();
        g_trace.end_call();
    }
    return first_err;
}

// The hit levels' question (hits_refusal / positions_refusal), asked of the whole call over every job's
// whole sample before anything is packed or enqueued, like check_jobs asks the budget's: a call may become
// several launches (parts), each of which asks again of its own plan, and a call whose whole samples hold
// equal windows has parts that do.  `hits` / `pos`: the caller's matrices, host or device, one per job (a
// job without work may pass NULL); with_pos: positions are asked for too.
ac_status check_jobs_hits(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs, uint32_t* const* hits,
                          bool with_pos, uint32_t* const* pos) {
    if (n_jobs && !hits) return fail(ctx, AC_ERR_INVALID, "window hits: hits is NULL");
    if (with_pos && n_jobs && !pos) return fail(ctx, AC_ERR_INVALID, "window positions: pos is NULL");
    bool live[AC_MAX_JOBS], has_pos[AC_MAX_JOBS];
    uint32_t ulen[AC_MAX_JOBS];
    for (uint32_t j = 0; j < n_jobs; ++j) {
        const ac_dna5_windows& s = jobs[j].sample;
        live[j] = jobs[j].n_kmers && s.n_windows;
        has_pos[j] = with_pos && pos[j];
        ulen[j] = s.n_windows ? s.length[0] : AC_NO_ULEN;
        for (uint32_t i = 1; i < s.n_windows && ulen[j] != AC_NO_ULEN; ++i)
            if (s.length[i] != ulen[j]) ulen[j] = AC_NO_ULEN;
    }
    if (const char* why = with_pos ? acamd::positions_refusal(ctx->max_errors, k, n_jobs, live, ulen, !ctx->peers.empty(), has_pos)
                                   : acamd::hits_refusal(ctx->max_errors, k, n_jobs, live, ulen, !ctx->peers.empty()))
        return fail(ctx, AC_ERR_INVALID, why);
    for (uint32_t j = 0; j < n_jobs; ++j)
        if (live[j] && !hits[j]) return fail(ctx, AC_ERR_INVALID, "window hits: hits[j] is NULL for a job with work");
    return AC_OK;
}

// ac_error_count_jobs, and -- hits_host: one host matrix per job -- ac_window_hits_jobs, and -- pos_host
// beside it -- ac_window_positions_jobs.
ac_status count_jobs(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs, uint32_t* const* hits_host,
                     bool with_pos, uint32_t* const* pos_host) {
    if (ac_status st = check_jobs(ctx, k, jobs, n_jobs)) return st;
    for (uint32_t j = 0; j < n_jobs; ++j)
        if (jobs[j].n_kmers && !jobs[j].counts) return fail(ctx, AC_ERR_INVALID, "job counts is NULL");
    if (n_jobs == 0) return AC_OK;
    HostMats mats{hits_host, with_pos ? pos_host : nullptr};
    const bool want_hits = hits_host != nullptr;
    if (want_hits) {
        if (ac_status st = check_jobs_hits(ctx, k, jobs, n_jobs, hits_host, with_pos, pos_host)) return st;
        // The context's device matrices, back to back in one block each, grown here: before any launch is
        // enqueued, so that no early launch -- which waits for this thread's packing -- waits on an allocation.
        size_t all = 0, all_pos = 0;
        for (uint32_t j = 0; j < n_jobs; ++j) {
            mats.hits_bytes[j] =
                sizeof(uint32_t) * (size_t)ac_window_hits_words(jobs[j].n_kmers, jobs[j].sample.n_windows, ctx->max_errors);
            mats.pos_bytes[j] = sizeof(uint32_t) * (size_t)ac_window_positions_words(jobs[j].n_kmers, jobs[j].sample.n_windows);
            all += align256(mats.hits_bytes[j]);
            all_pos += align256(mats.pos_bytes[j]);
        }
        AC_HIP(ctx, hipSetDevice(ctx->device));
        if (ac_status st = grow(ctx, &ctx->d_hits, &ctx->d_hits_cap, all)) return st;
        if (with_pos)
            if (ac_status st = grow(ctx, &ctx->d_pos, &ctx->d_pos_cap, all_pos)) return st;
        size_t at = 0, at_pos = 0;
        for (uint32_t j = 0; j < n_jobs; ++j) {
            const bool work = jobs[j].n_kmers && jobs[j].sample.n_windows;
            mats.d_hits[j] = work ? (uint32_t*)((char*)ctx->d_hits + at) : nullptr;
            at += align256(mats.hits_bytes[j]);
            if (with_pos) {
                mats.d_pos[j] = work ? (uint32_t*)((char*)ctx->d_pos + at_pos) : nullptr;
                at_pos += align256(mats.pos_bytes[j]);
            }
        }
    }
    bool stage_timeout = false;
    const ac_status st = count_jobs_sync(ctx, k, jobs, n_jobs, true, &stage_timeout, want_hits ? &mats : nullptr);
    // An early launch whose host inputs stopped arriving for 0.5 s (a stalled host: the kernel's waits
    // restart their clock on every bit of progress) skipped its work and said so: the call is run
    // again through the DMA path, which has no such wait, instead of failing.
    if (st != AC_OK && stage_timeout) {
        std::fprintf(stderr, "[approx_counter_amd] early launch timed out waiting for the host; retrying via DMA\n");
        // (with hits: the retry rewrites the matrices whole)
        return count_jobs_sync(ctx, k, jobs, n_jobs, false, &stage_timeout, want_hits ? &mats : nullptr);
    }
    return st;
}

// ac_error_count_jobs_submit, and -- d_hits: one device matrix per job -- ac_window_hits_jobs_submit, and --
// d_pos beside it -- ac_window_positions_jobs_submit.
ac_status submit_jobs(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs, uint32_t* d_counts, void* hip_stream,
                      uint32_t* const* d_hits, bool with_pos, uint32_t* const* d_pos);

}  // namespace

extern "C" {

ac_status ac_error_count_jobs(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs) {
    return count_jobs(ctx, k, jobs, n_jobs, nullptr, false, nullptr);
}

ac_status ac_window_hits_jobs(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs, uint32_t* const* hits_host) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    static uint32_t* const none[AC_MAX_JOBS] = {};
    if (n_jobs && !hits_host) return fail(ctx, AC_ERR_INVALID, "window hits: hits_host is NULL");
    return count_jobs(ctx, k, jobs, n_jobs, hits_host ? hits_host : none, false, nullptr);
}

ac_status ac_window_positions_jobs(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs,
                                   uint32_t* const* hits_host, uint32_t* const* pos_host) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    static uint32_t* const none[AC_MAX_JOBS] = {};
    if (n_jobs && !hits_host) return fail(ctx, AC_ERR_INVALID, "window hits: hits_host is NULL");
    if (n_jobs && !pos_host) return fail(ctx, AC_ERR_INVALID, "window positions: pos_host is NULL");
    return count_jobs(ctx, k, jobs, n_jobs, hits_host ? hits_host : none, true, pos_host ? pos_host : none);
}

ac_status ac_window_hits_jobs_submit(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs, uint32_t* d_counts,
                                     uint32_t* const* d_hits, void* hip_stream) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    static uint32_t* const none[AC_MAX_JOBS] = {};
    if (n_jobs && !d_hits) return fail(ctx, AC_ERR_INVALID, "window hits: d_hits is NULL");
    return submit_jobs(ctx, k, jobs, n_jobs, d_counts, hip_stream, d_hits ? d_hits : none, false, nullptr);
}

ac_status ac_window_positions_jobs_submit(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs,
                                          uint32_t* d_counts, uint32_t* const* d_hits, uint32_t* const* d_pos,
                                          void* hip_stream) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    static uint32_t* const none[AC_MAX_JOBS] = {};
    if (n_jobs && !d_hits) return fail(ctx, AC_ERR_INVALID, "window hits: d_hits is NULL");
    if (n_jobs && !d_pos) return fail(ctx, AC_ERR_INVALID, "window positions: d_pos is NULL");
    return submit_jobs(ctx, k, jobs, n_jobs, d_counts, hip_stream, d_hits ? d_hits : none, true, d_pos ? d_pos : none);
}

uint32_t ac_testing_stage_hooks(uint32_t flags) { return g_test_hooks.exchange(flags); }

int ac_testing_last_count_kernel(ac_ctx* ctx) { return ctx ? ctx->last_kernel : -1; }

ac_status ac_error_count_jobs_submit(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs,
                                     uint32_t* d_counts, void* hip_stream) {
    return submit_jobs(ctx, k, jobs, n_jobs, d_counts, hip_stream, nullptr, false, nullptr);
}

int ac_stage_mode(const ac_ctx* ctx) { return ctx ? ctx->last_mode : -1; }

}  // extern "C"

namespace {

ac_status submit_jobs(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs, uint32_t* d_counts, void* hip_stream,
                      uint32_t* const* d_hits, bool with_pos, uint32_t* const* d_pos) {
    if (ac_status st = check_jobs(ctx, k, jobs, n_jobs)) return st;
    // (hits: the matrices' own refusal names the context first)
    if (d_hits)
        if (ac_status st = check_jobs_hits(ctx, k, jobs, n_jobs, d_hits, with_pos, d_pos)) return st;
    if (!ctx->peers.empty())
        return fail(ctx, AC_ERR_INVALID, "ac_error_count_jobs_submit needs a single-device context");
    uint64_t n_counts = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) n_counts += jobs[j].n_kmers;
    if (n_counts && !d_counts) return fail(ctx, AC_ERR_INVALID, "d_counts is NULL");
    if (n_jobs == 0) return AC_OK;
    AC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t caller = (hipStream_t)hip_stream;
    // Large submits are cut into parts like the synchronous stage (a rank's shard of cfg4 is
    // 2^17-2^18 windows): part q + 1 is packed and sent while part q counts.  The parts add
    // into d_counts, zeroed first on the caller's stream; parts 1.. run on the context's
    // submit streams, ordered after the zeroing and joined back into the caller's stream.
    // Submits alternate between two sets of staging slots, so a submit packs while the
    // previous one's launch may still read its inputs.
    const CallShape s = call_shape(jobs, n_jobs, true);
    const int parts = s.parts;
    const int set = (int)ctx->next_slot;
    ctx->next_slot ^= 1u;
    if (parts > 1) {
        AC_HIP(ctx, hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * n_counts, caller));
        if (!ctx->sub_zero_ev) AC_HIP(ctx, hipEventCreateWithFlags(&ctx->sub_zero_ev, hipEventDisableTiming));
        AC_HIP(ctx, hipEventRecord(ctx->sub_zero_ev, caller));
    }
    for (int q = 0; q < parts; ++q) {
        hipStream_t st = caller;
        if (q > 0) {
            if (!ctx->sub_stream[q]) AC_HIP(ctx, hipStreamCreateWithFlags(&ctx->sub_stream[q], hipStreamNonBlocking));
            if (!ctx->sub_ev[q]) AC_HIP(ctx, hipEventCreateWithFlags(&ctx->sub_ev[q], hipEventDisableTiming));
            st = ctx->sub_stream[q];
            AC_HIP(ctx, hipStreamWaitEvent(st, ctx->sub_zero_ev, 0));
        }
        JobPlan p;
        set_ranges(p, s.cuts, n_jobs, (size_t)q);
        p.slot = AC_STAGE_MAX_PARTS * (1 + set) + q;
        p.scratch = AC_STAGE_MAX_PARTS + q;
        // one part: the early launch, counts and errors into device memory (ac_check reads them)
        p.early = s.early;
        if (ac_status rc = stage_and_launch(ctx, k, jobs, p, st, d_counts, q, (parts > 1 && q == 0) ? 2u : 0u,
                                            parts == 1, d_hits, with_pos ? d_pos : nullptr))
            return rc;
        if (q > 0) AC_HIP(ctx, hipEventRecord(ctx->sub_ev[q], st));
        if (q == 0) ctx->last_mode = stage_mode_of(p);
    }
    for (int q = 1; q < parts; ++q) AC_HIP(ctx, hipStreamWaitEvent(caller, ctx->sub_ev[q], 0));
    if (g_trace.on) {
        ++g_trace.calls;
        g_trace.skip_warmup();
        g_trace.end_call();
    }
    return AC_OK;
}

}  // namespace
