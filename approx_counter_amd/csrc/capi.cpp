// capi.cpp -- C ABI of the MI355X approximate-count stage (include/approx_counter_amd.h).
//
// Replaces errorCount (approx_counter.cpp:531-601): where the reference builds
// a bidirectional FM index over the sample (537-541) and runs SeqAn's
// find<0,2> per candidate under OpenMP (547-599), this layer uploads the
// packed sample once per call and launches one HIP kernel over the
// candidate x window grid.
//
// This file: context lifetime, the image and sample entry points, host-pool placement and the
// pinned allocator, with the helpers every C-ABI file shares (ctx.h).  The count launch plan is
// count_launch.cpp, the exact count capi_exact.cpp, the multi-process path capi_comm.cpp, and the
// jobs stage (ac_error_count_jobs / _submit) jobs_stage.cpp over stage_plan.cpp.
#include <sched.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bs_nfa.h"
#include "ctx.h"
#include "host_pack.h"
#include "stage_plan.h"

static_assert(AC_MAX_JOBS <= AC_MAX_SEGS, "every job of ac_error_count_jobs is one segment of one launch");

namespace {
thread_local std::string g_err;
}

namespace ac_detail {

ac_status fail(ac_ctx* ctx, ac_status st, const std::string& msg) {
    if (ctx) ctx->err = msg;
    g_err = msg;
    return st;
}

ac_status hip_fail(ac_ctx* ctx, hipError_t e, const char* what) {
    return fail(ctx, e == hipErrorOutOfMemory ? AC_ERR_NOMEM : AC_ERR_DEVICE,
                std::string(what) + ": " + hipGetErrorString(e));
}

ac_status check_k(ac_ctx* ctx, uint32_t k) {
    // approx_counter.cpp:781-783: k must lie in [2, 32].
    if (k < 2 || k > 32) return fail(ctx, AC_ERR_INVALID, "kmer size must be between 2 and 32 (included)");
    return AC_OK;
}

ac_status grow(ac_ctx* ctx, void** buf, size_t* cap, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (*cap >= bytes) return AC_OK;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    AC_HIP(ctx, hipMalloc(buf, bytes));
    *cap = bytes;
    return AC_OK;
}

// Host -> device copy of n host arrays through the context's pinned staging
// block.  Array i lands at offset off(i) = sum of the earlier sizes rounded up
// to 256 B, in the staging block and in the device block `dst` alike.  The
// block is filled and sent in 1 MB pieces, each piece's DMA queued as soon as
// it is filled, so the CPU fills the next piece while the previous one crosses
// PCIe (pageable copies, one per array, each paid the driver's own staging
// overhead; one DMA per array instead of per piece cost 70 us more at cfg2).
// Asynchronous on ctx->stream; the block is reused by the next call, so callers
// synchronise the stream before returning.  `extra` bytes after the arrays are
// reserved (the counts' way back).
size_t staged_bytes(int n, const size_t* sz) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (sz[i] + 255) / 256 * 256;
    return total;
}

ac_status h2d_staged(ac_ctx* ctx, int n, const void* const* src, const size_t* sz, void* dst, size_t extra) {
    const size_t in_bytes = staged_bytes(n, sz), total = in_bytes + extra;
    if (ctx->h_stage_cap < total) {
        if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
        ctx->h_stage = nullptr;
        ctx->h_stage_cap = 0;
        AC_HIP(ctx, hipHostMalloc(&ctx->h_stage, total, hipHostMallocDefault));
        ctx->h_stage_cap = total;
    }
    constexpr size_t CHUNK = size_t(1) << 20;
    char* h = (char*)ctx->h_stage;
    for (size_t c0 = 0; c0 < in_bytes; c0 += CHUNK) {
        const size_t c1 = std::min(in_bytes, c0 + CHUNK);
        size_t off = 0;
        for (int i = 0; i < n; ++i) {
            const size_t lo = std::max(c0, off), hi = std::min(c1, off + sz[i]);
            if (lo < hi) std::memcpy(h + lo, (const char*)src[i] + (lo - off), hi - lo);
            off += (sz[i] + 255) / 256 * 256;
        }
        AC_HIP(ctx, hipMemcpyAsync((char*)dst + c0, h + c0, c1 - c0, hipMemcpyHostToDevice, ctx->stream));
    }
    return AC_OK;
}


ac_status check_sample(ac_ctx* ctx, const ac_windows* s) {
    if (!s) return fail(ctx, AC_ERR_INVALID, "sample is NULL");
    if (s->n_bases % 32 || s->n_bases >= AC_MAX_IMAGE_BASES)
        return fail(ctx, AC_ERR_INVALID, "sample n_bases must be a multiple of 32 below 2^34 - 4096");
    if (s->n_windows && (!s->codes || !s->nmask || !s->start || !s->length))
        return fail(ctx, AC_ERR_INVALID, "sample has a NULL array");
    return AC_OK;
}

// Every window inside the image and 32-aligned, written so that no sum can
// wrap: a start near 2^64 must not pass as "start + length <= n_bases".
static inline bool window_ok(uint64_t start, uint32_t length, uint64_t n_bases) {
    return start % 32 == 0 && length <= n_bases && start <= n_bases - length;
}

// Status for a device error word read back after a launch (wm_count.h).
ac_status device_error(ac_ctx* ctx, uint32_t word) {
    if (word & AC_DEVERR_STAGE)
        return fail(ctx, AC_ERR_INTERNAL, "early launch: the kernel timed out waiting for the host's packed inputs");
    if (word & AC_DEVERR_SETUP)
        return fail(ctx, AC_ERR_INTERNAL, "count kernel set-up fault (~Eq table not at LDS 0): its work was skipped");
    if (word & AC_DEVERR_WINDOW)
        return fail(ctx, AC_ERR_INVALID,
                    "malformed window skipped on the device (misaligned start or past n_bases): counts are short");
    return AC_OK;
}

ac_status check_layout(ac_ctx* ctx, const ac_windows& s) {
    for (uint32_t i = 0; i < s.n_windows; ++i)
        if (!window_ok(s.start[i], s.length[i], s.n_bases))
            return fail(ctx, AC_ERR_INVALID, "window " + std::to_string(i) + " is misaligned or outside the image");
    return AC_OK;
}

int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e && *e ? std::atoi(e) : dflt;
}

}  // namespace ac_detail

using namespace ac_detail;

namespace {

// CPUs local to a device's PCIe root (sysfs local_cpulist), empty if unknown.
std::vector<int> device_local_cpus(int device) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof bus, device) != hipSuccess) return {};
    for (char* c = bus; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/local_cpulist";
    return acamd::read_cpulist(path.c_str());
}

std::vector<int> allowed_cpus() {
    std::vector<int> out;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) != 0) return out;
    for (int c = 0; c < CPU_SETSIZE; ++c)
        if (CPU_ISSET(c, &set)) out.push_back(c);
    return out;
}

// The host pool's CPUs, once per process, before its first use: it packs into
// memory this GPU reads, so it runs on the CPUs local to the GPU's PCIe root.
// One process per GPU (torchrun: LOCAL_RANK / LOCAL_WORLD_SIZE, local rank r
// on device r mod the visible devices): the local ranks whose GPUs share a
// CPU list split it into disjoint runs of physical cores, and each rank's pool
// takes at most its share of the cgroup CPU quota minus headroom (below; 16
// participants at most), so 8 ranks on one node never pin their workers onto the
// same CPUs nor spin more threads than the quota runs.  (The reference sizes its one OpenMP team
// with omp_set_num_threads(nb_thread), approx_counter.cpp:547.)
void plan_host_pool(int device, int n_dev) {
    if (acamd::host_plan().participants) return;  // set already (ac_set_host_cpus or an earlier context)
    int lws = env_int("LOCAL_WORLD_SIZE", 1), lr = env_int("LOCAL_RANK", 0);
    if (lws < 1 || lr < 0 || lr >= lws) lws = 1, lr = 0;
    std::vector<std::vector<int>> lists((size_t)lws);
    for (int r = 0; r < lws; ++r) lists[(size_t)r] = r == lr ? device_local_cpus(device) : device_local_cpus(r % n_dev);
    const std::vector<int> allowed = allowed_cpus();
    bool shared = false;
    acamd::HostPlan plan;
    plan.cpus = acamd::plan_host_cpus(lists, lr, allowed, acamd::sysfs_core_of, &shared);
    size_t n = plan.cpus.empty() ? allowed.size() : plan.cpus.size();
    // Headroom under the quota: a pool of all of it (16 participants spinning on a 16-CPU quota, with
    // Python's and the HIP runtime's threads beside them) was throttled in 91 of 100 CFS periods of a
    // 10-s cfg2 run (191 ms throttled, 59 of its 60 steps over 2x p50 inside throttled periods; 14
    // participants: none, p50 equal; profiles/r06_m3/stall_*.log): 2 CPUs of headroom above a share
    // of 4, 1 below.
    const double quota = acamd::cgroup_cpu_quota();
    if (quota > 0.0) {
        const double share = quota / lws;
        n = std::min<size_t>(n, (size_t)std::max(1.0, std::floor(share) - (share > 4.0 ? 2.0 : 1.0)));
    }
    plan.participants = shared ? 1u : (unsigned)std::max<size_t>(1, std::min<size_t>(16, n));
    (void)acamd::set_host_plan(plan);
}

}  // namespace

extern "C" {

int ac_abi_version(void) { return AC_ABI_VERSION; }

int ac_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* ac_last_error(const ac_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

ac_status ac_create(ac_ctx** out, int device) {
    if (!out) return fail(nullptr, AC_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, AC_ERR_DEVICE, "no HIP device available (the approximate count runs on the GPU only)");
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= n) return fail(nullptr, AC_ERR_INVALID, "device ordinal out of range");
    ac_ctx* ctx = new (std::nothrow) ac_ctx();
    if (!ctx) return fail(nullptr, AC_ERR_NOMEM, "cannot allocate context");
    ctx->device = device;
    hipDeviceProp_t prop;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) {
        ac_status st = hip_fail(nullptr, e, "device setup");
        delete ctx;
        return st;
    }
    ctx->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    plan_host_pool(device, n);
    if ((e = hipMalloc(&ctx->d_err, sizeof(uint32_t))) != hipSuccess ||
        (e = hipMemset(ctx->d_err, 0, sizeof(uint32_t))) != hipSuccess ||
        (e = hipHostMalloc(&ctx->h_err, sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess) {
        ac_status st = hip_fail(nullptr, e, "device setup");
        ac_destroy(ctx);
        return st;
    }
    // (a query that fails leaves its count 0: launch() queries again and reports the error there)
    // The warm-up also allocates the first scratch set at the sizes a few-candidate-group launch needs
    // (it grows on demand later), so that launch does not wait for allocations either.
    ctx->warm = std::thread([ctx] {
        if (hipSetDevice(ctx->device) != hipSuccess) return;
        for (uint32_t P = 1; P <= AC_MAX_PACK; ++P)
            for (int st = 0; st < 2; ++st)
                (void)acamd::resident_waves(P, st != 0, ctx->cu_count, &ctx->warm_resident[st][P]);
        // (the bit-sliced kernels' code with them: the k = 16 queries load the code object; another
        // k is queried at its first launch, so start-up does not grow with AC_BS_K_LIST)
        for (int st = 0; st < 2; ++st) {
            const acamd::BsFamily counting = acamd::bs_family(st != 0, false, false, 2u);
            (void)acamd::resident_waves_bs(counting, 16u, ctx->cu_count,
                                           &ctx->warm_resident_bs[acamd::bs_family_index(counting)][16]);
        }
        ac_ctx::Scratch& sc = ctx->sc[0];
        auto zeroed = [](void** p, size_t bytes) {
            if (hipMalloc(p, bytes) != hipSuccess) return false;
            if (hipMemset(*p, 0, bytes) == hipSuccess) return true;
            (void)hipFree(*p);
            *p = nullptr;
            return false;
        };
        constexpr uint32_t QCAP = 2048, ACC = 64 * 256, CHUNKS = 1024;
        if (zeroed((void**)&sc.queue, sizeof(uint32_t) * AC_QUEUE_LINE * 2 * QCAP)) sc.qcap = QCAP;
        if (zeroed((void**)&sc.acc, sizeof(uint64_t) * ACC)) sc.acc_cap = ACC;
        if (zeroed((void**)&sc.stage_gen, sizeof(uint32_t) * AC_QUEUE_LINE * CHUNKS)) sc.stage_gen_cap = CHUNKS;
    });
    *out = ctx;
    return AC_OK;
}

void ac_destroy(ac_ctx* ctx) {
    if (!ctx) return;
    if (ctx->warm.joinable()) ctx->warm.join();
    for (ac_ctx* p : ctx->peers) ac_destroy(p);
    (void)hipSetDevice(ctx->device);
    comm_destroy(ctx);
    if (ctx->d_kmers) (void)hipFree(ctx->d_kmers);
    if (ctx->d_counts) (void)hipFree(ctx->d_counts);
    if (ctx->d_stage) (void)hipFree(ctx->d_stage);
    if (ctx->d_hits) (void)hipFree(ctx->d_hits);
    if (ctx->d_pos) (void)hipFree(ctx->d_pos);
    if (ctx->d_start) (void)hipFree(ctx->d_start);
    if (ctx->d_flank) (void)hipFree(ctx->d_flank);
    if (ctx->d_edit) (void)hipFree(ctx->d_edit);
    if (ctx->d_cooc) (void)hipFree(ctx->d_cooc);
    if (ctx->d_cooc_io) (void)hipFree(ctx->d_cooc_io);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    for (auto& sc : ctx->sc) {
        if (sc.queue) (void)hipFree(sc.queue);
        if (sc.acc) (void)hipFree(sc.acc);
        if (sc.stage_gen) (void)hipFree(sc.stage_gen);
    }
    for (hipStream_t ps : ctx->part_stream)
        if (ps) (void)hipStreamDestroy(ps);
    for (hipStream_t ps : ctx->sub_stream)
        if (ps) (void)hipStreamDestroy(ps);
    for (hipEvent_t ev : ctx->sub_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->sub_zero_ev) (void)hipEventDestroy(ctx->sub_zero_ev);
    for (void* p : ctx->s_buf)
        if (p) (void)hipFree(p);
    for (void* p : ctx->e_buf)
        if (p) (void)hipFree(p);
    if (ctx->e_pin) (void)hipHostFree(ctx->e_pin);
    if (ctx->d_err) (void)hipFree(ctx->d_err);
    if (ctx->h_err) (void)hipHostFree(ctx->h_err);
    for (auto& sl : ctx->slot) {
        if (sl.ev) (void)hipEventSynchronize(sl.ev);
        if (sl.hdr) (void)hipHostFree(sl.hdr);
        if (sl.h) (void)hipHostFree(sl.h);
        if (sl.d) (void)hipFree(sl.d);
        if (sl.ev) (void)hipEventDestroy(sl.ev);
    }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// The device entry points' window_len (NULL: the segments come with window descriptors), checked and copied
// into ul: *ulen = ul, or NULL.
static ac_status take_window_len(ac_ctx* ctx, const uint32_t* window_len, uint32_t n_segments, uint32_t (&ul)[AC_MAX_SEGS],
                                 const uint32_t** ulen) {
    *ulen = window_len ? ul : nullptr;
    if (window_len)
        for (uint32_t i = 0; i < n_segments; ++i) {
            if (window_len[i] == AC_NO_ULEN) return fail(ctx, AC_ERR_INVALID, "window_len out of range");
            ul[i] = window_len[i];
        }
    return AC_OK;
}

ac_status ac_error_count_device(ac_ctx* ctx, uint32_t k, const ac_segment* segments, uint32_t n_segments,
                                const uint32_t* window_len, uint32_t flags, void* hip_stream) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (flags & ~AC_DEVICE_ACCUMULATE) return fail(ctx, AC_ERR_INVALID, "unknown flags");
    if (n_segments > AC_MAX_SEGS) return fail(ctx, AC_ERR_INVALID, "too many segments in one launch (max 4)");
    uint32_t ul[AC_MAX_SEGS];
    CountLaunch rq(k, segments, n_segments, (hipStream_t)hip_stream);
    if (ac_status st = take_window_len(ctx, window_len, n_segments, ul, &rq.ulen)) return st;
    AC_HIP(ctx, hipSetDevice(ctx->device));
    rq.zero = !(flags & AC_DEVICE_ACCUMULATE);
    return launch(ctx, rq);
}

}  // extern "C"

namespace {

// errorCount (approx_counter.cpp:531-601) for up to AC_MAX_JOBS host images on
// one device, ONE fused launch: every job's k-mers and image go up through the
// pinned staging block (h2d_staged), the counts and the device error word come
// back in one copy.  jobs[j].sample holds host pointers.
ac_status count_images_one(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (ac_status st = check_k(ctx, k)) return st;
    if (n > AC_MAX_JOBS) return fail(ctx, AC_ERR_INVALID, "too many jobs in one call (max 4)");
    uint64_t total_k = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const ac_sample_job& b = jobs[j];
        if (b.n_kmers && (!b.kmers || !b.counts)) return fail(ctx, AC_ERR_INVALID, "NULL argument");
        if (ac_status st = check_sample(ctx, &b.sample)) return st;
        if (ac_status st = check_layout(ctx, b.sample)) return st;
        total_k += b.n_kmers;
    }
    if (total_k == 0) return AC_OK;
    AC_HIP(ctx, hipSetDevice(ctx->device));
    // Device block: per job kmers | codes | nmask | start | length, then err | counts of every
    // job, each 256-B aligned (the staging offsets; the error word goes up as a zero).
    static const uint32_t zero_word = 0;
    std::vector<const void*> src;
    std::vector<size_t> sz;
    for (uint32_t j = 0; j < n; ++j) {
        const ac_windows& w = jobs[j].sample;
        src.insert(src.end(), {jobs[j].kmers, w.codes, w.nmask, w.start, w.length});
        sz.insert(sz.end(), {sizeof(uint64_t) * jobs[j].n_kmers, sizeof(uint32_t) * (w.n_bases / 16),
                             sizeof(uint32_t) * (w.n_bases / 32), sizeof(uint64_t) * w.n_windows,
                             sizeof(uint32_t) * w.n_windows});
    }
    src.push_back(&zero_word);
    sz.push_back(sizeof(uint32_t));
    const size_t in_bytes = staged_bytes((int)sz.size(), sz.data());
    size_t back = 0;
    for (uint32_t j = 0; j < n; ++j) back += align256(sizeof(uint32_t) * jobs[j].n_kmers);
    if (ac_status rc = grow(ctx, &ctx->d_stage, &ctx->d_stage_cap, in_bytes + back)) return rc;
    char* d = (char*)ctx->d_stage;
    if (ac_status rc = h2d_staged(ctx, (int)sz.size(), src.data(), sz.data(), d, back)) return rc;
    char* h = (char*)ctx->h_stage;
    const size_t off_err = in_bytes - align256(sizeof(uint32_t));
    ac_segment seg[AC_MAX_JOBS];
    size_t off = 0, coff = in_bytes;
    size_t c_off[AC_MAX_JOBS];
    for (uint32_t j = 0; j < n; ++j) {
        const ac_windows& w = jobs[j].sample;
        size_t o[5];
        for (int i = 0; i < 5; ++i) {
            o[i] = off;
            off += align256(sz[5 * j + i]);
        }
        seg[j].kmers = (const uint64_t*)(d + o[0]);
        seg[j].n_kmers = jobs[j].n_kmers;
        seg[j].sample = ac_windows{(const uint32_t*)(d + o[1]), (const uint32_t*)(d + o[2]), (const uint64_t*)(d + o[3]),
                                   (const uint32_t*)(d + o[4]), w.n_windows, w.n_bases};
        seg[j].counts = (uint32_t*)(d + coff);
        c_off[j] = coff;
        coff += align256(sizeof(uint32_t) * jobs[j].n_kmers);
    }
    hipStream_t st = ctx->stream;
    CountLaunch rq(k, seg, n, st);
    rq.err = (uint32_t*)(d + off_err);
    if (ac_status rc = launch(ctx, rq)) return rc;
    AC_HIP(ctx, hipMemcpyAsync(h + off_err, d + off_err, coff - off_err, hipMemcpyDeviceToHost, st));
    AC_HIP(ctx, hipStreamSynchronize(st));
    if (ac_status rc = device_error(ctx, *(const uint32_t*)(h + off_err))) return rc;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t* hc = (const uint32_t*)(h + c_off[j]);
        for (uint32_t i = 0; i < jobs[j].n_kmers; ++i) jobs[j].counts[i] = hc[i];
    }
    return AC_OK;
}

// The same over an ac_create_multi context: every job's windows cut into one
// contiguous shard per device (balanced by bases), each device counting its
// shards of all jobs in one fused launch, the shard counts summed on the host.
ac_status count_images(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n) {
    // (packed images come with window descriptors: never a bit-sliced launch, so another edit budget
    // than 2 is refused here, before any copy or shard's launch)
    if (ctx && ctx->max_errors != 2u)
        if (const char* why = acamd::budget_refusal(ctx->max_errors, k, 0, nullptr, nullptr))
            return fail(ctx, AC_ERR_INVALID, why);
    if (!ctx || ctx->peers.empty()) return count_images_one(ctx, k, jobs, n);
    if (ac_status st = check_k(ctx, k)) return st;
    if (n > AC_MAX_JOBS) return fail(ctx, AC_ERR_INVALID, "too many jobs in one call (max 4)");
    for (uint32_t j = 0; j < n; ++j) {
        if (jobs[j].n_kmers && (!jobs[j].kmers || !jobs[j].counts)) return fail(ctx, AC_ERR_INVALID, "NULL argument");
        if (ac_status st = check_sample(ctx, &jobs[j].sample)) return st;
        if (ac_status st = check_layout(ctx, jobs[j].sample)) return st;
    }
    const size_t G = ctx->peers.size() + 1;
    // shard g of job j: windows [cut[j][g], cut[j][g + 1]), a slice of the image from its
    // lowest start to its highest end (windows may come in any order and overlap;
    // window_ok guarantees start + length <= n_bases, so nothing here wraps)
    std::vector<std::vector<uint32_t>> cut(n);
    for (uint32_t j = 0; j < n; ++j) {
        const ac_windows& s = jobs[j].sample;
        uint64_t total = 0;
        for (uint32_t i = 0; i < s.n_windows; ++i) total += s.length[i];
        cut[j].assign(G + 1, s.n_windows);
        cut[j][0] = 0;
        uint64_t acc = 0;
        size_t g = 1;
        for (uint32_t i = 0; i < s.n_windows && g < G; ++i) {
            acc += s.length[i];
            while (g < G && acc * G >= total * g) cut[j][g++] = i + 1;
        }
    }
    std::vector<std::vector<std::vector<uint64_t>>> part(G, std::vector<std::vector<uint64_t>>(n));
    std::vector<ac_status> rc(G, AC_OK);
    auto run = [&](size_t g) {
        ac_ctx* c = g == 0 ? ctx : ctx->peers[g - 1];
        ac_sample_job sj[AC_MAX_JOBS];
        std::vector<std::vector<uint64_t>> st(n);
        uint32_t m = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const ac_windows& s = jobs[j].sample;
            const uint32_t lo = cut[j][g], hi = cut[j][g + 1];
            part[g][j].assign(jobs[j].n_kmers, 0);
            if (hi == lo || !jobs[j].n_kmers) continue;
            uint64_t b0 = s.start[lo], b1 = 0;
            for (uint32_t i = lo; i < hi; ++i) {
                b0 = std::min<uint64_t>(b0, s.start[i]);
                b1 = std::max<uint64_t>(b1, s.start[i] + s.length[i]);
            }
            b1 = std::max<uint64_t>(b0 + 32, (b1 + 31) / 32 * 32);  // empty windows still count (k = 2: d = 2)
            if (b1 > s.n_bases) b1 = s.n_bases;  // b0 + 32 <= n_bases: b0 is a 32-aligned start < n_bases or 0
            st[j].resize(hi - lo);
            for (uint32_t i = lo; i < hi; ++i) st[j][i - lo] = s.start[i] - b0;
            sj[m++] = ac_sample_job{jobs[j].kmers, jobs[j].n_kmers,
                                    ac_windows{s.codes + b0 / 16, s.nmask + b0 / 32, st[j].data(), s.length + lo, hi - lo,
                                               b1 - b0},
                                    part[g][j].data()};
        }
        if (m) rc[g] = count_images_one(c, k, sj, m);
    };
    std::vector<std::thread> th;
    for (size_t g = 1; g < G; ++g) th.emplace_back(run, g);
    run(0);
    for (auto& t : th) t.join();
    for (size_t g = 0; g < G; ++g)
        if (rc[g] != AC_OK) {
            ac_ctx* c = g == 0 ? ctx : ctx->peers[g - 1];
            return fail(ctx, rc[g], "shard " + std::to_string(g) + ": " + c->err);
        }
    for (uint32_t j = 0; j < n; ++j)
        for (uint32_t i = 0; i < jobs[j].n_kmers; ++i) {
            uint64_t v = 0;
            for (size_t g = 0; g < G; ++g) v += part[g][j][i];
            jobs[j].counts[i] = v;
        }
    return AC_OK;
}

}  // namespace

extern "C" {

ac_status ac_error_count(ac_ctx* ctx, uint32_t k, const uint64_t* kmers, uint32_t n_kmers,
                         const ac_windows* sample, uint64_t* counts) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (ac_status st = check_k(ctx, k)) return st;
    if (n_kmers == 0) return AC_OK;
    if (!kmers || !counts || !sample) return fail(ctx, AC_ERR_INVALID, "NULL argument");
    const ac_sample_job job{kmers, n_kmers, *sample, counts};
    return count_images(ctx, k, &job, 1);
}

ac_status ac_error_count_images(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs) {
    if (n_jobs && !jobs) return fail(ctx, AC_ERR_INVALID, "jobs is NULL");
    return count_images(ctx, k, jobs, n_jobs);
}

ac_status ac_create_multi(ac_ctx** out, int n_gpus) {
    if (!out) return fail(nullptr, AC_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n_gpus < 1) return fail(nullptr, AC_ERR_INVALID, "n_gpus must be >= 1");
    const int n_dev = ac_device_count();
    if (n_dev < 1) return fail(nullptr, AC_ERR_DEVICE, "no HIP device available (the approximate count runs on the GPU only)");
    ac_ctx* root = nullptr;
    if (ac_status st = ac_create(&root, 0)) return st;
    for (int g = 1; g < n_gpus; ++g) {
        ac_ctx* c = nullptr;
        if (ac_status st = ac_create(&c, g % n_dev)) {
            ac_destroy(root);
            return st;
        }
        root->peers.push_back(c);
    }
    *out = root;
    return AC_OK;
}

ac_status ac_count(ac_ctx* ctx, uint32_t k, const uint64_t* kmers, uint32_t n_kmers, const uint32_t* win_bits,
                   const uint32_t* win_nmask, const uint64_t* win_word_offset, const uint16_t* win_len,
                   uint32_t n_windows, uint64_t* counts_out) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (n_windows && (!win_bits || !win_nmask || !win_word_offset || !win_len))
        return fail(ctx, AC_ERR_INVALID, "NULL window array");
    std::vector<uint64_t> start(n_windows);
    std::vector<uint32_t> len(n_windows);
    uint64_t n_bases = 32;
    for (uint32_t i = 0; i < n_windows; ++i) {
        if (win_word_offset[i] % 2)
            return fail(ctx, AC_ERR_INVALID, "window " + std::to_string(i) + " starts at an odd 2-bit word");
        start[i] = win_word_offset[i] * 16;
        len[i] = win_len[i];
        n_bases = std::max<uint64_t>(n_bases, (start[i] + len[i] + 31) / 32 * 32);
    }
    const ac_windows w{win_bits, win_nmask, start.data(), len.data(), n_windows, n_bases};
    return ac_error_count(ctx, k, kmers, n_kmers, &w, counts_out);
}


// ac_error_count_samples, and -- hits_host: one host matrix per job -- ac_window_hits_samples, and --
// pos_host beside it -- ac_window_positions_samples, and -- start_host beside both: the span pass over every
// job's device matrices after the launch -- ac_window_spans_samples, and -- flank_host beside the three: the
// flank pass of `depth` bases over the top level plane and the two matrices after that --
// ac_window_flanks_samples (capi_flank.cpp), and -- edit_host beside the first three, with or without
// flank_host: the edit pass over the same plane and matrices -- ac_window_edits_samples (capi_edit.cpp).
}  // extern "C"

namespace ac_detail {
ac_status count_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs, uint32_t* const* hits_host,
                        uint32_t* const* pos_host, uint32_t* const* start_host, uint32_t* const* flank_host,
                        uint32_t depth, uint32_t* const* edit_host) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (ac_status st = check_k(ctx, k)) return st;
    if (n_jobs > AC_MAX_JOBS) return fail(ctx, AC_ERR_INVALID, "too many jobs in one call (max 4)");
    if (n_jobs && !jobs) return fail(ctx, AC_ERR_INVALID, "jobs is NULL");
    uint64_t total = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        if (jobs[j].n_kmers && (!jobs[j].kmers || !jobs[j].counts)) return fail(ctx, AC_ERR_INVALID, "NULL argument");
        if (ac_status st = check_sample(ctx, &jobs[j].sample)) return st;
        total += jobs[j].n_kmers;
    }
    if (total == 0) return AC_OK;
    // images this context uploaded: their equal-window / N-free findings (others: the general form)
    uint32_t ulen[AC_MAX_JOBS];
    bool no_n[AC_MAX_JOBS];
    for (uint32_t j = 0; j < n_jobs; ++j) {
        ulen[j] = AC_NO_ULEN;
        no_n[j] = false;
        for (int sl = 0; sl < AC_MAX_JOBS; ++sl)
            if (ctx->s_codes[sl] && ctx->s_codes[sl] == jobs[j].sample.codes &&
                jobs[j].sample.nmask == (const uint32_t*)((const char*)ctx->s_codes[sl] +
                                                          (sizeof(uint32_t) * (ctx->s_bases[sl] / 16) + 255) / 256 * 256) &&
                jobs[j].sample.n_windows == ctx->s_windows[sl] && jobs[j].sample.n_bases == ctx->s_bases[sl] &&
                jobs[j].sample.start == ctx->s_start[sl] &&
                (const char*)jobs[j].sample.length >= (const char*)ctx->s_buf[sl] &&
                (const char*)jobs[j].sample.length < (const char*)ctx->s_buf[sl] + ctx->s_cap[sl]) {
                ulen[j] = ctx->s_ulen[sl];
                no_n[j] = ctx->s_no_n[sl];
            }
        // (the launch's own check: equal windows must fit the image)
        if (ulen[j] != AC_NO_ULEN &&
            (uint64_t)jobs[j].sample.n_windows * (((uint64_t)ulen[j] + 31u) & ~31ull) > jobs[j].sample.n_bases)
            ulen[j] = AC_NO_ULEN;
    }
    // hits: refused here, before the k-mers' copy is enqueued (the launch asks again); then the jobs'
    // device matrices, back to back in one block
    uint32_t* d_hits[AC_MAX_JOBS] = {};
    size_t hits_bytes[AC_MAX_JOBS] = {};
    uint32_t* d_pos[AC_MAX_JOBS] = {};
    size_t pos_bytes[AC_MAX_JOBS] = {};
    uint32_t* d_start[AC_MAX_JOBS] = {};
    uint32_t* d_flank[AC_MAX_JOBS] = {};
    size_t flank_bytes[AC_MAX_JOBS] = {};
    uint32_t* d_edit[AC_MAX_JOBS] = {};
    size_t edit_bytes[AC_MAX_JOBS] = {};
    if (hits_host) {
        bool live[AC_MAX_JOBS];
        for (uint32_t j = 0; j < n_jobs; ++j) live[j] = jobs[j].n_kmers && jobs[j].sample.n_windows;
        if (const char* why = acamd::hits_refusal(ctx->max_errors, k, n_jobs, live, ulen, !ctx->peers.empty()))
            return fail(ctx, AC_ERR_INVALID, why);
        size_t all = 0;
        for (uint32_t j = 0; j < n_jobs; ++j) {
            hits_bytes[j] = sizeof(uint32_t) *
                            (size_t)ac_window_hits_words(jobs[j].n_kmers, jobs[j].sample.n_windows, ctx->max_errors);
            if (live[j] && !hits_host[j]) return fail(ctx, AC_ERR_INVALID, "window hits: hits_host[j] is NULL for a job with work");
            all += align256(hits_bytes[j]);
        }
        size_t all_pos = 0;
        if (pos_host)
            for (uint32_t j = 0; j < n_jobs; ++j) {
                pos_bytes[j] = sizeof(uint32_t) * (size_t)ac_window_positions_words(jobs[j].n_kmers, jobs[j].sample.n_windows);
                if (live[j] && !pos_host[j])
                    return fail(ctx, AC_ERR_INVALID, "window positions: pos_host[j] is NULL for a job with work");
                if (start_host && live[j] && !start_host[j])
                    return fail(ctx, AC_ERR_INVALID, "match spans: start_host[j] is NULL for a job with work");
                if (start_host && flank_host && live[j] && !flank_host[j])
                    return fail(ctx, AC_ERR_INVALID, "flank profile: flank_host[j] is NULL for a job with work");
                if (start_host && edit_host && live[j] && !edit_host[j])
                    return fail(ctx, AC_ERR_INVALID, "edit profile: edit_host[j] is NULL for a job with work");
                all_pos += align256(pos_bytes[j]);
            }
        size_t all_flank = 0;
        if (pos_host && start_host && flank_host)
            for (uint32_t j = 0; j < n_jobs; ++j) {
                flank_bytes[j] = live[j] ? sizeof(uint32_t) * (size_t)ac_hit_flank_words(jobs[j].n_kmers, depth) : 0;
                all_flank += align256(flank_bytes[j]);
            }
        size_t all_edit = 0;
        if (pos_host && start_host && edit_host)
            for (uint32_t j = 0; j < n_jobs; ++j) {
                edit_bytes[j] = live[j] ? sizeof(uint32_t) * (size_t)ac_hit_edit_words(jobs[j].n_kmers, k) : 0;
                all_edit += align256(edit_bytes[j]);
            }
        AC_HIP(ctx, hipSetDevice(ctx->device));
        if (ac_status s2 = grow(ctx, &ctx->d_hits, &ctx->d_hits_cap, all)) return s2;
        if (pos_host)
            if (ac_status s2 = grow(ctx, &ctx->d_pos, &ctx->d_pos_cap, all_pos)) return s2;
        if (pos_host && start_host)
            if (ac_status s2 = grow(ctx, &ctx->d_start, &ctx->d_start_cap, all_pos)) return s2;
        if (all_flank)
            if (ac_status s2 = grow(ctx, &ctx->d_flank, &ctx->d_flank_cap, all_flank)) return s2;
        if (all_edit)
            if (ac_status s2 = grow(ctx, &ctx->d_edit, &ctx->d_edit_cap, all_edit)) return s2;
        size_t at = 0, at_pos = 0, at_flank = 0, at_edit = 0;
        for (uint32_t j = 0; j < n_jobs; ++j) {
            d_hits[j] = (uint32_t*)((char*)ctx->d_hits + at);
            at += align256(hits_bytes[j]);
            if (pos_host) {
                d_pos[j] = (uint32_t*)((char*)ctx->d_pos + at_pos);
                if (start_host) d_start[j] = (uint32_t*)((char*)ctx->d_start + at_pos);
                at_pos += align256(pos_bytes[j]);
            }
            if (all_flank) {
                d_flank[j] = (uint32_t*)((char*)ctx->d_flank + at_flank);
                at_flank += align256(flank_bytes[j]);
            }
            if (all_edit) {
                d_edit[j] = (uint32_t*)((char*)ctx->d_edit + at_edit);
                at_edit += align256(edit_bytes[j]);
            }
        }
    }
    AC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // every job's k-mers in one upload; uint32 counts, one D2H
    std::vector<uint64_t> km;
    km.reserve(total);
    for (uint32_t j = 0; j < n_jobs; ++j) km.insert(km.end(), jobs[j].kmers, jobs[j].kmers + jobs[j].n_kmers);
    if (ac_status s2 = grow(ctx, &ctx->d_kmers, &ctx->d_kmers_cap, sizeof(uint64_t) * total)) return s2;
    if (ac_status s2 = grow(ctx, &ctx->d_counts, &ctx->d_counts_cap, sizeof(uint32_t) * total)) return s2;
    AC_HIP(ctx, hipMemcpyAsync(ctx->d_kmers, km.data(), sizeof(uint64_t) * total, hipMemcpyHostToDevice, st));
    ac_segment seg[AC_MAX_JOBS];
    uint64_t base = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        seg[j].kmers = (const uint64_t*)ctx->d_kmers + base;
        seg[j].n_kmers = jobs[j].n_kmers;
        seg[j].sample = jobs[j].sample;
        seg[j].counts = (uint32_t*)ctx->d_counts + base;
        base += jobs[j].n_kmers;
    }
    CountLaunch rq(k, seg, n_jobs, st);
    rq.no_n = no_n;
    rq.ulen = ulen;
    rq.hits = hits_host ? d_hits : nullptr;
    rq.pos = hits_host && pos_host ? d_pos : nullptr;
    if (ac_status rc = launch(ctx, rq)) return rc;
    ctx->h_counts.resize(total);
    AC_HIP(ctx, hipMemcpyAsync(ctx->h_counts.data(), ctx->d_counts, sizeof(uint32_t) * total, hipMemcpyDeviceToHost, st));
    if (hits_host)
        for (uint32_t j = 0; j < n_jobs; ++j)
            if (jobs[j].n_kmers && jobs[j].sample.n_windows)
                AC_HIP(ctx, hipMemcpyAsync(hits_host[j], d_hits[j], hits_bytes[j], hipMemcpyDeviceToHost, st));
    if (hits_host && pos_host)
        for (uint32_t j = 0; j < n_jobs; ++j)
            if (jobs[j].n_kmers && jobs[j].sample.n_windows)
                AC_HIP(ctx, hipMemcpyAsync(pos_host[j], d_pos[j], pos_bytes[j], hipMemcpyDeviceToHost, st));
    if (hits_host && pos_host && start_host)
        for (uint32_t j = 0; j < n_jobs; ++j)
            if (jobs[j].n_kmers && jobs[j].sample.n_windows) {
                // (hits_refusal has let only equal windows of 1..256 bases through: ulen[j] is their length)
                if (ac_status rc = span_device(ctx, k, seg[j].kmers, jobs[j].n_kmers, &jobs[j].sample, ulen[j], d_hits[j],
                                               d_pos[j], ctx->max_errors + 1u, d_start[j], st))
                    return rc;
                AC_HIP(ctx, hipMemcpyAsync(start_host[j], d_start[j], pos_bytes[j], hipMemcpyDeviceToHost, st));
                // (the top level plane: plane E of the E + 1, each one ac_window_hits_words at budget 0)
                const uint32_t* top = d_hits[j] + (size_t)ctx->max_errors *
                                                      (size_t)ac_window_hits_words(jobs[j].n_kmers, jobs[j].sample.n_windows, 0u);
                if (flank_host) {
                    if (ac_status rc = flank_device(ctx, &jobs[j].sample, ulen[j], top, d_pos[j], d_start[j], jobs[j].n_kmers,
                                                    depth, d_flank[j], st))
                        return rc;
                    AC_HIP(ctx, hipMemcpyAsync(flank_host[j], d_flank[j], flank_bytes[j], hipMemcpyDeviceToHost, st));
                }
                if (edit_host) {
                    if (ac_status rc = edit_device(ctx, k, seg[j].kmers, jobs[j].n_kmers, &jobs[j].sample, ulen[j], top, d_pos[j],
                                                   d_start[j], d_edit[j], st))
                        return rc;
                    AC_HIP(ctx, hipMemcpyAsync(edit_host[j], d_edit[j], edit_bytes[j], hipMemcpyDeviceToHost, st));
                }
            }
    if (ac_status rc = ac_check(ctx, st)) return rc;  // synchronises the stream
    base = 0;
    for (uint32_t j = 0; j < n_jobs; ++j)
        for (uint32_t i = 0; i < jobs[j].n_kmers; ++i) jobs[j].counts[i] = ctx->h_counts[base++];
    return AC_OK;
}
}  // namespace ac_detail

extern "C" {

ac_status ac_error_count_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs) {
    return count_samples(ctx, k, jobs, n_jobs, nullptr);
}

uint64_t ac_window_hits_words(uint32_t n_kmers, uint32_t n_windows, uint32_t max_errors) {
    return (uint64_t)(max_errors + 1u) * n_windows * (((uint64_t)n_kmers + 31u) / 32u);
}

// ac_window_hits_device, and -- with_pos: one position matrix per segment beside the hits --
// ac_window_positions_device.
static ac_status window_hits_device(ac_ctx* ctx, uint32_t k, const ac_segment* segments, uint32_t n_segments,
                                    const uint32_t* window_len, uint32_t* const* hits, bool with_pos, uint32_t* const* pos,
                                    void* hip_stream) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (n_segments > AC_MAX_SEGS) return fail(ctx, AC_ERR_INVALID, "too many segments in one launch (max 4)");
    if (n_segments && !hits) return fail(ctx, AC_ERR_INVALID, "window hits: hits is NULL");
    if (with_pos && n_segments && !pos) return fail(ctx, AC_ERR_INVALID, "window positions: pos is NULL");
    uint32_t ul[AC_MAX_SEGS];
    CountLaunch rq(k, segments, n_segments, (hipStream_t)hip_stream);
    if (ac_status st = take_window_len(ctx, window_len, n_segments, ul, &rq.ulen)) return st;
    static uint32_t* const none[AC_MAX_SEGS] = {};
    AC_HIP(ctx, hipSetDevice(ctx->device));
    rq.hits = hits ? hits : none;
    rq.pos = with_pos ? (pos ? pos : none) : nullptr;
    return launch(ctx, rq);
}

ac_status ac_window_hits_device(ac_ctx* ctx, uint32_t k, const ac_segment* segments, uint32_t n_segments,
                                const uint32_t* window_len, uint32_t* const* hits, void* hip_stream) {
    return window_hits_device(ctx, k, segments, n_segments, window_len, hits, false, nullptr, hip_stream);
}

uint64_t ac_window_positions_words(uint32_t n_kmers, uint32_t n_windows) {
    return 8ull * n_windows * (((uint64_t)n_kmers + 31u) / 32u);
}

ac_status ac_window_positions_device(ac_ctx* ctx, uint32_t k, const ac_segment* segments, uint32_t n_segments,
                                     const uint32_t* window_len, uint32_t* const* hits, uint32_t* const* pos,
                                     void* hip_stream) {
    return window_hits_device(ctx, k, segments, n_segments, window_len, hits, true, pos, hip_stream);
}

ac_status ac_window_positions_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs,
                                      uint32_t* const* hits_host, uint32_t* const* pos_host) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (n_jobs && !hits_host) return fail(ctx, AC_ERR_INVALID, "window hits: hits_host is NULL");
    if (n_jobs && !pos_host) return fail(ctx, AC_ERR_INVALID, "window positions: pos_host is NULL");
    static uint32_t* const none[AC_MAX_JOBS] = {};
    return count_samples(ctx, k, jobs, n_jobs, hits_host ? hits_host : none, pos_host ? pos_host : none);
}

ac_status ac_window_spans_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs,
                                  uint32_t* const* hits_host, uint32_t* const* pos_host, uint32_t* const* start_host) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (n_jobs && !hits_host) return fail(ctx, AC_ERR_INVALID, "window hits: hits_host is NULL");
    if (n_jobs && !pos_host) return fail(ctx, AC_ERR_INVALID, "window positions: pos_host is NULL");
    if (n_jobs && !start_host) return fail(ctx, AC_ERR_INVALID, "match spans: start_host is NULL");
    static uint32_t* const none[AC_MAX_JOBS] = {};
    return count_samples(ctx, k, jobs, n_jobs, hits_host ? hits_host : none, pos_host ? pos_host : none,
                         start_host ? start_host : none);
}

ac_status ac_hit_position_profile_device(ac_ctx* ctx, const uint32_t* hits, const uint32_t* pos, uint32_t n_kmers,
                                         uint32_t n_windows, uint32_t levels, uint32_t window_len, uint32_t* profile,
                                         void* hip_stream) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (levels < 1u || levels > 4u) return fail(ctx, AC_ERR_INVALID, "position profile: levels must be 1..4");
    if (window_len < 1u || window_len > 256u) return fail(ctx, AC_ERR_INVALID, "position profile: window_len must be 1..256");
    if (n_kmers && !profile) return fail(ctx, AC_ERR_INVALID, "position profile: profile is NULL");
    if (n_kmers && n_windows && (!hits || !pos)) return fail(ctx, AC_ERR_INVALID, "position profile: hits or pos is NULL");
    AC_HIP(ctx, hipSetDevice(ctx->device));
    AC_HIP(ctx, acamd::launch_hit_position_profile(hits, pos, n_kmers, n_windows, levels, window_len, profile,
                                                   (hipStream_t)hip_stream));
    return AC_OK;
}

ac_status ac_window_hits_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs,
                                 uint32_t* const* hits_host) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (n_jobs && !hits_host) return fail(ctx, AC_ERR_INVALID, "window hits: hits_host is NULL");
    static uint32_t* const none[AC_MAX_JOBS] = {};
    return count_samples(ctx, k, jobs, n_jobs, hits_host ? hits_host : none);
}

ac_status ac_hit_level_counts_device(ac_ctx* ctx, const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows,
                                     uint32_t levels, uint32_t* level_counts, void* hip_stream) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (levels < 1u || levels > 4u) return fail(ctx, AC_ERR_INVALID, "hit levels: levels must be 1..4");
    if (n_kmers && !level_counts) return fail(ctx, AC_ERR_INVALID, "hit levels: level_counts is NULL");
    if (n_kmers && n_windows && !hits) return fail(ctx, AC_ERR_INVALID, "hit levels: hits is NULL");
    AC_HIP(ctx, hipSetDevice(ctx->device));
    AC_HIP(ctx, acamd::launch_hit_level_counts(hits, n_kmers, n_windows, levels, level_counts, (hipStream_t)hip_stream));
    return AC_OK;
}

ac_status ac_set_max_errors(ac_ctx* ctx, uint32_t e) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (e > 3u) return fail(ctx, AC_ERR_INVALID, "max_errors must be 0..3");
    ctx->max_errors = e;
    for (ac_ctx* p : ctx->peers) p->max_errors = e;
    return AC_OK;
}

uint32_t ac_max_errors(const ac_ctx* ctx) { return ctx ? ctx->max_errors : 2u; }

ac_status ac_last_launch(const ac_ctx* ctx, uint64_t* waves, uint32_t* windows_per_wave, uint32_t* groups) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (waves) *waves = ctx->last_waves;
    if (windows_per_wave) *windows_per_wave = ctx->last_wpw;
    if (groups) *groups = ctx->last_groups;
    return AC_OK;
}

uint64_t ac_image_bases(const uint32_t* seq_len, uint32_t n) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += ((uint64_t)seq_len[i] + 31) / 32 * 32;
    return total ? total : 32;
}

ac_status ac_pack_windows(const uint8_t* dna5, const uint64_t* seq_start, const uint32_t* seq_len, uint32_t n,
                          uint32_t* codes, uint32_t* nmask, uint64_t* start, uint32_t* length, uint64_t n_bases) {
    if (n && (!dna5 || !seq_start || !seq_len || !start || !length))
        return fail(nullptr, AC_ERR_INVALID, "NULL argument");
    if (!codes || !nmask) return fail(nullptr, AC_ERR_INVALID, "NULL image");
    if (n_bases % 32 || n_bases < ac_image_bases(seq_len, n))
        return fail(nullptr, AC_ERR_INVALID, "image too small (use ac_image_bases)");
    // The same packer as the jobs stage (host_pack.cpp); it writes every
    // 32-base block the windows occupy, the rest of the image is zeroed here.
    uint64_t used = 0;
    for (uint32_t i = 0; i < n; ++i) used += acamd::image_span(seq_len[i]);
    acamd::pack_dna5_range(dna5, seq_start, seq_len, 0, n, 0, codes, nmask, start, length);
    std::memset(codes + used / 16, 0, sizeof(uint32_t) * ((n_bases - used) / 16));
    std::memset(nmask + used / 32, 0, sizeof(uint32_t) * ((n_bases - used) / 32));
    return AC_OK;
}

ac_status ac_check(ac_ctx* ctx, void* hip_stream) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    AC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    AC_HIP(ctx, hipMemcpyAsync(ctx->h_err, ctx->d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    AC_HIP(ctx, hipStreamSynchronize(st));
    const uint32_t word = *ctx->h_err;
    if (!word) return AC_OK;
    AC_HIP(ctx, hipMemsetAsync(ctx->d_err, 0, sizeof(uint32_t), st));
    AC_HIP(ctx, hipStreamSynchronize(st));
    return device_error(ctx, word);
}


ac_status ac_set_host_cpus(const int* cpus, int n_cpus, int participants) {
    if (n_cpus < 0 || (n_cpus && !cpus) || participants < 0) return fail(nullptr, AC_ERR_INVALID, "bad CPU list");
    acamd::HostPlan plan;
    plan.cpus.assign(cpus, cpus + n_cpus);
    std::sort(plan.cpus.begin(), plan.cpus.end());
    plan.participants = participants ? (unsigned)participants : (unsigned)std::max(1, std::min(16, n_cpus ? n_cpus : 16));
    if (!acamd::set_host_plan(plan))
        return fail(nullptr, AC_ERR_INVALID, "the host pool's CPUs are already fixed (set before the first ac_create)");
    return AC_OK;
}

int ac_host_pool_cpus(int* participants, int* cpus, int cap) {
    const acamd::HostPlan p = acamd::host_plan();
    if (participants) *participants = (int)p.participants;
    for (int i = 0; i < cap && i < (int)p.cpus.size(); ++i) cpus[i] = p.cpus[(size_t)i];
    return (int)p.cpus.size();
}

int ac_plan_host_cpus(const char* const* rank_cpulists, int n_ranks, int rank, const char* allowed_cpulist,
                      const int* core_of, int n_core_of, int* out, int cap) {
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks || !rank_cpulists || !allowed_cpulist) return -1;
    std::vector<std::vector<int>> lists((size_t)n_ranks);
    for (int r = 0; r < n_ranks; ++r) lists[(size_t)r] = acamd::parse_cpulist(rank_cpulists[r] ? rank_cpulists[r] : "");
    std::function<int(int)> core;
    if (core_of) core = [=](int c) { return c >= 0 && c < n_core_of ? core_of[c] : c; };
    const std::vector<int> v = acamd::plan_host_cpus(lists, rank, acamd::parse_cpulist(allowed_cpulist), core);
    for (int i = 0; i < cap && i < (int)v.size(); ++i) out[i] = v[(size_t)i];
    return (int)v.size();
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Pinned host blocks (ac_host_alloc): a sample whose Dna5 bytes and window offsets lie
// in them is read by the count kernel itself (device packing), so a jobs call does no per-window host
// work beyond the length scan.  Process-wide: one registry for every context and device.
namespace {
std::mutex g_blocks_m;
std::vector<HostBlock> g_blocks;
}  // namespace

// The block holding [p, p + bytes) (bytes >= 1), if any.
bool ac_detail::find_block(const void* p, size_t bytes, HostBlock* out) {
    const char* c = (const char*)p;
    std::lock_guard<std::mutex> lk(g_blocks_m);
    for (const HostBlock& b : g_blocks)
        if (c >= b.h && c < b.h + b.n && bytes <= (size_t)(b.h + b.n - c)) {
            *out = b;
            return true;
        }
    return false;
}

extern "C" {
ac_status ac_host_alloc(size_t bytes, void** out) {
    if (!out) return fail(nullptr, AC_ERR_INVALID, "out is NULL");
    *out = nullptr;
    HostBlock b;
    b.n = bytes ? bytes : 16;
    // (to a 4-byte boundary: the device packer reads a block in whole dwords, stage_pack_chunk)
    hipError_t e = hipHostMalloc((void**)&b.h, (b.n + 3) & ~size_t(3), hipHostMallocDefault);
    if (e != hipSuccess) return hip_fail(nullptr, e, "hipHostMalloc");
    e = hipHostGetDevicePointer((void**)&b.d, b.h, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(b.h);
        return hip_fail(nullptr, e, "hipHostGetDevicePointer");
    }
    {
        std::lock_guard<std::mutex> lk(g_blocks_m);
        g_blocks.push_back(b);
    }
    *out = b.h;
    return AC_OK;
}

ac_status ac_host_free(void* p) {
    if (!p) return AC_OK;
    HostBlock b;
    {
        std::lock_guard<std::mutex> lk(g_blocks_m);
        auto it = std::find_if(g_blocks.begin(), g_blocks.end(), [&](const HostBlock& x) { return x.h == p; });
        if (it == g_blocks.end()) return fail(nullptr, AC_ERR_INVALID, "ac_host_free: not a block of ac_host_alloc");
        b = *it;
        g_blocks.erase(it);
    }
    const hipError_t e = hipHostFree(b.h);
    return e == hipSuccess ? AC_OK : hip_fail(nullptr, e, "hipHostFree");
}

#ifdef AC_STAMPS
// Diagnostic builds only: per-wave timestamps of the last launch (not declared in the public header).
int ac_debug_stamps(void* host, size_t bytes) { return (int)acamd::debug_stamps(host, bytes); }
#endif

}  // extern "C"
