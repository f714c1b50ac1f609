// stage_plan.cpp -- see stage_plan.h.  Host-only: the count kernel's header is included for its
// constants and the candidate-group arithmetic, nothing of the HIP runtime is called.
#include "stage_plan.h"

#include <algorithm>
#include <cstdlib>

#include "approx_counter_amd_testing.h"
#include "bs_nfa.h"
#include "host_pack.h"
#include "wm_count.h"

namespace acamd {

bool bs_launch(uint32_t k, uint32_t n, const bool* live, const uint32_t* ulen) {
    static const bool enabled = [] {
        const char* e = std::getenv("AC_BITSLICE");
        return !e || !*e || std::atoi(e) != 0;
    }();
    if (!enabled || !bs::has_k(k) || !ulen) return false;
    for (uint32_t i = 0; i < n; ++i)
        if (live[i] && (ulen[i] == AC_NO_ULEN || ulen[i] == 0u || ulen[i] > 256u)) return false;
    return true;
}

const char* budget_refusal(uint32_t max_errors, uint32_t k, uint32_t n, const bool* live, const uint32_t* ulen) {
    if (max_errors == 2u) return nullptr;
    if (max_errors > 3u) return "max_errors must be 0..3";
    if (bs_launch(k, n, live, ulen)) return nullptr;
    if (!bs::has_k(k)) return "max_errors other than 2 needs k = 16 or 18..32 (the bit-sliced count kernel's lengths)";
    if (!ulen) return "max_errors other than 2 needs equal windows of 1..256 bases (this launch has ragged windows)";
    for (uint32_t i = 0; i < n; ++i) {
        if (!live[i]) continue;
        if (ulen[i] == AC_NO_ULEN)
            return "max_errors other than 2 needs equal windows of 1..256 bases in every job of a launch "
                   "(this launch has ragged windows)";
        if (ulen[i] == 0u || ulen[i] > 256u)
            return "max_errors other than 2 needs equal windows of 1..256 bases (this launch's are longer)";
    }
    return "max_errors other than 2 needs the bit-sliced count kernel (AC_BITSLICE=0 turns it off)";
}

const char* hits_refusal(uint32_t max_errors, uint32_t k, uint32_t n, const bool* live, const uint32_t* ulen,
                         bool multi_device) {
    if (max_errors > 3u) return "max_errors must be 0..3";
    if (multi_device) return "window hits need a single-device context (this one is an ac_create_multi context)";
    if (!bs::has_k(k)) return "window hits need k = 16 or 18..32 (the bit-sliced count kernel's lengths)";
    if (!ulen) return "window hits need equal windows of 1..256 bases (this launch has ragged windows)";
    for (uint32_t i = 0; i < n; ++i) {
        if (!live[i]) continue;
        if (ulen[i] == AC_NO_ULEN)
            return "window hits need equal windows of 1..256 bases in every job of a launch "
                   "(this launch has ragged windows)";
        if (ulen[i] == 0u || ulen[i] > 256u)
            return "window hits need equal windows of 1..256 bases (this launch's are longer)";
    }
    if (!bs_launch(k, n, live, ulen)) return "window hits need the bit-sliced count kernel (AC_BITSLICE=0 turns it off)";
    return nullptr;
}

const char* positions_refusal(uint32_t max_errors, uint32_t k, uint32_t n, const bool* live, const uint32_t* ulen,
                              bool multi_device, const bool* has_pos) {
    if (const char* why = hits_refusal(max_errors, k, n, live, ulen, multi_device)) return why;
    for (uint32_t i = 0; i < n; ++i)
        if (live[i] && !(has_pos && has_pos[i])) return "window positions: pos[i] is NULL for a segment with work";
    return nullptr;
}

uint32_t launch_group_size(uint32_t k, bool staged, bool bs) {
    return bs ? BS_GROUP : cands_per_wave(pack_factor(k), staged);
}

int stage_parts(uint64_t total_w) {
    return total_w >= STAGE_PARTS4_MIN_WINDOWS ? 4 : total_w >= STAGE_PARTS2_MIN_WINDOWS ? 2 : 1;
}

int stage_parts(uint64_t total_w, uint32_t hooks) {
    const int parts = stage_parts(total_w);
    return (hooks & AC_TESTING_TWO_PARTS) && parts < 2 ? 2 : parts;
}

std::vector<uint32_t> shard_cuts(const uint32_t* length, uint32_t n, size_t G) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += length[i];
    std::vector<uint32_t> cut(G + 1, n);
    cut[0] = 0;
    uint64_t acc = 0;
    size_t c = 1;
    for (uint32_t i = 0; i < n && c < G; ++i) {
        acc += length[i];
        while (c < G && acc * G >= total * c) cut[c++] = i + 1;
    }
    return cut;
}

uint32_t part_cut(const uint32_t* length, uint32_t n, double frac) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += length[i];
    const double want = frac * (double)total;
    uint64_t acc = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if ((double)acc >= want) return i;
        acc += length[i];
    }
    return n;
}

std::vector<std::vector<uint32_t>> part_cuts(const ac_job* jobs, uint32_t n_jobs, int parts) {
    std::vector<std::vector<uint32_t>> cuts;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        const uint32_t n = jobs[j].sample.n_windows;
        if (parts == 1)
            cuts.push_back({0u, n});
        else if (parts == 2)
            cuts.push_back({0u, part_cut(jobs[j].sample.length, n, 0.5), n});
        else
            cuts.push_back(shard_cuts(jobs[j].sample.length, n, (size_t)parts));
    }
    return cuts;
}

namespace {

inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// Tasks: contiguous window ranges, about 4 per pool thread.
// (tasks of 128 windows, or the first tasks of every job packed first, were slower: the claims
// contend on the pool's one state line, profiles/r03_m8/ab.log).  The early launch publishes
// progress a finished task at a time, so its tasks stay at most 2,048 windows (~20 us of one
// thread's packing): a large call's first windows then reach the GPU within tens of microseconds
// rather than after a 1/(4 x participants) share of the whole call.
// (Packing a small call with part of the pool -- the others sleeping through it -- was slower:
// cfg2 stage p50 0.129-0.138 vs 0.120-0.122 ms, with multi-ms stalls from waking the sleepers at
// every call; profiles/r04_m6/ab_table.txt.)
// Tasks of at least 1,280 windows: with the round-4 packer (~2.3 ns per 100-base window) a
// 313-window task is shorter than the pool's contended claim, so a cfg2 end took ~15 us to pack
// on 16 threads; 1,280 gave cfg2 stage p50 0.1189-0.1193 vs 0.1223-0.1243 ms at 256, 640 and 2,560
// in between (same box, profiles/r04_m7/ab_table.txt).  AC_TASK_WINDOWS overrides (A/B runs).
std::vector<Task> cut_tasks(const ac_job* jobs, JobPlan& p, unsigned pool_participants, uint64_t min_task) {
    p.total_w = 0;
    for (uint32_t j = 0; j < p.n; ++j)
        if (jobs[j].n_kmers) p.total_w += p.hi[j] - p.lo[j];
    const uint64_t per = std::max<uint64_t>(
        min_task, std::min<uint64_t>(p.early ? std::max<uint64_t>(2048, min_task) : 65536,
                                     p.total_w / (4ull * pool_participants) + 1));
    std::vector<Task> tasks;
    for (uint32_t j = 0; j < p.n; ++j) {
        if (!jobs[j].n_kmers) continue;  // nothing to count: its windows are not needed
        for (uint64_t w = p.lo[j]; w < p.hi[j]; w += per)
            tasks.push_back({j, (uint32_t)w, (uint32_t)std::min<uint64_t>(p.hi[j], w + per), 0, 0, 0u, 0u});
    }
    return tasks;
}

// Every task's span and lengths, then its first image base: a job's image is its tasks' ranges back
// to back.
void scan_spans(const ac_job* jobs, JobPlan& p, std::vector<Task>& tasks, unsigned pool_participants,
                BlockRunner run_blocks) {
    auto span_of = [&](uint32_t t) {
        Task& x = tasks[t];
        x.span = span_scan(jobs[x.job].sample.length + x.w0, x.w1 - x.w0, &x.first_len, &x.len_diff);
    };
    const uint32_t nt = (uint32_t)tasks.size();
    if (p.total_w <= SPAN_SCAN_SERIAL_MAX_WINDOWS || !run_blocks) {
        // a serial pass is cheaper than a pool round trip up to ~256k windows
        for (uint32_t t = 0; t < nt; ++t) span_of(t);
    } else {
        // in blocks of consecutive tasks, ~2 per participant: one pool task per packing task (~1,000 at
        // cfg4) spent ~220 us in contended claims for a ~30 us scan (profiles/r04_m1/bench_cfg4.log)
        const uint32_t nb = std::min<uint32_t>(nt, 2u * pool_participants);
        run_blocks(nb, [&](uint32_t b) {
            for (uint32_t t = (uint32_t)((uint64_t)nt * b / nb); t < (uint32_t)((uint64_t)nt * (b + 1) / nb); ++t) span_of(t);
        });
    }
    uint64_t acc[AC_MAX_JOBS] = {};
    for (Task& x : tasks) {
        x.first = acc[x.job];
        acc[x.job] += x.span;
    }
    // Image of each job: at least one 32-base block.
    for (uint32_t j = 0; j < p.n; ++j) {
        p.no_bases[j] = acc[j] == 0;
        p.n_bases[j] = std::max<uint64_t>(32, acc[j]);
    }
}

// The staging block: per job kmers | codes | nmask | start | length, then the error word, every
// job's counts and (tagged completion) the candidate groups' error words, each 256-B aligned.
void layout_block(uint32_t k, const ac_job* jobs, JobPlan& p, bool have_d_counts) {
    size_t off = 0;
    for (uint32_t j = 0; j < p.n; ++j) {
        const uint32_t nw = jobs[j].n_kmers ? p.hi[j] - p.lo[j] : 0;
        // the N bitmap, then the window descriptors: a job without N / with equal windows is
        // sent without them (job by job)
        p.off_kmers[j] = off;
        // (early launch: the k-mer section fills whole staging chunks, which the kernel copies
        // without waiting for the host -- the k-mers are in place before the launch)
        off = p.early ? off + (sizeof(uint64_t) * jobs[j].n_kmers + AC_STAGE_CHUNK - 1) / AC_STAGE_CHUNK * AC_STAGE_CHUNK
                      : align256(off + sizeof(uint64_t) * jobs[j].n_kmers);
        p.off_codes[j] = off;
        off = align256(off + sizeof(uint32_t) * (p.n_bases[j] / 16));
        p.off_nmask[j] = off;
        off = align256(off + sizeof(uint32_t) * (p.n_bases[j] / 32));
        p.off_start[j] = off;
        off = align256(off + sizeof(uint64_t) * nw);
        p.off_len[j] = off;
        off = align256(off + sizeof(uint32_t) * nw);
    }
    p.off_err = off;
    off = align256(off + sizeof(uint32_t));
    p.tag = p.early && !have_d_counts;
    for (uint32_t j = 0; j < p.n; ++j) {
        p.off_counts[j] = off;
        off = align256(off + (p.tag ? sizeof(uint64_t) : sizeof(uint32_t)) * jobs[j].n_kmers);
    }
    p.off_gerr = off;
    p.n_gerr = 0;
    if (p.tag) {
        // (tagged: a staged launch; the kernel is the one launch() will pick for these jobs)
        bool live[AC_MAX_JOBS];
        for (uint32_t j = 0; j < p.n; ++j) live[j] = jobs[j].n_kmers && p.hi[j] > p.lo[j];
        const uint32_t cpw = launch_group_size(k, true, bs_launch(k, p.n, live, p.ulen));
        for (uint32_t j = 0; j < p.n; ++j)
            if (jobs[j].n_kmers && p.hi[j] > p.lo[j]) p.n_gerr += (jobs[j].n_kmers + cpw - 1) / cpw;
        off = align256(off + sizeof(uint64_t) * p.n_gerr);
    }
    p.total = off;
    // (the early launch's header and buffer descriptors count a segment's bytes in 31 bits)
    if (p.early && p.total >= (size_t(1) << 31)) p.early = p.tag = false;
}

// Equal windows and inline N records, per job (JobPlan::ulen / nrec).
void window_forms(JobPlan& p, const std::vector<Task>& tasks) {
    for (uint32_t j = 0; j < p.n; ++j) {
        bool any = false, equal = true;
        uint32_t l0 = 0;
        for (const Task& x : tasks)
            if (x.job == j) {
                if (!any) l0 = x.first_len;
                any = true;
                equal = equal && x.len_diff == 0u && x.first_len == l0;
            }
        p.ulen[j] = (any && equal) ? l0 : AC_NO_ULEN;
        p.nrec[j] = p.ulen[j] != AC_NO_ULEN && nrec_bits(p.ulen[j]) != 0u;
    }
}

// Early launch: what the launch is made of -- the first `pre` jobs sent ahead of it (AC_STAGE_EARLY=2:
// the first; the test hook AC_TESTING_ALL_AHEAD: all), each job's region and chunks, the chunk tickets.
// The region of job j: k-mers, codes, then the N bitmap, and the window descriptors unless its
// windows have one length.
void early_regions(JobPlan& p, int early_mode, uint32_t hooks) {
    p.pre = (hooks & AC_TESTING_ALL_AHEAD) ? p.n : (early_mode == 2 && p.n > 1) ? 1u : 0u;
    p.tickets = 0;
    for (uint32_t j = 0; j < p.n; ++j) {
        const size_t end = p.ulen[j] != AC_NO_ULEN ? p.off_start[j] : (j + 1 < p.n ? p.off_kmers[j + 1] : p.off_err);
        p.region[j] = end - p.off_kmers[j];
        p.chunks[j] = j < p.pre ? 0u : (uint32_t)((p.region[j] + AC_STAGE_CHUNK - 1) / AC_STAGE_CHUNK);
        p.codes_off[j] = (uint32_t)(p.off_codes[j] - p.off_kmers[j]);
        p.tickets += p.chunks[j] ? p.chunks[j] + 1u : 0u;
    }
}

}  // namespace

std::vector<Task> plan_stage(uint32_t k, const ac_job* jobs, JobPlan& p, bool have_d_counts, unsigned pool_participants,
                             uint64_t min_task_windows, int early_mode, uint32_t hooks, BlockRunner run_blocks) {
    std::vector<Task> tasks = cut_tasks(jobs, p, pool_participants, min_task_windows);
    scan_spans(jobs, p, tasks, pool_participants, run_blocks);
    window_forms(p, tasks);  // (before the layout: the groups' error words depend on the kernel, that on ulen)
    {  // the launch's route decides whether it can count at the plan's edit budget
        bool live[AC_MAX_JOBS];
        for (uint32_t j = 0; j < p.n; ++j) live[j] = jobs[j].n_kmers && p.hi[j] > p.lo[j];
        p.refusal = nullptr;
        // (hits first: its refusal names the hits call's own constraint)
        if (p.want_hits)
            p.refusal = p.want_pos ? positions_refusal(p.max_errors, k, p.n, live, p.ulen, p.multi_device, p.has_pos)
                                   : hits_refusal(p.max_errors, k, p.n, live, p.ulen, p.multi_device);
        if (!p.refusal) p.refusal = budget_refusal(p.max_errors, k, p.n, live, p.ulen);
        for (uint32_t j = 0; j < p.n; ++j) {  // the launch's rows in the jobs' matrices
            const uint64_t words = ((uint64_t)jobs[j].n_kmers + 31u) / 32u;
            p.mat_windows[j] = jobs[j].sample.n_windows;
            p.mat_row_off[j] = (uint64_t)p.lo[j] * words;
            p.mat_plane[j] = (uint64_t)jobs[j].sample.n_windows * words;
        }
    }
    layout_block(k, jobs, p, have_d_counts);
    if (p.early) early_regions(p, early_mode, hooks);
    return tasks;
}

}  // namespace acamd
