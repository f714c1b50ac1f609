// jobs_hits_plan_check -- runs the jobs stage's planner (approx_counter_amd/csrc/stage_plan.cpp plan_stage) with
// hit levels or end positions asked for, for tests/test_jobs_hits_cpu.py (host-only; built there with the
// sanitizers on): the plan's refusal or route, and where each part's rows lie in the jobs' matrices.
//   jobs_hits_plan_check MAX_ERRORS K EARLY MULTI POS PARTS JOB...
//     EARLY: 1 = planned as an early launch;  MULTI: 1 = an ac_create_multi context
//     POS: 0 = hit levels, 1 = positions too, 2 = positions asked for but the first job with work has no
//          position matrix
//     PARTS: 1, 2 or 4 -- the call's parts (part_cuts), each planned on its own
//     JOB: n_kmers:ulen:n_windows, ulen = the job's equal window length, or "r": ragged windows (lengths
//          90, 91, ..)
//   prints per part "part Q: refused: <constraint>" or "part Q: ok early=E tag=T", then per job with windows
//   "part Q job J: rows LO..HI row_off OFF plane PLANE mat_windows N"; exit 0 either way (2: bad arguments).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stage_plan.h"
#include "wm_count.h"

int main(int argc, char** argv) {
    if (argc < 8 || argc - 7 > AC_MAX_JOBS) {
        std::fprintf(stderr, "usage: jobs_hits_plan_check MAX_ERRORS K EARLY MULTI POS PARTS JOB...\n");
        return 2;
    }
    auto num = [&](int i) { return (uint32_t)std::strtoul(argv[i], nullptr, 10); };
    const uint32_t E = num(1), k = num(2), early = num(3), multi = num(4), pos = num(5), parts = num(6);
    if (parts != 1 && parts != 2 && parts != 4) return 2;
    const uint32_t n = (uint32_t)(argc - 7);
    std::vector<uint64_t> kmers[AC_MAX_JOBS], offset[AC_MAX_JOBS];
    std::vector<uint32_t> length[AC_MAX_JOBS];
    std::vector<uint8_t> bases(1, 0);
    ac_job jobs[AC_MAX_JOBS];
    std::memset(jobs, 0, sizeof jobs);
    for (uint32_t j = 0; j < n; ++j) {
        char* end = nullptr;
        const unsigned long nk = std::strtoul(argv[7 + j], &end, 10);
        if (*end != ':') return 2;
        const bool ragged = end[1] == 'r';
        const uint32_t ulen = ragged ? 90u : (uint32_t)std::strtoul(end + 1, &end, 10);
        if (ragged) end += 2;
        if (*end != ':') return 2;
        const uint32_t nw = (uint32_t)std::strtoul(end + 1, nullptr, 10);
        kmers[j].assign(nk ? nk : 1, 0);
        offset[j].assign(nw ? nw : 1, 0);
        length[j].assign(nw ? nw : 1, 0);
        for (uint32_t i = 0; i < nw; ++i) length[j][i] = ragged ? ulen + i % 20u : ulen;
        jobs[j].kmers = kmers[j].data();
        jobs[j].n_kmers = (uint32_t)nk;
        jobs[j].sample.bases = bases.data();  // (the planner reads the lengths only)
        jobs[j].sample.offset = offset[j].data();
        jobs[j].sample.length = length[j].data();
        jobs[j].sample.n_windows = nw;
    }
    const std::vector<std::vector<uint32_t>> cuts = acamd::part_cuts(jobs, n, (int)parts);
    for (uint32_t q = 0; q < parts; ++q) {
        acamd::JobPlan p;
        p.n = n;
        bool first = true;
        for (uint32_t j = 0; j < n; ++j) {
            p.lo[j] = cuts[j][q];
            p.hi[j] = cuts[j][q + 1];
            const bool work = jobs[j].n_kmers && p.hi[j] > p.lo[j];
            p.has_pos[j] = pos == 1 || (pos == 2 && !(work && first));
            if (work) first = false;
        }
        p.early = early != 0;
        p.max_errors = E;
        p.want_hits = true;
        p.want_pos = pos != 0;
        p.multi_device = multi != 0;
        (void)acamd::plan_stage(k, jobs, p, false, 1, 1280, 1, 0);
        if (p.refusal) std::printf("part %u: refused: %s\n", q, p.refusal);
        else std::printf("part %u: ok early=%d tag=%d\n", q, (int)p.early, (int)p.tag);
        for (uint32_t j = 0; j < n; ++j)
            if (jobs[j].sample.n_windows)
                std::printf("part %u job %u: rows %u..%u row_off %llu plane %llu mat_windows %u\n", q, j, p.lo[j], p.hi[j],
                            (unsigned long long)p.mat_row_off[j], (unsigned long long)p.mat_plane[j], p.mat_windows[j]);
    }
    return 0;
}
