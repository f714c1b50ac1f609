// budget_plan_check -- asks the jobs stage's planner (approx_counter_amd/csrc/stage_plan.cpp) whether a
// launch may count at an edit budget (JobPlan::max_errors -> JobPlan::refusal, budget_refusal), for
// tests/test_budget_cpu.py (host-only; built there with the sanitizers on).
//   budget_plan_check MAX_ERRORS K EARLY JOB...
//     JOB: n_kmers:len[xcount][,len[xcount]...]   e.g. 300:100x37  or  5:100x3,101
//   prints "ok" when the plan accepts the launch, else "refused: <the constraint>"; exit 0 either way
//   (2: bad arguments).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "stage_plan.h"

int main(int argc, char** argv) {
    if (argc < 5 || argc - 4 > AC_MAX_JOBS) {
        std::fprintf(stderr, "usage: budget_plan_check MAX_ERRORS K EARLY JOB...\n");
        return 2;
    }
    acamd::JobPlan p;
    p.max_errors = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    const uint32_t k = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    p.early = std::strtoul(argv[3], nullptr, 10) != 0;
    p.n = (uint32_t)(argc - 4);
    std::vector<uint32_t> lengths[AC_MAX_JOBS];
    ac_job jobs[AC_MAX_JOBS] = {};
    for (uint32_t j = 0; j < p.n; ++j) {
        const std::string spec = argv[4 + j];
        const size_t colon = spec.find(':');
        if (colon == std::string::npos) return 2;
        jobs[j].n_kmers = (uint32_t)std::strtoul(spec.c_str(), nullptr, 10);
        for (size_t at = colon + 1; at < spec.size();) {
            char* end = nullptr;
            const uint32_t len = (uint32_t)std::strtoul(spec.c_str() + at, &end, 10);
            uint32_t count = 1;
            if (*end == 'x') count = (uint32_t)std::strtoul(end + 1, &end, 10);
            if (count > (1u << 20) || (*end && *end != ',')) return 2;
            lengths[j].insert(lengths[j].end(), count, len);
            at = (size_t)(end - spec.c_str()) + (*end ? 1 : 0);
        }
        jobs[j].sample.n_windows = (uint32_t)lengths[j].size();
        jobs[j].sample.length = lengths[j].data();
        p.lo[j] = 0;
        p.hi[j] = jobs[j].sample.n_windows;
    }
    (void)acamd::plan_stage(k, jobs, p, false, 1, 1280, 1, 0);
    if (p.refusal) std::printf("refused: %s\n", p.refusal);
    else std::printf("ok\n");
    return 0;
}
