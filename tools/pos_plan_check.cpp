// pos_plan_check -- asks the plan layer (approx_counter_amd/csrc/stage_plan.cpp positions_refusal) whether a
// launch may write match end positions, for tests/test_positions_cpu.py (host-only; built there with the
// sanitizers on).
//   pos_plan_check MAX_ERRORS K MULTI JOB...
//     MULTI: 1 = an ac_create_multi context
//     JOB: n_kmers:ulen:n_windows[:0], ulen = the job's equal window length, or "r" for ragged windows, a
//          trailing ":0" = the job's position matrix is NULL;
//          the one argument "none" instead of the jobs = a call without window lengths (window_len NULL)
//   prints "ok" or "refused: <the constraint>"; exit 0 either way (2: bad arguments).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "stage_plan.h"
#include "wm_count.h"

int main(int argc, char** argv) {
    if (argc < 5 || argc - 4 > AC_MAX_JOBS) {
        std::fprintf(stderr, "usage: pos_plan_check MAX_ERRORS K MULTI JOB...\n");
        return 2;
    }
    const uint32_t E = (uint32_t)std::strtoul(argv[1], nullptr, 10), k = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const bool multi = std::strtoul(argv[3], nullptr, 10) != 0;
    const char* why;
    if (!std::strcmp(argv[4], "none")) {
        const bool live[1] = {true};
        why = acamd::positions_refusal(E, k, 1, live, nullptr, multi, live);
    } else {
        bool live[AC_MAX_JOBS], has_pos[AC_MAX_JOBS];
        uint32_t ulen[AC_MAX_JOBS];
        const uint32_t n = (uint32_t)(argc - 4);
        for (uint32_t j = 0; j < n; ++j) {
            char* end = nullptr;
            const unsigned long nk = std::strtoul(argv[4 + j], &end, 10);
            if (*end != ':') return 2;
            ulen[j] = end[1] == 'r' ? AC_NO_ULEN : (uint32_t)std::strtoul(end + 1, &end, 10);
            if (end[1] == 'r') end += 2;
            if (*end != ':') return 2;
            live[j] = nk && std::strtoul(end + 1, &end, 10);
            has_pos[j] = !(end[0] == ':' && end[1] == '0');
        }
        why = acamd::positions_refusal(E, k, n, live, ulen, multi, has_pos);
    }
    if (why) std::printf("refused: %s\n", why);
    else std::printf("ok\n");
    return 0;
}
