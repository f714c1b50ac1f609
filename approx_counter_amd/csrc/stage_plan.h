// stage_plan.h -- the plan of one jobs-stage launch (ac_error_count_jobs / _submit; DESIGN.md §4c,
// §4d): how a call's windows are cut into packing tasks and where every array lies in the staging
// block.  Pure host arithmetic over the jobs' window lengths -- no HIP call, no context -- that the
// host stage (jobs_stage.cpp) and the count kernel both depend on; tests/test_stage_plan.py runs it
// on the CPU.  Private to the library.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <vector>

#include "approx_counter_amd.h"

#pragma GCC visibility push(hidden)

namespace acamd {

// A packing task: windows [w0, w1) of one job.
struct Task {
    uint32_t job, w0, w1;
    uint64_t first;  // the range's first image base (the earlier tasks' spans of its job)
    uint64_t span;   // image bases the range occupies
    uint32_t first_len, len_diff;  // the range's first window length; OR of (length ^ first_len)
};

// Where one device's part of a jobs call lives in its staging slot (the same
// offsets in the pinned host block and the device block).  Inputs first
// (sent by one DMA), then the device error word and the uint32 counts (the
// way back: one DMA from off_err to the end).
struct JobPlan {
    uint32_t n = 0;
    uint32_t lo[AC_MAX_JOBS] = {}, hi[AC_MAX_JOBS] = {};  // window range of each job on this device
    uint64_t total_w = 0;                                   // windows of the jobs that have candidates
    uint64_t n_bases[AC_MAX_JOBS] = {};
    bool no_bases[AC_MAX_JOBS] = {};  // no window base at all: the image is its one (zero) 32-base block
    size_t off_kmers[AC_MAX_JOBS] = {}, off_codes[AC_MAX_JOBS] = {}, off_nmask[AC_MAX_JOBS] = {};
    size_t off_start[AC_MAX_JOBS] = {}, off_len[AC_MAX_JOBS] = {}, off_counts[AC_MAX_JOBS] = {};
    size_t off_err = 0, total = 0;
    bool early = false;  // the early-launch stage (the kernel stages its own inputs, host-polled completion)
    // early launch with host counts (synchronous calls): tagged completion -- u64 counts (generation << 32 |
    // count) and one tagged error word per candidate group at off_gerr (n_gerr of them)
    bool tag = false;
    size_t off_gerr = 0;
    uint32_t n_gerr = 0;
    uint32_t gen = 0;    // its generation (the header flags and the tagged counts carry it)
    int slot = 0;     // staging slot (set by the caller: a synchronous part q uses slot q, a submit part its set's)
    int scratch = 0;  // count-kernel scratch set (ac_ctx::sc)
    // equal windows (the common case: every start window sl bases, every end window sl + 1): their
    // length, else AC_NO_ULEN; and whether such windows carry inline N records (nrec.h), so the job's
    // N bitmap is needed (and sent) only if some window overflowed its record
    uint32_t ulen[AC_MAX_JOBS] = {};
    bool nrec[AC_MAX_JOBS] = {};
    // early launch: what the launch is made of -- the first `pre` jobs sent ahead of it, each job's
    // region (bytes from its k-mers on) and chunks, the chunk tickets, the copier workgroups (set by
    // the caller from the tickets)
    size_t region[AC_MAX_JOBS] = {};
    uint32_t chunks[AC_MAX_JOBS] = {}, codes_off[AC_MAX_JOBS] = {};
    uint64_t tickets = 0;
    uint32_t pre = 0, copiers = 0;
    // device packing: job j's Dna5 bytes / offsets read by the kernel from pinned memory
    bool dp[AC_MAX_JOBS] = {};
    bool dp_any = false;
    // the edit budget the launch is to count at (set by the caller; 2 = the reference's), and, from the
    // plan, why this launch cannot (budget_refusal): the caller then fails the call instead of launching
    uint32_t max_errors = 2;
    const char* refusal = nullptr;
    // Hits from the jobs stage (ac_window_hits_jobs / ac_window_positions_jobs; DESIGN.md §4e "Hits from the
    // jobs stage"), set by the caller: this launch writes hit levels / end positions too, on a context of
    // several devices or not, and which jobs came with a position matrix.  plan_stage then asks hits_refusal /
    // positions_refusal of the launch (the answer in `refusal`, before the budget's) and says where the
    // launch's rows lie in each job's matrices: job j's windows [lo[j], hi[j]) are rows lo[j].. of a matrix of
    // mat_windows[j] = the job's n_windows rows -- mat_row_off[j] words from the matrix's start to the
    // launch's first row in every plane, the planes mat_plane[j] words apart.  Row w of a job's matrix is the
    // job's window w: the stage packs window i into slot i - lo[j] of the launch's image.
    bool want_hits = false, want_pos = false, multi_device = false;
    bool has_pos[AC_MAX_JOBS] = {};
    uint32_t mat_windows[AC_MAX_JOBS] = {};
    uint64_t mat_row_off[AC_MAX_JOBS] = {}, mat_plane[AC_MAX_JOBS] = {};
};

// Calls whose pack and DMA take hundreds of
// microseconds or more are cut into parts (equal bases, one stream each), so
// part q + 1 is packed and sent while part q counts: two parts from 2^17
// windows, four from 2^19.  Same box, interleaved (profiles/r02_stage_parts_ab2.log):
// cfg4 (2M windows) step p50 10.26-10.31 ms in four parts, 10.42-10.49 in three,
// 11.27 in two (13.3 in one, r02_stage_parts_ab.log); cfg3 (200k windows)
// 3.27-3.29 ms in two vs 3.24-3.40 one-part with round 2's (since removed) zero-copy / DMA chooser
// and 3.42 one-part DMA.  Eight parts from 2^20 windows: cfg4 9.77-9.86 vs 9.79-9.96 ms in four
// (profiles/r03_m14/parts_ab.log, round 3), not kept.
constexpr uint64_t STAGE_PARTS2_MIN_WINDOWS = 1ull << 17, STAGE_PARTS4_MIN_WINDOWS = 1ull << 19;
int stage_parts(uint64_t total_w);
// ... and with the test hooks (approx_counter_amd_testing.h): AC_TESTING_TWO_PARTS cuts a call that would
// take one part into two, whatever its size.
int stage_parts(uint64_t total_w, uint32_t hooks);

// Shard g of G of job windows [0, n): contiguous, balanced by bases (the rule
// of ac_error_count's multi-device split and approx_counter_amd/shard.py).
// All G + 1 cut points of job windows [0, n) in one pass (shard g = [cut[g], cut[g + 1])).
std::vector<uint32_t> shard_cuts(const uint32_t* length, uint32_t n, size_t G);
// The two parts of a single-device call: windows [0, cut) and [cut, n), the
// first holding `frac` of the bases.
uint32_t part_cut(const uint32_t* length, uint32_t n, double frac);
// Every job's part boundaries of a single-device call in `parts` parts, once
// (equal shares of the bases).
std::vector<std::vector<uint32_t>> part_cuts(const ac_job* jobs, uint32_t n_jobs, int parts);

// Which count kernel a launch runs on, decided once for the plan and the launch: the
// bit-sliced kernel counts it when k is in AC_BS_K_LIST, every live segment (one with candidates and
// windows: live[i]) holds equal windows of 1..256 bases (ulen[i]; ulen NULL = none does), and
// AC_BITSLICE is not 0 (A/B runs, the tests of the word-parallel kernel).
bool bs_launch(uint32_t k, uint32_t n, const bool* live, const uint32_t* ulen);
// The edit budget's question, asked of the same launch by the jobs stage's plan and by the launch: a
// budget other than 2 counts on bit-sliced launches only (DESIGN.md §4e "Edit budget").  NULL when the
// launch may run at `max_errors`, else the constraint it breaks, as the text of the caller's error --
// nothing is launched then: no launch ever counts under another budget than the one asked for.
const char* budget_refusal(uint32_t max_errors, uint32_t k, uint32_t n, const bool* live, const uint32_t* ulen);
// The hit levels' question (ac_window_hits_*; DESIGN.md §4e "Hit levels"), asked of the same launch: the
// hits-writing kernels are bit-sliced and plain, so a launch yields hits only where bs_launch routes it to
// the bit-sliced kernel, on a single-device context, at the context's budget 0..3.  NULL when it may, else
// the constraint it breaks -- nothing is launched then and nothing falls back.
const char* hits_refusal(uint32_t max_errors, uint32_t k, uint32_t n, const bool* live, const uint32_t* ulen,
                         bool multi_device);
// The match end positions' question (ac_window_positions_*; DESIGN.md §4e "Match end positions"): the hit
// levels' (hits_refusal, asked, not restated), and a position matrix for every segment with work --
// has_pos[i]: segment i's is not NULL.
const char* positions_refusal(uint32_t max_errors, uint32_t k, uint32_t n, const bool* live, const uint32_t* ulen,
                              bool multi_device, const bool* has_pos);
// Candidates of such a launch's candidate groups: BS_GROUP for a bit-sliced launch, else the
// word-parallel kernel's candidates per wave.  Everything counted per group goes by it: the work
// items, the acc slots, the sub-queues, a tagged launch's group error words and their polling.
uint32_t launch_group_size(uint32_t k, bool staged, bool bs);

// run(n, fn): fn(b) for every b in [0, n), on the caller's worker pool.
using BlockRunner = void (*)(uint32_t n, const std::function<void(uint32_t)>& fn);
// A span scan of more windows than this goes through the BlockRunner, when there is one.
constexpr uint64_t SPAN_SCAN_SERIAL_MAX_WINDOWS = 1ull << 18;

// Plans the launch of windows [p.lo[j], p.hi[j]) of jobs[0, p.n) (p.n, lo, hi, early, slot and scratch
// set by the caller, with want_hits / want_pos / multi_device / has_pos): cuts the packing tasks (the return value; of them the planner reads
// jobs[j].sample.length only), scans their spans, and fills in every other field of p but gen,
// copiers and dp.  `have_d_counts`: the counts go to device memory (a submit), so no tagged
// completion.  `pool_participants`: threads that will pack (caller included); `min_task_windows`: the
// smallest task (AC_TASK_WINDOWS).  `early_mode`: AC_STAGE_EARLY (2 = the first job sent ahead of the
// launch); `hooks`: the test hooks (approx_counter_amd_testing.h).  p.early may come back false: a
// block of 2^31 bytes or more takes the DMA path.
std::vector<Task> plan_stage(uint32_t k, const ac_job* jobs, JobPlan& p, bool have_d_counts, unsigned pool_participants,
                             uint64_t min_task_windows, int early_mode, uint32_t hooks,
                             BlockRunner run_blocks = nullptr);

}  // namespace acamd

#pragma GCC visibility pop
