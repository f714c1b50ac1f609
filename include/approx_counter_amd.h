/*
 * approx_counter_amd.h -- C ABI of the MI355X approximate-count stage.
 *
 * Drop-in boundary for qbonenfant/approx_counter's hot path.  The reference
 * has no plugin/FFI API; its one internal seam on the hot
 * path is
 *
 *     counter errorCount(sequence_set_type& sequences, pair_vector& exact_count,
 *                        uint8_t nb_thread, uint8_t k, uint8_t v);
 *                                              -- approx_counter.cpp:531
 *
 * called once per (run, end) from main (approx_counter.cpp:922).  Every entry
 * point below names the reference code it replaces.  Plain C types only; no
 * exceptions and no exit() cross this boundary: every call returns an
 * ac_status (0 = OK) and the text of the last failure is available from
 * ac_last_error().  The library has no CPU fallback: without a HIP device
 * ac_create() fails with AC_ERR_DEVICE.
 *
 * Counting contract (model M1): for every candidate k-mer,
 *     count = sum over windows w of max(0, 3 - d(kmer, w))
 * where d is the semi-global Levenshtein distance between the whole k-mer and
 * the best substring of w, a non-ACGT base matching nothing.  This equals the
 * reference's  sum_e popcount(tcount[e])  (approx_counter.cpp:553-593) under
 * SeqAn 2.4's find<0,2>(..., EditDistance()) semantics.
 */
#ifndef APPROX_COUNTER_AMD_H
#define APPROX_COUNTER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AC_ABI_VERSION 8

typedef int32_t ac_status;
#define AC_OK 0
#define AC_ERR_INVALID 1  /* bad argument (k outside [2,32], NULL pointer, layout) */
#define AC_ERR_DEVICE 2   /* no HIP device, or a HIP runtime failure               */
#define AC_ERR_NOMEM 3    /* device or host allocation failed                     */
#define AC_ERR_INTERNAL 4

typedef struct ac_ctx ac_ctx;

/*
 * Packed sample ("window image").  Replaces the StringSet<Dna5String> sample
 * (approx_counter.cpp:38, built by sampleSequences 415-476).
 *   codes : 2 bits per base (A0 C1 G2 T3; any value for N), base b at bits
 *           2*(b%16)..2*(b%16)+1 of codes[b/16]          (n_bases/16 words)
 *   nmask : bit (b%32) of nmask[b/32] set iff base b is not A/C/G/T
 *           (Dna5 ordValue 4, "N")                       (n_bases/32 words)
 *   start : window i occupies bases [start[i], start[i]+length[i]);
 *           start[i] % 32 == 0 (each window begins on a 32-base boundary)
 *   length: window length in bases (sl for a start window, sl+1 for an end
 *           window, approx_counter.cpp:463/466); 0 is allowed
 *   n_bases: size of the image in bases, a multiple of 32 below 2^34 - 4096
 *           (an image of that size or more is refused, AC_ERR_INVALID)
 * All pointers are host pointers for ac_error_count() and device pointers for
 * the *_device entry points.
 */
typedef struct ac_windows {
    const uint32_t* codes;
    const uint32_t* nmask;
    const uint64_t* start;
    const uint32_t* length;
    uint32_t n_windows;
    uint64_t n_bases;
} ac_windows;

/* One approximate-count job = one errorCount call (approx_counter.cpp:922). */
typedef struct ac_segment {
    const uint64_t* kmers; /* dna2int layout (approx_counter.cpp:55-62)     */
    uint32_t n_kmers;
    ac_windows sample;
    uint32_t* counts;      /* n_kmers counters, input order                 */
} ac_segment;

/* Opens a context on HIP device `device` (-1: the current device).  Replaces
 * the index construction + omp_set_num_threads of errorCount (537-547). */
ac_status ac_create(ac_ctx** out, int device);
void ac_destroy(ac_ctx* ctx);
/*
 * A context over `n_gpus` devices of this node (device g mod the visible
 * devices for shard g; SURVEY.md §8(b) "ac_create(ac_ctx**, int n_gpus)").
 * ac_error_count and ac_count on it split the windows into n_gpus contiguous
 * shards balanced by bases, count each shard on its device concurrently and
 * sum the counts on the host (errorCount's OpenMP loop, 547-599, spread over
 * GPUs; integer sums, so bit-identical to one device).  The device-buffer
 * entry points use the first device only.  n_gpus = 1 is ac_create(out, 0).
 */
ac_status ac_create_multi(ac_ctx** out, int n_gpus);

/*
 * SURVEY.md §8(b)'s count entry point, argument for argument: errorCount
 * (531-601) over windows given as a 2-bit image (win_bits, 16 bases per
 * little-endian u32, A0 C1 G2 T3) and an N bitmap (win_nmask, 32 bases per
 * u32); window i starts at 2-bit word win_word_offset[i] (an even word: 32-base
 * aligned, so the same offset indexes the bitmap) and holds win_len[i] bases.
 * counts_out[i] = M1 count of kmers[i].  Synchronous, host buffers.
 */
ac_status ac_count(ac_ctx* ctx, uint32_t k, const uint64_t* kmers, uint32_t n_kmers, const uint32_t* win_bits,
                   const uint32_t* win_nmask, const uint64_t* win_word_offset, const uint16_t* win_len,
                   uint32_t n_windows, uint64_t* counts_out);

/* Number of HIP devices visible to this process (0 without a GPU).  The
 * reference has no counterpart: its errorCount runs on the host's OpenMP
 * threads (approx_counter.cpp:547); the CLI uses this to map -g shards onto
 * devices. */
int ac_device_count(void);
/* Last failure text for ctx (or for the calling thread when ctx is NULL). */
const char* ac_last_error(const ac_ctx* ctx);
int ac_abi_version(void);

/*
 * errorCount (approx_counter.cpp:531-601), host buffers in and out:
 * counts[i] = M1 count of kmers[i] over `sample`.  Copies the inputs to the
 * device, runs the HIP kernel, copies the counts back; synchronous.
 * Replaces: index build (537-541), the omp parallel search loop (550-599),
 * the per-level bitfields and their sum (553, 580-593) and results[kmer]=total
 * (595-596).  Duplicate k-mers are allowed and counted independently.
 */
ac_status ac_error_count(ac_ctx* ctx, uint32_t k, const uint64_t* kmers, uint32_t n_kmers,
                         const ac_windows* sample, uint64_t* counts);

/*
 * Device-resident form (same semantics), asynchronous on `hip_stream`
 * (a hipStream_t; NULL = the default stream).  All segments share k and run
 * in ONE kernel launch (both read ends of one run, 858-953), uint32 counters.
 * The launch itself stores each segment's counts (no memset dispatch): the
 * last workgroup of every candidate group writes the group's sums.  Segments
 * whose count vectors overlap (window shards of one candidate set) are zeroed
 * on the stream first and summed.  The context's scratch (work queues, group
 * sums) is stream-ordered: do not run two launches of one context on
 * different streams at the same time.
 *   window_len  NULL: every window's start / length is read from the segment's sample.  Otherwise
 *               one length per segment for samples whose windows all have it -- the reference's
 *               own sample: every start window holds sl bases and every end window sl + 1
 *               (sampleSequences, approx_counter.cpp:415-476): segment i's window w starts at base
 *               w * ceil32(window_len[i]), n_windows * ceil32(window_len[i]) <= n_bases, and
 *               sample.start / .length are not read (may be NULL) -- the kernel computes each
 *               window's place instead of loading its descriptor, as the host-buffer stage does.
 *   flags       AC_DEVICE_ACCUMULATE: add into `counts` without zeroing them first (window shards
 *               combined on one device); 0: store them.
 * (ABI 8 folded ac_error_count_device_accumulate and ac_error_count_device_equal into this call.)
 */
#define AC_DEVICE_ACCUMULATE 1u
ac_status ac_error_count_device(ac_ctx* ctx, uint32_t k, const ac_segment* segments, uint32_t n_segments,
                                const uint32_t* window_len, uint32_t flags, void* hip_stream);

/*
 * Device copy of a packed sample, owned by the context (valid until the next
 * ac_sample_upload on ctx or ac_destroy).  Lets one upload serve both the
 * exact count and the approximate count of one read end.  The closest
 * reference step is the index build over the sample (approx_counter.cpp:537-541).
 * `dev` receives the device pointers.
 */
ac_status ac_sample_upload(ac_ctx* ctx, const ac_windows* host, ac_windows* dev);

/*
 * count_kmers (approx_counter.cpp:487-519) + get_most_frequent (396-405) or,
 * with solid > 0, get_solid_kmers (372-388), on the GPU over a device sample:
 * exact counts of the k-mers of every window that hold no N, pass the
 * low-complexity filter (float DUST score >= lc_threshold is dropped,
 * 214-234; lc_threshold already adjusted for k, 183-186) and are not in
 * `forbidden` (host array, any order, 330-332).  Writes the kept k-mers in
 * CompareCount order (275-305): the first `limit` of them, or all with count >=
 * solid when solid > 0 (the reference does not truncate solid k-mers).
 * *n_out = number written; if more than `capacity` are due, nothing is written,
 * *n_out = the number needed and AC_ERR_INVALID is returned.  *n_distinct =
 * distinct kept k-mers (the reference's count.size(), 883), *had_n = k-mer
 * positions skipped for holding an N (513-517).  Synchronous.
 */
ac_status ac_exact_count_device(ac_ctx* ctx, uint32_t k, const ac_windows* dev, float lc_threshold,
                                const uint64_t* forbidden, uint32_t n_forbidden, uint64_t limit, uint64_t solid,
                                uint64_t* kmers_out, uint64_t* counts_out, uint64_t capacity, uint64_t* n_out,
                                uint64_t* n_distinct, uint64_t* had_n);

/* Which counting path the last exact count of ctx took (for measurement and
 * tests): 1 = partitioned (dense keys, bucket partition, per-bucket LDS count;
 * every k, samples up to 2^27 k-mer positions), 0 = the global hash table
 * (larger samples, a bucket that outgrew its LDS table, or AC_EXACT_HASH=1),
 * -1 = none yet. */
int ac_exact_path(const ac_ctx* ctx);

/* Same with a host sample (uploads it with ac_sample_upload first). */
ac_status ac_exact_count(ac_ctx* ctx, uint32_t k, const ac_windows* host, float lc_threshold,
                         const uint64_t* forbidden, uint32_t n_forbidden, uint64_t limit, uint64_t solid,
                         uint64_t* kmers_out, uint64_t* counts_out, uint64_t capacity, uint64_t* n_out,
                         uint64_t* n_distinct, uint64_t* had_n);

/*
 * ac_sample_upload into upload slot `slot` (0 .. AC_MAX_JOBS-1; slot 0 is
 * ac_sample_upload's), so both read ends of a run stay on the device at once:
 * each is uploaded once and serves its exact count and the fused approximate
 * count below.  Valid until the next upload into the same slot.
 */
ac_status ac_sample_upload_slot(ac_ctx* ctx, int slot, const ac_windows* host, ac_windows* dev);

/* One errorCount call (approx_counter.cpp:922) over a packed sample: host
 * k-mers, host uint64 counts; `sample` is a device sample (ac_error_count_samples)
 * or a host image (ac_error_count_images). */
typedef struct ac_sample_job {
    const uint64_t* kmers;
    uint32_t n_kmers;
    ac_windows sample;
    uint64_t* counts;
} ac_sample_job;

/*
 * errorCount for up to AC_MAX_JOBS calls sharing k -- both read ends of one run
 * (the loop at approx_counter.cpp:858-953) -- in ONE fused kernel launch over
 * samples already on the device (ac_sample_upload_slot): the CLI's path, where
 * each end's upload first serves its exact count.  Synchronous.
 */
ac_status ac_error_count_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs);

/*
 * The same over host images: on one device one fused launch; on an
 * ac_create_multi context every job's windows are cut into one contiguous shard
 * per device (balanced by bases), each device counts its shards of all jobs in
 * one fused launch, and the shard counts are summed (the CLI's -g N).
 */
ac_status ac_error_count_images(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs);

/*
 * Host packing of Dna5 windows into a window image (no reference counterpart:
 * SeqAn keeps 1 byte per base; this is the boundary's wire format).
 *   dna5     : window bytes, ordValues 0..3 for ACGT, >= 4 for N
 *   seq_start/seq_len: window i = dna5[seq_start[i] .. +seq_len[i])
 * ac_image_bases() returns the image size (bases) needed for these lengths.
 * The caller allocates codes (n_bases/16 words), nmask (n_bases/32 words),
 * start (n windows) and length (n windows).
 */
uint64_t ac_image_bases(const uint32_t* seq_len, uint32_t n);
ac_status ac_pack_windows(const uint8_t* dna5, const uint64_t* seq_start, const uint32_t* seq_len,
                          uint32_t n, uint32_t* codes, uint32_t* nmask, uint64_t* start,
                          uint32_t* length, uint64_t n_bases);

/*
 * The sample exactly as errorCount receives it: a StringSet<Dna5String>
 * (approx_counter.cpp:38, filled by sampleSequences 415-476), one byte per
 * base.  Window i is bases[offset[i] .. offset[i] + length[i]); bases are
 * Dna5 ordinals (0..3 = A C G T, anything else = N; SeqAn's ordValue).
 * Windows may overlap or come in any order.  Precondition (the struct carries
 * no size for `bases`, so the library cannot check it): every
 * offset[i] + length[i] lies within the caller's `bases` buffer.
 */
typedef struct ac_dna5_windows {
    const uint8_t* bases;
    const uint64_t* offset;
    const uint32_t* length;
    uint32_t n_windows;
} ac_dna5_windows;

/*
 * Pinned host memory for the sample (ABI 7; no reference counterpart: the reference's
 * sampleSequences, approx_counter.cpp:415-476, fills an ordinary StringSet<Dna5String>).
 * A job of ac_error_count_jobs / _submit whose windows all have one length of 1..256 bases (a read
 * end: sl or sl + 1) and whose `bases` and `offset` arrays lie inside blocks of ac_host_alloc is
 * packed on the device when the call is large (>= 2^16 windows; AC_DEVICE_PACK_MIN_WINDOWS): the
 * count kernel's copier workgroups read its Dna5 bytes over PCIe and pack them into HBM themselves,
 * so the host does no per-window work for it beyond scanning the lengths (ac_stage_mode then reports
 * 3).  Smaller calls are packed by the host pool, which is faster there, a 1-participant pool
 * included (AC_DEVICE_PACK=1 / 0: always / never).  The bytes readable from `bases` are those up to
 * the end of its block; a window reaching past them is an error (AC_ERR_INVALID, its counts short).
 * Blocks are process-wide (any context, any device).  A submit's device-packed jobs are read by
 * the device until its stream work completes: do not change or free them before that.
 *   ac_host_alloc  a pinned, device-mapped block of `bytes` (AC_ERR_DEVICE without a HIP device)
 *   ac_host_free   releases a block of ac_host_alloc (NULL: no-op; another pointer: AC_ERR_INVALID)
 */
ac_status ac_host_alloc(size_t bytes, void** out);
ac_status ac_host_free(void* p);

/* One errorCount call (approx_counter.cpp:922) over a Dna5 sample. */
typedef struct ac_job {
    const uint64_t* kmers; /* dna2int layout (approx_counter.cpp:55-62)         */
    uint32_t n_kmers;
    ac_dna5_windows sample;
    uint64_t* counts;      /* host, n_kmers; ignored by ac_error_count_jobs_submit */
} ac_job;

/*
 * errorCount (approx_counter.cpp:531-601) for up to AC_MAX_JOBS calls that
 * share k -- both read ends of one run (the loop at 858-953) -- in one
 * synchronous call, host buffers in and out: jobs[j].counts[i] = M1 count of
 * jobs[j].kmers[i] over jobs[j].sample.  The whole stage runs here: the Dna5
 * windows are packed to 2-bit codes + N bitmap by the host worker pool
 * straight into a pinned staging block, moved into device memory job by job
 * (ac_stage_mode: by the count kernel itself -- launched first -- or by a copy
 * ahead of it), counted by ONE fused kernel launch over all jobs (every size
 * since ABI 4; with AC_STAGE_EARLY=0, calls of >= 2^17 windows are cut into 2-4
 * parts, each launched once it is sent), and the kernel writes the counts into
 * the pinned block.  An early launch that times out waiting for the host (0.5 s
 * without progress) is run again through the DMA path.  On an
 * ac_create_multi context every job's windows are split into contiguous shards
 * balanced by bases, one per device, and the shard counts are summed.
 * Replaces the index build (537-541), the OpenMP search loop (547-599) and
 * results[kmer] = total (595-596) of each call.
 */
#define AC_MAX_JOBS 4
ac_status ac_error_count_jobs(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs);

/*
 * (ABI 7 removed ac_idle -- a no-op since ABI 6 removed the armed launches it cancelled -- and
 * ac_error_count_sample, which ac_error_count_samples with one job replaces.)
 */

/*
 * The same stage without the way back, for callers that combine shards with
 * a device collective (one process per GPU, RCCL all-reduce of the count
 * vector): packs and sends the jobs and launches the count
 * kernel on `hip_stream`, which writes uint32 counts to DEVICE memory
 * d_counts (jobs concatenated in order, sum of n_kmers entries).  Returns once
 * the host inputs have been consumed (packed into the context's staging
 * block); the device work is asynchronous on `hip_stream`.  Consecutive
 * submits on one context must use the same stream.  Single-device contexts.
 */
ac_status ac_error_count_jobs_submit(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs,
                                     uint32_t* d_counts, void* hip_stream);

/*
 * Device-side error check.  The count kernels never read outside a window's
 * image: a window that is misaligned or reaches past n_bases is skipped, and
 * the kernel records that in a context-owned device word instead of failing
 * silently.  The host-buffer entry points check the word themselves (they
 * synchronise); after the asynchronous *_device entry points call ac_check:
 * it waits for `hip_stream`, reads and clears the word, and returns
 * AC_ERR_INVALID ("malformed window skipped") or AC_ERR_INTERNAL (kernel
 * set-up fault) if a launch since the last check hit one, AC_OK otherwise.
 */
ac_status ac_check(ac_ctx* ctx, void* hip_stream);

/*
 * Multi-process data parallelism (one process per GPU): window
 * shards are counted independently (ac_error_count_jobs_submit leaves each
 * shard's counts in device memory) and the count vectors are summed by one RCCL
 * all-reduce over xGMI, owned by the context.  There is no reference
 * counterpart (errorCount runs on one host's OpenMP threads, approx_counter.cpp:547).
 *   ac_comm_id_bytes    size of the RCCL unique id (128)
 *   ac_comm_unique_id   a fresh id (rank 0); the caller sends it to every rank
 *   ac_comm_init        join the n_ranks-rank communicator as `rank`
 *                       (single-device contexts; ranks on distinct devices)
 *   ac_allreduce_counts in-place uint32 sum of d_counts[0, n) over the ranks,
 *                       asynchronous on hip_stream
 * RCCL (librccl.so) is loaded at the first of these calls, not at library load.
 */
int ac_comm_id_bytes(void);
ac_status ac_comm_unique_id(ac_ctx* ctx, void* id_out);
ac_status ac_comm_init(ac_ctx* ctx, int n_ranks, int rank, const void* id);
ac_status ac_allreduce_counts(ac_ctx* ctx, uint32_t* d_counts, uint64_t n, void* hip_stream);

/*
 * The host worker pool that packs the Dna5 sample (ac_error_count_jobs*).  The
 * reference sizes its one OpenMP team with omp_set_num_threads(nb_thread)
 * (approx_counter.cpp:547); here the pool is process-wide and planned once, at
 * the first ac_create: the CPUs local to the GPU's PCIe root, split among the
 * local ranks (LOCAL_RANK / LOCAL_WORLD_SIZE, local rank r on device r mod the
 * visible devices) whose GPUs share them -- disjoint runs of physical cores per
 * rank -- with at most min(16, this rank's share of the cgroup CPU quota less
 * 2 CPUs of headroom, 1 for a share of 4 or less) participants (the calling
 * thread included): a pool spinning on the whole quota was throttled by the CFS.
 *   ac_set_host_cpus   the pool's CPUs and participants (0 = min(16, n_cpus))
 *                      instead; only before the first ac_create
 *                      (AC_ERR_INVALID afterwards)
 *   ac_host_pool_cpus  the plan in force: *participants, the CPUs (up to cap
 *                      written into cpus); returns the number of CPUs
 *   ac_plan_host_cpus  the rule itself, for callers that place threads on their
 *                      own: the CPUs of local rank `rank` given every local
 *                      rank's GPU cpulist ("0-63,128-191") and the CPUs the
 *                      process may use; core_of[c] = physical core of CPU c
 *                      (NULL: every CPU its own core).  Returns the count (up
 *                      to cap written), -1 on bad arguments.
 */
ac_status ac_set_host_cpus(const int* cpus, int n_cpus, int participants);
int ac_host_pool_cpus(int* participants, int* cpus, int cap);
int ac_plan_host_cpus(const char* const* rank_cpulists, int n_ranks, int rank, const char* allowed_cpulist,
                      const int* core_of, int n_core_of, int* out, int cap);

/*
 * How the last ac_error_count_jobs / _submit call on ctx moved its packed
 * inputs (no reference counterpart).  ABI note: the values changed in ABI 3 --
 * 1 (zero-copy, round 2) is no longer returned -- and in ABI 4 large calls moved
 * from 0 to 2; callers should compare against 2 / 0 only.
 * 3 = the early launch with at least one job packed on the device (ac_host_alloc samples, ABI 7).
 * 2 = the early launch, for every single-device call
 * (default; AC_STAGE_EARLY=0 turns it off): the count kernel is
 * launched before the host packs, the host flags each job in a pinned header as
 * soon as it is packed, the kernel copies the flagged job into device memory
 * itself and counts it while later jobs are still being packed, and each
 * candidate group's last workgroup stores its counts and error bits, tagged with
 * the call's generation, into pinned memory, which the host polls.  A few copier
 * workgroups of the kernel do the copying (every early-launch call) while the
 * others count.  0 = the DMA path (AC_STAGE_EARLY=0: calls
 * of >= 2^17 windows cut into 2-4 parts, each packed and copied by the copy
 * engine while the previous part counts; a multi-device context; a staging
 * region of 2^31 bytes or more; the retry of a timed-out early launch).  Either
 * way a job is sent without its N bitmap when no window needs it (no N, or, for
 * equal windows, every N inside the window's inline record) and without window
 * descriptors when its windows have one length.  -1 = no
 * call yet.  ac_error_count_jobs_submit takes the early launch too (its counts
 * and errors go to device memory; ac_check reports the errors).
 */
int ac_stage_mode(const ac_ctx* ctx);

/*
 * Launch geometry actually used for the last device launch of ctx (for
 * measurement): waves launched, windows per wave, candidate groups.
 */
ac_status ac_last_launch(const ac_ctx* ctx, uint64_t* waves, uint32_t* windows_per_wave,
                         uint32_t* groups);

/*
 * The edit budget of the approximate count (an additive export of ABI 8).  The
 * reference has no counterpart: it hard-codes find<0,2> (approx_counter.cpp:586),
 * the budget of 2 that stays the default of every context.  With budget E in 0..3
 * the counting contract is M1(E):
 *     count = sum over windows w of max(0, E + 1 - d(kmer, w))
 * with the same d (semi-global Levenshtein distance, a non-ACGT base matching
 * nothing); E = 2 is M1 above.  Counts stay <= 4 x windows.
 *
 * The budget is a property of the context: sticky, applied to every
 * approximate-count entry point (ac_error_count*, ac_count) from the next call
 * on, on every shard of an ac_create_multi context; the exact count
 * (ac_exact_count*) does not depend on it.  Setting it between a submit
 * (ac_error_count_jobs_submit, ac_error_count_device) and the completion of that
 * call's stream work is the caller's error, like using two streams at once.
 *
 * Where E != 2 runs: only on launches the bit-sliced count kernel takes -- k is 16
 * or 18..32, every job (segment) that has candidates and windows holds equal
 * windows of 1..256 bases, and AC_BITSLICE is not 0 in the environment.  That is
 * every launch of the jobs stage (ac_error_count_jobs / _submit) over equal read
 * ends at those k, ac_error_count_device with window_len, and
 * ac_error_count_samples over images this context uploaded.  Any other call made
 * with E != 2 -- ragged windows, a call mixing ragged and equal jobs, windows over
 * 256 bases, k <= 15, k = 17, packed images with window descriptors
 * (ac_error_count, ac_error_count_images, ac_count), AC_BITSLICE=0 -- returns
 * AC_ERR_INVALID before anything is launched; ac_last_error names the constraint.
 * Nothing falls back: no count is ever produced under another budget than the
 * one set.
 *
 * ac_set_max_errors: e > 3 or a NULL ctx returns AC_ERR_INVALID (the budget is
 * unchanged).  ac_max_errors: the context's budget (2 for a NULL ctx).
 */
ac_status ac_set_max_errors(ac_ctx* ctx, uint32_t e);
uint32_t ac_max_errors(const ac_ctx* ctx);

/*
 * Hit levels: which windows (reads) hold a k-mer within 0..E edits (additive
 * exports of ABI 8).  The reference fills one bitfield per error level and read,
 * tcount[errors][read] (approx_counter.cpp:553-565), and collapses them at once
 * with vectorSum into the one count per k-mer (580-596); these calls hand out
 * the bitfields themselves, as one dense bit matrix per level, beside the same
 * counts.  With E = the context's edit budget (ac_set_max_errors), a segment of
 * n_kmers candidates and n_windows windows has
 *     words = ceil(n_kmers / 32)            u32 per window and level
 *     hits[(e * n_windows + w) * words + c / 32], bit c % 32
 *         set iff d(kmer c, window w) <= e,   e = 0..E
 * (the levels nest: a bit set at level e is set at every level above it); bits
 * of candidates >= n_kmers are 0, and a window the kernel skipped (reported by
 * ac_check) holds zeros.  Every word of the matrix is written by the launch: the
 * buffer needs no clearing.  count[c] = the number of set bits of candidate c
 * over all levels and windows.
 *   ac_window_hits_words   u32 words of one segment's matrix:
 *                          (max_errors + 1) * n_windows * ceil(n_kmers / 32)
 *   ac_window_hits_device  ac_error_count_device with window_len required, plus
 *                          one device matrix per segment (hits[i], of
 *                          ac_window_hits_words u32 at the context's budget);
 *                          asynchronous on hip_stream, the counts stored to
 *                          segments[i].counts by the same launch.  No flags:
 *                          accumulate mode and count vectors that overlap are
 *                          refused.
 *   ac_window_hits_samples ac_error_count_samples (samples uploaded with
 *                          ac_sample_upload_slot: the CLI's route) that also
 *                          fills one host matrix per job (hits_host[j]);
 *                          synchronous.
 *   ac_hit_level_counts_device
 *                          level_counts[e * n_kmers + c] = the windows of level
 *                          plane e (e < levels, 1..4) that hold candidate c: a
 *                          column popcount of a device matrix, asynchronous on
 *                          hip_stream (level_counts, device memory, is zeroed
 *                          first).  Their sum over e is the count of c.
 * Where they run: only on launches the bit-sliced count kernel takes (k = 16 or
 * 18..32, every segment with candidates and windows holding equal windows of
 * 1..256 bases, AC_BITSLICE not 0), on single-device contexts, at any budget
 * 0..3.  Everything else -- ragged windows (window_len NULL, or a sample this
 * context did not upload as equal windows), a launch mixing ragged and equal
 * jobs, windows over 256 bases, k <= 15, k = 17, AC_BITSLICE=0, an
 * ac_create_multi context, a NULL matrix for a segment that has work -- returns
 * AC_ERR_INVALID before anything is enqueued; ac_last_error names the
 * constraint.  Nothing falls back, and the context stays usable.  The jobs stage
 * hands them out through calls of its own (ac_window_hits_jobs, below).
 */
uint64_t ac_window_hits_words(uint32_t n_kmers, uint32_t n_windows, uint32_t max_errors);
ac_status ac_window_hits_device(ac_ctx* ctx, uint32_t k, const ac_segment* segments, uint32_t n_segments,
                                const uint32_t* window_len, uint32_t* const* hits, void* hip_stream);
ac_status ac_window_hits_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs,
                                 uint32_t* const* hits_host);
ac_status ac_hit_level_counts_device(ac_ctx* ctx, const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows,
                                     uint32_t levels, uint32_t* level_counts, void* hip_stream);

/*
 * Match end positions: where in its window each k-mer's best occurrence ends
 * (additive exports of ABI 8).  The reference's search delegate is handed every
 * occurrence (approx_counter.cpp:553-565) and keeps the read and the error
 * level only; these calls also keep the end.  For a window w of L bases let e(j),
 * j = 0..L, be the least edit distance of the whole k-mer c against a substring
 * of w that ends at base j (exclusive; an N matches nothing), d = min over j.
 * Where d <= E (the context's budget),
 *     pos(c, w) = min { j : e(j) = d }              1 <= pos <= L
 * the exclusive end offset of the leftmost occurrence at the best distance.  A
 * segment's position matrix is eight bit planes of the hit matrix's shape:
 *     words = ceil(n_kmers / 32)
 *     pos[(b * n_windows + w) * words + c / 32], bit c % 32
 *         = bit b of pos(c, w) - 1,   b = 0..7
 * 0 in every plane where d > E, for candidates >= n_kmers and in windows the
 * kernel skipped.  Every word is written by the launch: no clearing needed.
 *   ac_window_positions_words    u32 words of one segment's position matrix:
 *                                8 * n_windows * ceil(n_kmers / 32)
 *   ac_window_positions_device   ac_window_hits_device plus one position matrix
 *                                per segment (pos[i]): counts, hit levels and
 *                                positions from one launch.
 *   ac_window_positions_samples  ac_window_hits_samples plus one host position
 *                                matrix per job (pos_host[j]); synchronous.
 *   ac_hit_position_profile_device
 *                                profile[(d * n_kmers + c) * window_len + p - 1]
 *                                = the windows that hold candidate c at distance
 *                                exactly d (d < levels, 1..4) with pos = p
 *                                (1..window_len, 1..256), from a device hit
 *                                matrix and its position matrix; asynchronous on
 *                                hip_stream (profile, device memory, is zeroed
 *                                first).  A position past window_len is dropped.
 * Where they run, and what is refused: exactly as the hit levels above, plus a
 * NULL position matrix for a segment that has work (AC_ERR_INVALID before
 * anything is enqueued).
 */
uint64_t ac_window_positions_words(uint32_t n_kmers, uint32_t n_windows);
ac_status ac_window_positions_device(ac_ctx* ctx, uint32_t k, const ac_segment* segments, uint32_t n_segments,
                                     const uint32_t* window_len, uint32_t* const* hits, uint32_t* const* pos,
                                     void* hip_stream);
ac_status ac_window_positions_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs,
                                      uint32_t* const* hits_host, uint32_t* const* pos_host);
ac_status ac_hit_position_profile_device(ac_ctx* ctx, const uint32_t* hits, const uint32_t* pos, uint32_t n_kmers,
                                         uint32_t n_windows, uint32_t levels, uint32_t window_len, uint32_t* profile,
                                         void* hip_stream);

/*
 * Match spans: where in its window each k-mer's best occurrence STARTS
 * (additive exports of ABI 8).  The end positions above give one edge of an
 * occurrence; for an end window, whose adapter runs from some base to the
 * read's last one, the informative edge is the other.  With w a window of L
 * bases, c a k-mer, E the budget, d = d(c, w) <= E, pos = pos(c, w) as above
 * (the exclusive end of the leftmost occurrence at distance d), ed the plain
 * global edit distance and an N of the window matching nothing,
 *     start(c, w) = max { s : ed(c, w[s, pos)) = d }    0 <= start <= pos - (k - d)
 *     len(c, w)   = pos - start                         k - d <= len <= k + d
 * the SHORTEST substring ending at pos at the best distance.  The end rule
 * already prefers the shorter occurrence at the right edge (ACGT in ..ACGA..
 * ends after ACG); the left edge does the same: a first base substituted in
 * the text is left out of the span, not covered as a mismatch.  Such an s
 * always exists, because e(pos) = d means exactly that.
 * A start matrix has exactly the layout of a position matrix: eight bit planes
 * of the hit matrix's shape,
 *     start_m[(b * n_windows + w) * words + c / 32], bit c % 32
 *         = bit b of start(c, w)            (the value as it is, 0..255)
 * 0 in every plane where d > E, for candidates >= n_kmers and in skipped
 * windows.  Every word is written by the pass: the caller clears nothing.  Its
 * size is ac_window_positions_words, and ac_hit_position_profile_device works
 * on it unchanged: its index p - 1 is then the start offset.
 *   ac_hit_start_positions_device
 *       the pass alone: from the device k-mers, the device sample (equal
 *       windows of window_len bases at ceil32(window_len)-base strides: codes
 *       and nmask are read, bases below window_len only; start / length are
 *       not), a device hit matrix of `levels` planes and its position matrix,
 *       into start_out (device memory).  Asynchronous on hip_stream.  Its work
 *       follows the hit pairs, not all pairs: a bit-vector alignment of the
 *       reversed k-mer against the reversed text before pos, at most
 *       k + levels - 1 steps a hit.  Runs on any context, whichever kernel wrote
 *       the matrices and whatever AC_BITSLICE is; an ac_create_multi context
 *       uses its first device.  Input planes may hold anything: a pair whose
 *       planes are inconsistent (a stored position past window_len, no
 *       substring ending there at the plane's distance, a level bit without the
 *       top level's) gets 0 bits, and nothing outside the windows is read.
 *       AC_ERR_INVALID before anything is enqueued, the constraint in
 *       ac_last_error, for: a NULL ctx; k outside 2..32; levels outside 1..4 or
 *       levels >= k (an occurrence could then be empty); window_len outside
 *       1..256; n_windows x ceil32(window_len) past n_bases; a NULL sample; a
 *       NULL hits, pos, codes, nmask, kmers or output when there is work.  The
 *       context stays usable.  n_kmers = 0 or n_windows = 0 is no work.
 *   ac_window_spans_samples
 *       ac_window_positions_samples followed, per job with work, by the pass on
 *       the context's stream over the resident sample and the context's device
 *       matrices, then copied out (start_host[j], ac_window_positions_words u32).
 *       Synchronous.  Refuses exactly what ac_window_positions_samples refuses,
 *       plus a NULL start matrix for a job with work.
 * Not built: spans from the jobs stage (ac_window_*_jobs*), whose image keeps N
 * in inline records, and from word-parallel launches, which write no hit matrix.
 */
ac_status ac_hit_start_positions_device(ac_ctx* ctx, uint32_t k, const uint64_t* kmers, uint32_t n_kmers,
                                        const ac_windows* sample, uint32_t window_len, const uint32_t* hits,
                                        const uint32_t* pos, uint32_t levels, uint32_t* start_out, void* hip_stream);
ac_status ac_window_spans_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs,
                                  uint32_t* const* hits_host, uint32_t* const* pos_host, uint32_t* const* start_host);

/*
 * Flank profiles: the bases after and before each k-mer's best occurrence
 * (additive exports of ABI 8).  Everything above reduces the hit matrix per
 * k-mer or per pair of k-mers; none of it reads the window's text around an
 * occurrence.  For a k-mer inside an adapter the bases after its occurrence are
 * the adapter's next bases in almost every read, for the adapter's last k-mer
 * they are insert: a per-k-mer histogram of the D bases after the end and the D
 * bases before the start extends every k-mer by majority vote and shows where
 * the adapter ends.  With w a window of L bases (equal windows, L in 1..256, at
 * ceil32(L)-base strides), c a k-mer, H a hit plane (n_windows x
 * ceil(n_kmers / 32) words: one level plane of a hit matrix), pos(c, w) the
 * exclusive end from the position matrix, start(c, w) the inclusive start from
 * the start matrix, the symbols A, C, G, T = 0..3 and N = 4 (any base whose N
 * bit is set) and the depth D in 1..32,
 *     right[c][j][s] = #{ w : H(w, c), q = pos(c, w) + j       <  L, sym(w[q]) = s }
 *     left [c][j][s] = #{ w : H(w, c), q = start(c, w) - 1 - j >= 0, sym(w[q]) = s }
 * for j = 0..D-1, stored as u32
 *     flank[((side * n_kmers + c) * D + j) * 5 + s]     side 0 = right, 1 = left
 * ac_hit_flank_words(n_kmers, depth) = 2 n_kmers D 5 words in all.  A base
 * outside [0, L) is not counted, so the sum over s of right[c][j] is the number
 * of hit windows whose occurrence ends at or before L - j - 1; slot padding is
 * never read as text.  Every word is defined when the stream work is done: the
 * caller clears nothing.  Bits of candidates >= n_kmers are ignored.  The
 * planes may hold anything: a pair whose stored position is past L or whose
 * start is not below its end contributes to neither side, and nothing outside
 * the windows is read.  Passing a lower plane e < E of a hit matrix selects the
 * pairs within e edits; their positions are the ones the matrices hold.
 *   ac_hit_flank_profile_device
 *       the pass alone: from the device sample (codes and nmask are read, bases
 *       below window_len only; start / length are not), one device level plane,
 *       the position matrix and the start matrix, into flank_out (device
 *       memory).  Asynchronous on hip_stream.  `start` may be NULL: the left
 *       half of the result is then zeros.  Its work follows the hit pairs; the
 *       observations of a tile of 32 k-mers over a strip of windows are summed
 *       in on-chip memory and added to the output once.  Runs on any context,
 *       whatever AC_BITSLICE, k and the budget are; an ac_create_multi context
 *       uses its first device.  AC_ERR_INVALID before anything is enqueued, the
 *       constraint in ac_last_error, for: a NULL ctx; depth outside 1..32;
 *       window_len outside 1..256; n_windows x ceil32(window_len) past n_bases;
 *       a NULL sample, codes or nmask; a NULL plane, pos or output when there
 *       is work.  The context stays usable.  n_kmers = 0 is no work;
 *       n_windows = 0 writes zeros.
 *   ac_window_flanks_samples
 *       ac_window_spans_samples followed, per job with work, by the pass on the
 *       context's stream over the resident sample and the context's device
 *       matrices at the top level E, then copied out (flank_host[j],
 *       ac_hit_flank_words u32).  Synchronous.  Refuses exactly what
 *       ac_window_spans_samples refuses, plus a depth outside 1..32 and a NULL
 *       flank buffer for a job with work.
 * Not built: flanks from the jobs stage and from word-parallel launches (as for
 * the spans), per-distance flank planes, and flanks of another occurrence than
 * the one the matrices hold.
 */
uint64_t ac_hit_flank_words(uint32_t n_kmers, uint32_t depth);
ac_status ac_hit_flank_profile_device(ac_ctx* ctx, const ac_windows* sample, uint32_t window_len,
                                      const uint32_t* hit_plane, const uint32_t* pos, const uint32_t* start,
                                      uint32_t n_kmers, uint32_t depth, uint32_t* flank_out, void* hip_stream);
ac_status ac_window_flanks_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs, uint32_t depth,
                                   uint32_t* const* hits_host, uint32_t* const* pos_host,
                                   uint32_t* const* start_host, uint32_t* const* flank_host);

/*
 * Edit profiles: how each k-mer's best occurrence differs from it, base by base
 * (additive exports of ABI 8).  The calls above say whether, where and beside
 * what a k-mer occurs; none looks inside the occurrence.  A true adapter k-mer
 * collects edits spread thinly over its bases; an erroneous variant of one
 * collects the same edit at the same base in most of its windows, and the
 * profile gives its corrected string (with the flanks: prefix, corrected k-mer,
 * extension).  With w a window of L bases (equal windows, L in 1..256, at
 * ceil32(L)-base strides), c a k-mer of k bases (k in 2..32), H a hit plane
 * (n_windows x ceil(n_kmers / 32) words: one level plane of a hit matrix),
 * p = pos(c, w) the exclusive end from the position matrix, s = start(c, w) the
 * inclusive start from the start matrix, t = w[s, p), m = p - s, an N of the
 * window matching nothing, and D[i][j] the plain global edit-distance table of
 * c[0, i) against t[0, j) (D[i][0] = i, D[0][j] = j): a pair counts only if
 * H(w, c), 1 <= p <= L, s < p, |m - k| <= 3 and D[k][m] <= 3 -- 3 is the largest
 * edit budget of this ABI and a constant of the pass, which takes no `levels`.
 * The pair's alignment is the canonical traceback from (k, m) to (0, 0); at
 * cell (i, j) the first rule that applies:
 *   1. diagonal   if i > 0, j > 0 and D[i-1][j-1] + (c[i-1] != t[j-1]) = D[i][j]:
 *                 k-mer base i-1 is matched if the bases are equal, otherwise
 *                 substituted by t[j-1] (A, C, G, T or N); i--, j--
 *   2. deletion   if i > 0 and D[i-1][j] + 1 = D[i][j]: k-mer base i-1 is
 *                 deleted, that is missing from the read; i--
 *   3. insertion  otherwise: t[j-1] is inserted after k-mer base i-1 (at i = 0
 *                 nothing is counted); j--
 * stored as u32
 *     edit[(c * k + i) * 12 + op]      op 0       match
 *                                         1..5    substituted by A C G T N
 *                                         6       deleted
 *                                         7..11   inserted after: A C G T N
 * ac_hit_edit_words(n_kmers, k) = n_kmers k 12 words in all.  The cell
 * "substituted by the k-mer's own base" stays 0.  For matrices that come from
 * a count launch and the span pass no pair is skipped, D[k][m] is the pair's
 * distance, no alignment begins or ends with an insertion, op 0..6 of every
 * base sum to the plane's level count of the k-mer, and op 1..11 of a k-mer sum
 * to the sum of its hit windows' distances.  Every word is defined when the
 * stream work is done: the caller clears nothing.  Bits of candidates >=
 * n_kmers are ignored.  The planes may hold anything: a pair that fails a
 * condition counts nowhere, and nothing outside [0, L) of a window is read.
 * Passing a lower plane e < E of a hit matrix selects the pairs within e edits.
 *   ac_hit_edit_profile_device
 *       the pass alone: from the k-mers (device memory, 2 bits a base, the
 *       first base highest), the device sample (codes and nmask are read, bases
 *       below window_len only), one device level plane, the position matrix and
 *       the start matrix, into edit_out (device memory).  Asynchronous on
 *       hip_stream.  Its work follows the hit pairs: a banded alignment (3
 *       diagonals on either side) with a traceback per pair; the observations
 *       of 32 k-mers over a strip of windows are summed in on-chip memory and
 *       added to the output once.  Runs on any context, whatever AC_BITSLICE
 *       and the budget are; an ac_create_multi context uses its first device.
 *       AC_ERR_INVALID before anything is enqueued, the constraint in
 *       ac_last_error, for: a NULL ctx; k outside 2..32; window_len outside
 *       1..256; n_windows x ceil32(window_len) past n_bases; a NULL sample,
 *       codes or nmask; a NULL kmers, plane, pos, start or output when there is
 *       work.  The context stays usable.  n_kmers = 0 is no work; n_windows = 0
 *       writes zeros.
 *   ac_window_edits_samples
 *       ac_window_spans_samples followed, per job with work, by the flank pass
 *       when flank_depth is 1..32 (0, with flank_host NULL or not: no flank
 *       pass) and by the edit pass on the context's stream over the resident
 *       sample and the context's device matrices at the top level E, then
 *       copied out (edit_host[j], ac_hit_edit_words u32).  Synchronous.
 *       Refuses what ac_window_flanks_samples refuses, except that a depth of 0
 *       is allowed, plus a NULL edit buffer for a job with work.
 * Not built: edit profiles from the jobs stage and from word-parallel launches
 * (as for the spans), per-distance planes (a lower plane can be passed), the
 * alignment of another occurrence than the one the matrices hold, and
 * assembling the corrected k-mers and flanks into adapters.
 */
uint64_t ac_hit_edit_words(uint32_t n_kmers, uint32_t k);
ac_status ac_hit_edit_profile_device(ac_ctx* ctx, uint32_t k, const uint64_t* kmers, uint32_t n_kmers,
                                     const ac_windows* sample, uint32_t window_len, const uint32_t* hit_plane,
                                     const uint32_t* pos, const uint32_t* start, uint32_t* edit_out, void* hip_stream);
ac_status ac_window_edits_samples(ac_ctx* ctx, uint32_t k, const ac_sample_job* jobs, uint32_t n_jobs,
                                  uint32_t flank_depth, uint32_t* const* hits_host, uint32_t* const* pos_host,
                                  uint32_t* const* start_host, uint32_t* const* flank_host,
                                  uint32_t* const* edit_host);

/*
 * Hit levels and end positions from the jobs stage (additive exports of ABI 8):
 * ac_error_count_jobs / _submit -- Dna5 windows in, the whole errorCount stage --
 * that also return the matrices above, from the same one launch: packing still
 * overlaps counting, pinned samples (ac_host_alloc) are still packed by the
 * kernel, and the launch still starts before the host has packed anything.
 *   ac_window_hits_jobs        ac_error_count_jobs that also fills one host hit
 *                              matrix per job (hits_host[j]); synchronous.  The
 *                              launch writes context-owned device matrices, which
 *                              the same stream then copies out: the call returns
 *                              when every matrix is complete.
 *   ac_window_positions_jobs   the same plus one host position matrix per job
 *                              (pos_host[j]).
 *   ac_window_hits_jobs_submit ac_error_count_jobs_submit that also stores into
 *                              one device hit matrix per job (d_hits[j]) the
 *                              caller gives; asynchronous on hip_stream, errors
 *                              through ac_check.
 *   ac_window_positions_jobs_submit
 *                              the same plus one device position matrix per job
 *                              (d_pos[j]).
 * Layouts: exactly ac_window_hits_words / ac_window_positions_words u32 per job,
 * as laid out above, at the context's budget E in 0..3.  Row w of job j's
 * matrices is the job's window w in the caller's order (sample.offset[w] /
 * length[w]): the stage packs window i into slot i.  The counts are stored as
 * by ac_error_count_jobs / _submit and equal the set bits of the hit matrix.
 * A job without k-mers or without windows has no work and may pass a NULL
 * matrix; a NULL matrix for a job that has work is refused (AC_ERR_INVALID
 * before anything is enqueued).
 * Where they run: where the hit levels run -- k = 16 or 18..32, every job with
 * work holding equal windows of 1..256 bases, AC_BITSLICE not 0, a single-device
 * context -- on every route such a call takes: the early launch, device
 * packing, the DMA path in one part or in several (each part writes its own
 * rows of the matrices; every word is still written exactly once, with no
 * clearing and no atomic).  Anything else -- ragged windows, a call mixing
 * ragged and equal jobs, windows over 256 bases, k <= 15, k = 17,
 * AC_BITSLICE=0, an ac_create_multi context -- returns AC_ERR_INVALID before
 * anything is packed or enqueued, with the constraint in ac_last_error.  Nothing
 * falls back, and the context stays usable.
 * On a call that returns AC_OK every word of every matrix has been written.  On
 * a call that returns an error (or whose ac_check does) -- a window reaching
 * past its pinned block, a staging timeout the retry could not cure -- the
 * matrices' contents are unspecified.  ac_stage_mode and ac_last_launch report
 * as for the plain calls.
 */
ac_status ac_window_hits_jobs(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs,
                              uint32_t* const* hits_host);
ac_status ac_window_positions_jobs(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs,
                                   uint32_t* const* hits_host, uint32_t* const* pos_host);
ac_status ac_window_hits_jobs_submit(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs,
                                     uint32_t* d_counts, uint32_t* const* d_hits, void* hip_stream);
ac_status ac_window_positions_jobs_submit(ac_ctx* ctx, uint32_t k, const ac_job* jobs, uint32_t n_jobs,
                                          uint32_t* d_counts, uint32_t* const* d_hits,
                                          uint32_t* const* d_pos, void* hip_stream);

/*
 * Co-occurrence: which k-mers share windows (additive exports of ABI 8).  The
 * reference's per-read bitfields tcount[errors][read] (approx_counter.cpp:553-565)
 * are collapsed by vectorSum into one count per k-mer (580-596); the hit levels
 * above hand them out, and their reductions so far (ac_hit_level_counts_device,
 * ac_hit_position_profile_device) are per k-mer as well.  These calls reduce a
 * hit matrix over pairs of k-mers, and over the k-mers of a window.
 * Input: `hits`, a matrix in exactly the layout of ac_window_hits_words --
 * `levels` (1..4) planes of n_windows rows of words = ceil(n_kmers / 32) u32,
 * bit c % 32 of word c / 32 = candidate c.  Bits of candidates >= n_kmers in a
 * row's last word may hold anything and are ignored.  To reduce one plane e of
 * a larger matrix pass hits + e * n_windows * words with levels = 1.
 *   ac_hit_cooccurrence_words    u32 words of a result: levels * n_kmers * n_kmers
 *                                (64-bit)
 *   ac_hit_cooccurrence_device   cooc[(e * n_kmers + a) * n_kmers + b] = the
 *                                windows whose row of plane e has bit a and bit
 *                                b both set: symmetric, its diagonal the
 *                                level_counts[e * n_kmers + a] of
 *                                ac_hit_level_counts_device; u32 values (<=
 *                                n_windows), every index computed in 64 bits.
 *                                hits and cooc are device memory; asynchronous
 *                                on hip_stream.
 *   ac_hit_cooccurrence          the same over host buffers (the command line's
 *                                route): the matrix is uploaded into context
 *                                scratch, reduced on the context's stream and
 *                                copied back; synchronous.
 *   ac_hit_window_counts_device  window_counts[e * n_windows + w] = the
 *                                candidates c < n_kmers whose bit is set in row
 *                                w of plane e -- the other marginal: how many of
 *                                the k-mers a window holds.  Device memory,
 *                                asynchronous on hip_stream.
 * Every word of a result is defined on return (of the stream work): the caller
 * clears nothing.  n_windows = 0 writes zeros; n_kmers = 0 is no work.
 * A NULL ctx, levels outside 1..4, a NULL output with n_kmers > 0 and
 * a NULL hits with n_kmers and n_windows both > 0 return AC_ERR_INVALID before
 * anything is enqueued, with the constraint in ac_last_error.
 * Where they run: on any context, whichever count kernel wrote the matrix and
 * whatever AC_BITSLICE, k and the edit budget are; an ac_create_multi context
 * uses its first device.  The product reads the planes transposed, from
 * context-owned scratch that is grown on demand (AC_ERR_NOMEM if it cannot be;
 * the context stays usable), freed by ac_destroy and stream-ordered like the
 * count scratch: no two launches of one context on different streams at the
 * same time.
 */
uint64_t ac_hit_cooccurrence_words(uint32_t n_kmers, uint32_t levels);
ac_status ac_hit_cooccurrence_device(ac_ctx* ctx, const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows,
                                     uint32_t levels, uint32_t* cooc, void* hip_stream);
ac_status ac_hit_cooccurrence(ac_ctx* ctx, const uint32_t* hits_host, uint32_t n_kmers, uint32_t n_windows,
                              uint32_t levels, uint32_t* cooc_host);
ac_status ac_hit_window_counts_device(ac_ctx* ctx, const uint32_t* hits, uint32_t n_kmers, uint32_t n_windows,
                                      uint32_t levels, uint32_t* window_counts, void* hip_stream);

/*
 * Cross co-occurrence (additive exports of ABI 8): the same reduction over two
 * hit matrices A (n_a candidates) and B (n_b) that share their windows -- row w
 * of both is the same read, as the paired sample of the command line
 * (--paired-sample) makes a run's start and end windows.  Both are in the layout
 * above over the same n_windows, `levels` planes each.
 *   ac_hit_cross_cooccurrence_words    u32 words of a result: levels * n_a * n_b
 *                                      (64-bit)
 *   ac_hit_cross_cooccurrence_device   cross[(e * n_a + a) * n_b + b] = the
 *                                      windows whose row of A's plane e has bit a
 *                                      and whose row of B's plane e has bit b;
 *                                      u32 values, 64-bit indices, stray bits
 *                                      ignored, every word of the result written.
 *                                      To pair plane d of A with plane d' of B
 *                                      pass the planes' offsets with levels = 1;
 *                                      A and B may be the same matrix.  Device
 *                                      memory; asynchronous on hip_stream.
 *   ac_hit_cross_cooccurrence          the same over host buffers; synchronous.
 * Refused with AC_ERR_INVALID before anything is enqueued: a NULL context,
 * levels outside 1..4, a NULL result when n_a and n_b are both > 0, a NULL
 * hits_a or hits_b when n_a, n_b and n_windows are all > 0.  n_windows = 0
 * writes zeros; n_a = 0 or n_b = 0 is no work.  Any context, k, budget and
 * AC_BITSLICE; an ac_create_multi context uses its first device.  The scratch
 * is the co-occurrence call's (both matrices' planes transposed: grown on demand,
 * AC_ERR_NOMEM if it cannot be, and stream-ordered with that call).
 */
uint64_t ac_hit_cross_cooccurrence_words(uint32_t n_a, uint32_t n_b, uint32_t levels);
ac_status ac_hit_cross_cooccurrence_device(ac_ctx* ctx, const uint32_t* hits_a, uint32_t n_a, const uint32_t* hits_b,
                                           uint32_t n_b, uint32_t n_windows, uint32_t levels, uint32_t* cross,
                                           void* hip_stream);
ac_status ac_hit_cross_cooccurrence(ac_ctx* ctx, const uint32_t* hits_a_host, uint32_t n_a, const uint32_t* hits_b_host,
                                    uint32_t n_b, uint32_t n_windows, uint32_t levels, uint32_t* cross_host);

#ifdef __cplusplus
}
#endif
#endif /* APPROX_COUNTER_AMD_H */
