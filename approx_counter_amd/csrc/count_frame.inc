// count_frame.inc -- the frame the two count kernel bodies share around their NFAs, included once by
// wm_count.hip (inside its anonymous namespace, after stage_dev.inc).  Used by count_body there and
// bs_body in bs_count.inc: the deal of workgroups to block-queues, the zeroing of the other queue
// bank, the claim counters' address, the early-counting gate and the count hand-off.  Used by bs_body
// alone: the staged launch's prologue (copier workgroups, wave 0's wait, the verdict) and the
// sub-queues (claim, steal).  count_body keeps its own text of those two, with its static first items
// and the whole-segment wait of ragged windows: through these helpers its cfg5 kernel ran 0.9 % slower
// and a staged k <= 10 kernel spilled four more VGPRs (profiles/r09_frame_ab.log, r09_frame_codegen.txt).
// Everything is __forceinline__ and takes values: the state structs (SubQueues, Gate) are locals of
// the body, which the compiler splits into registers; the kernels are register-tight.

// Workgroup b serves one block-queue (all its waves on one candidate group); its waves take the
// block-queue's AC_WAVES_PER_BLOCK sub-queues.  Workgroups are dealt round-robin over the
// block-queues, so every sub-queue is served by waves of every dispatch age (see SubQueues).
struct Deal {
    uint32_t nqb, blocks;  // block-queues, workgroups of the launch
    uint32_t rank, bq;     // this workgroup's round of the deal and its block-queue
    // Rank r's workgroups are dealt to the block-queues rotated by shift(r):
    // with a plain b mod nqb deal every workgroup a CU receives belongs to one
    // block-queue, so each candidate group ran on a fixed slice of the chip
    // and inherited its speed (stamps: group median ends 93-101 us, the same
    // order run after run), with no stealing across groups to even it out.
    // Rotated, a CU's workgroups come from all groups and every group runs on
    // every XCD: group median ends 95.1-96.1 us, cfg2 kernel 109.6 -> 103.8 us
    // (profiles/r01_kernel_log.md, round 2).
    __device__ __forceinline__ uint32_t shift(uint32_t r) const { return (r + (r >> 3) * 4u) % nqb; }
    // workgroups dealt to block-queue qb (a complete rank gives each one; the
    // partial last rank the blocks % nqb queues from shift(last) on)
    __device__ __forceinline__ uint32_t wgs_of(uint32_t qb) const {
        return blocks / nqb + ((qb + nqb - shift(blocks / nqb)) % nqb < blocks % nqb ? 1u : 0u);
    }
};
__device__ __forceinline__ Deal deal_of(const LaunchArgs& a) {
    Deal d;
    d.nqb = a.n_queues / WAVES_PER_BLOCK;
    d.blocks = (uint32_t)(a.total_waves / WAVES_PER_BLOCK);
    d.rank = blockIdx.x / d.nqb;
    d.bq = (blockIdx.x % d.nqb + d.shift(d.rank)) % d.nqb;
    return d;
}
// Wave wib's sub-queue q -> (segment, candidate group g, sub-queue j of that group).  A group's
// sub-queues are contiguous (g * subq + j), so a workgroup's sub-queues lie in one group.
struct Place {
    int si;
    uint32_t g, j;
};
__device__ __forceinline__ Place place_of(const LaunchArgs& a, uint32_t bq, uint32_t wib) {
    const uint32_t q = bq * WAVES_PER_BLOCK + wib;
    int si = 0;
#pragma unroll
    for (int i = 1; i < AC_MAX_SEGS; ++i)
        if (i < (int)a.n_segs && q >= a.seg[i].queue_begin) si = i;
    const uint32_t ql = q - a.seg[si].queue_begin;
    return Place{si, ql / a.seg[si].subq, ql % a.seg[si].subq};
}

// The prologue of a staged launch's workgroup whose segment has chunks: the segment's inputs are
// not there yet; the copier workgroups stage every segment's, wave 0 waits for this segment's --
// only for the k-mers (the ~Eq table): windows are equal, counting starts early (Gate) -- the
// workgroup's other waves wait at a barrier, then everyone reads the verdict from LDS (`stage_r`): ~0u skip the segment,
// 2 count early (the segment is not known complete), 0 / 1 complete, without / with N.
__device__ __forceinline__ uint32_t staged_prologue(const LaunchArgs& a, const SegDev& sg, uint32_t* st_words, uint32_t wib,
                                                    uint32_t lane, uint64_t wave, uint32_t* stage_r) {
    if (blockIdx.x < a.copier_wgs)  // copier workgroup: every wave serves every segment's tickets (as in count_body)
        for (uint32_t i2 = 0; i2 < a.n_segs; ++i2) {
            const uint32_t s2 = (blockIdx.x + i2) % a.n_segs;
            const SegDev& c2 = a.seg[s2];
            if (!c2.stage_chunks) continue;
            bool ok;
#ifndef AC_NO_DEVICE_PACK  // (A/B builds without the device packer: its code out of the staged kernel, the host never asks for it)
            if (c2.dp_src) ok = stage_copy_dp(c2, a.stage + AC_STAGE_L_SEG(s2) * AC_QUEUE_LINE, a.gen, a.err);
            else
#endif
                ok = stage_copy(c2.stage_src, c2.stage_dst, c2.stage_chunks, c2.stage_codes_off / AC_STAGE_CHUNK,
                                a.host_hdr + s2 * AC_QUEUE_LINE, a.stage + AC_STAGE_L_SEG(s2) * AC_QUEUE_LINE, c2.stage_gen,
                                a.gen, s2);
            if (!__builtin_amdgcn_readfirstlane((uint32_t)ok))
                if (lane == 0) atomicOr(a.err, AC_DEVERR_STAGE);
        }
    if (wib == 0) {
        uint32_t r = ~0u;
        if (!a.copier_wgs) {
            if (lane == 0) atomicOr(a.err, AC_DEVERR_STAGE);
        } else {
            // the k-mer section fills whole chunks and is in the pinned block before the launch
            r = (uint32_t)stage_gate(st_words, sg.stage_gen, sg.stage_chunks, blockIdx.x % AC_STAGE_REPL, a.gen, 0u,
                                     8u * sg.n_kmers, a.err, sg.stage_codes_off);
        }
        if (lane == 0) *stage_r = r;
        stamp(wave, 7);  // diagnostic builds (staged): the staging wait is over
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    return __builtin_amdgcn_readfirstlane(*stage_r);
}

// Counters of the other queue bank are zeroed for the next launch (strided
// over the waves; nobody dequeues from that bank in this launch).
__device__ __forceinline__ void zero_other_bank(const LaunchArgs& a, uint64_t wave, uint32_t lane) {
    for (uint64_t z = wave; z < a.zero_count; z += a.total_waves)
        if (lane == 0)
            __hip_atomic_exchange(&a.queue[((a.bank ^ 1u) * (uint64_t)a.qstride + z) * AC_QUEUE_LINE], 0u,
                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The claim counters of group g's sub-queues, one line each.  (They stay addressed from the kernel
// argument: an opaque pointer would turn the claim into a flat atomic, which also counts in lgkmcnt
// and so would be waited for by the NFA blocks' LDS waits.)
__device__ __forceinline__ uint32_t* group_counters(const LaunchArgs& a, const SegDev& sg, uint32_t g) {
    return a.queue + ((uint64_t)a.bank * a.qstride + sg.queue_begin + g * sg.subq) * AC_QUEUE_LINE;
}

// Dynamic work queues of a candidate group: count_body's (wm_count.hip, where the comments say why they
// are strided sub-queues with a wave-wide steal probe), without static first items.
// Every item is claimed, the first one too (the bit-sliced kernel; count_body's own queues give every
// wave a static first item and count claims from there).
struct SubQueues {
    uint32_t* counters;  // group_counters()
    uint32_t S, n_items, j, lane;
    // The served sub-queue and its item count (serve), recomputed only when a steal changes it.
    uint32_t jc = 0, jc_items = 0;

    __device__ __forceinline__ void serve(uint32_t jj) {
        jc = jj;
        jc_items = n_in(jj);
    }
    __device__ __forceinline__ uint32_t* counter(uint32_t jj) const { return counters + (uint64_t)jj * AC_QUEUE_LINE; }
    // sub-queue jj holds items jj, jj + S, jj + 2S, ... (strided)
    __device__ __forceinline__ uint32_t n_in(uint32_t jj) const { return jj < n_items ? (n_items - jj + S - 1u) / S : 0u; }
    // item c of the served sub-queue, or n_items
    __device__ __forceinline__ uint32_t item_of(uint32_t c) const { return c < jc_items ? jc + c * S : n_items; }
    __device__ __forceinline__ uint32_t dequeue_issue() const {  // lane 0 holds the result; read with readfirstlane
        uint32_t v = 0;
        if (lane == 0) v = __hip_atomic_fetch_add(counter(jc), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return v;
    }
    // Next item from a sibling sub-queue, or n_items: one wave-wide probe of up to 63 sibling counters,
    // then a claim from the first that still had items (a failed claim: that sibling is dry for good).
    __device__ __forceinline__ uint32_t steal() {
        for (;;) {
            uint32_t found = S;
            for (uint32_t b = 1; b < S && found == S; b += 63u) {  // siblings j+b .. j+b+62
                bool have = false;
                if (lane < 63u && b + lane < S) {
                    const uint32_t jj = (j + b + lane) % S;
                    const uint32_t v = __hip_atomic_load(counter(jj), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    have = v < n_in(jj);
                }
                const uint64_t mk = __ballot(have);
                if (mk) found = b + (uint32_t)__builtin_ctzll(mk);
            }
            if (found == S) return n_items;
            serve((j + found) % S);
            const uint32_t c = __builtin_amdgcn_readfirstlane(dequeue_issue());
            if (c < jc_items) return item_of(c);
        }
    }
};

// Early counting (staged, equal windows): `partial` while the segment is not known complete; a
// fetch is then issued only once stage_gate has seen the chunks it touches -- region bytes
// [r0, r1), which each body works out for its own fetches from `codes_off` -- in device memory and
// inside the N-free prefix ([v_lo, v_hi): chunks already checked), and counted with an all-zero N
// bitmap.  `has_n`: whether the segment's own N bitmap is read, known once it is complete.
struct Gate {
    bool partial = false;
    uint32_t has_n = 0, v_lo = 0, v_hi = 0;
    uint32_t* words = nullptr;      // the segment's device words (stage_words)
    uint32_t* chunk_gen = nullptr;  // its chunks' flags, ...
    uint32_t nchunks = 0, codes_off = 0;  // ... their number and where the codes start in the region
#ifdef AC_STAMPS
    uint64_t ticks = 0, calls = 0;  // (diagnostic: time in the gate's slow path)
#endif
    // The prologue's verdict r: true = skip the segment.
    __device__ __forceinline__ bool open(uint32_t r) {
        const bool skip = r == ~0u;
        partial = r == 2u;
        has_n = (skip || partial) ? 0u : r;
        return skip;
    }
    // The segment's fields read inside the loops, pinned in SGPRs (see count_body's other pins).
    __device__ __forceinline__ void pin(const SegDev& sg) {
        codes_off = sg.stage_codes_off;
        nchunks = sg.stage_chunks;
        chunk_gen = sg.stage_gen;
        asm volatile("" : "+s"(codes_off), "+s"(nchunks), "+s"(chunk_gen));
    }
    // The segment is complete (verdict r: 0 / 1) or skipped (~0u, false): from here on its own N
    // bitmap, if it has one.
    __device__ __forceinline__ bool completed(uint32_t r) {
        partial = false;
        if (r == ~0u) return false;
        has_n = r;
        return true;
    }
    // While partial: waits for region bytes [r0, r1); true = they are in, fetch.  When the wait finds
    // the segment complete or skipped instead, done(verdict) decides: completed(), or the body's own
    // wrapper of it.  (Returning the verdict for the body to act on cost the staged P = 4 kernel four
    // VGPR spills.)
    template <class Done>
    __device__ __forceinline__ bool pass(uint32_t r0, uint32_t r1, uint32_t gen, uint32_t* err, Done done) {
        if (r0 >= v_lo && r1 <= v_hi) return true;
#ifdef AC_STAMPS
        const uint64_t tg = __builtin_amdgcn_s_memrealtime();
#endif
        const uint64_t g = stage_gate(words, chunk_gen, nchunks, blockIdx.x % AC_STAGE_REPL, gen, r0, r1, err);
#ifdef AC_STAMPS
        ticks += __builtin_amdgcn_s_memrealtime() - tg;
        ++calls;
#endif
        // (a call's results come back in VGPRs: made wave-uniform again, or everything they
        // touch -- the item cursor, window bases -- would turn divergent)
        const uint32_t r = __builtin_amdgcn_readfirstlane((uint32_t)g);
        if (r == 2u) {
            v_lo = (r0 / AC_STAGE_CHUNK) * AC_STAGE_CHUNK;
            v_hi = __builtin_amdgcn_readfirstlane((uint32_t)(g >> 32));
            return true;
        }
        return done(r);
    }
    // Waits for the whole segment (a window that needs its N bitmap): the verdict, for completed().
    __device__ __forceinline__ uint32_t whole(uint32_t gen, uint32_t* err) const {
        return __builtin_amdgcn_readfirstlane(
            (uint32_t)stage_gate(words, chunk_gen, nchunks, blockIdx.x % AC_STAGE_REPL, gen, 0u, ~0u, err));
    }
};

// The count hand-off.  The workgroup's waves have summed their counts in LDS (`cnt`, 64 Q slots: slot
// q * 64 + lane is candidate g * 64 Q + q * 64 + lane); one wave adds the sums to the group's slots in
// `acc`, so each slot takes 1/AC_WAVES_PER_BLOCK of the same-address atomics (they serialise at
// the memory side: ~10 us of launch tail at cfg2 with one atomic per wave; profiles/r01_kernel_log.md).
// Each add is 64-bit, (1 << 32) + the sum: the returned word says how many workgroups of the group
// have added before this one, so the last to add -- per slot -- knows the total at once and moves it
// to the counts.  One device-scope round trip at the launch's end (round 4 had three: the adds, a
// group ticket taken after them, the slots read back and zeroed).  No fences: the arrival count and
// the sum change in one atomic.
template <int Q, bool STAGED>
__device__ __forceinline__ void count_hand_off(const LaunchArgs& a, const SegDev& sg, Deal deal, uint32_t g, uint32_t wib,
                                               uint32_t lane, const uint32_t* cnt) {
    // (every wave's error-word atomics are performed before its workgroup's adds: the staged launch's
    // last workgroup of a slot reads the word)
    if (STAGED) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (wib != 0) return;
    uint64_t* acc = a.acc + sg.acc_begin + g * (64u * Q);
    // Workgroups serving group g: those dealt to its subq / WPB block-queues.
    const uint32_t qb0 = (sg.queue_begin + g * sg.subq) / WAVES_PER_BLOCK, nq = sg.subq / WAVES_PER_BLOCK;
    uint32_t n_wg = 0;
    for (uint32_t i = 0; i < nq; ++i) n_wg += deal.wgs_of(qb0 + i);
    uint32_t mine[Q];
    uint64_t old[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        mine[q] = cnt[q * 64 + lane];
        old[q] = __hip_atomic_fetch_add(&acc[q * 64 + lane], (1ull << 32) | mine[q], __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if ((uint32_t)(old[q] >> 32) != n_wg - 1u) continue;  // not the slot's last workgroup
        const uint32_t v = (uint32_t)old[q] + mine[q];
        const uint32_t cand = g * (64u * Q) + (uint32_t)q * 64u + lane;
        __hip_atomic_store(&acc[q * 64 + lane], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cand < sg.n_kmers) {
            if (a.add_counts) {
                if (v) atomicAdd(&sg.counts[cand], v);
            } else if (STAGED && a.tag) {  // host memory, each count tagged with the launch's generation
                __hip_atomic_store((uint64_t*)sg.counts + cand, ((uint64_t)a.gen << 32) | v, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
            } else {  // (device memory: read after the stream has completed)
                sg.counts[cand] = v;
            }
        }
        if (STAGED && q == 0 && lane == 0) {
            // The group's error snapshot, by slot (0, lane 0)'s last workgroup: every workgroup's waves
            // performed their error atomics before that workgroup's add to the slot, so the word holds
            // every bit the group set; all groups' snapshots together hold the launch's.  Tagged
            // completion (synchronous calls): the host waits until every count and every group's word
            // carries this launch's generation, so no completion word, no wait for the counts' stores
            // and no launch-wide counter sit on the path to the host.  Submits (counts in device
            // memory): the bits go to the context's word (ac_check).
            const uint32_t e = __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (a.tag)
                __hip_atomic_store(a.grp_err + sg.group_begin + g, ((uint64_t)a.gen << 32) | e, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
            else if (e && a.err_out)
                atomicOr(a.err_out, e);
        }
    }
}
