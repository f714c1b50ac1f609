// bs_count.inc -- the bit-sliced count kernel's body (DESIGN.md §4e), included by wm_count.hip (three NFA
// rows: edit budgets 0..2) and, through bs_family.inc, by bs3_count.hip (four rows: budget 3), by
// bsh_count.hip (either, and the windows' hit words stored beside the counts), by bsp_count.hip (either, the
// hit words and the match end positions) and by bshs_count.hip / bsps_count.hip (the staged forms of those
// two) inside their anonymous namespaces:
// the NFA's place in the frame of count_frame.inc (deal, staged prologue,
// sub-queues, gate, count hand-off -- the word-parallel kernel's), with another mapping of a wave
// onto the work.
//
// Mapping: bit j of a lane word is candidate j of a block of 32 (bs_nfa.h); a candidate group
// (BS_GROUP candidates for every K, wm_count.h; the host plans the launch, the acc slots and the groups'
// error words by that size, launch_group_size) takes LW = max(2, next_pow2(ceil(candidates / 32)))
// lanes per window (bs_lane_shift), lane % LW = the candidate block, and a wave counts a ROW of 64 / LW
// consecutive windows at once.  A work item is `chunk` rows.
// Text is per lane: every lane loads its window's slot itself (buffer loads at its own offset, the
// next row's while this one is counted) and the window's first lane parks it in LDS -- 24 words per
// window, 16 of codes and 8 of N bits -- from where one code word is read back per 16 bases; per
// base the lane forms its character (2-bit code + 4 x N bit) and reads nE[0..K-1] for it from the
// workgroup's ~Eq table in LDS with ceil(K / 4) ds_read_b128.
// Table layout: [character 0..7][quad 0..ceil(K/4)-1][block 0..BS_LWMAX-1] x 16 B (the last quad's
// positions past K - 1 are padding of the table, never written or used: the pattern is not padded --
// leading wildcard positions would change the counts), the characters BS_ROW
// bytes further apart than their quads need, so that characters of different parity start in
// different bank halves (windows of one ds_read_b128 lane group that hold the same character read
// one address).  Characters 4..7 (an N base, whatever its code bits) are all ones, as are the bits
// of candidate slots past n_kmers.
// Only equal-window launches (every live segment has ulen in 1..256) with K in AC_BS_K_LIST; the
// residency of an instantiation is bs_waves_per_simd(family, K) (wm_count.h).
constexpr uint32_t BS_LWMAX = BS_GROUP / 32u;       // lanes per window of a full group
constexpr uint32_t BS_ROW = BS_LWMAX * 16u;         // bytes of one (character, quad) table row

template <int K>
struct BsLds {
    static constexpr uint32_t QUADS = (K + 3) / 4;
    static constexpr uint32_t CHAR_STRIDE = (QUADS + 1u) * BS_ROW;
    alignas(16) uint32_t tab[8u * CHAR_STRIDE / 4u];  // characters 4..7: an N base, whatever its code bits
    uint32_t cnt[BS_GROUP];
    uint32_t stage_r;
    // per wave, two buffers of a row's text: up to 32 windows' slots of up to 16 code words, and the
    // 8 words of N bits that go with them
    alignas(16) uint32_t text[AC_WAVES_PER_BLOCK][2][32][24];
};

typedef uint32_t bs_v4u __attribute__((ext_vector_type(4)));

// nE[0..K-1] of this lane's block for the character whose table row starts at byte `addr`
// (character * CHAR_STRIDE + block * 16): ceil(K / 4) ds_read_b128 at immediate offsets.
template <int K>
__device__ __forceinline__ void bs_read(const BsLds<K>& lds, uint32_t addr, uint32_t (&e)[K]) {
    const char* p = (const char*)lds.tab + addr;
#pragma unroll
    for (int q = 0; q < (K + 3) / 4; ++q) {
        const bs_v4u v = *(const bs_v4u*)(p + q * BS_ROW);
        e[4 * q] = v.x;
        if (4 * q + 1 < K) e[4 * q + 1] = v.y;
        if (4 * q + 2 < K) e[4 * q + 2] = v.z;
        if (4 * q + 3 < K) e[4 * q + 3] = v.w;
    }
}

// The table row of base b of a word of 2-bit codes and its N bits: character = code + 4 x N bit.
template <int K>
__device__ __forceinline__ uint32_t bs_row(uint32_t code, uint32_t nm, uint32_t b, uint32_t lane_off) {
    const uint32_t c = ((nm >> b & 1u) << 2) | ((code >> (2u * b)) & 3u);
    return c * BsLds<K>::CHAR_STRIDE + lane_off;
}

// 4 bases of every lane's window -- the one copy of the NFA code in the kernel (with a second, e.g. a
// 16-base form beside a tail form, the register allocator spilled the NFA state around both):
// `code` / `nm` hold their 2-bit codes and N bits from bit 0, `ncode` / `nnm` the next block's, `ea`
// comes in with the first base's table rows and leaves with the next block's first base's, so every
// base's table reads are issued one base ahead.  Bases in pairs: 1.5 ops of hit accumulation per base.
// One form for windows with and without N: a row of windows has an N in most blocks once some of
// its windows do.
// S: the NFA's state, bs::State<K> (three rows) or bs::StateR<K, R>.  AHEAD2 = false (the widest E = 3
// kernels, wm_count.h BS3_ONE_BASE_K): one base's table rows are held at a time -- a base's reads are
// issued when the previous base's rows have been used, K registers less; the SIMD's other wave covers
// the reads.
// A state S = BsWithPos<..> (the POS kernels of bsp_count.hip) carries the position planes (bs_pos.h), the
// block's number and the launch's E: its hits are accumulated per base (bs::hits_new), the candidates newly
// hit at a base written into the planes, the planes of the block's number at its end.  Any other state:
// hits in pairs, as above.
template <class B>
struct BsWithPos : B {
    bs::PosPlanes ps;
    uint32_t q, budget;  // (wave-uniform)
};
template <class S>
struct BsPosOf {
    static constexpr bool ON = false;
};
template <class B>
struct BsPosOf<BsWithPos<B>> {
    static constexpr bool ON = true;
};
template <int K, bool AHEAD2, class S>
__device__ __forceinline__ void bs_block4(S& s, const BsLds<K>& lds, uint32_t code, uint32_t nm, uint32_t ncode,
                                          uint32_t nnm, uint32_t lane_off, uint32_t (&ea)[K]) {
    constexpr bool POS = BsPosOf<S>::ON;
    if constexpr (!AHEAD2) {
#pragma unroll
        for (uint32_t b = 0; b < 4u; b += 2u) {
            bs::advance<K>(s, ea);
            const auto x = bs::last<K>(s);
            if constexpr (POS) bs::pos_base(s.ps, bs::hits_new(s, s.budget), b);
            bs_read<K>(lds, bs_row<K>(code, nm, b + 1u, lane_off), ea);
            bs::advance<K>(s, ea);
            if constexpr (POS) bs::pos_base(s.ps, bs::hits_new(s, s.budget), b + 1u);
            else bs::hits2<K>(s, x);
            bs_read<K>(lds, b + 2u < 4u ? bs_row<K>(code, nm, b + 2u, lane_off) : bs_row<K>(ncode, nnm, 0u, lane_off), ea);
        }
        if constexpr (POS) bs::pos_block(s.ps, s.q);
        return;
    }
    uint32_t eb[K];
#pragma unroll
    for (uint32_t b = 0; b < 4u; b += 2u) {
        bs_read<K>(lds, bs_row<K>(code, nm, b + 1u, lane_off), eb);
        bs::advance<K>(s, ea);
        const auto x = bs::last<K>(s);
        if constexpr (POS) bs::pos_base(s.ps, bs::hits_new(s, s.budget), b);
        bs_read<K>(lds, b + 2u < 4u ? bs_row<K>(code, nm, b + 2u, lane_off) : bs_row<K>(ncode, nnm, 0u, lane_off), ea);
        bs::advance<K>(s, eb);
        if constexpr (POS) bs::pos_base(s.ps, bs::hits_new(s, s.budget), b + 1u);
        else bs::hits2<K>(s, x);
    }
    if constexpr (POS) bs::pos_block(s.ps, s.q);
}

// The flush's plane merge: the 64 / lw lanes that hold one candidate block (lanes lw apart, one per window of
// the row) sum their planes in registers, a butterfly of bs::planes_add from 32 lanes apart down to lw --
// one plane more per round (N before the round D lanes apart), the partner's planes through ds_bpermute
// (the LDS crossbar: no memory, no conflict).  Every lane of the block leaves with the block's sums in
// `m`, whose planes past the first bs::VC_PLANES come in zero.
template <int N, uint32_t D>
__device__ __forceinline__ void bs_merge_round(uint32_t (&m)[bs::VC_MERGED_PLANES], uint32_t lane, uint32_t lw) {
    static_assert(N < bs::VC_MERGED_PLANES, "planes");
    if (D >= lw) {  // (wave-uniform: rounds are skipped from the last one backwards)
        uint32_t theirs[N];
#pragma unroll
        for (int b = 0; b < N; ++b) theirs[b] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane ^ D) << 2), (int)m[b]);
        bs::planes_add<N>(m, theirs, m);
    }
}
__device__ __forceinline__ void bs_merge(uint32_t (&m)[bs::VC_MERGED_PLANES], uint32_t lane, uint32_t lw) {
    static_assert(bs::VC_MERGED_PLANES == bs::VC_PLANES + 5, "five rounds");
    bs_merge_round<bs::VC_PLANES, 32u>(m, lane, lw);
    bs_merge_round<bs::VC_PLANES + 1, 16u>(m, lane, lw);
    bs_merge_round<bs::VC_PLANES + 2, 8u>(m, lane, lw);
    bs_merge_round<bs::VC_PLANES + 3, 4u>(m, lane, lw);
    bs_merge_round<bs::VC_PLANES + 4, 2u>(m, lane, lw);
}

// The state of R rows: bs_nfa.h's for the three rows of the E = 2 kernels, else bs_nfa_r.h's.
template <int K, int R>
struct BsNfa {
    typedef bs::StateR<K, R> State;
};
template <int K>
struct BsNfa<K, 3> {
    typedef bs::State<K> State;
};

// ... and with the position planes beside them (POS).
template <int K, int R, bool POS>
struct BsState {
    typedef typename BsNfa<K, R>::State type;
};
template <int K, int R>
struct BsState<K, R, true> {
    typedef BsWithPos<typename BsNfa<K, R>::State> type;
};

// R = 3: the edit budget E = a.max_errors is 0, 1 or 2 (a smaller budget drops levels where a row's
// hit masks become counts); R = 4: E = 3.
// HITS (bsh_count.hip: plain launches, bshs_count.hip: staged ones; DESIGN.md §4e "Hit levels", "Hits from the
// jobs stage"): where a row's masks become counts,
// every lane whose window and candidate block exist also stores its hit word of each level 0..E to the
// segment's matrix a.hits[si] -- one word, one lane, one row: no memset, no atomic.
// POS (bsp_count.hip / bsps_count.hip, implies HITS; DESIGN.md §4e "Match end positions"): the same lanes also store the
// eight plane words of their candidates' end positions to a.pos[si], masked to the pairs with a hit.
template <int K, bool STAGED, int R = 3, bool HITS = false, bool POS = false>
__device__ __forceinline__ void bs_body(const LaunchArgs& a, BsLds<K>& lds) {
    static_assert(K >= 3 && K <= 32, "a k-mer is one 64-bit word (dna2int layout: K = 32 fills it)");
    static_assert(HITS || !POS, "positions come with the hits");
    constexpr uint32_t CS = BsLds<K>::CHAR_STRIDE;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wib;
    stamp(wave, 0);
    const Deal deal = deal_of(a);
    const Place pl = place_of(a, deal.bq, wib);
    const int si = pl.si;
    const SegDev& sg = a.seg[si];
    const uint32_t g = pl.g, j = pl.j;

    Gate gt;  // staged: while the segment is not known complete, rows go through the gate
    gt.has_n = sg.has_n;
    bool skip = false;
    if (STAGED && sg.stage_chunks) {  // (every segment has equal windows: never the whole-segment wait)
        gt.words = a.stage + AC_STAGE_L_SEG(si) * AC_QUEUE_LINE;
        skip = gt.open(staged_prologue(a, sg, gt.words, wib, lane, wave, &lds.stage_r));
    }
    const uint32_t* codes_p = sg.codes;
    const uint32_t* nmask_p = sg.nmask;
    uint32_t code_bytes = (uint32_t)(sg.n_bases >> 2);
    uint32_t nmask_bytes = (uint32_t)(sg.n_bases >> 3);
    asm volatile("" : "+s"(codes_p), "+s"(nmask_p), "+s"(code_bytes), "+s"(nmask_bytes));
    const __amdgpu_buffer_rsrc_t r_codes = __builtin_amdgcn_make_buffer_rsrc((void*)codes_p, 0, (int)code_bytes, 0x00020000);
    // (the N bitmap is read only by windows that need it, and -- staged -- only once the segment is complete)
    const __amdgpu_buffer_rsrc_t r_nmask = __builtin_amdgcn_make_buffer_rsrc((void*)nmask_p, 0, (int)nmask_bytes, 0x00020000);
    uint32_t* g_queue = group_counters(a, sg, g);
    uint32_t ulen = sg.ulen;
    asm volatile("" : "+s"(ulen));
    const uint32_t sbytes = ((ulen + 31u) & ~31u) >> 2;  // bytes of a window's slot of code words (8..64)
    uint32_t seg_nw = sg.n_windows, seg_chunk = sg.chunk;
    asm volatile("" : "+s"(seg_nw), "+s"(seg_chunk));
    if constexpr (STAGED) gt.pin(sg);
    const bool rec = sg.nrec != 0u;  // inline N records (nrec.h) in the top bits of every slot's last code word
    const uint32_t rec_pb = nrec_pos_bits(ulen);

    // The group's lanes per window, and this lane's place in a row.
    const uint32_t ng = min(BS_GROUP, sg.n_kmers - g * BS_GROUP);
    const uint32_t lwsh = bs_lane_shift(ng), LW = 1u << lwsh, wpr = 64u >> lwsh;
    const uint32_t wl = lane >> lwsh, blk = lane & (LW - 1u);
    const uint32_t lane_off = blk * 16u;
    const uint32_t n_rows = (seg_nw + wpr - 1u) >> (6u - lwsh);

    zero_other_bank(a, wave, lane);

    // The group's work queues (SubQueues): items of `chunk` rows.  Every item is claimed from the
    // wave's sub-queue counter, the first one too (no static first item: a wave that starts late takes
    // what is left then, DESIGN.md §4e), further ones one row ahead.
    const uint32_t S = sg.subq;
    const uint32_t chunk = seg_chunk;
    const uint32_t n_items = (n_rows + chunk - 1u) / chunk;
    SubQueues sq = {g_queue, S, n_items, j, lane};
    sq.serve(j);

    // Staged early counting: before a row's fetch, every byte the fetch reads -- the row's slots, which
    // are contiguous in the image, and the 32 bytes a lane's 16-byte loads may reach past its slot -- is
    // in device memory and inside the N-free prefix; false = skip the segment.
    auto gate = [&](uint32_t rr) __attribute__((always_inline)) {
        if constexpr (STAGED) {
            if (!gt.partial) return true;
            const uint32_t b0 = rr * wpr * sbytes;
            const uint32_t r0 = gt.codes_off + b0, r1 = gt.codes_off + min(b0 + wpr * sbytes + 32u, code_bytes);
            return gt.pass(r0, r1, a.gen, a.err, [&](uint32_t r) { return gt.completed(r); });
        } else {
            (void)rr;
            return true;
        }
    };

    // A row's text goes through LDS, so that no window's code words sit in registers while it is counted:
    // every lane loads its window's slot (up to 64 bytes; the lanes of a window load the same lines), the
    // window's first lane stores it into the wave's text buffer, and every chunk of 16 bases reads its
    // one code word from there.  Two buffers: the next row's text is fetched while this row is counted.
    // A lane without a window (a partial last row) loads from an offset past the range check of every image
    // the host accepts -- AC_MAX_IMAGE_BASES keeps an image's code bytes below it (wm_count.h) -- i.e. zeros
    // without a memory access; and no window's slot offset equals it, so it also says "no window" below.
    constexpr uint32_t NO_WINDOW = 0xffffff00u;
    static_assert(AC_MAX_IMAGE_BASES / 4u <= NO_WINDOW, "an accepted image's code bytes end below NO_WINDOW");
    auto slot_off = [&](uint32_t rr) __attribute__((always_inline)) {
        const uint32_t w = rr * wpr + wl;
        return w < seg_nw ? w * sbytes : NO_WINDOW;
    };
    uint32_t buf = 0;   // the text buffer of the current row
    uint32_t bufn = 0;  // bit b: buffer b's N words came with its text (a segment without records that has a bitmap)
    auto fetch_row = [&](uint32_t rr, uint32_t bf) __attribute__((always_inline)) {
        const uint32_t off = slot_off(rr);
        bs_v4u* dst = (bs_v4u*)&lds.text[wib][bf][wl][0];
        const bs_v4u t0 = __builtin_amdgcn_raw_buffer_load_b128(r_codes, off, 0, 0);
        const bs_v4u t1 = __builtin_amdgcn_raw_buffer_load_b128(r_codes, off + 16u, 0, 0);
        if (sbytes > 32u) {
            const bs_v4u t2 = __builtin_amdgcn_raw_buffer_load_b128(r_codes, off + 32u, 0, 0);
            const bs_v4u t3 = __builtin_amdgcn_raw_buffer_load_b128(r_codes, off + 48u, 0, 0);
            if (blk == 0u) dst[2] = t2, dst[3] = t3;
        }
        if (blk == 0u) dst[0] = t0, dst[1] = t1;
        const bool with_n = !rec && gt.has_n;  // no records: every window's N bits are its bitmap words
        if (with_n) {
            const uint32_t noff = off == NO_WINDOW ? NO_WINDOW : off >> 1;
            const bs_v4u n0 = __builtin_amdgcn_raw_buffer_load_b128(r_nmask, noff, 0, 0);
            bs_v4u n1 = {0u, 0u, 0u, 0u};
            if (sbytes > 32u) n1 = __builtin_amdgcn_raw_buffer_load_b128(r_nmask, noff + 16u, 0, 0);
            if (blk == 0u) dst[4] = n0, dst[5] = n1;
        }
        bufn = (bufn & ~(1u << bf)) | ((with_n ? 1u : 0u) << bf);
        // (the other lanes of the window read what its first lane wrote: LDS serves a wave's
        // instructions in order; the fence keeps the compiler from moving the reads up)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };

    // The first item's claim goes out here and is read after the table barrier.
    const uint32_t pending0 = skip ? 0u : sq.dequeue_issue();
    uint32_t item = n_items, row = 0u, item_end = 0u;

    // The workgroup's ~Eq table: wave v takes candidates 64 v .. 64 v + 63 of the group (blocks 2 v and
    // 2 v + 1).  It parks their k-mers in its text buffer (free until the first fetch, after the table
    // barrier); in passes of 16 positions, lane 4 (i % 16) + c reads them back -- every lane the same
    // words: broadcast reads -- and forms the mask of position i and character c itself (bs::neq_mask: a
    // shift, a compare and an or per candidate instead of one ballot and a masked select per (position,
    // character) in every lane), then stores its two halves.  Wave 0 also writes the N rows and zeroes
    // the counts.
    if (!skip && (wib == 0 || 2u * wib < LW)) {
        const uint32_t first = wib * 64u;
        const uint32_t present = ng > first ? ng - first : 0u;  // (0: the blocks LW rounds up to, all ones)
        uint64_t* park = (uint64_t*)&lds.text[wib][0][0][0];
        park[lane] = lane < present ? sg.kmers[g * BS_GROUP + first + lane] : 0ull;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (uint32_t i0 = 0; i0 < (uint32_t)K; i0 += 16u) {
            const uint32_t i = i0 + (lane >> 2), cc = lane & 3u;  // (one lane per (position, character) of the pass)
            const uint64_t mine = bs::neq_mask<K>(park, present, min(i, (uint32_t)K - 1u), cc);
            if (i < (uint32_t)K) {
                uint32_t* p = lds.tab + (cc * CS + (i >> 2) * BS_ROW + (i & 3u) * 4u) / 4u;
                p[(2u * wib) * 4u] = (uint32_t)mine;
                if (2u * wib + 1u < BS_LWMAX) p[(2u * wib + 1u) * 4u] = (uint32_t)(mine >> 32);
            }
        }
    }
    if (wib == 0) {
        for (uint32_t x = lane; x < 4u * CS / 4u; x += 64u) lds.tab[4u * CS / 4u + x] = ~0u;
        for (uint32_t x = lane; x < BS_GROUP; x += 64u) lds.cnt[x] = 0u;
    }
    bool stage_ok = true;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    stamp(wave, 1);
    if (!skip) {
        item = __builtin_amdgcn_readfirstlane(sq.item_of(__builtin_amdgcn_readfirstlane(pending0)));
        if (item >= n_items && S > 1) item = __builtin_amdgcn_readfirstlane(sq.steal());
    }
    row = item * chunk;
    item_end = min(n_rows, row + chunk);
    if (item < n_items) {
        if (STAGED) stage_ok = gate(row);
        if (stage_ok) fetch_row(row, buf);
        else item = n_items;
    }

    bs::VCount vc;
    bs::vc_clear(vc);
    // The planes' counts into the workgroup's count array (the workgroup's waves sum there).  The lanes of
    // the wave that share a candidate block sum their planes in registers first (bs_merge); each then adds
    // its own 32 LW / 64 of the block's candidates, so no two lanes of an add meet on one word.
    auto flush = [&]() __attribute__((always_inline)) {
        uint32_t m[bs::VC_MERGED_PLANES];
#pragma unroll
        for (int b = 0; b < bs::VC_MERGED_PLANES; ++b) m[b] = b < bs::VC_PLANES ? vc.p[b < bs::VC_PLANES ? b : 0] : 0u;
        // (the lane's place is formed here from what the row loop keeps anyway, and pinned: formed outside, the
        // five rounds' partner addresses and the count slots are hoisted out of the row loop and held in
        // registers through the 4-base block)
        uint32_t w = wl, off = lane_off;
        asm volatile("" : "+v"(w), "+v"(off));
        bs_merge(m, (w << lwsh) | (off >> 4), LW);
        uint32_t* cnt = &lds.cnt[2u * off + bs::merged_first(lwsh, w)];  // (block * 32 + the lane's first candidate)
        for (uint32_t x = 0; x < bs::merged_per_lane(lwsh); ++x) {
            const uint32_t v = bs::planes_get(m, bs::merged_first(lwsh, w) + x);
            if (v) __hip_atomic_fetch_add(&cnt[x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        bs::vc_clear(vc);
    };

    const uint32_t nq = (ulen + 3u) >> 2;  // blocks of 4 bases per window
    const uint32_t budget = a.max_errors;  // (wave-uniform)
    while (item < n_items) {
        const uint32_t* text = &lds.text[wib][buf][wl][0];
        const uint32_t my_off = slot_off(row);
        bool has = my_off != NO_WINDOW;
        const bool last = row + 1u >= item_end;  // the item's last row: claim the next item
        uint32_t pending = 0;
        uint32_t nitem = item, nrow = row + 1u;

        // The window's N bits, 16 per chunk, are read from the row's buffer: they came with the text
        // (no records), or are written here from the window's record (the top bits of its slot's last
        // code word) -- from its N-bitmap words when the record overflowed (staged: only once the whole
        // segment is in).  Most rows have no N at all and skip this.
        bool row_n = (bufn >> buf & 1u) != 0u;
        const uint32_t rc = rec ? text[(sbytes >> 2) - 1u] >> 29 : 0u;
        if (__builtin_expect(__ballot(rc != 0u) != 0ull, 0)) {
            const uint32_t rw = text[(sbytes >> 2) - 1u];
            const bool ovf = has && rc == NREC_OVERFLOW;
            if (STAGED && gt.partial && __ballot(ovf)) {
                if (!gt.completed(gt.whole(a.gen, a.err))) stage_ok = false;
            }
            if (ovf && !gt.has_n) {  // no bitmap for an overflowed record: skipped, reported
                if (stage_ok) atomicOr(a.err, AC_DEVERR_WINDOW);
                has = false;
            }
            uint32_t n[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            for (uint32_t i = 0; i < 4u; ++i)
                if (rc != NREC_OVERFLOW && i < rc) {
                    const uint32_t pos = (rw >> nrec_pos_shift(rec_pb, i)) & ((1u << rec_pb) - 1u);
#pragma unroll
                    for (uint32_t x = 0; x < 8u; ++x)
                        if ((pos >> 5) == x) n[x] |= 1u << (pos & 31u);
                }
            const bool use_bm = ovf && has;
            if (__ballot(use_bm)) {
                const uint32_t noff = use_bm ? my_off >> 1 : NO_WINDOW;
                const bs_v4u b0 = __builtin_amdgcn_raw_buffer_load_b128(r_nmask, noff, 0, 0);
                bs_v4u b1 = {0u, 0u, 0u, 0u};
                if (sbytes > 32u) b1 = __builtin_amdgcn_raw_buffer_load_b128(r_nmask, noff + 16u, 0, 0);
                if (use_bm) n[0] = b0.x, n[1] = b0.y, n[2] = b0.z, n[3] = b0.w, n[4] = b1.x, n[5] = b1.y, n[6] = b1.z, n[7] = b1.w;
            }
            if (blk == 0u) {
                bs_v4u* dst = (bs_v4u*)&lds.text[wib][buf][wl][16];
                dst[0] = bs_v4u{n[0], n[1], n[2], n[3]};
                dst[1] = bs_v4u{n[4], n[5], n[6], n[7]};
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            row_n = true;
        }
        uint32_t live = has ? ~0u : 0u;  // (a lane without a window adds nothing to the counts)
        asm volatile("" : "+v"(live));

        // The window's bases in blocks of 4, the last one filled up with N: an N matches nothing, and an
        // occurrence that would end on a filling N also ends on the window's last base at no more edits
        // (its N bases deleted), so the filling adds no hit.  word(gc): the codes and N bits of bases
        // 16 gc .. 16 gc + 15.
        auto n_word = [&](uint32_t gc) __attribute__((always_inline)) {
            const uint32_t real = ulen > 16u * gc ? min(16u, ulen - 16u * gc) : 0u;
            const uint32_t nmw = row_n ? text[16u + (gc >> 1)] >> ((gc & 1u) * 16u) : 0u;
            return (nmw | (0xffffu << real)) & 0xffffu;
        };
        typename BsState<K, R, POS>::type s;
        bs::init<K>(s);
        if constexpr (POS) {
            bs::pos_clear(s.ps);
            s.budget = budget;
        }
        uint32_t code = text[0], nm = n_word(0u);
        uint32_t ea[K];
        bs_read<K>(lds, bs_row<K>(code, nm, 0u, lane_off), ea);
        // The claim of the next item goes out 20 bases before the row's end and is read before its last
        // block, with the next row's gate and text: late, so that the items left when the waves' first
        // ones end go to the waves that end first, wherever they run (claimed at the row's start, a
        // nearly one-round launch's second items all went to the first workgroups dispatched -- a few
        // CUs ran two rounds while the others idled).
        const uint32_t q_claim = nq > 5u ? nq - 5u : 0u, q_next = nq - 1u;
        for (uint32_t q = 0; q < nq && stage_ok; ++q) {
            if (__builtin_expect(q == q_claim && last, 0)) pending = sq.dequeue_issue();
            if (__builtin_expect(q == q_next, 0)) {  // (unlikely: the register allocator keeps the NFA state in registers around the blocks, not around this)
                if (last) {
                    nitem = __builtin_amdgcn_readfirstlane(sq.item_of(__builtin_amdgcn_readfirstlane(pending)));
                    if (nitem >= n_items && S > 1) nitem = __builtin_amdgcn_readfirstlane(sq.steal());
                    nrow = nitem * chunk;
                }
                if (nitem < n_items) {
                    if (gate(nrow)) fetch_row(nrow, buf ^ 1u);
                    else stage_ok = false;
                }
                // (read again, so that the rows read ahead are not kept in registers across this)
                bs_read<K>(lds, bs_row<K>(code, nm, 0u, lane_off), ea);
            }
            if constexpr (POS) s.q = q;
            uint32_t ncode = code >> 8, nnm = nm >> 4;
            if ((q & 3u) == 3u) {
                ncode = text[(q >> 2) + 1u];
                nnm = n_word((q >> 2) + 1u);
            }
            bs_block4<K, !(R == 4 && K >= (POS ? BSP3_ONE_BASE_K : BS3_ONE_BASE_K))>(s, lds, code, nm, ncode, nnm, lane_off, ea);
            code = ncode;
            nm = nnm;
        }
        if (STAGED && !stage_ok) {  // the segment is skipped (the error word says so)
            item = n_items;
            break;
        }
        if constexpr (HITS) {
            // Level e's word: bit j set iff candidate 32 (8 g + blk) + j lies within e edits of this
            // window; bits of candidates past n_kmers are 0, and a window the kernel skipped (`has`
            // false: live = 0) stores zeros.  A block past the group's last one has no word.
            const uint32_t nblk = (ng + 31u) >> 5;
            if (my_off != NO_WINDOW && blk < nblk) {
                const uint32_t left = ng - 32u * blk;  // (>= 1) candidates of this block
                const uint32_t keep = live & (left >= 32u ? ~0u : (1u << left) - 1u);
                const uint64_t words = (uint64_t)((sg.n_kmers + 31u) >> 5);
                uint32_t* hp = a.hits[si] + (uint64_t)(row * wpr + wl) * words + (BS_GROUP / 32u) * g + blk;
                // (the planes lie the matrix's window count apart: the segment's own, unless the launch counts a
                // window sub-range of a job into the job's matrix -- a part of a DMA-path jobs call)
                const uint64_t plane = (uint64_t)a.mat_nw[si] * words;
                if constexpr (R == 3) {
                    hp[0] = ~s.a0 & keep;
                    if (budget >= 1u) hp[plane] = ~s.a1 & keep;
                    if (budget >= 2u) hp[2u * plane] = ~s.a2 & keep;
                } else {
#pragma unroll
                    for (int e = 0; e < R; ++e) hp[(uint64_t)e * plane] = ~s.a[e] & keep;
                }
                if constexpr (POS) {
                    // Plane b's word: bit j = bit b of pos - 1 of candidate j and this window, 0 where the
                    // pair has no hit within the budget.
                    uint32_t aE;
                    if constexpr (R == 3) aE = budget >= 2u ? s.a2 : budget == 1u ? s.a1 : s.a0;
                    else aE = s.a[R - 1];
                    const uint32_t hit = ~aE & keep;
                    uint32_t* pp = a.pos[si] + (uint64_t)(row * wpr + wl) * words + (BS_GROUP / 32u) * g + blk;
#pragma unroll
                    for (int b = 0; b < bs::POS_PLANES; ++b) pp[(uint64_t)b * plane] = s.ps.p[b] & hit;
                }
            }
        }
        if constexpr (R == 3) {
            bs::vc_add_e(vc, budget, s.a0, s.a1, s.a2, live);
            if (bs::vc_full(vc)) flush();
        } else {
            bs::vc_add_r<R>(vc, s.a, live);
            if (bs::vc_full_r<R>(vc)) flush();
        }
        if (last) item_end = min(n_rows, nrow + chunk);
        item = nitem;
        row = nrow;
        buf ^= 1u;
    }
    if (vc.n) flush();
    stamp(wave, 2);

    // The workgroup's sums, slot = candidate of the group (blk * 32 + bit), to the counts.
    count_hand_off<(int)(BS_GROUP / 64u), STAGED>(a, sg, deal, g, wib, lane, lds.cnt);
    stamp(wave, 3);
}
