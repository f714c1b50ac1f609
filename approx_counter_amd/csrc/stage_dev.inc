// stage_dev.inc -- the device side of the staged launch's protocol (DESIGN.md §4c) and the device
// packer (§4d), included once by wm_count.hip inside its anonymous namespace, before the count
// frame (count_frame.inc) and the two kernel bodies that use it: the device words (StageWords), the
// bounded waits' clock (StageClock), the copier loops (stage_copy, stage_copy_dp with
// stage_pack_chunk) and the readers' waits (stage_wait_all, stage_gate).
#ifndef AC_COPY_AHEAD
#define AC_COPY_AHEAD 32 // chunks a copier may run ahead of its segment's copied count (0: no limit; 8 / 16 / 32 measured, profiles/r03_m10/ab.log)
#endif
#ifndef AC_STAGE_LOAD_AUX
#define AC_STAGE_LOAD_AUX 2  // cache policy of the staging copy's loads: nt (A/B builds: 17 = sc0 sc1)
#endif

// Staged launch (DESIGN.md §4c, "early launch"): the kernel is launched before
// the host has packed its inputs.  Wave 0 of every workgroup runs stage_copy
// before the workgroup reads the segment.  It claims tickets of the segment (an
// agent-scope counter): ticket 0 makes it the segment's only host poller,
// ticket c >= 1 the copier of AC_STAGE_CHUNK-byte chunk c - 1 of the region.
// The host packs the region front to back and publishes the packed N-free
// prefix (progress record) as it grows, then the final byte count and N verdict
// (flag).  The poller reads the header with one 16-byte system-scope load per
// poll (~2 us apart: one PCIe round trip) and republishes it in device words:
// the N-free bytes so far, then the final verdict, bytes and a final-seen word.
// A copier waits (polling the device words) until its chunk lies inside the
// N-free prefix -- so chunks cross PCIe while later ones are still being packed
// -- or the final header is out; it copies the chunk from the pinned block to
// device memory with write-through (sc1) stores, waits for them, stores the
// launch's generation into the chunk's flag and adds 1 to every replica of the
// segment's done counter.  Readers either wait for the done counter (the whole
// segment, then its N verdict), or -- equal-window segments -- count a window
// as soon as the chunks its fetches touch are flagged and lie in the N-free
// prefix (stage_gate).  No acquire: the copied lines were not in any L2 at
// launch start and are touched by no one before their flag says so (a fetch
// never reaches past the chunks checked for it, and 128-B lines never straddle
// chunks), so the readers' plain loads fetch them fresh (the hand-off form of
// MI355X_MICROARCH.md's visibility section).  Every wait is bounded
// (AC_STAGE_TIMEOUT_TICKS): a host that never flags makes the waves report
// AC_DEVERR_STAGE and skip, never hang.  (The chunk count covers the region's
// largest layout, N bitmap included, so the last chunk always waits for the
// final header: once the done counter is complete, the verdict words are written.)
struct StageWords {
    uint32_t* claim;
    uint32_t* verdict;  // ~0u: skip; else 1 = has N
    uint32_t* bytes;
    uint32_t* fin;      // 1 once verdict / bytes are written
    uint32_t* avail;    // N-free bytes of the region published so far: AC_STAGE_REPL replicas, one per line
    uint32_t* done;     // chunks copied: AC_STAGE_REPL replicas, one per line
};
__device__ __forceinline__ StageWords stage_words(uint32_t* words) {
    // (one word per line: a launch zeroes only word 0 of each line of the next launch's bank)
    return StageWords{words, words + AC_QUEUE_LINE, words + 2 * AC_QUEUE_LINE, words + 3 * AC_QUEUE_LINE,
                      words + 4 * AC_QUEUE_LINE, words + (4 + AC_STAGE_REPL) * AC_QUEUE_LINE};
}
// per chunk flag: one line each (a chunk's readers poll only its own line)
__device__ __forceinline__ uint32_t* chunk_flag(uint32_t* chunk_gen, uint32_t x) { return chunk_gen + x * AC_QUEUE_LINE; }
__device__ __forceinline__ const uint32_t* chunk_flag(const uint32_t* chunk_gen, uint32_t x) {
    return chunk_gen + x * AC_QUEUE_LINE;
}
__device__ __forceinline__ uint32_t wave_load(const uint32_t* p) {  // lane 0's agent-scope load, wave-uniform
    uint32_t v = 0;
    if ((threadIdx.x & 63u) == 0) v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ void wave_store(uint32_t* p, uint32_t v) {
    if ((threadIdx.x & 63u) == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// A staged wait's bound: AC_STAGE_TIMEOUT_TICKS without progress.  The clock is read lazily -- only on
// a poll that saw no progress (the first such poll starts it), and progress() stops it -- so a wait
// that never stalls, e.g. a chunk copy whose chunk is already packed, reads no clock at all.
struct StageClock {
    uint64_t t0 = 0;
    __device__ __forceinline__ void progress() { t0 = 0; }
    __device__ __forceinline__ bool late() {
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        if (t0 == 0) {
            t0 = now;
            return false;
        }
        return now - t0 > AC_STAGE_TIMEOUT_TICKS;
    }
};

// The two steps the copier loops (stage_copy, stage_copy_dp) share.  (Not their copy-ahead waits: as a helper
// the wait cost the staged k <= 10 kernels VGPR spills around the inlined stage_copy_dp, profiles/r09_frame_codegen.txt.)
// The chunk at byte `lo` of a region whose first `limit` bytes are valid: 64 lanes x 4 x 16 bytes,
// through range-checked descriptors (bytes past the valid prefix read as 0 and are not stored).
__device__ __forceinline__ void copy_chunk(const uint8_t* src, uint8_t* dst, uint32_t limit, uint32_t lo, uint32_t lane) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)limit, 0x00020000);
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)dst, 0, (int)limit, 0x00020000);
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    v4u v[4];
    const uint32_t o = lo + lane * 16u;
#pragma unroll
    // (nontemporal, like the copy kernel's loads of the same pinned block: nothing read these
    // lines before the flag in this launch, so no cache holds them; system-scope loads
    // were split into narrow PCIe reads: 330 KB took ~15 us instead of ~6)
    for (int u = 0; u < 4; ++u) v[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, o + u * 1024u, 0, AC_STAGE_LOAD_AUX);
#pragma unroll
    for (int u = 0; u < 4; ++u) __builtin_amdgcn_raw_buffer_store_b128(v[u], rd, o + u * 1024u, 0, 16);  // sc1
}
// Chunk x is in (its stores waited for): its flag takes the launch's generation and every replica of
// the segment's done counter one more; the count before this chunk (lanes < AC_STAGE_REPL).
__device__ __forceinline__ uint32_t publish_chunk(StageWords sw, uint32_t* chunk_gen, uint32_t x, uint32_t gen, uint32_t lane) {
    wave_store(chunk_flag(chunk_gen, x), gen);
    uint32_t prev = 0;
    if (lane < AC_STAGE_REPL)
        prev = __hip_atomic_fetch_add(sw.done + lane * AC_QUEUE_LINE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return prev;
}

#ifndef AC_PACK_BLOCKS
#define AC_PACK_BLOCKS 4  // 32-base blocks whose host loads a packing lane keeps in flight at once
#endif
// 4 Dna5 bytes (one per base, ordinal 0-3 = A C G T, anything else N) -> the byte of their four
// 2-bit codes (base i at bits 2i..2i+1) and, in `n`, bit i set iff base i is N.
__device__ __forceinline__ uint32_t dna5_codes4(uint32_t x) {
    uint32_t c = x & 0x03030303u;
    c = (c | (c >> 6)) & 0x000f000fu;  // bases 0-1 at bits 0-3, bases 2-3 at bits 16-19
    return (c | (c >> 12)) & 0xffu;
}
__device__ __forceinline__ uint32_t dna5_n4(uint32_t x) {
    const uint32_t t = x & 0xfcfcfcfcu;                                  // nonzero byte <=> ordinal >= 4
    const uint32_t nz = (((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u;  // bit 7 of each such byte
    return (((nz >> 7) * 0x00204081u) >> 21) & 0xfu;                    // bits 7, 15, 23, 31 -> 0..3
}

// Device packing (DESIGN.md §4d) of codes chunk `lo_b` (byte offset in the codes section) of an
// equal-window segment: the windows whose slots overlap the chunk are read as Dna5 bytes from
// pinned host memory (offset of window w at offs[w], relative to src; src_bytes readable), one
// window per lane, and packed exactly as the host packer does (host_pack.cpp pack_dna5_range with
// records): 2-bit codes, padding bases code 0, the window's inline N record (nrec.h) in the top bits
// of its slot's last code word when the segment has records (rec), and its N-bitmap words.  Only
// the code words inside the chunk are stored (a slot that straddles two chunks is packed by both
// owners, each storing its own words), with write-through stores like the copy; the N-bitmap words
// of the chunk's blocks go to the bitmap section (read only by a window whose record overflowed, or
// by every window of a segment without records, and then only once the whole segment is in).
// A window outside src_bytes is stored as zeros and reported (AC_DEVERR_WINDOW).
// Each PCIe round trip costs ~2 us: a lane has its next windows' offsets in flight while it packs,
// and all of a window's loads (AC_PACK_BLOCKS blocks of 32 bases) in flight together.
struct PackOut {
    uint32_t cnt = 0, pos = 0, last_lo = 0, last_hi = 0;
};
struct PackCtx {
    __amdgpu_buffer_rsrc_t rc, rn;
    uint32_t ulen, nblk, SW, cw_lo, cw_hi, cap, pb;
};
typedef uint32_t pk_v2u __attribute__((ext_vector_type(2)));
typedef uint32_t pk_v4u __attribute__((ext_vector_type(4)));
// One 32-base block b of a window from its 9 loaded dwords (the 32 bytes from byte `sh` of the first).
__device__ __forceinline__ void pack_block(const PackCtx& pc, const pk_v4u& d0, const pk_v4u& d1, uint32_t e, uint32_t b,
                                           bool ok, uint32_t sh, uint32_t cw_w, PackOut& o) {
    const uint32_t raw[9] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w, e};
    const uint32_t nv = ok ? min(32u, pc.ulen - 32u * b) : 0u;  // real bases of the block
    uint32_t code0 = 0, code1 = 0, nmw = 0;
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q) {
        uint32_t x = (uint32_t)((((uint64_t)raw[q + 1] << 32) | raw[q]) >> (8u * sh));
        const uint32_t have = nv > 4u * q ? nv - 4u * q : 0u;  // bytes of this dword that are bases
        x = have >= 4u ? x : (have ? x & ((1u << (8u * have)) - 1u) : 0u);
        if (q < 4) code0 |= dna5_codes4(x) << (8u * q);
        else code1 |= dna5_codes4(x) << (8u * (q - 4u));
        nmw |= dna5_n4(x) << (4u * q);
    }
    for (uint32_t m = nmw; m; m &= m - 1u) {  // the record's N positions, in window order
        if (o.cnt < pc.cap) o.pos |= (32u * b + (uint32_t)__builtin_ctz(m)) << nrec_pos_shift(pc.pb, o.cnt);
        ++o.cnt;
    }
    const uint32_t cw = cw_w + 2u * b;
    const bool mine = cw >= pc.cw_lo && cw < pc.cw_hi;  // (a block never straddles a chunk)
    if (b + 1u == pc.nblk) {  // the slot's last block: its second word takes the record
        o.last_lo = code0;
        o.last_hi = code1;
    } else if (mine) {
        __builtin_amdgcn_raw_buffer_store_b64(pk_v2u{code0, code1}, pc.rc, cw * 4u, 0, 16);  // sc1
    }
    if (mine) __builtin_amdgcn_raw_buffer_store_b32(nmw, pc.rn, cw * 2u, 0, 16);
}
__device__ __forceinline__ void pack_finish(const PackCtx& pc, uint32_t rec, uint32_t cw_w, PackOut& o) {
    if (rec && o.cnt) o.last_hi |= o.cnt <= pc.cap ? (o.pos | o.cnt << 29) : (NREC_OVERFLOW << 29);
    const uint32_t cw = cw_w + pc.SW - 2u;
    if (cw >= pc.cw_lo && cw < pc.cw_hi)
        __builtin_amdgcn_raw_buffer_store_b64(pk_v2u{o.last_lo, o.last_hi}, pc.rc, cw * 4u, 0, 16);
}

__device__ __forceinline__ void stage_pack_chunk(const uint8_t* src, const uint64_t* offs, uint32_t src_bytes,
                                                 uint32_t n_windows, uint32_t ulen, uint32_t rec, uint32_t code_bytes,
                                                 uint8_t* codes_dst, uint8_t* nmask_dst, uint32_t lo_b, uint32_t* err) {
    const uint32_t lane = threadIdx.x & 63u;
    PackCtx pc;
    pc.ulen = ulen;
    pc.SW = ((ulen + 31u) & ~31u) / 16u;  // code words per slot (2..16)
    pc.nblk = pc.SW / 2u;                 // 32-base blocks per slot, each holding real bases
    const uint32_t hi_b = min(lo_b + AC_STAGE_CHUNK, code_bytes);
    pc.cw_lo = lo_b / 4u;
    pc.cw_hi = hi_b / 4u;  // the chunk's code words
    pc.cap = nrec_cap(ulen);
    pc.pb = nrec_pos_bits(ulen);
    const uint32_t w0 = pc.cw_lo / pc.SW, w1 = min(n_windows, (pc.cw_hi + pc.SW - 1u) / pc.SW);
    // (the range check is per dword: a dword that holds the block's last bytes and reaches past them
    // would read as zero and the last window lose up to 3 bases, so the range ends at the next 4-byte
    // boundary of the block -- ac_host_alloc allocates up to there; the bytes past a window are masked)
    const uint32_t mis = (uint32_t)(uintptr_t)src & 3u;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)(((src_bytes + mis + 3u) & ~3u) - mis), 0x00020000);
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)offs, 0, (int)(n_windows * 8u), 0x00020000);
    pc.rc = __builtin_amdgcn_make_buffer_rsrc((void*)codes_dst, 0, (int)code_bytes, 0x00020000);
    pc.rn = __builtin_amdgcn_make_buffer_rsrc((void*)nmask_dst, 0, (int)(code_bytes / 2u), 0x00020000);
    uint32_t bad = 0;
    // The offsets of the lane's first two windows in one round trip (a chunk holds <= 128 slots of
    // >= 128 bases, 2 rounds of 64; shorter slots take more rounds, their offsets loaded per round).
    pk_v2u onext = w0 + lane < w1 ? __builtin_amdgcn_raw_buffer_load_b64(ro, (w0 + lane) * 8u, 0, 0) : pk_v2u{0u, 0u};
    pk_v2u onext2 = w0 + lane + 64u < w1 ? __builtin_amdgcn_raw_buffer_load_b64(ro, (w0 + lane + 64u) * 8u, 0, 0)
                                          : pk_v2u{0u, 0u};
    constexpr uint32_t PB = AC_PACK_BLOCKS;  // blocks per pass: their loads in flight together
    for (uint32_t w = w0 + lane; w < w1; w += 64u) {
        const pk_v2u ov = onext;
        onext = onext2;
        if (w + 128u < w1) onext2 = __builtin_amdgcn_raw_buffer_load_b64(ro, (w + 128u) * 8u, 0, 0);
        const bool ok = ov.y == 0u && ov.x <= src_bytes - ulen;  // (the host checked src_bytes >= ulen)
        bad |= ok ? 0u : 1u;
        const uint32_t off = ok ? ov.x : 0u, a = off & ~3u, sh = off & 3u;  // out of range: read as zeros
        PackOut o;
#pragma unroll 1
        for (uint32_t b0 = 0; b0 < pc.nblk; b0 += PB) {
            pk_v4u d[PB][2];
            uint32_t e[PB];
#pragma unroll
            for (uint32_t i = 0; i < PB; ++i)
                if (b0 + i < pc.nblk) {
                    const uint32_t x = a + 32u * (b0 + i);
                    d[i][0] = __builtin_amdgcn_raw_buffer_load_b128(rs, x, 0, 0);
                    d[i][1] = __builtin_amdgcn_raw_buffer_load_b128(rs, x + 16u, 0, 0);
                    e[i] = __builtin_amdgcn_raw_buffer_load_b32(rs, x + 32u, 0, 0);
                }
#pragma unroll
            for (uint32_t i = 0; i < PB; ++i)
                if (b0 + i < pc.nblk) pack_block(pc, d[i][0], d[i][1], e[i], b0 + i, ok, sh, w * pc.SW, o);
        }
        pack_finish(pc, rec, w * pc.SW, o);
    }
    if (__ballot(bad != 0u) && lane == 0) atomicOr(err, AC_DEVERR_WINDOW);
}

// Claims and serves tickets until none is left; false on timeout.  Chunks below `pre_chunks` (the
// k-mer section, in place in the pinned block before the launch) are copied without waiting.
__device__ __attribute__((noinline)) bool stage_copy(const uint8_t* src, uint8_t* dst, uint32_t chunks,
                                                     uint32_t pre_chunks, uint32_t* hdr, uint32_t* words,
                                                     uint32_t* chunk_gen, uint32_t gen, uint32_t si) {
    const uint32_t lane = threadIdx.x & 63u;
    const StageWords sw = stage_words(words);
    StageClock clk;
    for (;;) {
        uint32_t c = 0;
        if (lane == 0) c = __hip_atomic_fetch_add(sw.claim, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        c = __builtin_amdgcn_readfirstlane(c);
        if (c > chunks) return true;
        clk.progress();  // (each ticket's wait is bounded on its own)
        if (c == 0) {  // the segment's host poller
            // The header's four words in ONE 16-byte system-scope load (one PCIe read): the host
            // stores the progress record as one 8-byte store and the flag after INFO, so a read
            // that returns the flag returns the INFO stored before it.
            typedef uint32_t v4u __attribute__((ext_vector_type(4)));
            static_assert(AC_HDR_PGEN == 0 && AC_HDR_READY == 1 && AC_HDR_FLAG == 2 && AC_HDR_INFO == 3,
                          "header layout");
            const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc((void*)hdr, 0, 16, 0x00020000);
            uint32_t published = 0;
            for (;;) {
                const v4u hv = __builtin_amdgcn_raw_buffer_load_b128(rh, 0, 0, 17);  // sc0 sc1: system scope
                uint32_t ready = __builtin_amdgcn_readfirstlane(hv.x) == gen ? __builtin_amdgcn_readfirstlane(hv.y) : 0u;
                const bool fin = __builtin_amdgcn_readfirstlane(hv.z) == gen;
                uint32_t verdict = 0, bytes = 0;
                if (fin) {
                    const uint32_t info = __builtin_amdgcn_readfirstlane(hv.w);
                    bytes = info & ~AC_HDR_INFO_HAS_N;
                    verdict = (info == AC_HDR_INFO_ABORT || bytes > chunks * AC_STAGE_CHUNK || ready > bytes)
                                  ? ~0u
                                  : (info & AC_HDR_INFO_HAS_N ? 1u : 0u);
                    if (verdict == 0u) ready = bytes;  // no N anywhere: the whole region is N-free
                    // the final words before the prefix they complete: a copier released by the prefix can
                    // finish the segment's last chunk, and a reader that then sees the done count complete
                    // reads the verdict (so it must be there first)
                    wave_store(sw.verdict, verdict);
                    wave_store(sw.bytes, verdict == ~0u ? 0u : bytes);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                if (verdict != ~0u && ready > published && ready <= chunks * AC_STAGE_CHUNK) {
                    if (published == 0) stage_stamp(si, 1);
                    if (published <= pre_chunks * AC_STAGE_CHUNK && ready > pre_chunks * AC_STAGE_CHUNK) stage_stamp(si, 3);
                    if (lane < AC_STAGE_REPL)  // every replica in one wave instruction
                        __hip_atomic_store(sw.avail + lane * AC_QUEUE_LINE, ready, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                    published = ready;
                    clk.progress();  // the host is making progress
                }
                if (fin) {
                    stage_stamp(si, 0);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    wave_store(sw.fin, 1u);
                    break;
                }
                if (clk.late()) return false;
                __builtin_amdgcn_s_sleep(8);
            }
            continue;
        }
        // copier of chunk c - 1: wait until it lies inside the N-free prefix or the segment is final
        const uint32_t x = c - 1u, lo = x * AC_STAGE_CHUNK, hi = lo + AC_STAGE_CHUNK;
        uint32_t* my_avail = sw.avail + (x % AC_STAGE_REPL) * AC_QUEUE_LINE;
        uint32_t limit = x < pre_chunks ? hi : 0u;  // bytes of the region known to be valid
        uint32_t seen = 0;  // N-free bytes seen published (the wait's clock restarts when they grow)
        while (limit == 0u) {
            // both words in one wave instruction (lane 0: N-free bytes, lane 1: final seen)
            uint32_t v = 0;
            if (lane < 2u) v = __hip_atomic_load(lane ? sw.fin : my_avail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t av = __builtin_amdgcn_readlane(v, 0);
            if (av >= hi) {
                limit = hi;
                break;
            }
            if (__builtin_amdgcn_readlane(v, 1)) {
                limit = wave_load(sw.verdict) == ~0u ? 0u : wave_load(sw.bytes);
                break;
            }
            if (av > seen) {
                seen = av;
                clk.progress();
            } else if (clk.late()) {
                return false;
            }
            __builtin_amdgcn_s_sleep(8);
        }
#if AC_COPY_AHEAD
        // In chunk order: at most AC_COPY_AHEAD chunks of the segment in flight ahead of the copied
        // count, so the first windows' chunks are not held up behind the whole region's PCIe reads
        // (a segment packed before the poller's first look released all its copiers at once and the
        // first codes chunk landed anywhere in the next 5-18 us: profiles/r03_m9/stamps.log).
        if (x >= AC_COPY_AHEAD) {
            uint32_t* my_done = sw.done + (x % AC_STAGE_REPL) * AC_QUEUE_LINE;
            uint32_t dn = 0, dseen = 0;
            clk.progress();
            while ((dn = wave_load(my_done)) < x - AC_COPY_AHEAD) {
                if (dn > dseen) {  // (the copies ahead of it are moving)
                    dseen = dn;
                    clk.progress();
                } else if (clk.late()) {
                    return false;
                }
                __builtin_amdgcn_s_sleep(2);
            }
        }
#endif
        if (limit > lo) copy_chunk(src, dst, limit, lo, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t prev = publish_chunk(sw, chunk_gen, x, gen, lane);
        if (__builtin_amdgcn_readfirstlane(prev) + 1u == chunks) stage_stamp(si, 2);  // (diagnostic builds) last chunk in
        if (x == pre_chunks) stage_stamp(si, 4);  // (diagnostic builds) first codes chunk in
    }
}

// The copier loop of a device-packed segment (DESIGN.md §4d): the host published nothing and packs
// nothing -- its Dna5 bytes sit in pinned memory from before the launch -- so ticket 0 publishes the
// segment's final words at once (no header read over PCIe): the verdict (1: the N bitmap is there for
// the windows that need it), the byte count, the whole region as available (with inline N records;
// without them only the k-mers, so readers wait for the whole segment and its bitmap) and `fin`.
// Tickets c >= 1: k-mer chunks are copied from the staging block, codes chunks packed from the Dna5
// bytes (stage_pack_chunk), N-bitmap chunks have no work of their own (their words are stored by the
// codes chunks' owners); then, as in stage_copy, the chunk's flag and the done replicas -- only once
// `fin` is out, so a reader that sees the segment complete reads its verdict.  Inlined into the
// kernel: as a called function its registers came from the budget of the 8-wave kernels (64 VGPRs)
// and it spilled inside the packing loop.
__device__ __forceinline__ bool stage_copy_dp(const SegDev& sg, uint32_t* words, uint32_t gen, uint32_t* err) {
    const uint32_t lane = threadIdx.x & 63u;
    const StageWords sw = stage_words(words);
    const uint32_t chunks = sg.stage_chunks, pre_chunks = sg.stage_codes_off / AC_STAGE_CHUNK;
    const uint32_t code_bytes = (uint32_t)(sg.n_bases >> 2);
    const uint32_t nmask_off = pre_chunks * AC_STAGE_CHUNK + ((code_bytes + 255u) & ~255u);  // (256-B aligned sections)
    StageClock clk;
    bool fin_seen = false;
    for (;;) {
        uint32_t c = 0;
        if (lane == 0) c = __hip_atomic_fetch_add(sw.claim, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        c = __builtin_amdgcn_readfirstlane(c);
        if (c > chunks) return true;
        clk.progress();
        if (c == 0) {
            const uint32_t bytes = chunks * AC_STAGE_CHUNK;  // (the host sized the region: codes + bitmap)
            wave_store(sw.verdict, 1u);
            wave_store(sw.bytes, bytes);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane < AC_STAGE_REPL)
                __hip_atomic_store(sw.avail + lane * AC_QUEUE_LINE, sg.nrec ? bytes : sg.stage_codes_off,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            wave_store(sw.fin, 1u);
            continue;
        }
        const uint32_t x = c - 1u, lo = x * AC_STAGE_CHUNK;
#if AC_COPY_AHEAD
        if (x >= AC_COPY_AHEAD) {  // in chunk order, as stage_copy
            uint32_t* my_done = sw.done + (x % AC_STAGE_REPL) * AC_QUEUE_LINE;
            uint32_t dn = 0, dseen = 0;
            while ((dn = wave_load(my_done)) < x - AC_COPY_AHEAD) {
                if (dn > dseen) {
                    dseen = dn;
                    clk.progress();
                } else if (clk.late()) {
                    return false;
                }
                __builtin_amdgcn_s_sleep(2);
            }
        }
#endif
        if (x < pre_chunks) {  // k-mers: in the pinned staging block since before the launch
            copy_chunk(sg.stage_src, sg.stage_dst, pre_chunks * AC_STAGE_CHUNK, lo, lane);
        } else if (lo - pre_chunks * AC_STAGE_CHUNK < code_bytes) {
            stage_pack_chunk(sg.dp_src, sg.dp_off, sg.dp_src_bytes, sg.n_windows, sg.ulen, sg.nrec, code_bytes,
                             sg.stage_dst + pre_chunks * AC_STAGE_CHUNK, sg.stage_dst + nmask_off,
                             lo - pre_chunks * AC_STAGE_CHUNK, err);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        while (!fin_seen) {  // (ticket 0's words out before the first chunk counts as done)
            fin_seen = wave_load(sw.fin) != 0u;
            if (!fin_seen) {
                if (clk.late()) return false;
                __builtin_amdgcn_s_sleep(2);
            }
        }
        publish_chunk(sw, sg.stage_gen, x, gen, lane);
    }
}

// Waits for the whole segment (every chunk copied): its N verdict (0 / 1), or ~0u to skip it.
__device__ __attribute__((noinline)) uint32_t stage_wait_all(uint32_t* words, uint32_t chunks, uint32_t replica,
                                                             uint32_t* err) {
    const StageWords sw = stage_words(words);
    StageClock clk;
    uint32_t dn = 0, seen = 0;
    while ((dn = wave_load(sw.done + replica * AC_QUEUE_LINE)) < chunks) {
        if (dn > seen) {  // copies are landing: the wait's clock restarts
            seen = dn;
            clk.progress();
        } else if (clk.late()) {
            if ((threadIdx.x & 63u) == 0) atomicOr(err, AC_DEVERR_STAGE);
            return ~0u;
        }
        __builtin_amdgcn_s_sleep(16);
    }
    // No acquire fence: it would only invalidate this CU's L1, and no CU can hold a line of the
    // region (nothing reads it before the counter says it is complete, and a launch starts with
    // clean caches).  With 8 workgroups per CU the fences cost ~8 us of staging per call (an A/B:
    // profiles/r03_m1/summary.log; -DAC_STAGE_ACQUIRE builds restore it).  Stale-line hazards are
    // what tests/test_gpu_jobs.py::test_early_launch_rotating_inputs_bit_exact rotates data for.
#ifdef AC_STAGE_ACQUIRE
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    return wave_load(sw.verdict);
}

#ifndef AC_GATE_SLEEP
#define AC_GATE_SLEEP 12  // s_sleep units (64 clocks) between a gate's polls
#endif
// Early counting: waits until region bytes [r0, r1) are in device memory (their chunks flagged)
// and inside the N-free prefix, or until the whole segment is in.  Low word: 2 for "count it
// with an all-zero N bitmap" (high word: the byte where the checked chunks' N-free part ends, at
// least r1), the
// segment's verdict (0 / 1) once it is complete, ~0u to skip (timeout: error bit set).
__device__ __forceinline__ uint64_t stage_gate(uint32_t* words, const uint32_t* chunk_gen, uint32_t chunks,
                                                         uint32_t replica, uint32_t gen, uint32_t r0, uint32_t r1,
                                                         uint32_t* err, uint32_t pre = 0u) {
    const uint32_t lane = threadIdx.x & 63u;
    const StageWords sw = stage_words(words);
    StageClock clk;
    const uint32_t x0 = r0 / AC_STAGE_CHUNK, x1 = (r1 - 1u) / AC_STAGE_CHUNK;
    // (more chunks than lanes, or past the launch's chunks: wait for the whole segment)
    const uint32_t nx = (x1 < chunks && x1 - x0 < 62u) ? x1 - x0 + 1u : 0u;
    bool in_prefix = nx && r1 <= pre;  // the N-free prefix covers [r0, r1) (it only grows; `pre`: at launch)
    uint32_t seen = 0;  // done + N-free bytes last seen (the wait's clock restarts when they move)
    for (;;) {
        // one wave instruction: lane 0 the done count, lane 1 the N-free bytes (this workgroup's
        // replicas), lanes 2.. the chunks' flags once the prefix covers them
        const uint32_t* p = lane == 0u ? sw.done + replica * AC_QUEUE_LINE
                          : lane == 1u ? sw.avail + replica * AC_QUEUE_LINE
                                       : (in_prefix && lane - 2u < nx ? chunk_flag(chunk_gen, x0 + (lane - 2u)) : nullptr);
        uint32_t v = 0;
        if (p) v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t dn = __builtin_amdgcn_readlane(v, 0), av = __builtin_amdgcn_readlane(v, 1);
        if (dn >= chunks) return wave_load(sw.verdict);
        const uint64_t miss = __ballot(lane >= 2u && lane - 2u < nx && v != gen);
        if (in_prefix && miss == 0) {
            // the chunks checked, up to where the N-free prefix ends: once the final header is out a
            // flagged chunk may reach past it, and its bytes there can hold N
            const uint32_t lim = av > pre ? av : pre, hi = (x1 + 1u) * AC_STAGE_CHUNK;
            return ((uint64_t)(hi < lim ? hi : lim) << 32) | 2u;
        }
        in_prefix = nx && (r1 <= pre || av >= r1);
        if (dn + av != seen) {
            seen = dn + av;
            clk.progress();
        } else if (clk.late()) {
            if (lane == 0) atomicOr(err, AC_DEVERR_STAGE);
            return ~0u;
        }
        if (!in_prefix) __builtin_amdgcn_s_sleep(AC_GATE_SLEEP);
    }
}
