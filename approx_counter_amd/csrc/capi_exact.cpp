// capi_exact.cpp -- sample upload and the exact count of the C ABI (kernels: exact_count.hip).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "exact_count.h"

using namespace ac_detail;

namespace {

// getComplexity (approx_counter.cpp:247-267) and CompareCount (275-305), for the
// final ranking of the exact count's short list.
float complexity(uint64_t kmer, uint32_t k) {
    uint64_t counts[16] = {0};
    for (uint32_t i = 0; i + 1 < k; ++i) {
        counts[kmer & 15u]++;
        kmer >>= 2;
    }
    size_t sum = 0;
    for (uint64_t v : counts) sum += v * (v - 1);
    return (float)sum / float(2 * ((int)k - 2));
}

}  // namespace

extern "C" {

ac_status ac_sample_upload_slot(ac_ctx* ctx, int slot, const ac_windows* host, ac_windows* dev) {
    if (!ctx || !dev) return fail(ctx, AC_ERR_INVALID, "ctx or dev is NULL");
    if (slot < 0 || slot >= AC_MAX_JOBS) return fail(ctx, AC_ERR_INVALID, "upload slot outside [0, AC_MAX_JOBS)");
    if (ac_status st = check_sample(ctx, host)) return st;
    if (ac_status st = check_layout(ctx, *host)) return st;  // on the host copy
    AC_HIP(ctx, hipSetDevice(ctx->device));
    // the slot's notes describe its image only once the upload below has completed (a
    // failure part way must not leave notes that a later count matches to a freed or partial buffer)
    ctx->s_codes[slot] = nullptr;
    ctx->s_start[slot] = nullptr;
    ctx->s_ulen[slot] = AC_NO_ULEN;
    ctx->s_no_n[slot] = false;
    const size_t sz[4] = {sizeof(uint32_t) * (host->n_bases / 16), sizeof(uint32_t) * (host->n_bases / 32),
                          sizeof(uint64_t) * host->n_windows, sizeof(uint32_t) * host->n_windows};
    const void* src[4] = {host->codes, host->nmask, host->start, host->length};
    // one device block (s_buf[slot]) holding the four arrays at the staging offsets
    if (ac_status st = grow(ctx, &ctx->s_buf[slot], &ctx->s_cap[slot], staged_bytes(4, sz))) return st;
    if (ac_status st = h2d_staged(ctx, 4, src, sz, ctx->s_buf[slot])) return st;
    AC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const char* blk = (const char*)ctx->s_buf[slot];
    size_t off = 0;
    const void* at[4];
    for (int i = 0; i < 4; ++i) {
        at[i] = blk + off;
        off += (sz[i] + 255) / 256 * 256;
    }
    dev->codes = (const uint32_t*)at[0];
    dev->nmask = (const uint32_t*)at[1];
    dev->start = (const uint64_t*)at[2];
    dev->length = (const uint32_t*)at[3];
    dev->n_windows = host->n_windows;
    dev->n_bases = host->n_bases;
    // equal windows back to back at ceil32(length) strides (the CLI's samples: every start window
    // sl bases, every end window sl + 1), and an N-free image
    uint32_t ulen = host->n_windows ? host->length[0] : AC_NO_ULEN;
    const uint64_t stride = ((uint64_t)ulen + 31u) & ~31ull;
    for (uint32_t i = 0; i < host->n_windows && ulen != AC_NO_ULEN; ++i)
        if (host->length[i] != ulen || host->start[i] != (uint64_t)i * stride) ulen = AC_NO_ULEN;
    uint32_t any_n = 0;
    for (uint64_t i = 0; i < host->n_bases / 32; ++i) any_n |= host->nmask[i];
    ctx->s_codes[slot] = dev->codes;
    ctx->s_start[slot] = dev->start;
    ctx->s_ulen[slot] = ulen;
    ctx->s_no_n[slot] = any_n == 0u;
    ctx->s_windows[slot] = host->n_windows;
    ctx->s_bases[slot] = host->n_bases;
    return AC_OK;
}

ac_status ac_sample_upload(ac_ctx* ctx, const ac_windows* host, ac_windows* dev) {
    return ac_sample_upload_slot(ctx, 0, host, dev);
}

ac_status ac_exact_count_device(ac_ctx* ctx, uint32_t k, const ac_windows* dev, float lc_threshold,
                                const uint64_t* forbidden, uint32_t n_forbidden, uint64_t limit, uint64_t solid,
                                uint64_t* kmers_out, uint64_t* counts_out, uint64_t capacity, uint64_t* n_out,
                                uint64_t* n_distinct, uint64_t* had_n) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (ac_status st = check_k(ctx, k)) return st;
    if (ac_status st = check_sample(ctx, dev)) return st;
    if (!n_out || (capacity && (!kmers_out || !counts_out)) || (n_forbidden && !forbidden))
        return fail(ctx, AC_ERR_INVALID, "NULL output or forbidden array");
    AC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // The partitioned path (exact_count.hip: dense keys -- 32-bit for k <= 16, 64-bit above --,
    // bucket partition, per-bucket LDS count; no global table); a sample too large for it, or
    // a bucket that outgrows its LDS table, takes the hash-table path.  AC_EXACT_HASH=1 forces
    // the hash table (A/B; tests/test_gpu_exact.py runs both).
    const bool compact = k <= acamd::EXACT_COMPACT_MAX_K;
    static const bool force_hash = std::getenv("AC_EXACT_HASH") != nullptr;
    bool partitioned = !force_hash;
    const size_t key_bytes = compact ? sizeof(uint32_t) : sizeof(uint64_t);
    // k-mer positions <= image bases: the capacity of the dense key arrays,
    // and of the list when every kept entry must be listed (threshold 1).
    const uint64_t key_cap = std::max<uint64_t>(32, dev->n_bases);
    // Up to 2^16 buckets of <= ~2,048 keys (the per-bucket LDS table holds 4,096; super-buckets
    // of at most 2^AC_SUB_LOG2 buckets, one LDS cursor each in the scatters): 134M positions, cfg4's 10^6 windows per
    // read end included; larger samples take the hash table.
    if (key_cap > (uint64_t(1) << (16 + 11))) partitioned = false;
    // Distinct kept k-mers <= image positions (a k-mer is fixed by its image position, whichever
    // overlapping windows cover it), so this list never overflows; n_bases / 2 (entries seen at
    // least twice, disjoint windows) did for duplicated windows.
    const uint64_t list_cap = key_cap + 2;
    // small block: special[0..1] u32, had_n u64 @16, n_out u64 @24, n_list u64 @32, err u32 @40,
    // overflow u32 @44, n_keys u64 @48, hist[EXACT_HIST_BINS] u32 @64
    const size_t small_bytes = 64 + sizeof(uint32_t) * EXACT_HIST_BINS;
    std::vector<uint64_t> fb(forbidden, forbidden + n_forbidden);
    std::vector<uint64_t> fbb;  // (the partitioned path: fb by bucket, and the bucket starts; host copies
    std::vector<uint32_t> fst;  // live until the call's syncs)
    std::sort(fb.begin(), fb.end());
    fb.erase(std::unique(fb.begin(), fb.end()), fb.end());
    if (ac_status s2 = grow(ctx, &ctx->e_buf[1], &ctx->e_cap[1], (sizeof(uint64_t) + sizeof(uint32_t)) * list_cap))
        return s2;
    if (ac_status s2 = grow(ctx, &ctx->e_buf[2], &ctx->e_cap[2], small_bytes)) return s2;
    if (ac_status s2 = grow(ctx, &ctx->e_buf[3], &ctx->e_cap[3], sizeof(uint64_t) * std::max<size_t>(1, fb.size())))
        return s2;
    if (!fb.empty())
        AC_HIP(ctx, hipMemcpyAsync(ctx->e_buf[3], fb.data(), sizeof(uint64_t) * fb.size(), hipMemcpyHostToDevice, st));
    char* small = (char*)ctx->e_buf[2];
    acamd::ExactArgs a;
    std::memset(&a, 0, sizeof a);
    a.codes = dev->codes;
    a.nmask = dev->nmask;
    a.start = dev->start;
    a.length = dev->length;
    a.n_bases = dev->n_bases;
    a.n_windows = dev->n_windows;
    a.k = k;
    a.compact = compact ? 1u : 0u;
    a.special = (uint32_t*)small;
    a.had_n = (unsigned long long*)(small + 16);
    a.n_out = (unsigned long long*)(small + 24);
    a.n_list = (unsigned long long*)(small + 32);
    a.err = (uint32_t*)(small + 40);
    a.overflow = (uint32_t*)(small + 44);
    a.n_keys = (unsigned long long*)(small + 48);
    a.hist = (uint32_t*)(small + 64);
    a.list_keys = (uint64_t*)ctx->e_buf[1];
    a.list_cnts = (uint32_t*)((char*)ctx->e_buf[1] + sizeof(uint64_t) * list_cap);
    a.list_cap = list_cap;
    a.lc_threshold = lc_threshold;
    a.forbidden = (const uint64_t*)ctx->e_buf[3];
    a.n_forbidden = (uint32_t)fb.size();
    a.list_min = EXACT_LIST_MIN;
    // readbacks into the context's pinned block: [0, 32 KB) the small block and the list / gather counts,
    // then the gathered entries when they fit (else pageable vectors)
    constexpr size_t PIN_HEAD = 32768, PIN_MAX = size_t(16) << 20;
    static_assert(64 + sizeof(uint32_t) * EXACT_HIST_BINS + 16 <= PIN_HEAD, "small block fits the pinned head");
    if (!ctx->e_pin) {  // (allocated once at its full size: no pinned block freed or moved while a call runs)
        AC_HIP(ctx, hipHostMalloc((void**)&ctx->e_pin, PIN_HEAD + PIN_MAX, hipHostMallocDefault));
        ctx->e_pin_cap = PIN_HEAD + PIN_MAX;
    }
    char* h_small = ctx->e_pin;
    if (partitioned) {
        // buckets: about 1,024-2,048 keys each (the LDS table holds 4,096)
#ifndef AC_BUCKET_KEYS
#define AC_BUCKET_KEYS 2048  // (A/B builds: the bucket size target)
#endif
        uint32_t nb_log2 = 6;
        while (nb_log2 < 16 && (key_cap >> nb_log2) > AC_BUCKET_KEYS) ++nb_log2;
        a.nb_log2 = nb_log2;
        a.key_cap = key_cap;
        // super-buckets of <= 2^AC_SUB_LOG2 (128) buckets, at least 128 of them when there are that many buckets
        a.s_log2 = std::max(std::min(nb_log2, 7u), nb_log2 > AC_SUB_LOG2 ? nb_log2 - (uint32_t)AC_SUB_LOG2 : 0u);
        const uint32_t chunk = acamd::exact_part_chunk(k);
        a.n_chunks = (uint32_t)((key_cap + chunk - 1) / chunk);
        a.n_chunks2 = a.n_chunks + (1u << a.s_log2);
        const size_t NB = size_t(1) << nb_log2, S = size_t(1) << a.s_log2;
        const size_t h1 = S * a.n_chunks, h2 = (NB / S) * a.n_chunks2;
        if (ac_status s2 = grow(ctx, &ctx->e_buf[6], &ctx->e_cap[6], key_bytes * key_cap)) return s2;
        if (ac_status s2 = grow(ctx, &ctx->e_buf[7], &ctx->e_cap[7], key_bytes * key_cap)) return s2;
        if (ac_status s2 = grow(ctx, &ctx->e_buf[8], &ctx->e_cap[8], key_bytes * key_cap)) return s2;
        const size_t slabs = (a.n_chunks + EXACT_SCAN_SLAB - 1) / EXACT_SCAN_SLAB;
        if (ac_status s2 = grow(ctx, &ctx->e_buf[9], &ctx->e_cap[9], sizeof(uint32_t) * (h1 + h2 + S + slabs * S)))
            return s2;
        if (ac_status s2 = grow(ctx, &ctx->e_buf[10], &ctx->e_cap[10], sizeof(uint32_t) * (NB + 1))) return s2;
        if (ac_status s2 = grow(ctx, &ctx->e_buf[11], &ctx->e_cap[11], sizeof(uint32_t) * NB * EXACT_PHIST)) return s2;
        a.phist = (uint32_t*)ctx->e_buf[11];
        a.keys = ctx->e_buf[6];
        a.parts = ctx->e_buf[7];
        a.tmp = ctx->e_buf[8];
        a.h1 = (uint32_t*)ctx->e_buf[9];
        a.h2 = a.h1 + h1;
        a.stot = a.h2 + h2;
        a.slab = a.stot + S;
        a.bstart = (uint32_t*)ctx->e_buf[10];
        if (!fb.empty()) {  // the forbidden set by bucket: the count kernel searches only its bucket's entries
            std::vector<std::pair<uint32_t, uint64_t>> byb(fb.size());
            for (size_t i = 0; i < fb.size(); ++i)
                byb[i] = {compact ? acamd::bucket_of((uint32_t)fb[i], nb_log2) : acamd::bucket_of(fb[i], nb_log2), fb[i]};
            std::sort(byb.begin(), byb.end());
            fbb.assign(fb.size(), 0);
            fst.assign(NB + 1, 0);
            for (size_t i = 0; i < byb.size(); ++i) {
                fbb[i] = byb[i].second;
                ++fst[byb[i].first + 1];
            }
            for (size_t b = 0; b < NB; ++b) fst[b + 1] += fst[b];
            if (ac_status s2 = grow(ctx, &ctx->e_buf[12], &ctx->e_cap[12], sizeof(uint64_t) * fbb.size())) return s2;
            if (ac_status s2 = grow(ctx, &ctx->e_buf[13], &ctx->e_cap[13], sizeof(uint32_t) * (NB + 1))) return s2;
            AC_HIP(ctx, hipMemcpyAsync(ctx->e_buf[12], fbb.data(), sizeof(uint64_t) * fbb.size(), hipMemcpyHostToDevice, st));
            AC_HIP(ctx, hipMemcpyAsync(ctx->e_buf[13], fst.data(), sizeof(uint32_t) * (NB + 1), hipMemcpyHostToDevice, st));
            a.fb_bucketed = (const uint64_t*)ctx->e_buf[12];
            a.fb_start = (const uint32_t*)ctx->e_buf[13];
        }
        AC_HIP(ctx, hipMemsetAsync(small, 0, small_bytes, st));
        AC_HIP(ctx, acamd::launch_exact_partitioned(a, st));
        AC_HIP(ctx, hipMemcpyAsync(h_small, small, small_bytes, hipMemcpyDeviceToHost, st));
        AC_HIP(ctx, hipStreamSynchronize(st));
        if (*(const uint32_t*)(h_small + 44)) partitioned = false;  // a bucket overflowed its LDS table
        // Overlapping windows (allowed by ac_windows) hold more k-mer positions than the image
        // has bases: the dense key arrays dropped the excess, so count on the hash table instead
        // (its distinct keys are still bounded by the image's positions).
        if (*(const unsigned long long*)(h_small + 48) > key_cap) partitioned = false;
    }
    if (!partitioned) {
        // Table: a power of two >= 1.5 x the image size (an upper bound on k-mer
        // positions): load <= 2/3 even when every position is a new k-mer.  (1.25 x,
        // 2^24 slots at 10^5 windows: insert 530 -> 644 us from the longer probe
        // chains, scan 139 -> 104 us; profiles/r02_exact_log.md.)
        uint64_t slots = 1024;
        while (slots < dev->n_bases + dev->n_bases / 2) slots <<= 1;
        const size_t slot_bytes = compact ? sizeof(unsigned long long) : sizeof(acamd::ExactSlot);
        if (ac_status s2 = grow(ctx, &ctx->e_buf[0], &ctx->e_cap[0], slot_bytes * slots)) return s2;
        a.table = (acamd::ExactSlot*)ctx->e_buf[0];
        a.ctable = (unsigned long long*)ctx->e_buf[0];
        a.slots = slots;
        a.mask = slots - 1;
        AC_HIP(ctx, hipMemsetAsync(ctx->e_buf[0], 0, slot_bytes * slots, st));
        AC_HIP(ctx, hipMemsetAsync(small, 0, small_bytes, st));
        AC_HIP(ctx, acamd::launch_exact_insert(a, st));
        AC_HIP(ctx, acamd::launch_exact_scan(a, st));
        AC_HIP(ctx, hipMemcpyAsync(h_small, small, small_bytes, hipMemcpyDeviceToHost, st));
        AC_HIP(ctx, hipStreamSynchronize(st));
    }
    if (ac_status rc = device_error(ctx, *(const uint32_t*)(h_small + 40))) return rc;
    ctx->exact_path = partitioned ? 1 : 0;
    const uint32_t* hist = (const uint32_t*)(h_small + 64);
    uint64_t kept = 0;
    for (int i = 0; i < EXACT_HIST_BINS; ++i) kept += hist[i];
    if (n_distinct) *n_distinct = kept;
    if (had_n) *had_n = *(const unsigned long long*)(h_small + 16);
    uint64_t n_list = *(const unsigned long long*)(h_small + 32);
    if (n_list > list_cap) return fail(ctx, AC_ERR_INTERNAL, "exact count: candidate list overflow");
    // Threshold: solid mode keeps count >= solid; otherwise the largest count c
    // such that at least `limit` kept entries have count >= c (all if fewer).
    uint64_t thr = 1, due = kept;
    if (solid) {
        thr = solid;
        due = 0;
        for (uint64_t c = std::min<uint64_t>(solid, EXACT_HIST_BINS - 1); c < EXACT_HIST_BINS; ++c) due += hist[c];
    } else if (limit < kept) {
        uint64_t acc = 0;
        for (int c = EXACT_HIST_BINS - 1; c >= 1; --c) {
            acc += hist[c];
            if (acc >= limit) {
                thr = (uint64_t)c;
                due = acc;
                break;
            }
        }
    }
    bool from_list = thr >= EXACT_LIST_MIN;
    if (!from_list && partitioned) {
        // threshold 1: list every kept entry (the count kernel again, listing only)
        a.list_min = 1;
        a.emit_only = 1;
        AC_HIP(ctx, hipMemsetAsync(a.n_list, 0, sizeof(unsigned long long), st));
        AC_HIP(ctx, acamd::launch_exact_part_count(a, st));
        unsigned long long* nl = (unsigned long long*)(ctx->e_pin + PIN_HEAD - 16);
        AC_HIP(ctx, hipMemcpyAsync(nl, a.n_list, sizeof *nl, hipMemcpyDeviceToHost, st));
        AC_HIP(ctx, hipStreamSynchronize(st));
        n_list = *nl;
        if (n_list > list_cap) return fail(ctx, AC_ERR_INTERNAL, "exact count: candidate list overflow");
        from_list = true;
    }
    // (a solid threshold past the last bin is applied exactly on the gathered list)
    const uint64_t gather_cap = std::max<uint64_t>(1, due);
    if (ac_status s2 = grow(ctx, &ctx->e_buf[4], &ctx->e_cap[4], sizeof(uint64_t) * gather_cap)) return s2;
    if (ac_status s2 = grow(ctx, &ctx->e_buf[5], &ctx->e_cap[5], sizeof(uint32_t) * gather_cap)) return s2;
    a.threshold = (uint32_t)std::min<uint64_t>(thr, 0xffffffffu);
    a.out_keys = (uint64_t*)ctx->e_buf[4];
    a.out_cnts = (uint32_t*)ctx->e_buf[5];
    a.out_cap = gather_cap;
    AC_HIP(ctx, acamd::launch_exact_gather(a, from_list, n_list, st));
    // The gathered count is at most gather_cap (the histogram's due entries): with room in the pinned
    // block, the count and gather_cap entries come back in one synchronised batch of DMAs (the extra
    // entries, if any, are ignored); otherwise the count first, then exactly that many entries.
    unsigned long long* got_p = (unsigned long long*)(ctx->e_pin + PIN_HEAD - 8);
    const size_t entry_bytes = (sizeof(uint64_t) + sizeof(uint32_t)) * gather_cap;
    const bool pin_entries = entry_bytes <= PIN_MAX;
    uint64_t* gk_p = (uint64_t*)(ctx->e_pin + PIN_HEAD);
    uint32_t* gc_p = (uint32_t*)(ctx->e_pin + PIN_HEAD + sizeof(uint64_t) * gather_cap);
    std::vector<uint64_t> gk;
    std::vector<uint32_t> gc;
    AC_HIP(ctx, hipMemcpyAsync(got_p, a.n_out, sizeof *got_p, hipMemcpyDeviceToHost, st));
    if (pin_entries) {
        AC_HIP(ctx, hipMemcpyAsync(gk_p, a.out_keys, sizeof(uint64_t) * gather_cap, hipMemcpyDeviceToHost, st));
        AC_HIP(ctx, hipMemcpyAsync(gc_p, a.out_cnts, sizeof(uint32_t) * gather_cap, hipMemcpyDeviceToHost, st));
    }
    AC_HIP(ctx, hipStreamSynchronize(st));
    const unsigned long long got = *got_p;
    if (got > gather_cap) return fail(ctx, AC_ERR_INTERNAL, "exact count: gathered more entries than the histogram");
    if (!pin_entries && got) {
        gk.resize(got);
        gc.resize(got);
        AC_HIP(ctx, hipMemcpyAsync(gk.data(), a.out_keys, sizeof(uint64_t) * got, hipMemcpyDeviceToHost, st));
        AC_HIP(ctx, hipMemcpyAsync(gc.data(), a.out_cnts, sizeof(uint32_t) * got, hipMemcpyDeviceToHost, st));
        AC_HIP(ctx, hipStreamSynchronize(st));
        gk_p = gk.data();
        gc_p = gc.data();
    }
    // CompareCount (275-305): count descending, DUST score ascending, k-mer descending.  For k > 2 the
    // score is a non-negative float, so its bits order like it and the whole order is one 128-bit key
    // ((~count, score bits), ~k-mer) compared as two integers; the first n by nth_element, then sorted
    // (partial_sort with the three-field comparator was most of a cfg3 call's host time).  k = 2 (a
    // score of 0 / 0) keeps the comparator, whose NaN ties are the reference's.
    const size_t n_all = solid ? (size_t)std::count_if(gc_p, gc_p + got, [&](uint32_t c) { return c >= solid; })
                               : (size_t)got;
    const size_t n = solid ? n_all : std::min<size_t>(n_all, limit);
    *n_out = n;
    if (n > capacity) return fail(ctx, AC_ERR_INVALID, "exact count: capacity too small (n_out holds the size needed)");
    if (k > 2) {
        struct Key {
            uint64_t hi, lo;
        };
        std::vector<Key> w;
        w.reserve(n_all);
        for (uint64_t i = 0; i < got; ++i)
            if (!solid || gc_p[i] >= solid) {
                const float c = complexity(gk_p[i], k);
                uint32_t cb;
                std::memcpy(&cb, &c, sizeof cb);
                w.push_back({((uint64_t)(0xffffffffu - gc_p[i]) << 32) | cb, ~gk_p[i]});
            }
        auto kl = [](const Key& x, const Key& y) { return x.hi < y.hi || (x.hi == y.hi && x.lo < y.lo); };
        if (n < w.size()) std::nth_element(w.begin(), w.begin() + n, w.end(), kl);
        std::sort(w.begin(), w.begin() + n, kl);
        for (size_t i = 0; i < n; ++i) {
            kmers_out[i] = ~w[i].lo;
            counts_out[i] = 0xffffffffu - (uint32_t)(w[i].hi >> 32);
        }
        return AC_OK;
    }
    struct Entry {
        uint64_t count, kmer;
        float comp;
    };
    std::vector<Entry> v;
    v.reserve(n_all);
    for (uint64_t i = 0; i < got; ++i)
        if (!solid || gc_p[i] >= solid) v.push_back({gc_p[i], gk_p[i], complexity(gk_p[i], k)});
    auto less = [](const Entry& x, const Entry& y) {
        if (x.count != y.count) return x.count > y.count;
        if (x.comp != y.comp) return x.comp < y.comp;
        return x.kmer > y.kmer;
    };
    std::partial_sort(v.begin(), v.begin() + n, v.end(), less);
    for (size_t i = 0; i < n; ++i) {
        kmers_out[i] = v[i].kmer;
        counts_out[i] = v[i].count;
    }
    return AC_OK;
}

ac_status ac_exact_count(ac_ctx* ctx, uint32_t k, const ac_windows* host, float lc_threshold,
                         const uint64_t* forbidden, uint32_t n_forbidden, uint64_t limit, uint64_t solid,
                         uint64_t* kmers_out, uint64_t* counts_out, uint64_t capacity, uint64_t* n_out,
                         uint64_t* n_distinct, uint64_t* had_n) {
    if (!ctx) return fail(nullptr, AC_ERR_INVALID, "ctx is NULL");
    if (ac_status st = check_k(ctx, k)) return st;
    ac_windows dev;
    if (ac_status st = ac_sample_upload(ctx, host, &dev)) return st;
    return ac_exact_count_device(ctx, k, &dev, lc_threshold, forbidden, n_forbidden, limit, solid, kmers_out,
                                 counts_out, capacity, n_out, n_distinct, had_n);
}

int ac_exact_path(const ac_ctx* ctx) { return ctx ? ctx->exact_path : -1; }

}  // extern "C"
