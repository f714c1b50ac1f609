// count_launch.cpp -- the launch plan of the fused count kernel.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "bs_nfa.h"
#include "ctx.h"
#include "nrec.h"
#include "stage_plan.h"

namespace ac_detail {

// Copier workgroups of a large staged launch (AC_COPIER_WGS overrides, for A/B runs): 16 = 2 per XCD,
// 4 CUs' worth of resident slots, 64 waves, enough to keep the AC_COPY_AHEAD window of chunk reads in
// flight over PCIe.
static uint32_t stage_copier_wgs() {
    static const uint32_t v = [] {
        const char* e = std::getenv("AC_COPIER_WGS");
        return e ? (uint32_t)std::max(1, std::atoi(e)) : 16u;
    }();
    return v;
}

// Who stages a staged launch (wm_count.h LaunchArgs::copier_wgs): a few copier workgroups stage
// every chunk while the others count as chunks land.  Round 3 let every workgroup's wave 0 claim
// tickets instead: fine while a call's chunks are packed within microseconds of the launch, but each
// such wave held its workgroup's other three waves at the table barrier until its chunk was in (the
// p90 workgroup started counting ~30 us into a cfg2 launch, profiles/r04_m1/stamps_staged.log), and a
// large call's chunks arrive over the whole packing time.  Copier workgroups at cfg2: stage p50
// 0.1143-0.1146 vs 0.1189-0.1193 ms (same box, profiles/r04_m7/ab_table.txt); the round-3 scheme was
// removed in round 5.
uint32_t stage_copiers(uint64_t tickets) { return tickets ? stage_copier_wgs() : 0u; }

// Joins ac_create's warm-up thread (once) and takes the resident-wave counts it queried.
void ensure_warm(ac_ctx* ctx) {
    if (!ctx->warm.joinable()) return;
    ctx->warm.join();
    for (int st = 0; st < 2; ++st)
        for (uint32_t P = 1; P <= AC_MAX_PACK; ++P)
            if (!ctx->resident[st][P]) ctx->resident[st][P] = ctx->warm_resident[st][P];
    for (int f = 0; f < acamd::BS_FAMILIES; ++f)
        for (uint32_t kk = 0; kk <= 32; ++kk)
            if (!ctx->resident_bs[f][kk]) ctx->resident_bs[f][kk] = ctx->warm_resident_bs[f][kk];
}

// Waves of a bit-sliced launch of `items` row items, of `resident` that fit at once: a
// launch of more than one and at most 1.25 rounds (measured at 1.05 and 1.22; at 1.5 and 2.0 rounds the
// step is no shorter or longer) takes 3 of every 4 resident workgroups.  A SIMD's
// issue slots are filled by three of these waves; the fourth one is starved through its table build
// and reaches its first row when the others finish theirs, so in a short launch it is the tail.
// That was measured at four waves per SIMD and holds for the kernels of that residency (k = 16) only:
// the wider patterns' kernels, at 2-3 waves per SIMD, launch every resident workgroup.
// AC_BS_WAVES_PCT (1..100) sets the share for every bit-sliced launch instead, for A/B runs.
static uint64_t bs_launch_waves(acamd::BsFamily family, uint32_t k, uint64_t items, uint64_t resident) {
    static const int pct = env_int("AC_BS_WAVES_PCT", 0);
    const int per_simd = acamd::bs_waves_per_simd(family, (int)k);
    const bool three_of_four = per_simd == 4 && items > resident &&
                               4 * items <= 5 * resident;
    const uint64_t want = pct > 0 ? resident * (uint64_t)std::min(pct, 100) / 100
                                  : three_of_four ? resident * 3 / 4 : resident;
    return std::max<uint64_t>(AC_WAVES_PER_BLOCK, want / AC_WAVES_PER_BLOCK * AC_WAVES_PER_BLOCK);
}

// One fused count launch (ctx.h CountLaunch: what each input means).
ac_status launch(ac_ctx* ctx, const CountLaunch& rq) {
    const uint32_t k = rq.k, n = rq.n;
    const ac_segment* const segs = rq.segs;
    ensure_warm(ctx);
    ac_ctx::Scratch& sc = ctx->sc[rq.scratch];
    if (ac_status st = check_k(ctx, k)) return st;
    if (n > AC_MAX_SEGS) return fail(ctx, AC_ERR_INVALID, "too many segments in one launch (max 4)");
    if (n && !segs) return fail(ctx, AC_ERR_INVALID, "segments is NULL");
    const uint32_t P = acamd::pack_factor(k);
    const bool staged = rq.stage != nullptr;
    acamd::LaunchArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_segs = n;
    a.m = k;
    a.P = P;
    // The bit-sliced kernel counts the launch when k is one of its instantiations and
    // every live segment holds equal windows of 1..256 bases (one slot of the packed image): decided
    // once (bs_launch, as the jobs stage's plan decided it), with the size of the launch's candidate
    // groups; its work items are rows of windows.
    bool live[AC_MAX_SEGS];
    for (uint32_t i = 0; i < n; ++i) live[i] = segs[i].n_kmers && segs[i].sample.n_windows;
    const bool bs = acamd::bs_launch(k, n, live, rq.ulen);
    // The context's edit budget (ac_set_max_errors): another one than 2 counts on a bit-sliced launch
    // or not at all -- refused here, before anything is enqueued.
    const uint32_t E = ctx->max_errors;
    // (hits first: its refusal names the hits call's own constraint)
    if (rq.hits) {
        bool has_pos[AC_MAX_SEGS];
        for (uint32_t i = 0; i < n; ++i) has_pos[i] = rq.pos && rq.pos[i];
        if (const char* why = rq.pos ? acamd::positions_refusal(E, k, n, live, rq.ulen, !ctx->peers.empty(), has_pos)
                                     : acamd::hits_refusal(E, k, n, live, rq.ulen, !ctx->peers.empty()))
            return fail(ctx, AC_ERR_INVALID, why);
        for (uint32_t i = 0; i < n; ++i)
            if (rq.mat_windows && live[i] && rq.mat_windows[i] < segs[i].sample.n_windows)
                return fail(ctx, AC_ERR_INVALID, "window hits: a segment has more windows than its matrix");
        for (uint32_t i = 0; i < n; ++i)
            if (live[i] && !rq.hits[i])
                return fail(ctx, AC_ERR_INVALID, "window hits: hits[i] is NULL for a segment with work");
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = i + 1; j < n; ++j)
                if (live[i] && live[j] && segs[i].counts < segs[j].counts + segs[j].n_kmers &&
                    segs[j].counts < segs[i].counts + segs[i].n_kmers)
                    return fail(ctx, AC_ERR_INVALID, "window hits: segments' count vectors overlap");
    }
    if (rq.pos && !rq.hits) return fail(ctx, AC_ERR_INVALID, "window positions come with the window hits");
    if (const char* why = acamd::budget_refusal(E, k, n, live, rq.ulen)) return fail(ctx, AC_ERR_INVALID, why);
    const uint32_t cpw = acamd::launch_group_size(k, staged, bs);
    uint64_t items = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const ac_segment& s = segs[i];
        if (s.n_kmers && (!s.kmers || !s.counts)) return fail(ctx, AC_ERR_INVALID, "segment kmers/counts is NULL");
        const bool equal = rq.ulen && rq.ulen[i] != AC_NO_ULEN;  // windows back to back at ceil32(ulen[i])
        if (s.n_kmers && s.sample.n_windows &&
            (!s.sample.codes || !s.sample.nmask || (!equal && (!s.sample.start || !s.sample.length))))
            return fail(ctx, AC_ERR_INVALID, "segment sample has a NULL array");
        if (equal && (uint64_t)s.sample.n_windows * ((rq.ulen[i] + 31ull) & ~31ull) > s.sample.n_bases)
            return fail(ctx, AC_ERR_INVALID, "equal windows reach past n_bases");
        if (s.sample.n_bases % 32 || s.sample.n_bases >= AC_MAX_IMAGE_BASES)
            return fail(ctx, AC_ERR_INVALID, "sample n_bases must be a multiple of 32 below 2^34 - 4096");
        // The count hand-off adds (1 << 32) + sum into 64-bit slots (wm_count.hip): a candidate's sum,
        // at most 3 per window (4 at an edit budget of 3), must stay below 2^32 or its carry would count
        // as an arrival and the slot would never see its last workgroup.
        if (s.n_kmers && (E == 3u ? 4ull : 3ull) * s.sample.n_windows >= (1ull << 32))
            return fail(ctx, AC_ERR_INVALID,
                        E == 3u ? "a segment of 2^32 / 4 windows or more at max_errors = 3: its counts would overflow"
                                : "a segment of 2^32 / 3 windows or more: its counts would overflow");
        const uint32_t groups = (s.n_kmers + cpw - 1) / cpw;
        if (bs)
            for (uint32_t g = 0; g < groups; ++g) items += acamd::bs_rows(s.n_kmers, g, cpw, s.sample.n_windows);
        else
            items += (uint64_t)groups * s.sample.n_windows;
    }
    // Launch plan.  One round of resident waves; work is pulled
    // from dynamic queues: items of `chunk` windows (1 when waves get few
    // windows, so the launch tail is about one window; up to 8 when they get
    // hundreds, for fewer atomics), each candidate group's items spread over
    // sub-queues of about 64 waves.  A segment gets sub-queues in proportion
    // to its windows, so every sub-queue holds about the same work.  Workgroups
    // of AC_WAVES_PER_BLOCK waves are dealt round-robin over blocks of that many
    // consecutive sub-queues (one candidate group each).
    const acamd::BsFamily family = acamd::bs_family(staged, rq.hits != nullptr, rq.pos != nullptr, E);
    uint32_t& res_p = bs ? ctx->resident_bs[acamd::bs_family_index(family)][k] : ctx->resident[staged][P];
    if (!res_p)
        AC_HIP(ctx, bs ? acamd::resident_waves_bs(family, k, ctx->cu_count, &res_p)
                       : acamd::resident_waves(P, staged, ctx->cu_count, &res_p));
    const uint64_t fit =
        rq.wave_div > 1 ? std::max<uint64_t>(AC_WAVES_PER_BLOCK, res_p / rq.wave_div / AC_WAVES_PER_BLOCK * AC_WAVES_PER_BLOCK)
                        : res_p;
    const uint64_t resident = bs ? bs_launch_waves(family, k, items, fit) : fit;
    const uint32_t wpw = (uint32_t)std::max<uint64_t>(1, (items + resident - 1) / resident);
#ifdef AC_FORCE_CHUNK  // A/B builds (tools/variants.sh): fixed item size
    const uint32_t chunk = AC_FORCE_CHUNK;
    (void)wpw;
#else
    const uint32_t chunk = std::max<uint32_t>(1, std::min<uint32_t>(8, wpw / 64));
#endif
    uint32_t groups_live = 0, max_nw = 1;
    for (uint32_t i = 0; i < n; ++i)
        if (segs[i].n_kmers && segs[i].sample.n_windows) {
            groups_live += (segs[i].n_kmers + cpw - 1) / cpw;
            max_nw = std::max<uint32_t>(max_nw, segs[i].sample.n_windows);
        }
#ifndef AC_SUBQ_WAVES
#define AC_SUBQ_WAVES 64  // waves per sub-queue (16 / 32 / 128 measured equal or slower, profiles/r05_m36)
#endif
    const uint64_t s_base = std::max<uint64_t>(
        1, std::min<uint64_t>(32, resident / ((uint64_t)AC_SUBQ_WAVES * std::max(1u, groups_live))));
    uint64_t wave = 0;
    uint32_t groups_total = 0, qbegin = 0, acc_slots = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const ac_segment& s = segs[i];
        acamd::SegDev& d = a.seg[i];
        d.kmers = s.kmers;
        d.codes = s.sample.codes;
        d.nmask = s.sample.nmask;
        d.has_n = (rq.no_n && rq.no_n[i]) ? 0u : 1u;
        d.ulen = rq.ulen ? rq.ulen[i] : AC_NO_ULEN;
        d.nrec = (rq.nrec && rq.nrec[i] && d.ulen != AC_NO_ULEN) ? acamd::nrec_bits(d.ulen) : 0u;
        d.start = s.sample.start;
        d.length = s.sample.length;
        d.n_bases = s.sample.n_bases;
        d.counts = s.counts;
        if (rq.stage) {
            d.stage_src = rq.stage->src[i];
            d.stage_dst = rq.stage->dst[i];
            d.stage_chunks = rq.stage->chunks[i];
            d.stage_codes_off = rq.stage->codes_off[i];
            d.dp_src = rq.stage->dp_src[i];
            d.dp_off = rq.stage->dp_off[i];
            d.dp_src_bytes = rq.stage->dp_bytes[i];
        }
        d.n_kmers = s.n_kmers;
        d.n_windows = s.sample.n_windows;
        d.groups = std::max<uint32_t>(1, (s.n_kmers + cpw - 1) / cpw);
        d.chunk = chunk;
        {  // a multiple of the workgroup size: a workgroup's waves take consecutive sub-queues of one group
            const uint64_t sq = std::max<uint64_t>(1, (s_base * s.sample.n_windows + max_nw / 2) / max_nw);
            d.subq = (uint32_t)((sq + AC_WAVES_PER_BLOCK - 1) / AC_WAVES_PER_BLOCK * AC_WAVES_PER_BLOCK);
        }
        d.queue_begin = qbegin;
        d.acc_begin = acc_slots;
        d.group_begin = groups_total;
        if (s.n_kmers && s.sample.n_windows) {
            qbegin += d.groups * d.subq;
            acc_slots += d.groups * cpw;
            groups_total += d.groups;
        } else {
            d.queue_begin = ~0u;  // never selected by the kernel's segment lookup
            // no workgroup writes this segment's counts
            if (rq.zero && s.n_kmers) AC_HIP(ctx, hipMemsetAsync(s.counts, 0, sizeof(uint32_t) * s.n_kmers, rq.stream));
        }
    }
    // The group's last workgroup stores its counts (no memset), unless live
    // segments share count slots (window shards of one candidate set): then
    // zero them once and let every group add.
    bool alias = false;
    for (uint32_t i = 0; i < n && !alias; ++i)
        for (uint32_t j = i + 1; j < n && !alias; ++j) {
            const acamd::SegDev &x = a.seg[i], &y = a.seg[j];
            if (x.queue_begin == ~0u || y.queue_begin == ~0u) continue;
            alias = x.counts < y.counts + y.n_kmers && y.counts < x.counts + x.n_kmers;
        }
    a.add_counts = (!rq.zero || alias) ? 1u : 0u;
    if (rq.zero && alias)
        for (uint32_t i = 0; i < n; ++i)
            if (a.seg[i].queue_begin != ~0u)
                AC_HIP(ctx, hipMemsetAsync(a.seg[i].counts, 0, sizeof(uint32_t) * a.seg[i].n_kmers, rq.stream));
    if (acc_slots > sc.acc_cap) {
        if (sc.acc) AC_HIP(ctx, hipFree(sc.acc));
        sc.acc = nullptr;
        sc.acc_cap = 0;
        AC_HIP(ctx, hipMalloc(&sc.acc, sizeof(uint64_t) * acc_slots));
        AC_HIP(ctx, hipMemsetAsync(sc.acc, 0, sizeof(uint64_t) * acc_slots, rq.stream));
        sc.acc_cap = acc_slots;
    }
    a.acc = sc.acc;
    a.err = rq.err ? rq.err : ctx->d_err;
    const uint32_t n_counters = qbegin;
    if (n_counters) wave = std::max<uint64_t>(resident, n_counters);
    // a staged launch's device words follow its sub-queue counters in the bank (zeroed with them)
    const uint32_t used = n_counters + (rq.stage ? AC_STAGE_LINES : 0u);
    if (used > sc.qcap) {
        if (sc.queue) AC_HIP(ctx, hipFree(sc.queue));
        sc.queue = nullptr;
        sc.qcap = 0;
        const uint32_t cap = std::max<uint32_t>(used, 1024);
        const size_t bytes = sizeof(uint32_t) * AC_QUEUE_LINE * 2 * (size_t)cap;
        AC_HIP(ctx, hipMalloc(&sc.queue, bytes));
        AC_HIP(ctx, hipMemsetAsync(sc.queue, 0, bytes, rq.stream));
        sc.qcap = cap;
        sc.bank = 0;
        sc.dirty[0] = sc.dirty[1] = 0;
    }
    a.queue = sc.queue;
    a.qstride = sc.qcap;
    a.bank = sc.bank;
    a.zero_count = sc.dirty[sc.bank ^ 1u];
    a.n_queues = std::max<uint32_t>(1, n_counters);
    if (rq.stage) {
        uint32_t total_chunks = 0;
        for (uint32_t i = 0; i < n; ++i) total_chunks += rq.stage->chunks[i];
        if (total_chunks > sc.stage_gen_cap) {  // (zeroed once: generations are never 0)
            if (sc.stage_gen) AC_HIP(ctx, hipFree(sc.stage_gen));
            sc.stage_gen = nullptr;
            sc.stage_gen_cap = 0;
            const uint32_t cap = std::max<uint32_t>(total_chunks, 1024);
            const size_t bytes = sizeof(uint32_t) * AC_QUEUE_LINE * (size_t)cap;  // one line per chunk flag
            AC_HIP(ctx, hipMalloc(&sc.stage_gen, bytes));
            AC_HIP(ctx, hipMemsetAsync(sc.stage_gen, 0, bytes, rq.stream));
            sc.stage_gen_cap = cap;
        }
        uint32_t off = 0;
        for (uint32_t i = 0; i < n; ++i) {
            a.seg[i].stage_gen = sc.stage_gen + (size_t)off * AC_QUEUE_LINE;
            off += rq.stage->chunks[i];
        }
        a.staged = 1;
        a.gen = rq.stage->gen;
        a.host_hdr = rq.stage->host_hdr;
        a.stage = sc.queue + ((uint64_t)sc.bank * sc.qcap + n_counters) * AC_QUEUE_LINE;
        a.err = a.stage + AC_STAGE_L_ERR * AC_QUEUE_LINE;
        a.err_out = rq.stage->err_out;
        a.tag = rq.stage->tag;
        a.grp_err = rq.stage->grp_err;
        const uint64_t blocks = (wave + AC_WAVES_PER_BLOCK - 1) / AC_WAVES_PER_BLOCK;
        a.copier_wgs = (uint32_t)std::min<uint64_t>(blocks, rq.stage->copiers);
    }
    // the equal-window instantiation when every live segment has equal windows (their fit in the
    // image checked above)
    a.eq = 1u;
    for (uint32_t i = 0; i < n; ++i)
        if (a.seg[i].queue_begin != ~0u && a.seg[i].ulen == AC_NO_ULEN) a.eq = 0u;
    // Live segments' queue_begin values are increasing; the kernel picks the
    // last live segment whose queue_begin <= its sub-queue.
    a.bs = bs ? 1u : 0u;
    a.max_errors = E;
    if (rq.hits) {
        a.want_hits = 1u;
        for (uint32_t i = 0; i < n; ++i) a.hits[i] = a.seg[i].queue_begin != ~0u ? rq.hits[i] : nullptr;
        for (uint32_t i = 0; i < n; ++i) a.mat_nw[i] = rq.mat_windows ? rq.mat_windows[i] : a.seg[i].n_windows;
    }
    if (rq.pos) {
        a.want_pos = 1u;
        for (uint32_t i = 0; i < n; ++i) a.pos[i] = a.seg[i].queue_begin != ~0u ? rq.pos[i] : nullptr;
    }
    a.total_waves = wave;
    if (wave) ctx->last_kernel = bs ? 1 : 0;
    ctx->last_waves = wave;
    ctx->last_wpw = wpw;
    ctx->last_groups = groups_total;
    AC_HIP(ctx, acamd::launch_wm2_count(a, rq.stream));
    if (wave) {  // the launch dequeued from `bank` and zeroed the other one
        sc.dirty[sc.bank] = used;
        sc.dirty[sc.bank ^ 1u] = 0;
        sc.bank ^= 1u;
    }
    return AC_OK;
}

}  // namespace ac_detail
