// stage_plan_dump -- runs the jobs stage's planner (approx_counter_amd/csrc/stage_plan.cpp) on a case
// read from a file and writes what it planned, for tests/test_stage_plan.py (host-only; built there
// with the sanitizers on).
//   stage_plan_dump plan IN OUT
//     IN : u32 k, early, have_d_counts, pool_participants, early_mode, hooks, n_jobs; u64 min_task_windows;
//          per job u32 n_kmers, n_windows, lo, hi, then n_windows u32 lengths
//     OUT: u64 early, tag, total_w, off_err, total, off_gerr, n_gerr, pre, tickets; then for each of these
//          fields its AC_MAX_JOBS values as u64: lo, hi, n_bases, no_bases, off_kmers, off_codes, off_nmask,
//          off_start, off_len, off_counts, ulen, nrec, region, chunks, codes_off; then u64 n_tasks and per
//          task u64 job, w0, w1, first, span, first_len, len_diff
//   stage_plan_dump cuts IN OUT
//     IN : u32 n, n u32 lengths, f64 frac, u32 G, u32 n_totals, n_totals u64 window totals
//     OUT: u32 part_cut(frac), G + 1 u32 shard_cuts(G), n_totals u32 stage_parts
// The jobs' k-mers and bases are never read by the planner, so they are not part of a case (NULL here).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "stage_plan.h"

namespace {

struct Reader {
    std::vector<unsigned char> buf;
    size_t at = 0;
    explicit Reader(const char* path) {
        FILE* f = std::fopen(path, "rb");
        if (!f) return;
        unsigned char tmp[4096];
        for (size_t n; (n = std::fread(tmp, 1, sizeof tmp, f)) > 0;) buf.insert(buf.end(), tmp, tmp + n);
        std::fclose(f);
    }
    template <class T>
    T get() {
        T v{};
        if (at + sizeof v <= buf.size()) std::memcpy(&v, buf.data() + at, sizeof v);
        at += sizeof v;
        return v;
    }
    bool ok() const { return !buf.empty() && at == buf.size(); }  // read exactly to the end
};

struct Writer {
    FILE* f;
    explicit Writer(const char* path) : f(std::fopen(path, "wb")) {}
    ~Writer() {
        if (f) std::fclose(f);
    }
    void u64(uint64_t v) { std::fwrite(&v, sizeof v, 1, f); }
    void u32(uint32_t v) { std::fwrite(&v, sizeof v, 1, f); }
};

int dump_plan(Reader& in, Writer& out) {
    const uint32_t k = in.get<uint32_t>();
    acamd::JobPlan p;
    p.early = in.get<uint32_t>() != 0;
    const bool have_d_counts = in.get<uint32_t>() != 0;
    const uint32_t participants = in.get<uint32_t>(), early_mode = in.get<uint32_t>(), hooks = in.get<uint32_t>();
    p.n = in.get<uint32_t>();
    const uint64_t min_task = in.get<uint64_t>();
    if (p.n > AC_MAX_JOBS || !participants || !min_task) return 2;
    std::vector<uint32_t> lengths[AC_MAX_JOBS];
    ac_job jobs[AC_MAX_JOBS] = {};
    for (uint32_t j = 0; j < p.n; ++j) {
        jobs[j].n_kmers = in.get<uint32_t>();
        jobs[j].sample.n_windows = in.get<uint32_t>();
        p.lo[j] = in.get<uint32_t>();
        p.hi[j] = in.get<uint32_t>();
        if (p.lo[j] > p.hi[j] || p.hi[j] > jobs[j].sample.n_windows || jobs[j].sample.n_windows > in.buf.size()) return 2;
        lengths[j].resize(jobs[j].sample.n_windows);
        for (uint32_t& l : lengths[j]) l = in.get<uint32_t>();
        jobs[j].sample.length = lengths[j].data();
    }
    if (!in.ok()) return 2;
    const std::vector<acamd::Task> tasks =
        acamd::plan_stage(k, jobs, p, have_d_counts, participants, min_task, (int)early_mode, hooks);
    for (uint64_t v : {(uint64_t)p.early, (uint64_t)p.tag, p.total_w, (uint64_t)p.off_err, (uint64_t)p.total,
                       (uint64_t)p.off_gerr, (uint64_t)p.n_gerr, (uint64_t)p.pre, p.tickets})
        out.u64(v);
    auto per_job = [&](auto field) {
        for (uint32_t j = 0; j < AC_MAX_JOBS; ++j) out.u64((uint64_t)field(j));
    };
    per_job([&](uint32_t j) { return p.lo[j]; });
    per_job([&](uint32_t j) { return p.hi[j]; });
    per_job([&](uint32_t j) { return p.n_bases[j]; });
    per_job([&](uint32_t j) { return p.no_bases[j]; });
    per_job([&](uint32_t j) { return p.off_kmers[j]; });
    per_job([&](uint32_t j) { return p.off_codes[j]; });
    per_job([&](uint32_t j) { return p.off_nmask[j]; });
    per_job([&](uint32_t j) { return p.off_start[j]; });
    per_job([&](uint32_t j) { return p.off_len[j]; });
    per_job([&](uint32_t j) { return p.off_counts[j]; });
    per_job([&](uint32_t j) { return p.ulen[j]; });
    per_job([&](uint32_t j) { return p.nrec[j]; });
    per_job([&](uint32_t j) { return p.region[j]; });
    per_job([&](uint32_t j) { return p.chunks[j]; });
    per_job([&](uint32_t j) { return p.codes_off[j]; });
    out.u64(tasks.size());
    for (const acamd::Task& x : tasks)
        for (uint64_t v : {(uint64_t)x.job, (uint64_t)x.w0, (uint64_t)x.w1, x.first, x.span, (uint64_t)x.first_len,
                           (uint64_t)x.len_diff})
            out.u64(v);
    return 0;
}

int dump_cuts(Reader& in, Writer& out) {
    const uint32_t n = in.get<uint32_t>();
    if (n > in.buf.size()) return 2;
    std::vector<uint32_t> len(n);
    for (uint32_t& l : len) l = in.get<uint32_t>();
    const double frac = in.get<double>();
    const uint32_t G = in.get<uint32_t>(), n_totals = in.get<uint32_t>();
    if (!G || n_totals > in.buf.size()) return 2;
    std::vector<uint64_t> totals(n_totals);
    for (uint64_t& t : totals) t = in.get<uint64_t>();
    if (!in.ok()) return 2;
    out.u32(acamd::part_cut(len.data(), n, frac));
    for (uint32_t c : acamd::shard_cuts(len.data(), n, G)) out.u32(c);
    for (uint64_t t : totals) out.u32((uint32_t)acamd::stage_parts(t));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: stage_plan_dump plan|cuts IN OUT\n");
        return 2;
    }
    Reader in(argv[2]);
    Writer out(argv[3]);
    if (in.buf.empty() || !out.f) return 2;
    const std::string mode = argv[1];
    return mode == "plan" ? dump_plan(in, out) : mode == "cuts" ? dump_cuts(in, out) : 2;
}
