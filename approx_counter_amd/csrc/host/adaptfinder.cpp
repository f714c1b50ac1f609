// adaptfinder.cpp -- the drop-in command line (binary `adaptFinder`).
//
// Same flags, config file, precedence, defaults, messages and output files as
// qbonenfant/approx_counter's main (approx_counter.cpp:604-958), so that
// Porechop_ABI can run it unchanged.  The approximate count (errorCount,
// approx_counter.cpp:531-601) goes through the C ABI of
// include/approx_counter_amd.h to the HIP kernel; there is no CPU fallback.
//
// Extensions (not in the reference, documented in DESIGN.md):
//   -g, --gpus N    shard the sampled windows over N GPUs of this node (default 1)
//   --seed N        seed the read sampling (the reference always uses std::random_device)
//   --max-errors E  edit budget of the approximate count, 0..3 (the reference hard-codes 2, the default):
//                   a window adds max(0, E + 1 - d) to a k-mer's count (ac_set_max_errors)
//   --levels        beside every <out>_<run>.<end> file a <out>_<run>.<end>.levels file: per k-mer, in the
//                   same order, the sampled windows that hold it within 0, 1, .. E edits (the reference's
//                   per-level bitfields, approx_counter.cpp:553-565, before their sum; ac_window_hits_samples)
//   --positions     beside every <out>_<run>.<end> file a <out>_<run>.<end>.positions file: per k-mer, in the
//                   same order, for every base 1..L of the sampled windows how many of the windows within E
//                   edits have their best occurrence ending there (ac_window_positions_samples)
//   --spans         beside every <out>_<run>.<end> file a <out>_<run>.<end>.starts and a <out>_<run>.<end>.lengths
//                   file: per k-mer, in the same order, for every base 1..L how many of the windows within E edits
//                   have their best occurrence starting there, and for every occurrence length k - E .. k + E how
//                   many have that length (ac_window_spans_samples)
//   --flanks D      beside every <out>_<run>.<end> file a <out>_<run>.<end>.flanks file: per k-mer, in the same
//                   order, the windows within E edits by the base (a,c,g,t,n) at each of the D bases before its
//                   best occurrence's start and the D bases after its end, in reading order
//                   (ac_window_flanks_samples)
//   --edits         beside every <out>_<run>.<end> file a <out>_<run>.<end>.edits file: per k-mer, in the same
//                   order, for every base of the k-mer the windows within E edits by what its best occurrence
//                   holds there: the base, another base, nothing, or an inserted base after it
//                   (ac_window_edits_samples)
//   --cooccurrence  beside every <out>_<run>.<end> file a <out>_<run>.<end>.cooc file: per k-mer, in the same
//                   order, for every k-mer of the file how many sampled windows hold the two together within
//                   E edits (two of the reference's bitfields at once; ac_hit_cooccurrence)
//   --paired-sample one sample of reads a run for both ends: window i of the start sample and window i of the end
//                   sample come from the same read (the reference, approx_counter.cpp:867, shuffles once an end)
//   --cross-cooccurrence
//                   a <out>_<run>.cross file: per k-mer of the .start file, in its order, for every k-mer of the
//                   .end file in its order how many sampled reads hold the first in their start window and the
//                   second in their end window, both within E edits (ac_hit_cross_cooccurrence); needs
//                   --paired-sample
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <iostream>
#include <map>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../bs_pos.h"
#include "../hit_levels.h"
#include "approx_counter_amd.h"
#include "host_stages.h"

using namespace achost;

namespace {

const auto boot_time = std::chrono::steady_clock::now();

// print (approx_counter.cpp:85-94)
template <typename T>
void print(const T& text, int tab = 0) {
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - boot_time).count();
    std::cout << "[" << ms << " ms]\t";
    for (int i = 0; i < tab; ++i) std::cout << "\t";
    std::cout << text << std::endl;
}

// ---------------------------------------------------------------------------
// Argument parsing with the SeqAn ArgumentParser spellings (get_args, 604-669)
// ---------------------------------------------------------------------------
enum class Kind { Int, Double, String, Flag };
struct Opt {
    const char* s;
    const char* l;
    Kind kind;
    const char* help;
};
const Opt OPTS[] = {
    {"lc", "low_complexity", Kind::Double, "low complexity filter threshold (for k=16), default 1.5"},
    {"sn", "sample_n", Kind::Int, "sample n sequences from dataset, default 10k sequences"},
    {"sl", "sample_length", Kind::Int, "size of the sampled portion, default 100 bases"},
    {"nt", "nb_thread", Kind::Int, "Number of thread to work with, default is 4"},
    {"k", "kmer_size", Kind::Int, "Size of the kmers, default is 16"},
    {"lim", "limit", Kind::Int, "limit the number of kmer used after initial counting, default is 500"},
    {"mr", "multi_run", Kind::Int, "Number of time the count must be performed. Each count is exported separately."},
    {"v", "verbosity", Kind::Int, "Level of details printed out"},
    {"e", "exact_file", Kind::String, "path to export the exact k-mer count, if needed. Default: no export"},
    {"conf", "config", Kind::String, "path to the config file"},
    {"fk", "forbidden_kmer", Kind::String,
     "take a file containing 'forbidden' kmers, excluding them from the search pool. One kmer per line."},
    {"sk", "solid_km", Kind::Int,
     "Use solid kmer instead of most frequents. This option will override sample number (-sn / --sample_n)."},
    {"se", "skip_end", Kind::Flag,
     "Skip end adapter ressearch (only search start). /!\\ If this option is set, and adaptFinder is run trough "
     "PorechopABI, the --guess_only / -go MUST be set."},
    {"o", "out_file", Kind::String, "path to the output file, default is ./out.txt"},
    {"g", "gpus", Kind::Int, "[MI355X build] number of GPUs of this node to shard the count over, default 1"},
    {"", "seed", Kind::Int, "[MI355X build] seed of the read sampling, default: std::random_device"},
    {"", "max-errors", Kind::Int,
     "[MI355X build] edit budget E of the approximate count, 0 to 3: a window adds max(0, E + 1 - distance); "
     "default 2, the reference's. Another value needs a kmer size of 16 or 18 to 32, a sampling length up to 255 "
     "and one GPU."},
    {"", "levels", Kind::Flag,
     "[MI355X build] also write <out>_<run>.<end>.levels: one line per k-mer of the main file, in its order, the "
     "k-mer and the number of sampled windows holding it within 0, 1, .. max-errors edits (they sum to its count). "
     "Needs a kmer size of 16 or 18 to 32, a sampling length up to 255, one GPU and reads of at least the sampling "
     "length."},
    {"", "positions", Kind::Flag,
     "[MI355X build] also write <out>_<run>.<end>.positions: one line per k-mer of the main file, in its order, the "
     "k-mer and, for every base 1 to L of the sampled windows, the number of windows holding it within max-errors "
     "edits whose leftmost best occurrence ends at that base (they sum to the last column of its .levels line). "
     "Same needs as --levels, with which it can be combined."},
    {"", "spans", Kind::Flag,
     "[MI355X build] also write <out>_<run>.<end>.starts and <out>_<run>.<end>.lengths: one line per k-mer of the main "
     "file, in its order. A .starts line is the k-mer and, for every base 1 to L of the sampled windows, the number of "
     "windows holding it within max-errors edits whose best occurrence (the shortest one ending where .positions says) "
     "starts at that base; a .lengths line is the k-mer and the number of those windows by occurrence length, from "
     "k - max-errors to k + max-errors. Both sum to the last column of its .levels line. Same needs as --levels, with "
     "which and with --positions it can be combined."},
    {"", "flanks", Kind::Int,
     "[MI355X build] also write <out>_<run>.<end>.flanks, for a depth D of 1 to 32: one line per k-mer of the main "
     "file, in its order. A line is the k-mer and 2 D groups a,c,g,t,n: of the sampled windows holding it within "
     "max-errors edits, how many have that base at each of the D bases before its best occurrence's start (from the "
     "farthest to the nearest) and at each of the D bases after its end (from the nearest to the farthest), so that a "
     "line reads like the window; a base outside the window is not counted. Same needs as --levels, with which and "
     "with --positions and --spans it can be combined."},
    {"", "edits", Kind::Flag,
     "[MI355X build] also write <out>_<run>.<end>.edits: one line per k-mer of the main file, in its order. A line is "
     "the k-mer and one group of 12 counts per base of it: of the sampled windows holding it within max-errors edits, "
     "how many have that base matched, substituted by a,c,g,t,n, deleted (missing from the read), and followed by an "
     "inserted a,c,g,t,n in the alignment of the k-mer against its best occurrence. Same needs as --levels, with "
     "which and with --positions, --spans and --flanks it can be combined."},
    {"", "cooccurrence", Kind::Flag,
     "[MI355X build] also write <out>_<run>.<end>.cooc: one line per k-mer of the main file, in its order, the "
     "k-mer and, for every k-mer of the main file in the same order, the number of sampled windows holding both "
     "within max-errors edits (entry i of line i is the last column of its .levels line). Same needs as --levels, "
     "with which and with --positions it can be combined."},
    {"", "paired-sample", Kind::Flag,
     "[MI355X build] draw one sample of reads per run for both ends: window i of the start sample and window i of "
     "the end sample come from the same read (by default each end is sampled on its own, as the reference does). "
     "Cannot be combined with -se."},
    {"", "cross-cooccurrence", Kind::Flag,
     "[MI355X build] also write <out>_<run>.cross: one line per k-mer of the .start file, in its order, the k-mer "
     "and, for every k-mer of the .end file in its order, the number of sampled reads holding the first in their "
     "start window and the second in their end window, both within max-errors edits. Needs --paired-sample; "
     "otherwise the needs of --levels, with which and with --positions and --cooccurrence it can be combined."},
    {"", "host-exact", Kind::Flag,
     "[MI355X build] the reference's host stages: whole reads in memory, exact k-mer count on the CPU"},
    {"", "dump-sample", Kind::String,
     "[MI355X build] write each sampled window image to <path>_<run>.<end> and stop before counting"},
};

struct Args {
    std::map<std::string, std::string> val;  // by long name
    std::string input;
};

void usage(std::ostream& os) {
    os << "adaptFinder\n===========\n\nSYNOPSIS\n    adaptFinder [OPTIONS] \"input filename\"\n\n"
          "REQUIRED ARGUMENTS\n    input filename STRING\n\nOPTIONS\n    -h, --help\n          Display the help message.\n";
    for (const Opt& o : OPTS) {
        os << "    ";
        if (*o.s) os << "-" << o.s << ", ";
        os << "--" << o.l;
        switch (o.kind) {
            case Kind::Int: os << " INTEGER"; break;
            case Kind::Double: os << " DOUBLE"; break;
            case Kind::String: os << " STRING"; break;
            case Kind::Flag: break;
        }
        os << "\n          " << o.help << "\n";
    }
}

bool valid_value(Kind kind, const std::string& v) {
    if (v.empty()) return false;
    char* end = nullptr;
    if (kind == Kind::Int) {
        std::strtoll(v.c_str(), &end, 10);
        return *end == '\0';
    }
    if (kind == Kind::Double) {
        std::strtod(v.c_str(), &end);
        return *end == '\0';
    }
    return true;
}

// Returns 0 = OK, 1 = parse error, 2 = help printed.
int parse_args(int argc, char const** argv, Args& a) {
    std::vector<std::string> positional;
    for (int i = 1; i < argc; ++i) {
        std::string t = argv[i];
        if (t == "-h" || t == "--help") {
            usage(std::cout);
            return 2;
        }
        if (t.size() > 1 && t[0] == '-' && !(t.size() > 1 && (std::isdigit((unsigned char)t[1]) || t[1] == '.'))) {
            std::string name = t.substr(t[1] == '-' ? 2 : 1), value;
            bool has_inline = false;
            const size_t eq = name.find('=');
            if (eq != std::string::npos) {
                value = name.substr(eq + 1);
                name = name.substr(0, eq);
                has_inline = true;
            }
            const Opt* opt = nullptr;
            for (const Opt& o : OPTS)
                if ((t[1] == '-' && name == o.l) || (t[1] != '-' && *o.s && name == o.s)) opt = &o;
            if (!opt) {
                std::cerr << "adaptFinder: illegal option -- " << name << "\n";
                return 1;
            }
            if (opt->kind == Kind::Flag) {
                a.val[opt->l] = "1";
                continue;
            }
            if (!has_inline) {
                if (i + 1 >= argc) {
                    std::cerr << "adaptFinder: option requires an argument -- " << name << "\n";
                    return 1;
                }
                value = argv[++i];
            }
            if (!valid_value(opt->kind, value)) {
                std::cerr << "adaptFinder: the given value '" << value << "' cannot be casted to "
                          << (opt->kind == Kind::Int ? "integer" : "double") << "\n";
                return 1;
            }
            a.val[opt->l] = value;
        } else {
            positional.push_back(t);
        }
    }
    if (positional.size() != 1) {
        std::cerr << "adaptFinder: " << (positional.empty() ? "Not enough" : "Too many") << " arguments given.\n";
        return 1;
    }
    a.input = positional[0];
    return 0;
}

template <typename T>
void get_option(const Args& a, const char* long_name, T& out);
template <>
void get_option(const Args& a, const char* n, uint64_t& out) {
    auto it = a.val.find(n);
    if (it != a.val.end()) out = (uint64_t)std::strtoll(it->second.c_str(), nullptr, 10);
}
template <>
void get_option(const Args& a, const char* n, float& out) {
    auto it = a.val.find(n);
    if (it != a.val.end()) out = (float)std::strtod(it->second.c_str(), nullptr);
}
template <>
void get_option(const Args& a, const char* n, std::string& out) {
    auto it = a.val.find(n);
    if (it != a.val.end()) out = it->second;
}

// ---------------------------------------------------------------------------
// errorCount (approx_counter.cpp:531-601) through the C ABI, windows sharded
// over n_gpus devices (contiguous ranges balanced by bases), counts summed.
// ---------------------------------------------------------------------------
ac_windows view(const PackedImage& p) {
    return ac_windows{p.codes.data(), p.nmask.data(), p.start.data(), p.length.data(), (uint32_t)p.size(), p.n_bases};
}

// The device context: -g N opens N shards (device g mod the visible devices,
// ac_create_multi); the exact count and the one-GPU approximate count use the
// first device, the sharded count goes through ac_error_count_images.
struct Devices {
    ac_ctx* ctx = nullptr;
    uint64_t shards = 1;
    ~Devices() { ac_destroy(ctx); }
};

// --dump-sample: u64 n_windows, u64 n_bases, start[n] u64, length[n] u32,
// codes[n_bases/16] u32, nmask[n_bases/32] u32 (little endian).
bool write_image(const PackedImage& p, const std::string& path) {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const uint64_t hdr[2] = {p.size(), p.n_bases};
    bool ok = std::fwrite(hdr, sizeof hdr, 1, f) == 1;
    ok = ok && std::fwrite(p.start.data(), sizeof(uint64_t), p.size(), f) == p.size();
    ok = ok && std::fwrite(p.length.data(), sizeof(uint32_t), p.size(), f) == p.size();
    ok = ok && std::fwrite(p.codes.data(), sizeof(uint32_t), p.codes.size(), f) == p.codes.size();
    ok = ok && std::fwrite(p.nmask.data(), sizeof(uint32_t), p.nmask.size(), f) == p.nmask.size();
    return std::fclose(f) == 0 && ok;
}

// --levels: `ranked` is the main file's content; one line per k-mer of it, the k-mer and its `levels` level
// counts -- column sums of the job's hit matrix (hits: levels x n_windows x ceil(n / 32) words, candidate c =
// kmers[c]), by the column counter the library's level-count kernel runs (hit_levels.h).
bool export_levels(const pair_vector& ranked, const std::vector<uint64_t>& kmers, const std::vector<uint32_t>& hits,
                   uint32_t n_windows, uint32_t levels, uint32_t k, const std::string& path) {
    const uint32_t n = (uint32_t)kmers.size(), words = (n + 31u) / 32u;
    std::vector<uint32_t> lc((size_t)levels * n, 0u);
    for (uint32_t e = 0; e < levels; ++e)
        for (uint32_t col = 0; col < words; ++col) {
            uint32_t cnt[32] = {};
            acamd::bs::hc_column(hits.data() + (size_t)e * n_windows * words, words, col, 0u, n_windows, 1u, cnt);
            for (uint32_t j = 0; j < 32u && 32u * col + j < n; ++j) lc[(size_t)e * n + 32u * col + j] = cnt[j];
        }
    std::map<uint64_t, uint32_t> index;  // (the exact count's k-mers are distinct)
    for (uint32_t c = 0; c < n; ++c) index.emplace(kmers[c], c);
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::string line;
    for (const auto& kv : ranked) {
        const uint32_t c = index.at(kv.first);
        line = int2dna(kv.first, k);
        for (uint32_t e = 0; e < levels; ++e) line += '\t' + std::to_string(lc[(size_t)e * n + c]);
        line += '\n';
        std::fwrite(line.data(), 1, line.size(), f);
    }
    return std::fclose(f) == 0;
}

// --positions: one line per k-mer of `ranked`, the k-mer and window_len counts -- the position profile of the
// job's hit and position matrices folded over the distances, by the walk the library's profile kernel runs
// (bs_pos.h pp_column).
bool export_positions(const pair_vector& ranked, const std::vector<uint64_t>& kmers, const std::vector<uint32_t>& hits,
                      const std::vector<uint32_t>& pos, uint32_t n_windows, uint32_t levels, uint32_t window_len, uint32_t k,
                      const std::string& path) {
    const uint32_t n = (uint32_t)kmers.size(), words = (n + 31u) / 32u, L = window_len;
    std::vector<uint32_t> prof((size_t)n * L, 0u);
    for (uint32_t d = 0; d < levels; ++d)
        for (uint32_t col = 0; col < words; ++col)
            acamd::bs::pp_column(hits.data(), pos.data(), n, n_windows, d, col, 0u, n_windows, 1u, [&](uint32_t j, uint32_t p) {
                if (p < L) ++prof[(size_t)(32u * col + j) * L + p];
            });
    std::map<uint64_t, uint32_t> index;  // (the exact count's k-mers are distinct)
    for (uint32_t c = 0; c < n; ++c) index.emplace(kmers[c], c);
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::string line;
    for (const auto& kv : ranked) {
        const uint32_t c = index.at(kv.first);
        line = int2dna(kv.first, k);
        for (uint32_t p = 0; p < L; ++p) line += '\t' + std::to_string(prof[(size_t)c * L + p]);
        line += '\n';
        std::fwrite(line.data(), 1, line.size(), f);
    }
    return std::fclose(f) == 0;
}

// --spans: two files, one line per k-mer of `ranked` each.  .starts: the k-mer and window_len counts -- the
// position profile's fold (export_positions) over the job's START matrix, whose stored value is the 0-based
// start, so column p + 1 counts the windows whose best occurrence starts at base p + 1.  .lengths: the k-mer
// and 2 E + 1 counts, the windows by end - start = k - E .. k + E, from the two matrices together.
bool export_spans(const pair_vector& ranked, const std::vector<uint64_t>& kmers, const std::vector<uint32_t>& hits,
                  const std::vector<uint32_t>& pos, const std::vector<uint32_t>& start, uint32_t n_windows, uint32_t levels,
                  uint32_t window_len, uint32_t k, const std::string& starts_path, const std::string& lengths_path) {
    if (!export_positions(ranked, kmers, hits, start, n_windows, levels, window_len, k, starts_path)) return false;
    const uint32_t n = (uint32_t)kmers.size(), words = (n + 31u) / 32u, E = levels - 1u, bins = 2u * E + 1u;
    const size_t plane = (size_t)n_windows * words;
    std::vector<uint32_t> prof((size_t)n * bins, 0u);
    for (uint32_t w = 0; w < n_windows; ++w)
        for (uint32_t col = 0; col < words; ++col) {
            const size_t at = (size_t)w * words + col;
            const uint32_t left = n - 32u * col;
            uint32_t m = hits[(size_t)E * plane + at] & (left >= 32u ? ~0u : (1u << left) - 1u);
            if (!m) continue;
            uint32_t p[acamd::bs::POS_PLANES], s[acamd::bs::POS_PLANES];
            for (int b = 0; b < acamd::bs::POS_PLANES; ++b) {
                p[b] = pos[(size_t)b * plane + at];
                s[b] = start[(size_t)b * plane + at];
            }
            for (; m; m &= m - 1u) {
                const uint32_t j = (uint32_t)__builtin_ctz(m);
                const uint32_t len = acamd::bs::pos_get(p, j) + 1u - acamd::bs::pos_get(s, j);  // (end - start)
                if (len + E >= k && len + E - k < bins) ++prof[(size_t)(32u * col + j) * bins + (len + E - k)];
            }
        }
    std::map<uint64_t, uint32_t> index;  // (the exact count's k-mers are distinct)
    for (uint32_t c = 0; c < n; ++c) index.emplace(kmers[c], c);
    std::FILE* f = std::fopen(lengths_path.c_str(), "wb");
    if (!f) return false;
    std::string line;
    for (const auto& kv : ranked) {
        const uint32_t c = index.at(kv.first);
        line = int2dna(kv.first, k);
        for (uint32_t b = 0; b < bins; ++b) line += '\t' + std::to_string(prof[(size_t)c * bins + b]);
        line += '\n';
        std::fwrite(line.data(), 1, line.size(), f);
    }
    return std::fclose(f) == 0;
}

// --flanks: one line per k-mer of `ranked`, the k-mer and 2 D groups a,c,g,t,n -- `flank` is the result of
// ac_window_flanks_samples (2 sides x n x D x 5, candidate c = kmers[c]): the left side's columns from the
// farthest base to the nearest, then the right side's from the nearest to the farthest.
bool export_flanks(const pair_vector& ranked, const std::vector<uint64_t>& kmers, const std::vector<uint32_t>& flank,
                   uint32_t depth, uint32_t k, const std::string& path) {
    const size_t n = kmers.size(), D = depth;
    std::map<uint64_t, uint32_t> index;  // (the exact count's k-mers are distinct)
    for (uint32_t c = 0; c < n; ++c) index.emplace(kmers[c], c);
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::string line;
    auto group = [&](size_t side, size_t c, size_t j) {
        const uint32_t* g = flank.data() + ((side * n + c) * D + j) * 5;
        line += '\t';
        for (int s = 0; s < 5; ++s) line += (s ? "," : "") + std::to_string(g[s]);
    };
    for (const auto& kv : ranked) {
        const uint32_t c = index.at(kv.first);
        line = int2dna(kv.first, k);
        for (size_t j = D; j-- > 0;) group(1, c, j);
        for (size_t j = 0; j < D; ++j) group(0, c, j);
        line += '\n';
        std::fwrite(line.data(), 1, line.size(), f);
    }
    return std::fclose(f) == 0;
}

// --edits: one line per k-mer of `ranked`, the k-mer and k groups of 12 counts -- `edit` is the result of
// ac_window_edits_samples (n x k x 12, candidate c = kmers[c]): match, substituted by a,c,g,t,n, deleted,
// inserted after: a,c,g,t,n.
bool export_edits(const pair_vector& ranked, const std::vector<uint64_t>& kmers, const std::vector<uint32_t>& edit, uint32_t k,
                  const std::string& path) {
    const size_t n = kmers.size();
    std::map<uint64_t, uint32_t> index;  // (the exact count's k-mers are distinct)
    for (uint32_t c = 0; c < n; ++c) index.emplace(kmers[c], c);
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::string line;
    for (const auto& kv : ranked) {
        const uint32_t c = index.at(kv.first);
        line = int2dna(kv.first, k);
        for (size_t i = 0; i < k; ++i) {
            const uint32_t* g = edit.data() + ((size_t)c * k + i) * 12;
            line += '\t';
            for (int op = 0; op < 12; ++op) line += (op ? "," : "") + std::to_string(g[op]);
        }
        line += '\n';
        std::fwrite(line.data(), 1, line.size(), f);
    }
    return std::fclose(f) == 0;
}

// --cooccurrence: one line per k-mer of `ranked`, the k-mer and one count per k-mer of `ranked` in the same
// order -- `cooc` is the n x n result of ac_hit_cooccurrence over the job's top level plane, candidate c =
// kmers[c], permuted here into the main file's order.
bool export_cooccurrence(const pair_vector& ranked, const std::vector<uint64_t>& kmers, const std::vector<uint32_t>& cooc,
                         uint32_t k, const std::string& path) {
    const size_t n = kmers.size();
    std::map<uint64_t, uint32_t> index;  // (the exact count's k-mers are distinct)
    for (uint32_t c = 0; c < n; ++c) index.emplace(kmers[c], c);
    std::vector<uint32_t> order;
    for (const auto& kv : ranked) order.push_back(index.at(kv.first));
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::string line;
    for (size_t i = 0; i < order.size(); ++i) {
        line = int2dna(ranked[i].first, k);
        for (const uint32_t c : order) line += '\t' + std::to_string(cooc[(size_t)order[i] * n + c]);
        line += '\n';
        std::fwrite(line.data(), 1, line.size(), f);
    }
    return std::fclose(f) == 0;
}

// --cross-cooccurrence: one line per k-mer of the .start file (`rows`), the k-mer and one count per k-mer of the
// .end file (`cols`) in its order -- `cross` is the n_a x n_b result of ac_hit_cross_cooccurrence over the two
// jobs' top level planes, candidates kmers_a[a] and kmers_b[b], permuted here into the files' orders.
bool export_cross(const pair_vector& rows, const pair_vector& cols, const std::vector<uint64_t>& kmers_a,
                  const std::vector<uint64_t>& kmers_b, const std::vector<uint32_t>& cross, uint32_t k, const std::string& path) {
    const size_t nb = kmers_b.size();
    std::map<uint64_t, uint32_t> index_a, index_b;  // (the exact count's k-mers are distinct)
    for (uint32_t c = 0; c < kmers_a.size(); ++c) index_a.emplace(kmers_a[c], c);
    for (uint32_t c = 0; c < nb; ++c) index_b.emplace(kmers_b[c], c);
    std::vector<uint32_t> order_b;
    for (const auto& kv : cols) order_b.push_back(index_b.at(kv.first));
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::string line;
    for (const auto& kv : rows) {
        const size_t a = index_a.at(kv.first);
        line = int2dna(kv.first, k);
        for (const uint32_t b : order_b) line += '\t' + std::to_string(cross[a * nb + b]);
        line += '\n';
        std::fwrite(line.data(), 1, line.size(), f);
    }
    return std::fclose(f) == 0;
}

void open_devices(Devices& dev, uint64_t n_gpus, uint64_t max_errors) {
    if (dev.ctx) return;
    if (n_gpus < 1) n_gpus = 1;
    const int n_dev = ac_device_count();
    if (n_dev < 1) throw std::runtime_error("no HIP device available (the approximate count runs on the GPU only)");
    if ((int)n_gpus > n_dev)
        std::cerr << "/!\\ WARNING: " << n_gpus << " shards requested on " << n_dev << " visible GPU(s)\n";
    if (ac_create_multi(&dev.ctx, (int)n_gpus) != AC_OK) throw std::runtime_error(ac_last_error(nullptr));
    if (ac_set_max_errors(dev.ctx, (uint32_t)max_errors) != AC_OK) throw std::runtime_error(ac_last_error(dev.ctx));
    dev.shards = n_gpus;
}

// count_kmers + get_most_frequent / get_solid_kmers (approx_counter.cpp:874-899)
// on the GPU over a sample already uploaded to ctx (ac_exact_count_device).
pair_vector exact_count_gpu(ac_ctx* ctx, const ac_windows& dsample, uint32_t k, float lc, const kmer_set& forbidden,
                            uint64_t limit, uint64_t solid, uint64_t* n_distinct, uint64_t* had_n) {
    std::vector<uint64_t> fb(forbidden.begin(), forbidden.end());
    // Start small: a huge -lim (used to mean "keep all") must not allocate
    // `limit` entries up front; the call reports the size it needs.
    uint64_t cap = std::max<uint64_t>(1, solid ? 4096 : std::min<uint64_t>(limit, 4096));
    for (;;) {
        std::vector<uint64_t> km(cap), ct(cap);
        uint64_t n_out = 0;
        const ac_status st = ac_exact_count_device(ctx, k, &dsample, lc, fb.data(), (uint32_t)fb.size(), limit, solid,
                                                   km.data(), ct.data(), cap, &n_out, n_distinct, had_n);
        if (st == AC_ERR_INVALID && n_out > cap) {  // more kept k-mers than room
            cap = n_out;
            continue;
        }
        if (st != AC_OK) throw std::runtime_error(std::string("exact count failed: ") + ac_last_error(ctx));
        pair_vector out(n_out);
        for (uint64_t i = 0; i < n_out; ++i) out[i] = {km[i], ct[i]};
        return out;
    }
}

}  // namespace

int main(int argc, char const** argv) {
    Args args;
    const int pr = parse_args(argc, argv, args);
    if (pr != 0) return pr == 1;

    // Defaults (approx_counter.cpp:700-715)
    std::string output = "out.txt", exact_out, config_file, forbid_kmer;
    uint64_t solid_km = 0, nb_thread = 4, k = 16, sl = 100, sn = 40000, limit = 500, v = 1, nb_of_runs = 1;
    float param_lc = 1.0f, lc = 1.0f;
    bool skip_end = false;
    uint64_t n_gpus = 1, max_errors = 2, flank_depth = 0;
    std::string seed_str;

    // Config file (721-737): CLI > config > defaults
    get_option(args, "config", config_file);
    if (!config_file.empty()) {
        bool opened = false;
        arg_map p = parse_config(config_file, &opened);
        if (!opened) std::cerr << "/!\\ WARNING: Could not open config file\n";
        param_lc = p.count("lc") ? std::stof(p["lc"]) : lc;
        k = p.count("k") ? std::stoi(p["k"]) : k;
        v = p.count("v") ? std::stoi(p["v"]) : v;
        sn = p.count("sn") ? std::stoi(p["sn"]) : sn;
        sl = p.count("sl") ? std::stoi(p["sl"]) : sl;
        limit = p.count("lim") ? std::stoi(p["lim"]) : limit;
        nb_thread = p.count("nt") ? std::stoi(p["nt"]) : nb_thread;
        solid_km = p.count("sk") ? std::stoi(p["sk"]) : solid_km;
        skip_end = p.count("se") > 0;
        forbid_kmer = p.count("fk") ? p["fk"] : forbid_kmer;
        exact_out = p.count("e") ? p["e"] : exact_out;
        nb_of_runs = p.count("mr") ? std::stoi(p["mr"]) : nb_of_runs;
    }
    get_option(args, "limit", limit);
    get_option(args, "low_complexity", param_lc);
    get_option(args, "kmer_size", k);
    get_option(args, "verbosity", v);
    get_option(args, "sample_length", sl);
    get_option(args, "sample_n", sn);
    get_option(args, "nb_thread", nb_thread);
    get_option(args, "out_file", output);
    get_option(args, "exact_file", exact_out);
    get_option(args, "forbidden_kmer", forbid_kmer);
    get_option(args, "solid_km", solid_km);
    get_option(args, "multi_run", nb_of_runs);
    get_option(args, "gpus", n_gpus);
    get_option(args, "seed", seed_str);
    get_option(args, "max-errors", max_errors);
    get_option(args, "flanks", flank_depth);
    skip_end = skip_end || args.val.count("skip_end");
    const bool host_exact = args.val.count("host-exact") > 0;
    const bool levels = args.val.count("levels") > 0;
    const bool positions = args.val.count("positions") > 0;
    const bool spans = args.val.count("spans") > 0;
    const bool flanks = args.val.count("flanks") > 0;
    const bool edits = args.val.count("edits") > 0;
    const bool cooccurrence = args.val.count("cooccurrence") > 0;
    const bool paired = args.val.count("paired-sample") > 0;
    const bool cross = args.val.count("cross-cooccurrence") > 0;
    std::string dump_sample;
    get_option(args, "dump-sample", dump_sample);
    const std::string input_file = args.input;

    kmer_set forbidden;
    if (!forbid_kmer.empty()) {
        print("Parsing the fobidden kmer list");
        if (!parse_kmer_list(forbid_kmer, forbidden)) {
            std::cerr << "/!\\ ERROR: COULD NOT OPEN EXCLUDED KMER FILE, must quit\n";
            std::exit(1);
        }
    }
    const int mr_v = (nb_of_runs > 1 && v < 2) ? 0 : (int)v;
    const std::string warning = "/!\\ WARNING: ", error_pref = "/!\\ ERROR: ";
    if (k < 2 || k > 32) throw std::invalid_argument(error_pref + "kmer size must be between 2 and 32 (included)");
    if (k > sl) throw std::invalid_argument(error_pref + "kmer size must be smaller than the sampling length (k <= sl)");
    // --max-errors: checked here, before the input is parsed or a device opened.  Another budget than
    // the reference's counts only on the library's bit-sliced kernel (ac_set_max_errors,
    // include/approx_counter_amd.h): its k-mer sizes, equal windows of up to 256 bases (an end window is
    // sl + 1), the sample on one device.
    if (max_errors > 3) {
        std::cerr << error_pref << "--max-errors must be 0, 1, 2 or 3" << std::endl;
        return 1;
    }
    if (max_errors != 2) {
        const char* why = !(k == 16 || (k >= 18 && k <= 32))
                              ? "--max-errors other than 2 needs a kmer size (-k) of 16 or 18 to 32"
                          : sl > 255       ? "--max-errors other than 2 needs a sampling length (-sl) of at most 255"
                          : n_gpus > 1     ? "--max-errors other than 2 needs one GPU (-g 1)"
                          : host_exact     ? "--max-errors other than 2 cannot be combined with --host-exact"
                                           : nullptr;
        if (why) {
            std::cerr << error_pref << why << std::endl;
            return 1;
        }
    }
    // --paired-sample pairs the two ends; --cross-cooccurrence pairs rows of the two ends' hit matrices
    if (paired && skip_end) {
        std::cerr << error_pref << "--paired-sample cannot be combined with -se / --skip_end: there is no second end to pair"
                  << std::endl;
        return 1;
    }
    if (cross && !paired) {
        std::cerr << error_pref
                  << "--cross-cooccurrence needs --paired-sample: sampled on their own, the two ends' rows would be "
                     "different reads"
                  << std::endl;
        return 1;
    }
    // --levels: the hit levels come from the same kernel family under the same constraints
    // (ac_window_hits_samples); what only the sample can tell -- read ends of unequal length -- the
    // library refuses when the count is asked for.
    // --positions: the same kernels' sibling family, the same constraints and messages.
    // --spans: a pass over the positions call's matrices, so the same again.
    // --flanks: a pass over the spans call's matrices, so the same again; and its depth.
    // --edits: another pass over the spans call's matrices, so the same again.
    // --cooccurrence, --cross-cooccurrence: reductions of the same hit matrices, so the same again.
    const std::pair<const char*, bool> hit_flags[] = {{"--levels", levels},
                                                      {"--positions", positions},
                                                      {"--spans", spans},
                                                      {"--flanks", flanks},
                                                      {"--edits", edits},
                                                      {"--cooccurrence", cooccurrence},
                                                      {"--cross-cooccurrence", cross}};
    for (const auto& hf : hit_flags) {
        const char* flag = hf.first;
        if (!hf.second) continue;
        const char* why = !(k == 16 || (k >= 18 && k <= 32)) ? " needs a kmer size (-k) of 16 or 18 to 32"
                          : sl > 255                         ? " needs a sampling length (-sl) of at most 255"
                          : n_gpus > 1                       ? " needs one GPU (-g 1)"
                          : host_exact                       ? " cannot be combined with --host-exact"
                                                             : nullptr;
        if (why) {
            std::cerr << error_pref << flag << why << std::endl;
            return 1;
        }
    }
    if (flanks && (flank_depth < 1 || flank_depth > 32)) {
        std::cerr << error_pref << "--flanks needs a depth of 1 to 32" << std::endl;
        return 1;
    }
    lc = adjust_threshold(param_lc, 16, (uint32_t)k);

    if (v > 0) {
        std::cout << "Kmer size:             " << k << std::endl;
        std::cout << "Sampled sequences:     " << sn << std::endl;
        std::cout << "Sampling length        " << sl << std::endl;
        std::cout << "LC filter threshold:   " << param_lc << std::endl;
        std::cout << "Adjusted LC threshold: " << lc << std::endl;
        std::cout << "Nb thread:             " << nb_thread << std::endl;
        if (solid_km != 0) std::cout << "Solid kmers:           " << solid_km << std::endl;
        else std::cout << "Number of kept kmer:   " << limit << std::endl;
        std::cout << "Number of runs:        " << nb_of_runs << std::endl;
        std::cout << "Verbosity level:       " << v << std::endl;
    }
    int tab_level = 0;
    if (v > 0 && nb_of_runs > 1) std::cout << "\nA total of " << nb_of_runs << " runs will be performed." << std::endl;

    // Reads: by default only their sampling windows are kept, packed while the
    // file is parsed (read_windows); --host-exact keeps whole reads as the
    // reference does.  Both throw (uncaught, like SeqAn's IOError) on an
    // unreadable file.
    std::vector<std::string> ids;
    SeqSet seqs;
    WindowStore store;
    // The GPU contexts (the reference builds its index inside errorCount; the
    // device set is opened once).  Opening them (HIP runtime + device
    // initialisation, ~75 ms) runs on a helper thread while the input is parsed;
    // the first GPU stage waits for it and reports its failure, if any.
    Devices dev;
    std::future<void> dev_ready;
    if (dump_sample.empty()) dev_ready = std::async(std::launch::async, [&dev, n_gpus, max_errors] { open_devices(dev, n_gpus, max_errors); });
    auto devices = [&]() {
        if (dev_ready.valid()) dev_ready.get();  // rethrows the helper's exception
        open_devices(dev, n_gpus, max_errors);
    };
    if (v > 0) print("Parsing FASTA file", tab_level);
    if (host_exact) read_records(input_file, ids, seqs);
    else read_windows(input_file, sl, store);
    const uint64_t n_reads = host_exact ? seqs.size() : store.size();
    if (v > 0) print("Number of sequences found: " + std::to_string(n_reads) + ".", tab_level);

    std::mt19937 rng(seed_str.empty() ? std::random_device{}() : (uint32_t)std::strtoull(seed_str.c_str(), nullptr, 10));

    // One run samples both read ends, counts each end's k-mers exactly, then counts both
    // ends approximately in ONE fused launch (errorCount, approx_counter.cpp:922, for the
    // two iterations of the loop at 858-953, whose inputs are independent), and ranks and
    // exports each end.  Output files and their contents are the reference's; only the
    // order of the progress messages differs.
    struct End {
        std::string which;
        PackedImage img;
        ac_windows dsample{};
        pair_vector first_n;
    };
    for (uint64_t run = 0; run < nb_of_runs; ++run) {
        const std::string run_suffix = "_" + std::to_string(run);
        if (nb_of_runs > 1 && v > 0) std::cout << "Starting run number " << run + 1 << std::endl;
        if (sn > n_reads) {
            std::cerr << warning << "Sequence set too small for the requested sample size\n";
            std::cerr << warning << "The whole set will be used.\n";
            sn = n_reads;
        }
        bool bottom = false;
        tab_level += 1;
        std::vector<End> pending;
        // the approximate count of the pending ends, then their ranking and export
        auto flush = [&]() -> bool {
            if (pending.empty()) return true;
            std::vector<std::vector<uint64_t>> km(pending.size()), ct(pending.size());
            std::vector<ac_sample_job> jobs(pending.size());
            for (size_t e = 0; e < pending.size(); ++e) {
                if (mr_v > 0) print("Approximate k-mer count (" + pending[e].which + ")", tab_level);
                for (const auto& x : pending[e].first_n) km[e].push_back(x.first);
                ct[e].assign(km[e].size(), 0);
                jobs[e] = ac_sample_job{km[e].data(), (uint32_t)km[e].size(), ac_windows{}, ct[e].data()};
            }
            // --levels: the hits call in place of the plain count (the same launch yields the counts)
            std::vector<std::vector<uint32_t>> hits(pending.size());
            std::vector<uint32_t*> hits_p(pending.size());
            // --positions: the positions call, which yields the counts and the levels as well
            std::vector<std::vector<uint32_t>> pos(pending.size());
            std::vector<uint32_t*> pos_p(pending.size());
            // --spans: the spans call, which yields all of that and the start matrices
            std::vector<std::vector<uint32_t>> start(pending.size());
            std::vector<uint32_t*> start_p(pending.size());
            // --flanks: the flanks call, which yields all of that and the flank profiles
            std::vector<std::vector<uint32_t>> flank(pending.size());
            std::vector<uint32_t*> flank_p(pending.size());
            // --edits: the edits call, which yields all of that (the flank profiles when --flanks is given too) and
            // the edit profiles
            std::vector<std::vector<uint32_t>> edit(pending.size());
            std::vector<uint32_t*> edit_p(pending.size());
            // --cooccurrence: the hits call as well, then the top level plane's co-occurrence
            std::vector<std::vector<uint32_t>> cooc(pending.size());
            // --cross-cooccurrence: the hits call as well, then the two ends' top level planes against each other
            const bool do_cross = cross && pending.size() == 2;
            std::vector<uint32_t> cross_m;
            try {
                devices();
                const bool on_device = !host_exact && dev.shards == 1;  // the samples uploaded for the exact count
                for (size_t e = 0; e < pending.size(); ++e)
                    jobs[e].sample = on_device ? pending[e].dsample : view(pending[e].img);
                if (levels || positions || spans || flanks || edits || cooccurrence || cross)
                    for (size_t e = 0; e < pending.size(); ++e) {
                        hits[e].assign((size_t)ac_window_hits_words(jobs[e].n_kmers, jobs[e].sample.n_windows,
                                                                    (uint32_t)max_errors) + 1, 0u);
                        hits_p[e] = hits[e].data();
                        if (positions || spans || flanks || edits) {
                            pos[e].assign((size_t)ac_window_positions_words(jobs[e].n_kmers, jobs[e].sample.n_windows) + 1, 0u);
                            pos_p[e] = pos[e].data();
                        }
                        if (spans || flanks || edits) {
                            start[e].assign(pos[e].size(), 0u);
                            start_p[e] = start[e].data();
                        }
                        if (flanks) {
                            flank[e].assign((size_t)ac_hit_flank_words(jobs[e].n_kmers, (uint32_t)flank_depth) + 1, 0u);
                            flank_p[e] = flank[e].data();
                        }
                        if (edits) {
                            edit[e].assign((size_t)ac_hit_edit_words(jobs[e].n_kmers, (uint32_t)k) + 1, 0u);
                            edit_p[e] = edit[e].data();
                        }
                    }
                const ac_status st =
                    edits       ? ac_window_edits_samples(dev.ctx, (uint32_t)k, jobs.data(), (uint32_t)jobs.size(),
                                                          flanks ? (uint32_t)flank_depth : 0u, hits_p.data(), pos_p.data(),
                                                          start_p.data(), flanks ? flank_p.data() : nullptr, edit_p.data())
                    : flanks    ? ac_window_flanks_samples(dev.ctx, (uint32_t)k, jobs.data(), (uint32_t)jobs.size(),
                                                           (uint32_t)flank_depth, hits_p.data(), pos_p.data(), start_p.data(),
                                                           flank_p.data())
                    : spans     ? ac_window_spans_samples(dev.ctx, (uint32_t)k, jobs.data(), (uint32_t)jobs.size(), hits_p.data(),
                                                          pos_p.data(), start_p.data())
                    : positions ? ac_window_positions_samples(dev.ctx, (uint32_t)k, jobs.data(), (uint32_t)jobs.size(),
                                                              hits_p.data(), pos_p.data())
                    : levels || cooccurrence || cross
                        ? ac_window_hits_samples(dev.ctx, (uint32_t)k, jobs.data(), (uint32_t)jobs.size(), hits_p.data())
                    : on_device ? ac_error_count_samples(dev.ctx, (uint32_t)k, jobs.data(), (uint32_t)jobs.size())
                                : ac_error_count_images(dev.ctx, (uint32_t)k, jobs.data(), (uint32_t)jobs.size());
                if (st != AC_OK) throw std::runtime_error(ac_last_error(dev.ctx));
                if (cooccurrence)
                    for (size_t e = 0; e < pending.size(); ++e) {
                        const uint32_t n = jobs[e].n_kmers, nw = jobs[e].sample.n_windows;
                        cooc[e].assign((size_t)ac_hit_cooccurrence_words(n, 1) + 1, 0u);
                        // (plane E of the E + 1: one plane is ac_window_hits_words at budget 0)
                        const uint32_t* top = hits[e].data() + (size_t)max_errors * (size_t)ac_window_hits_words(n, nw, 0u);
                        if (ac_hit_cooccurrence(dev.ctx, top, n, nw, 1u, cooc[e].data()) != AC_OK)
                            throw std::runtime_error(ac_last_error(dev.ctx));
                    }
                if (do_cross) {
                    const uint32_t na = jobs[0].n_kmers, nb = jobs[1].n_kmers, nw = jobs[0].sample.n_windows;
                    if (jobs[1].sample.n_windows != nw)
                        throw std::runtime_error("--cross-cooccurrence: the two ends hold " + std::to_string(nw) + " and " +
                                                 std::to_string(jobs[1].sample.n_windows) + " windows, not the same reads");
                    cross_m.assign((size_t)ac_hit_cross_cooccurrence_words(na, nb, 1) + 1, 0u);
                    const uint32_t* top_a = hits[0].data() + (size_t)max_errors * (size_t)ac_window_hits_words(na, nw, 0u);
                    const uint32_t* top_b = hits[1].data() + (size_t)max_errors * (size_t)ac_window_hits_words(nb, nw, 0u);
                    if (ac_hit_cross_cooccurrence(dev.ctx, top_a, na, top_b, nb, nw, 1u, cross_m.data()) != AC_OK)
                        throw std::runtime_error(ac_last_error(dev.ctx));
                }
            } catch (const std::exception& e) {
                std::cerr << error_pref << "approximate count failed: " << e.what() << std::endl;
                return false;
            }
            std::vector<pair_vector> ranked(pending.size());
            for (size_t e = 0; e < pending.size(); ++e) {
                pair_vector error_counter(km[e].size());
                for (size_t i = 0; i < km[e].size(); ++i) error_counter[i] = {km[e][i], ct[e][i]};
                pair_vector sorted_error_count = get_most_frequent(std::move(error_counter), limit, (uint32_t)k);
                if (mr_v > 0) print("Exporting approximate count", tab_level);
                const std::string path = output + run_suffix + "." + pending[e].which;
                if (!export_counter(sorted_error_count, (uint32_t)k, path)) {
                    std::cerr << error_pref + "Failed to export approximate k-mer count" << std::endl;
                    std::cerr << "Path: " << path << std::endl;
                    return false;
                }
                if (levels && !export_levels(sorted_error_count, km[e], hits[e], jobs[e].sample.n_windows,
                                             (uint32_t)max_errors + 1, (uint32_t)k, path + ".levels")) {
                    std::cerr << error_pref + "Failed to export the hit levels" << std::endl;
                    std::cerr << "Path: " << path + ".levels" << std::endl;
                    return false;
                }
                if (positions &&
                    !export_positions(sorted_error_count, km[e], hits[e], pos[e], jobs[e].sample.n_windows,
                                      (uint32_t)max_errors + 1, pending[e].img.length.empty() ? 0u : pending[e].img.length[0],
                                      (uint32_t)k, path + ".positions")) {
                    std::cerr << error_pref + "Failed to export the match end positions" << std::endl;
                    std::cerr << "Path: " << path + ".positions" << std::endl;
                    return false;
                }
                if (spans &&
                    !export_spans(sorted_error_count, km[e], hits[e], pos[e], start[e], jobs[e].sample.n_windows,
                                  (uint32_t)max_errors + 1, pending[e].img.length.empty() ? 0u : pending[e].img.length[0],
                                  (uint32_t)k, path + ".starts", path + ".lengths")) {
                    std::cerr << error_pref + "Failed to export the match spans" << std::endl;
                    std::cerr << "Path: " << path + ".starts" << std::endl;
                    return false;
                }
                if (flanks && !export_flanks(sorted_error_count, km[e], flank[e], (uint32_t)flank_depth, (uint32_t)k,
                                             path + ".flanks")) {
                    std::cerr << error_pref + "Failed to export the flank profiles" << std::endl;
                    std::cerr << "Path: " << path + ".flanks" << std::endl;
                    return false;
                }
                if (edits && !export_edits(sorted_error_count, km[e], edit[e], (uint32_t)k, path + ".edits")) {
                    std::cerr << error_pref + "Failed to export the edit profiles" << std::endl;
                    std::cerr << "Path: " << path + ".edits" << std::endl;
                    return false;
                }
                if (cooccurrence && !export_cooccurrence(sorted_error_count, km[e], cooc[e], (uint32_t)k, path + ".cooc")) {
                    std::cerr << error_pref + "Failed to export the co-occurrence" << std::endl;
                    std::cerr << "Path: " << path + ".cooc" << std::endl;
                    return false;
                }
                if (mr_v > 0) print("Done", tab_level);
                ranked[e] = std::move(sorted_error_count);
            }
            if (do_cross) {
                const std::string path = output + run_suffix + ".cross";
                if (!export_cross(ranked[0], ranked[1], km[0], km[1], cross_m, (uint32_t)k, path)) {
                    std::cerr << error_pref + "Failed to export the cross co-occurrence" << std::endl;
                    std::cerr << "Path: " << path << std::endl;
                    return false;
                }
            }
            pending.clear();
            return true;
        };
        // --paired-sample: one draw for both ends, before the first
        std::pair<PackedImage, PackedImage> pair_img;
        std::pair<SeqSet, SeqSet> pair_seq;
        if (paired) {
            if (host_exact) {
                pair_seq = sample_sequences_pair(seqs, sn, sl, rng);
                pair_img = {pack_sample(pair_seq.first, 0, pair_seq.first.size()),
                            pack_sample(pair_seq.second, 0, pair_seq.second.size())};
            } else {
                pair_img = sample_windows_pair(store, sn, rng);
            }
        }
        for (const std::string which_end : {"start", "end"}) {
            if (v > 0) print("Working on sequence " + which_end + ".", tab_level - 1);
            if (mr_v > 0) print("Sampling", tab_level);
            if (mr_v > 0) print(bottom ? "Sampling the ends of reads" : "Sampling the start of reads", 1);
            End cur;
            cur.which = which_end;
            SeqSet sample;
            if (paired) {
                sample = std::move(bottom ? pair_seq.second : pair_seq.first);
                cur.img = std::move(bottom ? pair_img.second : pair_img.first);
            } else if (host_exact) {
                sample = sample_sequences(seqs, sn, sl, bottom, rng);
                cur.img = pack_sample(sample, 0, sample.size());
            } else {
                cur.img = sample_windows(store, sn, bottom, rng);
            }
            if (mr_v > 0) print("Sampled " + std::to_string(cur.img.size()) + " sequences", 1);
            if (!dump_sample.empty()) {
                if (!write_image(cur.img, dump_sample + run_suffix + "." + which_end)) {
                    std::cerr << error_pref << "could not write " << dump_sample + run_suffix + "." + which_end << "\n";
                    return 1;
                }
                if (!skip_end) bottom = true;
                else if (mr_v > 0) break;  // the -se quirk below
                continue;
            }
            if (mr_v > 0) print("Exact k-mer count", tab_level);
            uint64_t had_n = 0, n_found = 0;
            if (host_exact) {  // the reference's host stages (approx_counter.cpp:874-899)
                pair_vector count = count_kmers(sample, (uint32_t)k, lc, forbidden, &had_n);
                n_found = count.size();
                cur.first_n = solid_km != 0 ? get_solid_kmers(std::move(count), solid_km, (uint32_t)k)
                                            : get_most_frequent(std::move(count), limit, (uint32_t)k);
            } else {  // the same on GPU 0; the upload (one slot per end) also serves the approximate count
                try {
                    devices();
                    const ac_windows hw = view(cur.img);
                    if (ac_sample_upload_slot(dev.ctx, (int)pending.size(), &hw, &cur.dsample) != AC_OK)
                        throw std::runtime_error(ac_last_error(dev.ctx));
                    cur.first_n = exact_count_gpu(dev.ctx, cur.dsample, (uint32_t)k, lc, forbidden, limit, solid_km,
                                                  &n_found, &had_n);
                } catch (const std::exception& e) {
                    std::cerr << error_pref << "exact count failed: " << e.what() << std::endl;
                    // the reference exported the earlier end's approximate count before reaching this end
                    // (ADVICE r3): its own upload slot is intact, so count and write it first
                    flush();
                    return 1;
                }
            }
            if (had_n > 0) {
                std::cerr << "/!\\ WARNING: This dataset contained sequences with 'N' symbols. ";
                std::cerr << "/!\\ WARNING: Current implementation ignores k-mers containing 'N'.";
                std::cerr << "/!\\ WARNING: A total of " << had_n << " k-mers were ignored." << std::endl;
            }
            if (mr_v > 0) print("Number of kmer found: " + std::to_string(n_found), tab_level);
            if (mr_v > 0) print(solid_km != 0 ? "Keeping solid k-mer" : "Keeping most frequent k-mer", tab_level);
            if (mr_v > 0) print("Number of kmer kept:  " + std::to_string(cur.first_n.size()), tab_level);
            if (!exact_out.empty()) {
                if (mr_v > 0) print("Exporting exact kmer count", tab_level);
                if (!export_counter(cur.first_n, (uint32_t)k, exact_out + run_suffix + "." + which_end)) {
                    std::cerr << error_pref + "Failed to export exact k-mer count" << std::endl;
                    std::cerr << "Path: " << exact_out + run_suffix + "." + which_end << std::endl;
                    flush();  // the reference wrote the earlier end's approximate count before failing here
                    return 1;
                }
            }
            pending.push_back(std::move(cur));
            // approx_counter.cpp:943-951: the break only happens when verbose
            // (without it the second pass samples read STARTS again and writes
            // them to the .end file -- kept for drop-in fidelity).
            if (skip_end) {
                if (mr_v > 0) {
                    print("Skipping end adapter ressearch");
                    break;
                }
            } else {
                bottom = true;
            }
        }
        if (!flush()) return 1;
        tab_level--;
    }
    return 0;
}
