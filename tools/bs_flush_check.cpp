// bs_flush_check -- runs the host build of the bit-sliced count kernel's flush and table helpers
// (approx_counter_amd/csrc/bs_nfa.h: planes_add, planes_get, merged_first / merged_per_lane, neq_mask) on a
// case read from a file, for tests/test_bs_flush_cpu.py (host-only; built there with the sanitizers on).
//   bs_flush_check merge R LWSH IN OUT
//     One wave's flush.  IN : u32 n, then for each of the 64 lanes n x (u32 a0, a1, a2, a3, live): the
//          windows that lane added to its VCount since the last flush (levels a0 .. a[R-1], vc_add_r<R>).
//     The lanes are merged as bs_count.inc's bs_merge does it -- LW = 1 << LWSH lanes per window, lane %
//     LW the candidate block, partners 32, 16, .. LW lanes apart, one plane more per round -- and every
//     lane then takes its candidates of the block.
//     OUT: u32 planes the merge ended with; then per lane, in lane order, merged_per_lane(LWSH) x (u32 slot
//          = block * 32 + candidate, u32 value): the adds to the workgroup's count array.
//   bs_flush_check neq K IN OUT
//     IN : u32 n, then 64 u64 k-mer slots (those past n hold anything)
//     OUT: K x 4 u64: neq_mask<K>(slots, n, i, c) for i = 0 .. K - 1, c = 0 .. 3
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bs_nfa.h"
#include "bs_nfa_r.h"

namespace {

using namespace acamd;

std::vector<unsigned char> slurp(const char* path) {
    std::vector<unsigned char> buf;
    if (FILE* f = std::fopen(path, "rb")) {
        unsigned char tmp[4096];
        for (size_t n; (n = std::fread(tmp, 1, sizeof tmp, f)) > 0;) buf.insert(buf.end(), tmp, tmp + n);
        std::fclose(f);
    }
    return buf;
}

struct Reader {
    std::vector<unsigned char> buf;
    size_t at = 0;
    bool bad = false;
    template <class T>
    T get() {
        T v{};
        if (at + sizeof v <= buf.size()) std::memcpy(&v, buf.data() + at, sizeof v);
        else bad = true;
        at += sizeof v;
        return v;
    }
};

void put(FILE* out, uint32_t v) { std::fwrite(&v, sizeof v, 1, out); }

// bs_merge's rounds over the 64 lanes of a wave at once: lane l's partner of a round is lane l ^ D.
template <int N, uint32_t D>
void merge(const uint32_t (&p)[64][N], uint32_t lw, uint32_t (&m)[64][bs::VC_MERGED_PLANES], uint32_t& planes) {
    static_assert(N <= bs::VC_MERGED_PLANES, "planes");
    if constexpr (D >= 2u) {
        if (D >= lw) {
            static uint32_t sum[64][N + 1];
            for (uint32_t l = 0; l < 64u; ++l) bs::planes_add<N>(p[l], p[l ^ D], sum[l]);
            merge<N + 1, D / 2u>(sum, lw, m, planes);
            return;
        }
    }
    planes = N;
    for (uint32_t l = 0; l < 64u; ++l)
        for (int b = 0; b < bs::VC_MERGED_PLANES; ++b) m[l][b] = b < N ? p[l][b < N ? b : 0] : 0u;
}

template <int R>
int run_merge(uint32_t lwsh, Reader& in, FILE* out) {
    const uint32_t n = in.get<uint32_t>();
    if (in.bad || n > in.buf.size()) return 2;
    static uint32_t p[64][bs::VC_PLANES];
    for (uint32_t l = 0; l < 64u; ++l) {
        bs::VCount vc;
        bs::vc_clear(vc);
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t a[4], lv[R];
            for (uint32_t& x : a) x = in.get<uint32_t>();
            const uint32_t live = in.get<uint32_t>();
            if (in.bad) return 2;
            for (int r = 0; r < R; ++r) lv[r] = a[r];
            bs::vc_add_r<R>(vc, lv, live);
        }
        for (int b = 0; b < bs::VC_PLANES; ++b) p[l][b] = vc.p[b];
    }
    if (in.at != in.buf.size()) return 2;
    static uint32_t m[64][bs::VC_MERGED_PLANES];
    uint32_t planes = 0;
    merge<bs::VC_PLANES, 32u>(p, 1u << lwsh, m, planes);
    put(out, planes);
    for (uint32_t l = 0; l < 64u; ++l) {
        const uint32_t wl = l >> lwsh, blk = l & ((1u << lwsh) - 1u);
        const uint32_t j0 = bs::merged_first(lwsh, wl);
        for (uint32_t x = 0; x < bs::merged_per_lane(lwsh); ++x) {
            put(out, blk * 32u + j0 + x);
            put(out, bs::planes_get(m[l], j0 + x));
        }
    }
    return 0;
}

template <int K>
void run_neq(const uint64_t* km, uint32_t n, FILE* out) {
    for (uint32_t i = 0; i < (uint32_t)K; ++i)
        for (uint32_t c = 0; c < 4u; ++c) {
            const uint64_t m = bs::neq_mask<K>(km, n, i, c);
            std::fwrite(&m, sizeof m, 1, out);
        }
}

}  // namespace

int main(int argc, char** argv) {
    const bool mg = argc == 6 && !std::strcmp(argv[1], "merge");
    const bool nq = argc == 5 && !std::strcmp(argv[1], "neq");
    if (!mg && !nq) {
        std::fprintf(stderr, "usage: bs_flush_check merge R LWSH IN OUT | neq K IN OUT\n");
        return 2;
    }
    const unsigned long num = std::strtoul(argv[2], nullptr, 10);
    Reader in;
    in.buf = slurp(argv[argc - 2]);
    FILE* out = std::fopen(argv[argc - 1], "wb");
    if (!out) return 2;
    int rc = 2;
    if (mg) {
        const unsigned long lwsh = std::strtoul(argv[3], nullptr, 10);
        if (lwsh >= 1 && lwsh <= 5 && num >= 1 && num <= 4)
            rc = num == 4   ? run_merge<4>((uint32_t)lwsh, in, out)
                 : num == 3 ? run_merge<3>((uint32_t)lwsh, in, out)
                 : num == 2 ? run_merge<2>((uint32_t)lwsh, in, out)
                            : run_merge<1>((uint32_t)lwsh, in, out);
    } else {
        const uint32_t n = in.get<uint32_t>();
        uint64_t km[64];
        for (uint64_t& v : km) v = in.get<uint64_t>();
        if (!in.bad && in.at == in.buf.size() && n <= 64) {
            rc = 3;  // not an instantiated pattern length
#define AC_BS_RUN(KK)               \
    if (num == KK) {                \
        run_neq<KK>(km, n, out);    \
        rc = 0;                     \
    }
            AC_BS_K_LIST(AC_BS_RUN)
#undef AC_BS_RUN
        }
    }
    std::fclose(out);
    return rc;
}
