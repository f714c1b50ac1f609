"""Cross co-occurrence (ac_hit_cross_cooccurrence*; DESIGN.md §4e "Cross co-occurrence") on the CPU: the
kernel's arithmetic (hit_cross.h over hit_cooc.h: the full tile grid, the thread's sums, the launch rule) through
a stand-alone program built with g++ under the address and undefined-behaviour sanitizers, against numpy; the
four C-ABI symbols; the Python surface; paired sampling through the command line's --dump-sample (which stops
before any device call); the command line's refusals."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib
from tests.hits_cases import pack_hits
from tests.test_cooc_cpu import gram, stray
from tests.test_hits_cpu import SANITIZE
from tests.test_reader import decode, dump, load_image, write_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")


def cross(hit_a, hit_b):
    """uint32 (levels, n_a, n_b) of two bool (levels, n_windows, n): H_a^t H_b per plane, in float32 -- exact,
    every sum being an integer below 2^24."""
    assert hit_a.shape[:2] == hit_b.shape[:2] and hit_a.shape[1] < 1 << 24
    return np.stack([a.T @ b for a, b in zip(hit_a.astype(np.float32), hit_b.astype(np.float32))]).astype(np.uint32)


def planes(rng, n_windows, n):
    """Densities 0.5 and 0.03, all ones, all zero."""
    return np.stack([rng.random((n_windows, n)) < 0.5, rng.random((n_windows, n)) < 0.03,
                     np.ones((n_windows, n), bool), np.zeros((n_windows, n), bool)])


# ---- the host-compiled core -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cross") / "hit_cross_check")
    subprocess.run(["g++"] + SANITIZE + ["-I" + CSRC, os.path.join(ROOT, "tools", "hit_cross_check.cpp"), "-o", exe],
                   check=True)
    return exe


def run_cross(exe, tmp_path, ma, n_a, mb, n_b):
    src, dst = tmp_path / "m.bin", tmp_path / "out.bin"
    lv, nw, _ = ma.shape
    assert mb.shape[:2] == (lv, nw)
    with open(src, "wb") as fh:
        fh.write(struct.pack("<4I", n_a, n_b, nw, lv))
        fh.write(np.ascontiguousarray(ma, "<u4").tobytes())
        fh.write(np.ascontiguousarray(mb, "<u4").tobytes())
    subprocess.run([exe, "cross", str(src), str(dst)], check=True, timeout=300)
    out = np.fromfile(dst, dtype=np.uint32)
    assert out.size == lv * n_a * n_b
    return out.reshape(lv, n_a, n_b)


@pytest.mark.parametrize("n_windows", [1, 32, 33, 257])
def test_core_against_numpy(tool, tmp_path, n_windows):
    """The program's product over four planes (densities 0.5 and 0.03, all ones, all zero) with the stray bits
    of both matrices set, at every (n_a, n_b) of {1, 32, 33, 70} x {1, 33, 64, 65, 130}: one word, a full one and
    a partial second; one tile, a full one, a partial second and third."""
    rng = np.random.default_rng(n_windows)
    for n_a in (1, 32, 33, 70):
        for n_b in (1, 33, 64, 65, 130):
            ha, hb = planes(rng, n_windows, n_a), planes(rng, n_windows, n_b)
            got = run_cross(tool, tmp_path, stray(pack_hits(ha), n_a), n_a, stray(pack_hits(hb), n_b), n_b)
            np.testing.assert_array_equal(got, cross(ha, hb), err_msg=f"{n_a} x {n_b}")
            assert (got[2] == n_windows).all() and not got[3].any()


def rule(exe, n_a, n_b, n_windows, levels):
    r = subprocess.run([exe, "rule", str(n_a), str(n_b), str(n_windows), str(levels)], check=True, capture_output=True,
                       text=True, timeout=60)
    return tuple(int(x) for x in r.stdout.split())


def test_core_on_the_split_walk(tool, tmp_path):
    """70 x 130 over 3 slabs of windows (2049): the launch rule splits the window axis in two, the partial
    sums add up."""
    rng = np.random.default_rng(5)
    ha = np.stack([rng.random((2049, 70)) < 0.5, np.ones((2049, 70), bool)])
    hb = np.stack([rng.random((2049, 130)) < 0.03, np.ones((2049, 130), bool)])
    assert rule(tool, 70, 130, 2049, 2)[:2] == (2, 2)
    got = run_cross(tool, tmp_path, stray(pack_hits(ha), 70), 70, stray(pack_hits(hb), 130), 130)
    np.testing.assert_array_equal(got, cross(ha, hb))


def test_launch_rule(tool):
    """(splits, slabs a workgroup, slabs, tiles): co_splits' rule over tiles_a x tiles_b x levels workgroups.
    Up to 2048 windows (one or two slabs) never split; 4096 workgroups and more never split: at four planes
    32 x 31 tiles (2048 x 1984) are 3968, split, and 32 x 32 (2048 x 1985) are 4096, not."""
    assert rule(tool, 70, 300, 5000, 3) == (3, 2, 5, 10)
    assert rule(tool, 70, 70, 2049, 3) == (2, 2, 3, 4)
    for nw in (1, 1024, 1025, 2048):
        for shape in ((1, 1), (70, 300), (2048, 1984)):
            assert rule(tool, *shape, nw, 1)[0] == 1
    assert rule(tool, 2048, 1984, 2049, 4) == (2, 2, 3, 32 * 31)
    assert rule(tool, 2048, 1985, 2049, 4) == (1, 3, 3, 32 * 32)
    assert rule(tool, 1, 2000, 100000, 1) == (49, 2, 98, 32)   # a lopsided shape: its 32 tiles, cut to the floor
    assert rule(tool, 0, 9, 9, 3)[0] == 1 and rule(tool, 9, 0, 9, 3)[0] == 1 and rule(tool, 9, 9, 0, 3)[0] == 1


# ---- C ABI ------------------------------------------------------------------------------------------

PUBLIC = {"ac_hit_cross_cooccurrence_words", "ac_hit_cross_cooccurrence_device", "ac_hit_cross_cooccurrence"}


def test_abi_symbols_and_null_arguments():
    L = _lib.load()
    assert PUBLIC <= set(_lib.header_functions())
    assert all(hasattr(L, n) for n in PUBLIC | {"ac_testing_hit_cross_stages"})
    assert L.ac_abi_version() == 8
    assert L.ac_hit_cross_cooccurrence_words(33, 7, 3) == 693 == ac.cross_cooccurrence_words(33, 7, 3)
    assert L.ac_hit_cross_cooccurrence_words(0, 7, 3) == 0 and L.ac_hit_cross_cooccurrence_words(7, 0, 3) == 0
    assert L.ac_hit_cross_cooccurrence_words(2 ** 20, 2 ** 20, 4) == 2 ** 42  # (no 32-bit wrap)
    assert L.ac_hit_cross_cooccurrence_device(None, None, 1, None, 1, 1, 1, None, None) == _lib.AC_ERR_INVALID
    assert b"ctx is NULL" in L.ac_last_error(None)
    assert L.ac_hit_cross_cooccurrence(None, None, 1, None, 1, 1, 1, None) == _lib.AC_ERR_INVALID
    assert L.ac_testing_hit_cross_stages(None, None, 1, None, 1, 1, 1, None, 3, None) == _lib.AC_ERR_INVALID


# ---- Python surface ---------------------------------------------------------------------------------

def test_python_surface():
    assert "cross_cooccurrence_words" in ac.__all__
    for name in ("hit_cross_cooccurrence", "cross_cooccurrence_host"):
        assert callable(getattr(ac.ApproxCounter, name))
    assert callable(ac.WindowHits.cross_cooccurrence)
    assert ac.cross_cooccurrence_words(33, 7) == 231 and ac.cross_cooccurrence_words(0, 7, 3) == 0


def nested(rng, n_windows, n):
    """bool (3, n_windows, n) whose levels nest, as a hits launch's do."""
    h0 = rng.random((n_windows, n)) < 0.05
    h1 = h0 | (rng.random((n_windows, n)) < 0.3)
    return np.stack([h0, h1, h1 | (rng.random((n_windows, n)) < 0.4)])


@pytest.mark.parametrize("n_a,n_b", [(1, 33), (33, 70), (70, 1)])
def test_window_hits_without_a_counter_use_numpy(n_a, n_b):
    """Hand-built WindowHits (no counter attached), stray bits set: x.cross(x) is x.cooccurrence(); a.cross(b) is
    b.cross(a) transposed and the numpy product, at the default (top) levels and at given ones; the level-pair
    form x.cross(x, 0, E) has level_counts()[0] as its diagonal; unequal window counts and levels past E raise."""
    rng = np.random.default_rng(100 * n_a + n_b)
    ha, hb = nested(rng, 50, n_a), nested(rng, 50, n_b)[:2]
    a = ac.WindowHits(None, stray(pack_hits(ha), n_a), n_a)
    b = ac.WindowHits(None, stray(pack_hits(hb), n_b), n_b)
    got = a.cross_cooccurrence(b)
    assert got.dtype == np.uint32 and got.shape == (n_a, n_b)
    np.testing.assert_array_equal(got, cross(ha[2:3], hb[1:2])[0])
    np.testing.assert_array_equal(got, b.cross_cooccurrence(a).T)
    np.testing.assert_array_equal(a.cross_cooccurrence(b, 0, 1), cross(ha[0:1], hb[1:2])[0])
    np.testing.assert_array_equal(a.cross_cooccurrence(b, 1, 0), b.cross_cooccurrence(a, 0, 1).T)
    for x, h in ((a, ha), (b, hb)):
        np.testing.assert_array_equal(x.cross_cooccurrence(x), x.cooccurrence())
        np.testing.assert_array_equal(x.cross_cooccurrence(x), gram(h)[-1])
        pair = x.cross_cooccurrence(x, 0, x.max_errors)
        np.testing.assert_array_equal(pair, cross(h[0:1], h[-1:])[0])
        np.testing.assert_array_equal(np.diag(pair), x.level_counts()[0])
    other = ac.WindowHits(None, pack_hits(nested(rng, 49, n_b)), n_b)
    with pytest.raises(ValueError):
        a.cross_cooccurrence(other)
    for e, eo in ((3, None), (-1, None), (None, 2), (0, -1)):
        with pytest.raises(ValueError):
            a.cross_cooccurrence(b, e, eo)


# ---- paired sampling through the command line -------------------------------------------------------

SL = 24


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """(path, reads): about 60 reads of lengths from below 2 SL up to several hundred, a few holding N, the
    eligible ones (length >= 2 SL) with distinct first SL and last SL + 1 bases."""
    rng = random.Random(77)
    lengths = [0, 5, SL, SL + 1, 2 * SL - 1, 2 * SL - 1, 2 * SL, 2 * SL, 2 * SL + 1] + [rng.randint(2 * SL, 400) for _ in range(51)]
    rng.shuffle(lengths)
    seqs = ["".join(rng.choice("ACGT") for _ in range(n)) for n in lengths]
    for i in (3, 17, 29, 44):  # N at the very ends, where the windows are
        if len(seqs[i]) >= 2:
            seqs[i] = "N" + seqs[i][1:-2] + "N" + seqs[i][-1:]
    elig = [s for s in seqs if len(s) >= 2 * SL]
    assert len({s[:SL] for s in elig}) == len(elig) == len({s[-(SL + 1):] for s in elig})
    assert any("N" in s for s in elig) and len(elig) < len(seqs)
    path = tmp_path_factory.mktemp("paired") / "reads.fa"
    write_reads(path, seqs, "fa", width=60)
    return path, seqs


def images(tmp_path, inp, tag, extra):
    files = dump(tmp_path, inp, tag, ["-sl", SL, "-k", 8, "-v", 0] + extra)
    assert files == [f"{tag}_0.end", f"{tag}_0.start"]
    return tuple(open(tmp_path / f"{tag}_0.{end}", "rb").read() for end in ("start", "end"))


@pytest.mark.parametrize("sn", [20, 1000])
def test_paired_sample_draws_both_ends_from_the_same_reads(tmp_path, reads, sn):
    """--paired-sample --dump-sample: window i of the start image is the first SL bases and window i of the end
    image the last SL + 1 bases of the same read, for every i; the reads are distinct and eligible, min(sn,
    eligible) of them; --host-exact dumps the same images; another seed picks another order."""
    inp, seqs = reads
    elig = {s[:SL]: s for s in seqs if len(s) >= 2 * SL}
    seen = []
    for seed in (5, 6):
        images(tmp_path, inp, f"p{seed}", ["-sn", sn, "--seed", seed, "--paired-sample"])
        start = decode(load_image(tmp_path / f"p{seed}_0.start"))
        end = decode(load_image(tmp_path / f"p{seed}_0.end"))
        assert len(start) == len(end) == min(sn, len(elig))
        assert len(set(start)) == len(start)
        for i, (s, e) in enumerate(zip(start, end)):
            assert s in elig, f"window {i}: not the start of an eligible read"
            assert e == elig[s][-(SL + 1):], f"window {i}: the end window is another read's"
        host = images(tmp_path, inp, f"h{seed}", ["-sn", sn, "--seed", seed, "--paired-sample", "--host-exact"])
        assert host == tuple(open(tmp_path / f"p{seed}_0.{x}", "rb").read() for x in ("start", "end"))
        seen.append(start)
    assert seen[0] != seen[1]


DRAW_SRC = r"""
// The default sampling's documented draw order: one mt19937 seeded once, sample_windows for the start windows,
// then sample_windows for the end windows (each its own shuffle), written as --dump-sample writes them.
#include <cstdio>
#include <cstdlib>
#include <string>
#include "host_stages.h"
using namespace achost;
static void put(const PackedImage& p, const std::string& path) {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    const uint64_t hdr[2] = {p.size(), p.n_bases};
    std::fwrite(hdr, sizeof hdr, 1, f);
    std::fwrite(p.start.data(), 8, p.size(), f);
    std::fwrite(p.length.data(), 4, p.size(), f);
    std::fwrite(p.codes.data(), 4, p.codes.size(), f);
    std::fwrite(p.nmask.data(), 4, p.nmask.size(), f);
    std::fclose(f);
}
int main(int, char** argv) {
    WindowStore ws;
    read_windows(argv[1], std::strtoull(argv[2], nullptr, 10), ws, 1);
    const uint64_t sn = std::strtoull(argv[3], nullptr, 10);
    std::mt19937 rng((uint32_t)std::strtoull(argv[4], nullptr, 10));
    put(sample_windows(ws, sn, false, rng), std::string(argv[5]) + ".start");
    put(sample_windows(ws, sn, true, rng), std::string(argv[5]) + ".end");
    return 0;
}
"""


@pytest.fixture(scope="module")
def draw_tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("draw")
    src, exe = str(d / "draw.cpp"), str(d / "draw")
    with open(src, "w") as fh:
        fh.write(DRAW_SRC)
    host = os.path.join(CSRC, "host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + host, src,
                    os.path.join(host, "host_stages.cpp"), "-o", exe, "-pthread"], check=True)
    return exe


def test_default_sampling_keeps_its_draw_order(tmp_path, reads, draw_tool):
    """Without --paired-sample the two dumped images are what one rng, seeded once, gives sample_windows for the
    start and then for the end -- two shuffles, in that order -- at two seeds.  The paired start image is the
    first of those shuffles too (the same first draw, the same eligibility here); its end image is not the second."""
    inp, _ = reads
    for seed in (5, 6):
        got = images(tmp_path, inp, f"d{seed}", ["-sn", 20, "--seed", seed])
        subprocess.run([draw_tool, str(inp), str(SL), "20", str(seed), str(tmp_path / f"w{seed}")], check=True, timeout=60)
        want = tuple(open(tmp_path / f"w{seed}.{end}", "rb").read() for end in ("start", "end"))
        assert got == want
        paired = images(tmp_path, inp, f"q{seed}", ["-sn", 20, "--seed", seed, "--paired-sample"])
        assert paired[0] == got[0] and paired[1] != got[1]


# ---- command line refusals --------------------------------------------------------------------------

def cli(*args):
    return subprocess.run([CLI] + list(args) + [os.path.join(ROOT, "no_such_input.fasta")], capture_output=True,
                          text=True, timeout=60)


def test_cli_refusals_come_before_anything_is_opened():
    """Each exits 1 with the constraint named, before the input is parsed (the file does not exist) or a device
    opened (none here)."""
    cases = [
        (["--cross-cooccurrence"], "--cross-cooccurrence needs --paired-sample"),
        (["--paired-sample", "-se"], "--paired-sample cannot be combined with -se"),
        (["--cross-cooccurrence", "--paired-sample", "-se"], "--paired-sample cannot be combined with -se"),
        (["--cross-cooccurrence", "--paired-sample", "--host-exact"], "--cross-cooccurrence cannot be combined with --host-exact"),
        (["--cross-cooccurrence", "--paired-sample", "-g", "2"], "--cross-cooccurrence needs one GPU"),
        (["--cross-cooccurrence", "--paired-sample", "-k", "17"], "--cross-cooccurrence needs a kmer size (-k) of 16 or 18 to 32"),
        (["--cross-cooccurrence", "--paired-sample", "-k", "22", "-sl", "300"],
         "--cross-cooccurrence needs a sampling length (-sl) of at most 255"),
    ]
    for args, msg in cases:
        r = cli(*args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
        assert "Parsing FASTA" not in r.stdout
    assert "different reads" in cli("--cross-cooccurrence").stderr


def test_cli_help_lists_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "    --paired-sample\n" in r.stdout and "    --cross-cooccurrence\n" in r.stdout
    assert ".cross" in r.stdout
