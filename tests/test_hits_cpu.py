"""Hit levels (ac_window_hits_*; DESIGN.md §4e "Hit levels") on the CPU: the expected-value helper pinned
to the oracle; the pure Python helpers on hand-built matrices; the level-count kernel's column counter
(hit_levels.h) and the plan layer's refusals (stage_plan.cpp hits_refusal) through stand-alone programs
built with g++ under the address and undefined-behaviour sanitizers; the four C-ABI symbols."""
import os
import struct
import subprocess

import numpy as np
import pytest

import approx_counter_amd as ac
import oracle
from approx_counter_amd import _lib
from tests import cases
from tests.hits_cases import expected_hits, pack_hits
from tests.test_budget_cpu import count_e

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


# ---- the expected-value helper ----------------------------------------------------------------------

@pytest.mark.parametrize("k", [16, 22, 32])
def test_helper_level_sums_are_the_counts(k):
    """Ragged windows, N, empty and short windows: the helper's level sums equal oracle.count_myers at
    E = 2 and count_e at E = 0, 1, 3, and its levels nest."""
    km, w = cases.planted_case(1200 + k, k, 37, 60, win_len=(k - 4, 110), p_n=0.01)
    w += ["", "A", "N" * k, cases.kmer_string(km[0], k)]
    hit, counts = expected_hits(k, km, w, 2)
    np.testing.assert_array_equal(counts, oracle.count_myers(k, km, w))
    for E in (0, 1, 3):
        hit, counts = expected_hits(k, km, w, E)
        assert hit.shape == (E + 1, len(w), len(km))
        np.testing.assert_array_equal(counts, count_e(E, k, km, w))
        assert not (hit[:-1] & ~hit[1:]).any()
    assert (hit[3] & ~hit[2]).any() and hit[0].any()


def test_helper_levels_are_the_references_bitfields():
    """One small case against the literal simulation of the reference's per-level bitfields
    (oracle.count_scheme(..., return_levels=True): bit e of levels[c][w] = tcount[e][w] of k-mer c)."""
    k = 16
    km, w = cases.planted_case(77, k, 12, 25, win_len=(30, 60), p_n=0.01)
    hit, counts = expected_hits(k, km, w, 2)
    want_counts, levels = oracle.count_scheme(k, km, w, return_levels=True)
    np.testing.assert_array_equal(counts, want_counts)
    for e in range(3):
        np.testing.assert_array_equal(hit[e], ((levels >> e) & 1).astype(bool).T, err_msg=f"level {e}")


# ---- the pure Python helpers ------------------------------------------------------------------------

@pytest.mark.parametrize("n_kmers", [1, 32, 33])
def test_unpack_and_distances_on_hand_built_matrices(n_kmers):
    """A matrix built word by word: window w holds candidate c at distance (w + c) % 5 (4: not within 3
    edits); bits past n_kmers are set in the words and must not come out."""
    E, nw, words = 3, 6, (n_kmers + 31) // 32
    assert ac.hits_words(n_kmers, nw, E) == (E + 1) * nw * words
    d = np.array([[(w + c) % 5 for c in range(n_kmers)] for w in range(nw)])
    m = np.zeros((E + 1, nw, words), np.uint32)
    for e in range(E + 1):
        for w in range(nw):
            for c in range(words * 32):
                if c >= n_kmers or d[w][c] <= e:
                    m[e, w, c // 32] |= np.uint32(1 << (c % 32))
    hit = ac.unpack_hits(m, n_kmers)
    assert hit.shape == (E + 1, nw, n_kmers) and hit.dtype == bool
    for e in range(E + 1):
        np.testing.assert_array_equal(hit[e], d <= e)
    np.testing.assert_array_equal(ac.distances_from_hits(hit), np.minimum(d, E + 1))
    wh = ac.WindowHits(None, m, n_kmers)
    assert wh.max_errors == E and wh.distances().dtype == np.uint8
    np.testing.assert_array_equal(wh.hit(1), d <= 1)
    np.testing.assert_array_equal(wh.distances(), np.minimum(d, 4))
    np.testing.assert_array_equal(wh.level_counts(), np.stack([(d <= e).sum(axis=0) for e in range(E + 1)]))
    np.testing.assert_array_equal(pack_hits(hit), m & pack_hits(np.ones_like(hit)))


def test_helpers_refuse_bad_matrices():
    with pytest.raises(ValueError):
        ac.unpack_hits(np.zeros((3, 4, 2), np.uint32), 32)  # (32 candidates are one word)
    hit = np.zeros((2, 1, 1), bool)
    hit[0, 0, 0] = True  # within 0 edits but not within 1
    with pytest.raises(ValueError):
        ac.distances_from_hits(hit)
    assert ac.hits_words(0, 5) == 0 and ac.hits_words(5, 0) == 0 and ac.hits_words(33, 7, 0) == 14


# ---- the column counter of the level-count kernel ---------------------------------------------------

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hc") / "hit_levels_check")
    subprocess.run(["g++"] + SANITIZE + ["-I" + CSRC, os.path.join(ROOT, "tools", "hit_levels_check.cpp"), "-o", exe],
                   check=True)
    return exe


def run_count(exe, tmp_path, m, n_kmers, slab):
    src, dst = tmp_path / "m.bin", tmp_path / "lc.bin"
    lv, nw, _ = m.shape
    with open(src, "wb") as fh:
        fh.write(struct.pack("<4I", n_kmers, nw, lv, slab))
        fh.write(np.ascontiguousarray(m, "<u4").tobytes())
    subprocess.run([exe, "count", str(src), str(dst)], check=True, timeout=120)
    out = np.fromfile(dst, dtype=np.uint32)
    return int(out[0]), int(out[1]), out[2:].reshape(lv, n_kmers)


def raw(exe, n, word):
    r = subprocess.run([exe, "raw", str(n), f"{word:x}"], check=True, capture_output=True, text=True, timeout=60)
    return [int(x) for x in r.stdout.split()]


def test_plane_counter_at_the_flush_threshold(tool):
    """Five planes hold 31 one-bit adds: hc_full turns true at 31 and not before, the count is exact
    there, and one add past it without a flush wraps to 0 -- the add the owner's flush must come before."""
    assert raw(tool, 30, 0x80000001) == [0, 30, 30]
    assert raw(tool, 31, 0x80000001) == [1, 31, 31]
    assert raw(tool, 32, 0x80000001) == [1, 0, 0]
    assert raw(tool, 31, 0x00000001) == [1, 31, 0]


@pytest.mark.parametrize("n_windows", [1, 30, 31, 32, 63, 64, 65, 300])
def test_column_counts_against_numpy(tool, tmp_path, n_windows):
    """Random planes of three densities and an all-ones plane (every counter reaches n_windows: through
    the flush at 31 adds and past it, in batches of 8 words and one by one), 33 and 70 candidates (a partial
    last word), each column counted in one walk, and in 64 and 7 interleaved walks of that stride (as the
    kernel's waves walk theirs: 64 | 65 windows leave 63 walks of one window and one of two)."""
    rng = np.random.default_rng(n_windows)
    for n_kmers in (33, 70):
        hit = np.stack([rng.random((n_windows, n_kmers)) < p for p in (0.02, 0.5, 0.97)] +
                       [np.ones((n_windows, n_kmers), bool)])
        m = pack_hits(hit)
        for slab in (1, 64, 7):
            planes, windows, got = run_count(tool, tmp_path, m, n_kmers, slab)
            assert planes == 5 and windows == 31
            np.testing.assert_array_equal(got, hit.sum(axis=1), err_msg=f"{n_kmers} {slab}")
            assert (got[3] == n_windows).all()


# ---- the plan layer's refusals ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hits") / "hits_plan_check")
    subprocess.run(["g++"] + SANITIZE + ["-pthread", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                                         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                                         os.path.join(ROOT, "tools", "hits_plan_check.cpp"),
                                         os.path.join(CSRC, "stage_plan.cpp"), os.path.join(CSRC, "host_pack.cpp"),
                                         "-o", exe], check=True)
    return exe


def plan(exe, E, k, *jobs, multi=0, **env):
    r = subprocess.run([exe, str(E), str(k), str(multi)] + list(jobs), capture_output=True, text=True, timeout=60,
                       check=True, env=dict(os.environ, **env))
    return r.stdout.strip()


def test_plan_accepts_and_refuses(plan_tool):
    """Hits at every budget 0..3 where the launch is bit-sliced; refused, with the constraint named, for
    ragged windows, an equal job beside a ragged one, windows over 256 bases, k <= 15, k = 17,
    AC_BITSLICE=0, a multi-device context and a budget over 3.  A job without candidates or windows is
    not live: its windows do not matter."""
    on = dict(AC_BITSLICE="1")
    for E in (0, 1, 2, 3):
        for k in (16, 18, 22, 32):
            assert plan(plan_tool, E, k, "300:100:37", **on) == "ok"
        assert plan(plan_tool, E, 22, "300:100:37", "40:101:9", "1:256:1", "5:1:3", **on) == "ok"
        assert plan(plan_tool, E, 22, "300:100:37", "0:r:9", "7:r:0", **on) == "ok"
        assert "ragged" in plan(plan_tool, E, 22, "300:r:37", **on)
        assert "ragged" in plan(plan_tool, E, 22, "none", **on)
        assert "ragged" in plan(plan_tool, E, 22, "300:100:37", "5:r:4", **on)
        assert "1..256" in plan(plan_tool, E, 22, "300:257:5", **on)
        assert "1..256" in plan(plan_tool, E, 22, "300:0:5", **on)
        for k in (15, 17, 8):
            assert "k = 16 or 18..32" in plan(plan_tool, E, k, "300:100:37", **on)
        assert "AC_BITSLICE" in plan(plan_tool, E, 22, "300:100:37", AC_BITSLICE="0")
        assert "single-device" in plan(plan_tool, E, 22, "300:100:37", multi=1, **on)
    assert plan(plan_tool, 4, 22, "300:100:37", **on).startswith("refused: max_errors must be 0..3")
    for line in (plan(plan_tool, 2, 17, "300:100:37", **on), plan(plan_tool, 2, 22, "300:r:37", **on)):
        assert line.startswith("refused: window hits need")


# ---- C ABI ------------------------------------------------------------------------------------------

def test_abi_symbols_and_null_arguments():
    """The four symbols are declared in the header and exported; a NULL context is refused; the word
    count is the layout's; the ABI version stays 8 (additive exports)."""
    L = _lib.load()
    names = {"ac_window_hits_words", "ac_window_hits_device", "ac_window_hits_samples", "ac_hit_level_counts_device"}
    assert names <= set(_lib.header_functions())
    assert all(hasattr(L, n) for n in names)
    assert L.ac_abi_version() == 8
    for nk, nw, E in ((1, 1, 0), (32, 7, 2), (33, 7, 3), (500, 37, 2), (0, 9, 2), (9, 0, 3)):
        assert L.ac_window_hits_words(nk, nw, E) == (E + 1) * nw * ((nk + 31) // 32) == ac.hits_words(nk, nw, E)
    assert L.ac_window_hits_words(2 ** 32 - 1, 2 ** 32 - 1, 3) == 4 * (2 ** 32 - 1) * 2 ** 27  # (no 32-bit wrap)
    assert L.ac_window_hits_device(None, 16, None, 0, None, None, None) == _lib.AC_ERR_INVALID
    assert L.ac_window_hits_samples(None, 16, None, 0, None) == _lib.AC_ERR_INVALID
    assert L.ac_hit_level_counts_device(None, None, 1, 1, 3, None, None) == _lib.AC_ERR_INVALID


def test_python_surface():
    import inspect

    assert callable(ac.ApproxCounter.window_hits) and callable(ac.ApproxCounter.hit_level_counts)
    assert inspect.signature(ac.ApproxCounter.count_device).parameters["hits"].default is None
    assert {"WindowHits", "hits_words", "unpack_hits", "distances_from_hits"} <= set(ac.__all__)


# ---- command line -----------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")


def cli(*args):
    return subprocess.run([CLI] + list(args) + [os.path.join(ROOT, "no_such_input.fasta")], capture_output=True,
                          text=True, timeout=60)


def test_cli_levels_is_refused_before_anything_is_opened():
    """--levels where the hits kernels cannot run: refused with the constraint named before the input is
    parsed (the file does not exist: parsing it would throw) or a device opened (none here)."""
    for k in ("17", "15"):
        r = cli("--levels", "-k", k)
        assert r.returncode == 1 and "--levels needs a kmer size (-k) of 16 or 18 to 32" in r.stderr, r.stderr
        assert "Parsing FASTA" not in r.stdout
    r = cli("--levels", "-k", "22", "-sl", "256")
    assert r.returncode == 1 and "--levels needs a sampling length (-sl) of at most 255" in r.stderr
    r = cli("--levels", "-g", "2")
    assert r.returncode == 1 and "--levels needs one GPU" in r.stderr
    r = cli("--levels", "--host-exact")
    assert r.returncode == 1 and "--levels cannot be combined with --host-exact" in r.stderr
    r = cli("--levels", "--max-errors", "4")
    assert r.returncode == 1 and "--max-errors must be 0, 1, 2 or 3" in r.stderr


def test_cli_help_lists_levels():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "    --levels\n" in r.stdout and ".levels" in r.stdout
