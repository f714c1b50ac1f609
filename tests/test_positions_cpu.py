"""Match end positions (ac_window_positions_*; DESIGN.md §4e "Match end positions") on the CPU: the
host-compiled NFA step with positions and the profile kernel's column walk (bs_pos.h) through
tools/bs_pos_check.cpp, and the plan layer's refusal of a NULL position matrix (stage_plan.cpp
positions_refusal) through tools/pos_plan_check.cpp -- stand-alone programs built with g++ under the
address and undefined-behaviour sanitizers; the expected-value helper; the pure Python helpers; the four
C-ABI symbols; the command line's preconditions."""
import os
import struct
import subprocess

import numpy as np
import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib
from tests import cases
from tests.positions_cases import (expected_positions, last_rows, pack_hits, pack_positions, positions_case,
                                   profile_of)
from tests.test_bs_nfa_k import LISTED_K
from tests.test_budget_cpu import write_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


# ---- the expected-value helper ----------------------------------------------------------------------

def test_last_row_by_hand():
    """ACGT against windows whose rows are easy to write down."""
    km = [cases.kmer_value("ACGT")]
    e = last_rows(4, km, ["ACGTACGT", "TTACGTTT", "ACGNACGA", "NNNNNNNN"])[:, 0]
    assert e[0].tolist() == [4, 3, 2, 1, 0, 1, 2, 1, 0]
    assert e[1].tolist() == [4, 3, 3, 3, 2, 1, 0, 1, 2]
    assert e[2].tolist() == [4, 3, 2, 1, 1, 2, 2, 1, 1]
    assert e[3].tolist() == [4] * 9


@pytest.mark.parametrize("E", [0, 1, 2, 3])
def test_the_standard_case_holds_every_planted_property(E):
    """40 k-mers x 30 windows x 100 bases, k = 16: every property of positions_case that the shape has room
    for is established (the builder asserts each; the DP's minimum is pinned to the oracle inside)."""
    km, w, hit, pos, counts, did = positions_case(500 + E, 16, 40, 30, 100, E)
    want = {"b", "e16", "e17", "e32", "h"} | ({"a", "c"} if E else set()) | ({"g"} if E == 3 else set())
    assert want <= did, (want - did)
    assert ((pos >= 1) == hit[E]).all() and (pos[~hit[E]] == -1).all() and pos.max() <= 100
    km, w, hit, pos, counts, did = positions_case(510 + E, 22, 40, 12, 255, E)
    assert {"d", "f128", "f129", "f255"} <= did, did


# ---- the NFA step with positions ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bsp") / "bs_pos_check")
    subprocess.run(["g++"] + SANITIZE + ["-I" + CSRC, os.path.join(ROOT, "tools", "bs_pos_check.cpp"), "-o", exe], check=True)
    return exe


def run_pos(exe, tmp_path, E, k, km, w):
    src, dst = tmp_path / "case.bin", tmp_path / f"out_{E}.bin"
    write_case(src, k, km, w)
    subprocess.run([exe, "pos", str(E), str(src), str(dst)], check=True, timeout=300)
    out = np.fromfile(dst, dtype=np.int32).reshape(len(w), len(km), 2)
    return out[:, :, 0], out[:, :, 1]


def window_lengths(k):
    return sorted({1, k - 3, k, 4 * ((k + 7) // 4) - 1, 4 * ((k + 7) // 4) + 1, 63, 65, 256})


@pytest.mark.parametrize("k", LISTED_K)
def test_nfa_positions_against_the_dp(tool, tmp_path, k):
    """Every listed K x E = 0..3 x window lengths 1, K - 3, K, 4 n - 1, 4 n + 1, 63, 65 and 256, 1 % N, 40
    candidates (a partial second block): the distance level and the position of every pair -- the kernel's
    form: blocks of 4 bases, the last one filled up with N, planes 0-1 per base and 2-7 per block, the
    stored word masked with ~a_E -- equal the Sellers DP's, and no bit is stored for a pair without a hit."""
    pairs = 0
    for L in window_lengths(k):
        for E in (0, 1, 2, 3):
            km, w, hit, pos, _, _ = positions_case(k * 1000 + L, k, 40, 14 if L < 256 else 8, L, E, p_n=0.01)
            d_got, p_got = run_pos(tool, tmp_path, E, k, km, w)
            d_want = np.where(hit[E], hit.shape[0] - hit.sum(axis=0), -1)
            np.testing.assert_array_equal(d_got, d_want, err_msg=f"levels k {k} L {L} E {E}")
            np.testing.assert_array_equal(p_got, np.where(pos > 0, pos, 0), err_msg=f"positions k {k} L {L} E {E}")
            pairs += int(hit[E].sum())
    assert pairs > 500


def test_n_inside_and_at_the_ends(tool, tmp_path):
    """An N inside an occurrence, before it and right after it, an all-N window, and the k-mer cut at the
    window's two ends: the positions with N in play."""
    k = 16
    km, _ = cases.planted_case(4, k, 33, 2, win_len=(40, 40), p_n=0.0)
    s = cases.kmer_string(km[3], k)
    pad = lambda t: (t + "C" * 40)[:40]  # noqa: E731
    w = [pad(s[:5] + "N" + s[6:]), pad("N" + s), pad(s + "N"), "N" * 40, pad(s[2:]), ("G" * 40 + s[:-2])[-40:],
         pad("NNN" + s[:8] + "N" + s[8:])]
    for E in (0, 1, 2, 3):
        hit, pos, _ = expected_positions(k, km, w, E)
        d_got, p_got = run_pos(tool, tmp_path, E, k, km, w)
        np.testing.assert_array_equal(d_got, np.where(hit[E], hit.shape[0] - hit.sum(axis=0), -1))
        np.testing.assert_array_equal(p_got, np.where(pos > 0, pos, 0))
    hit, pos, _ = expected_positions(k, km, w, 3)
    assert pos[1, 3] == 17 and pos[2, 3] == 16 and pos[0, 3] == 16 and (pos[3] == -1).all() and pos[5, 3] == 40


# ---- the profile kernel's column walk ----------------------------------------------------------------

def run_profile(exe, tmp_path, m, planes, n_kmers, L, walks):
    src, dst = tmp_path / "p.bin", tmp_path / "prof.bin"
    lv, nw, _ = m.shape
    with open(src, "wb") as fh:
        fh.write(struct.pack("<5I", n_kmers, nw, lv, L, walks))
        fh.write(np.ascontiguousarray(m, "<u4").tobytes())
        fh.write(np.ascontiguousarray(planes, "<u4").tobytes())
    subprocess.run([exe, "profile", str(src), str(dst)], check=True, timeout=120)
    return np.fromfile(dst, dtype=np.uint32).reshape(lv, n_kmers, L)


def random_planes(rng, n_kmers, n_windows, levels, L, junk=True):
    """Nested random levels and random positions below L; with `junk`, the words' bits past n_kmers are set
    in every plane (they must not come out)."""
    d = rng.integers(0, levels + 2, size=(n_windows, n_kmers))
    hit = np.stack([d <= e for e in range(levels)])
    pos = np.where(hit[-1], rng.integers(1, L + 1, size=d.shape), -1)
    m, planes = pack_hits(hit), pack_positions(pos)
    if junk and n_kmers % 32:
        top = np.uint32((0xFFFFFFFF << (n_kmers % 32)) & 0xFFFFFFFF)
        m[:, :, -1] |= top
        planes[:, :, -1] |= top
    return hit, pos, m, planes


@pytest.mark.parametrize("n_windows", [1, 7, 64, 300])
def test_profile_walk_against_numpy(tool, tmp_path, n_windows):
    rng = np.random.default_rng(n_windows)
    for n_kmers, levels, L in ((33, 4, 256), (70, 3, 100), (5, 1, 1)):
        hit, pos, m, planes = random_planes(rng, n_kmers, n_windows, levels, L)
        for walks in (1, 256, 7):
            got = run_profile(tool, tmp_path, m, planes, n_kmers, L, walks)
            np.testing.assert_array_equal(got, profile_of(hit, pos, L), err_msg=f"{n_kmers} {levels} {L} {walks}")
        np.testing.assert_array_equal(got.sum(axis=2)[0], hit[0].sum(axis=0))


def test_profile_walk_drops_positions_past_the_window(tool, tmp_path):
    rng = np.random.default_rng(5)
    hit, pos, m, planes = random_planes(rng, 40, 50, 3, 200)
    got = run_profile(tool, tmp_path, m, planes, 40, 120, 3)
    np.testing.assert_array_equal(got, profile_of(hit & (pos <= 120), pos, 120))


# ---- the pure Python helpers ------------------------------------------------------------------------

@pytest.mark.parametrize("n_kmers", [1, 32, 33])
def test_unpack_positions_on_hand_built_planes(n_kmers):
    """Planes built bit by bit: window w holds candidate c ending at 1 + (37 w + 11 c) % 256 when (w + c) % 3
    is not 0; bits of pairs without a hit and past n_kmers are set in the planes and must not come out."""
    nw, words = 9, (n_kmers + 31) // 32
    assert ac.positions_words(n_kmers, nw) == 8 * nw * words
    hit_E = np.array([[(w + c) % 3 != 0 for c in range(n_kmers)] for w in range(nw)])
    want = np.array([[1 + (37 * w + 11 * c) % 256 if hit_E[w][c] else -1 for c in range(n_kmers)] for w in range(nw)])
    planes = np.zeros((8, nw, words), np.uint32)
    for w in range(nw):
        for c in range(words * 32):
            v = (want[w][c] - 1) if c < n_kmers and hit_E[w][c] else 0xFF
            for b in range(8):
                if v >> b & 1:
                    planes[b, w, c // 32] |= np.uint32(1 << (c % 32))
    got = ac.unpack_positions(planes, hit_E, n_kmers)
    assert got.dtype == np.int16 and got.shape == (nw, n_kmers)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(pack_positions(want), planes & pack_hits(np.broadcast_to(hit_E, (8,) + hit_E.shape)))
    wh = ac.WindowHits(None, pack_hits(hit_E[None]), n_kmers, planes, 256)
    np.testing.assert_array_equal(wh.end_positions(), want)


def test_helpers_refuse_bad_planes():
    with pytest.raises(ValueError):
        ac.unpack_positions(np.zeros((7, 4, 1), np.uint32), np.zeros((4, 32), bool), 32)
    with pytest.raises(ValueError):
        ac.unpack_positions(np.zeros((8, 4, 2), np.uint32), np.zeros((4, 32), bool), 32)
    with pytest.raises(ValueError):
        ac.unpack_positions(np.zeros((8, 4, 1), np.uint32), np.zeros((5, 32), bool), 32)
    with pytest.raises(ValueError):
        ac.WindowHits(None, np.zeros((3, 4, 1), np.uint32), 32).end_positions()
    assert ac.positions_words(0, 5) == 0 and ac.positions_words(5, 0) == 0 and ac.positions_words(33, 7) == 112


# ---- the plan layer's refusal -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plan_tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pos") / "pos_plan_check")
    subprocess.run(["g++"] + SANITIZE + ["-pthread", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                                         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                                         os.path.join(ROOT, "tools", "pos_plan_check.cpp"),
                                         os.path.join(CSRC, "stage_plan.cpp"), os.path.join(CSRC, "host_pack.cpp"),
                                         "-o", exe], check=True)
    return exe


def plan(exe, E, k, *jobs, multi=0, **env):
    r = subprocess.run([exe, str(E), str(k), str(multi)] + list(jobs), capture_output=True, text=True, timeout=60,
                       check=True, env=dict(os.environ, **env))
    return r.stdout.strip()


def test_plan_refuses_a_null_position_matrix(plan_tool):
    """The hit levels' refusals, asked through positions_refusal (reused, not restated), and one more: a
    NULL position matrix for a segment with work.  A segment without work may have none."""
    on = dict(AC_BITSLICE="1")
    for E in (0, 1, 2, 3):
        assert plan(plan_tool, E, 22, "300:100:37", "40:101:9", **on) == "ok"
        assert plan(plan_tool, E, 22, "300:100:37", "0:r:9:0", "7:100:0:0", **on) == "ok"
        assert plan(plan_tool, E, 22, "300:100:37:0", **on) == "refused: window positions: pos[i] is NULL for a segment with work"
        assert "pos[i] is NULL" in plan(plan_tool, E, 16, "300:100:37", "40:101:9:0", **on)
        assert "ragged" in plan(plan_tool, E, 22, "300:r:37", **on)
        assert "ragged" in plan(plan_tool, E, 22, "none", **on)
        assert "1..256" in plan(plan_tool, E, 22, "300:257:5", **on)
        assert "k = 16 or 18..32" in plan(plan_tool, E, 17, "300:100:37", **on)
        assert "AC_BITSLICE" in plan(plan_tool, E, 22, "300:100:37", AC_BITSLICE="0")
        assert "single-device" in plan(plan_tool, E, 22, "300:100:37", multi=1, **on)
        # (the hits' constraint is named first)
        assert "ragged" in plan(plan_tool, E, 22, "300:r:37:0", **on)
    assert plan(plan_tool, 4, 22, "300:100:37", **on).startswith("refused: max_errors must be 0..3")


# ---- C ABI ------------------------------------------------------------------------------------------

def test_abi_symbols_and_null_arguments():
    L = _lib.load()
    names = {"ac_window_positions_words", "ac_window_positions_device", "ac_window_positions_samples",
             "ac_hit_position_profile_device"}
    assert names <= set(_lib.header_functions())
    assert all(hasattr(L, n) for n in names)
    assert L.ac_abi_version() == 8
    for nk, nw in ((1, 1), (32, 7), (33, 7), (500, 37), (0, 9), (9, 0)):
        assert L.ac_window_positions_words(nk, nw) == 8 * nw * ((nk + 31) // 32) == ac.positions_words(nk, nw)
    assert L.ac_window_positions_words(2 ** 32 - 1, 2 ** 32 - 1) == 8 * (2 ** 32 - 1) * 2 ** 27  # (no 32-bit wrap)
    assert L.ac_window_positions_device(None, 16, None, 0, None, None, None, None) == _lib.AC_ERR_INVALID
    assert L.ac_window_positions_samples(None, 16, None, 0, None, None) == _lib.AC_ERR_INVALID
    assert L.ac_hit_position_profile_device(None, None, None, 1, 1, 3, 100, None, None) == _lib.AC_ERR_INVALID


def test_python_surface():
    import inspect

    assert callable(ac.ApproxCounter.hit_position_profile)
    assert inspect.signature(ac.ApproxCounter.count_device).parameters["positions"].default is None
    assert inspect.signature(ac.ApproxCounter.window_hits).parameters["positions"].default is False
    assert {"positions_words", "unpack_positions"} <= set(ac.__all__)
    assert callable(ac.WindowHits.end_positions) and callable(ac.WindowHits.position_profile)


# ---- command line -----------------------------------------------------------------------------------

def cli(*args):
    return subprocess.run([CLI] + list(args) + [os.path.join(ROOT, "no_such_input.fasta")], capture_output=True,
                          text=True, timeout=60)


def test_cli_positions_is_refused_before_anything_is_opened():
    """--positions where the kernels cannot run: --levels' preconditions and messages, with the flag named."""
    for k in ("17", "15"):
        r = cli("--positions", "-k", k)
        assert r.returncode == 1 and "--positions needs a kmer size (-k) of 16 or 18 to 32" in r.stderr, r.stderr
        assert "Parsing FASTA" not in r.stdout
    r = cli("--positions", "-k", "22", "-sl", "256")
    assert r.returncode == 1 and "--positions needs a sampling length (-sl) of at most 255" in r.stderr
    r = cli("--positions", "-g", "2")
    assert r.returncode == 1 and "--positions needs one GPU" in r.stderr
    r = cli("--positions", "--host-exact")
    assert r.returncode == 1 and "--positions cannot be combined with --host-exact" in r.stderr
    r = cli("--positions", "--levels", "-k", "17")
    assert r.returncode == 1 and "needs a kmer size (-k) of 16 or 18 to 32" in r.stderr
    r = cli("--positions", "--max-errors", "4")
    assert r.returncode == 1 and "--max-errors must be 0, 1, 2 or 3" in r.stderr


def test_cli_help_lists_positions():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "    --positions\n" in r.stdout and ".positions" in r.stdout
