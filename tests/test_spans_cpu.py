"""Match spans (ac_hit_start_positions_device, ac_window_spans_samples; DESIGN.md §4e "Match spans") on the
CPU: the expected-value helper by hand, the case builder's properties, the host build of the per-pair step and
the hit word's walk (hit_span.h) through tools/hit_span_check.cpp -- a stand-alone program built with g++
under the address and undefined-behaviour sanitizers -- on real and on hostile planes, the pure Python helpers,
the two C-ABI symbols and the command line's preconditions."""
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib
from tests import cases
from tests.span_cases import (expected_spans, length_profile_of, pack_hits, pack_positions, pack_starts, plain_case,
                              spans_case)
from tests.test_bs_nfa_k import LISTED_K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


# ---- the expected-value helper ----------------------------------------------------------------------

def test_spans_by_hand():
    """ACGT against windows whose spans are easy to write down: an exact occurrence; the first base
    substituted (GCGT and CGT both qualify: the shorter wins); the first base missing at the window's first
    base; an N inside (the only substring at distance 1 is the whole ACNGT)."""
    km = [cases.kmer_value("ACGT")]
    hit, pos, start, _, nqual = expected_spans(4, km, ["TTACGTTT", "GGCGTAAA", "CGTAAAAA", "ACNGTAAA"], 1)
    assert (hit.shape[0] - hit.sum(axis=0))[:, 0].tolist() == [0, 1, 1, 1]
    assert pos[:, 0].tolist() == [6, 5, 3, 5]
    assert start[:, 0].tolist() == [2, 2, 0, 0]
    assert (pos - start)[:, 0].tolist() == [4, 3, 3, 5]
    assert nqual[:, 0].tolist() == [1, 2, 1, 1]


@pytest.mark.parametrize("E", [0, 1, 2, 3])
def test_the_standard_case_holds_every_planted_property(E):
    """40 k-mers x (30 + plants) windows x 100 bases: every property of spans_case that the shape has room for
    is established (the builder asserts each; the DP's minimum is pinned to the oracle inside)."""
    seams = {"s0", "s15", "s16", "s17", "s31", "s32", "s33", "sEnd"}
    for k in (16, 22, 32):
        km, w, hit, pos, start, counts, did = spans_case(600 + E, k, 40, 30, 100, E)
        want = seams | {"h", "len"} | {f"{n}{e}" for n in ("ins", "del") for e in range(1, E + 1)}
        want |= {"lead", "leadN", "clip", "multi"} if E else set()
        assert want <= did, (want - did)
        assert len(w) > 30 and ((start >= 0) == hit[E]).all() and (start[~hit[E]] == -1).all()
        ln = (pos - start)[hit[E]]
        d = (hit.shape[0] - hit.sum(axis=0))[hit[E]]
        assert ((ln >= k - d) & (ln <= k + d)).all()
        np.testing.assert_array_equal(length_profile_of(hit, pos, start, k).sum(axis=(0, 2)), hit[E].sum(axis=0))
    km, w, hit, pos, start, counts, did = spans_case(610 + E, 22, 40, 12, 255, E)
    assert {"s127", "s128", "s129", "sEnd"} <= did, did


# ---- the step and the walk --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("span") / "hit_span_check")
    subprocess.run(["g++"] + SANITIZE + ["-I" + CSRC, os.path.join(ROOT, "tools", "hit_span_check.cpp"), "-o", exe], check=True)
    return exe


def run_tool(exe, tmp_path, k, km, w, m, planes, levels):
    """`m`: (levels, n_windows, words) hit words; `planes`: (8, n_windows, words) position words."""
    src, dst = tmp_path / "span.bin", tmp_path / "start.bin"
    nk, nw, L = len(km), len(w), len(w[0])
    with open(src, "wb") as fh:
        fh.write(struct.pack("<5I", k, nk, nw, levels, L))
        fh.write(struct.pack(f"<{nk}Q", *[int(v) for v in km]))
        for x in w:
            fh.write(bytes("ACGT".index(c) if c in "ACGT" else 4 for c in x))
        fh.write(np.ascontiguousarray(m, "<u4").tobytes())
        fh.write(np.ascontiguousarray(planes, "<u4").tobytes())
    subprocess.run([exe, str(src), str(dst)], check=True, timeout=120)
    return np.fromfile(dst, dtype="<u4").reshape(8, nw, (nk + 31) // 32)


def window_lengths(k):
    return sorted({1, max(k - 3, 1), k, 63, 65, 256})


@pytest.mark.parametrize("k", list(LISTED_K) + [5, 17])
def test_step_and_walk_against_the_dp(tool, tmp_path, k):
    """Every listed K, and 5 and 17 (no count kernel's K: the pass runs at any), x E = 0..3 (levels < K) x
    window lengths 1, K - 3, K, 63, 65 and 256, 1 % N, 40 candidates (a partial second word): the start matrix
    from hit_span.h's walk and step equals the plain DP's, word for word."""
    pairs = multi = 0
    for L in window_lengths(k):
        for E in (0, 1, 2, 3):
            if k in LISTED_K:
                km, w, hit, pos, start, _, _ = spans_case(k * 1000 + L, k, 40, 14 if L < 256 else 8, L, E)
            else:
                km, w = plain_case(k * 1000 + L + E, k, 40, 14 if L < 256 else 8, L, E)
                hit, pos, start, _, nq = expected_spans(k, km, w, E)
                multi += int((nq > 1).sum())
            got = run_tool(tool, tmp_path, k, km, w, pack_hits(hit), pack_positions(pos), E + 1)
            np.testing.assert_array_equal(got, pack_starts(start, hit[E]), err_msg=f"k {k} L {L} E {E}")
            pairs += int(hit[E].sum())
    assert pairs > 300 and (k in LISTED_K or multi > 0)


def hostile_planes(k, seed=3):
    """A real case's planes (E = 2) with, per third of the pairs WITHOUT a hit: the top level's bit set where the
    position planes store 0 (pos = 1: no substring of one base is within 2 edits of a k-mer of 5 bases or
    more); the top bit set and a stored position past the window; a bit in levels 0 and 1 without the top
    one (planes that do not nest).  Returns (km, w, m, planes, want): `want` the start matrix of the real
    pairs alone -- the hostile ones must give 0 bits."""
    E, L = 2, 60 if k > 8 else 7  # (a short k-mer is within 2 edits of almost any longer window)
    km, w = plain_case(seed, k, 40, 12, L, E)
    hit, pos, start, _, _ = expected_spans(k, km, w, E)
    free = np.argwhere(~hit[E])
    assert len(free) >= 30
    h2 = hit.copy()
    past = np.zeros(hit[E].shape, bool)
    for i, (wi, c) in enumerate(free):
        if i % 3 == 0:
            h2[E, wi, c] = True           # (its position planes stay 0)
        elif i % 3 == 1:
            h2[E, wi, c] = True
            past[wi, c] = True
        else:
            h2[0, wi, c] = h2[1, wi, c] = True
    planes = pack_positions(np.where(hit[E], pos, -1))
    planes |= pack_positions(np.where(past, 200, -1))  # (199 stored: past the window)
    return km, w, pack_hits(h2), planes, pack_starts(start, hit[E])


@pytest.mark.parametrize("k", [5, 17])
def test_hostile_planes_give_no_bits(tool, tmp_path, k):
    """(and a clean sanitizer run: the tool's second pass has every window in buffers of exactly its size)"""
    km, w, m, planes, want = hostile_planes(k)
    got = run_tool(tool, tmp_path, k, km, w, m, planes, 3)
    np.testing.assert_array_equal(got, want)
    # stray bits past n_kmers in every plane are not walked either
    top = np.uint32((0xFFFFFFFF << (40 % 32)) & 0xFFFFFFFF)
    m[:, :, -1] |= top
    planes[:, :, -1] |= top
    np.testing.assert_array_equal(run_tool(tool, tmp_path, k, km, w, m, planes, 3), want)


def test_tool_refuses_malformed_input(tool, tmp_path):
    src = tmp_path / "bad.bin"
    src.write_bytes(struct.pack("<5I", 4, 1, 1, 4, 8))  # (levels >= k)
    assert subprocess.run([tool, str(src), str(tmp_path / "o.bin")], timeout=60).returncode == 2


# ---- the pure Python helpers ------------------------------------------------------------------------

@pytest.mark.parametrize("n_kmers", [1, 32, 33])
def test_helpers_on_hand_built_planes(n_kmers):
    """Planes built bit by bit: window w holds candidate c at distance (w + c) % 4 (3 = no hit, E = 2), its
    occurrence starting at (37 w + 11 c) % 200 with length k - d + (w % (2 d + 1)); bits of pairs without a
    hit and past n_kmers are set in the planes and must not come out."""
    k, E, nw, words = 16, 2, 9, (n_kmers + 31) // 32
    d = np.array([[(w + c) % 4 for c in range(n_kmers)] for w in range(nw)])
    hit = np.stack([d <= e for e in range(E + 1)])
    start = np.array([[(37 * w + 11 * c) % 200 for c in range(n_kmers)] for w in range(nw)])
    ln = np.array([[k - d[w][c] + (w % (2 * d[w][c] + 1)) for c in range(n_kmers)] for w in range(nw)])
    start, ln = np.where(hit[E], start, -1), np.where(hit[E], ln, -1)
    end = np.where(hit[E], start + ln, -1)
    junk = ~pack_hits(np.broadcast_to(hit[E], (8,) + hit[E].shape))
    sp, pp = pack_starts(start, hit[E]) | junk, pack_positions(end) | junk
    got = ac.unpack_starts(sp, hit[E], n_kmers)
    assert got.dtype == np.int16 and got.shape == (nw, n_kmers)
    np.testing.assert_array_equal(got, start)
    wh = ac.WindowHits(None, pack_hits(hit), n_kmers, pp, 256, starts=sp, k=k)
    np.testing.assert_array_equal(wh.start_positions(), start)
    np.testing.assert_array_equal(wh.end_positions(), end)
    lens = wh.span_lengths()
    assert lens.dtype == np.int16
    np.testing.assert_array_equal(lens, ln)
    prof = wh.length_profile()
    assert prof.dtype == np.uint32 and prof.shape == (E + 1, n_kmers, 2 * E + 1)
    np.testing.assert_array_equal(prof, length_profile_of(hit, end, start, k))
    np.testing.assert_array_equal(prof.sum(axis=(0, 2)), hit[E].sum(axis=0))


def test_helpers_refuse_what_they_cannot_answer():
    wh = ac.WindowHits(None, np.zeros((3, 4, 1), np.uint32), 32, np.zeros((8, 4, 1), np.uint32), 100)
    for fn in (wh.start_positions, wh.span_lengths, wh.length_profile, wh.start_profile):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(ValueError):
        ac.unpack_starts(np.zeros((7, 4, 1), np.uint32), np.zeros((4, 32), bool), 32)
    with pytest.raises(ValueError):  # (a start matrix, but no k)
        ac.WindowHits(None, np.zeros((3, 4, 1), np.uint32), 32, np.zeros((8, 4, 1), np.uint32), 100,
                      starts=np.zeros((8, 4, 1), np.uint32)).length_profile()


def test_python_surface():
    assert callable(ac.ApproxCounter.hit_start_positions)
    assert inspect.signature(ac.ApproxCounter.count_device).parameters["spans"].default is None
    assert inspect.signature(ac.ApproxCounter.window_hits).parameters["spans"].default is False
    # (the jobs stage has no spans: its image keeps N in inline records the pass does not decode)
    assert "spans" not in inspect.signature(ac.ApproxCounter.window_hits_jobs).parameters
    assert "unpack_starts" in ac.__all__
    for name in ("start_positions", "span_lengths", "length_profile", "start_profile"):
        assert callable(getattr(ac.WindowHits, name))
    assert "not built" in ac.ApproxCounter.window_hits_jobs.__doc__ and "window_hits(..., spans=True)" in \
        ac.ApproxCounter.window_hits_jobs.__doc__
    with pytest.raises(ValueError, match="spans come with hits and positions"):
        ac.ApproxCounter.count_device(None, 16, [], spans=[])


# ---- C ABI ------------------------------------------------------------------------------------------

def test_abi_symbols_and_null_arguments():
    L = _lib.load()
    names = {"ac_hit_start_positions_device", "ac_window_spans_samples"}
    assert names <= set(_lib.header_functions())
    assert all(hasattr(L, n) for n in names)
    assert L.ac_abi_version() == 8
    assert L.ac_hit_start_positions_device(None, 16, None, 0, None, 100, None, None, 3, None, None) == _lib.AC_ERR_INVALID
    assert L.ac_window_spans_samples(None, 16, None, 0, None, None, None) == _lib.AC_ERR_INVALID


# ---- command line -----------------------------------------------------------------------------------

def cli(*args):
    return subprocess.run([CLI] + list(args) + [os.path.join(ROOT, "no_such_input.fasta")], capture_output=True,
                          text=True, timeout=60)


def test_cli_spans_is_refused_before_anything_is_opened():
    """--spans where the kernels cannot run: --positions' preconditions and messages, with the flag named."""
    for k in ("17", "15"):
        r = cli("--spans", "-k", k)
        assert r.returncode == 1 and "--spans needs a kmer size (-k) of 16 or 18 to 32" in r.stderr, r.stderr
        assert "Parsing FASTA" not in r.stdout
    r = cli("--spans", "-k", "22", "-sl", "256")
    assert r.returncode == 1 and "--spans needs a sampling length (-sl) of at most 255" in r.stderr
    r = cli("--spans", "-g", "2")
    assert r.returncode == 1 and "--spans needs one GPU" in r.stderr
    r = cli("--spans", "--host-exact")
    assert r.returncode == 1 and "--spans cannot be combined with --host-exact" in r.stderr
    r = cli("--spans", "--positions", "--levels", "-k", "17")
    assert r.returncode == 1 and "needs a kmer size (-k) of 16 or 18 to 32" in r.stderr
    r = cli("--spans", "--max-errors", "4")
    assert r.returncode == 1 and "--max-errors must be 0, 1, 2 or 3" in r.stderr


def test_cli_help_lists_spans():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "    --spans\n" in r.stdout and ".starts" in r.stdout and ".lengths" in r.stdout
