"""Co-occurrence (ac_hit_cooccurrence*, ac_hit_window_counts_device; DESIGN.md §4e "Co-occurrence") on the
CPU: the kernels' arithmetic (hit_cooc.h: the 32 x 32 bit transposition, the tile's inner product, the tile-pair
numbering, the launch rule) through a stand-alone program built with g++ under the address and
undefined-behaviour sanitizers, against numpy; the four C-ABI symbols; the Python surface; the command line's
refusals."""
import os
import struct
import subprocess

import numpy as np
import pytest

import approx_counter_amd as ac
from approx_counter_amd import _lib
from tests.hits_cases import pack_hits
from tests.test_hits_cpu import SANITIZE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
CLI = os.path.join(ROOT, "approx_counter_amd", "bin", "adaptFinder")
SLAB_WINDOWS = 1024  # windows of one slab of the transposed planes (32 x CO_SLAB)


def gram(hit):
    """uint32 (levels, n, n) of bool (levels, n_windows, n): H^t H per plane, in float32 -- exact, every sum
    being an integer below 2^24 -- so that BLAS does it."""
    assert hit.shape[1] < 1 << 24
    h = hit.astype(np.float32)
    return np.stack([p.T @ p for p in h]).astype(np.uint32)


def stray(m, n_kmers):
    """The matrix with every bit past n_kmers set in the rows' last words."""
    m = m.copy()
    if n_kmers % 32:
        m[:, :, -1] |= np.uint32((0xFFFFFFFF << (n_kmers % 32)) & 0xFFFFFFFF)
    return m


def planes(rng, n_windows, n_kmers):
    """Densities 0.5 and 0.03, all ones, all zero."""
    return np.stack([rng.random((n_windows, n_kmers)) < 0.5, rng.random((n_windows, n_kmers)) < 0.03,
                     np.ones((n_windows, n_kmers), bool), np.zeros((n_windows, n_kmers), bool)])


# ---- the host-compiled core -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cooc") / "hit_cooc_check")
    subprocess.run(["g++"] + SANITIZE + ["-I" + CSRC, os.path.join(ROOT, "tools", "hit_cooc_check.cpp"), "-o", exe],
                   check=True)
    return exe


def run_cooc(exe, tmp_path, m, n_kmers):
    """(T, cooc, window_counts) of the program: T (levels, rows, t_words)."""
    src, dst = tmp_path / "m.bin", tmp_path / "out.bin"
    lv, nw, _ = m.shape
    with open(src, "wb") as fh:
        fh.write(struct.pack("<3I", n_kmers, nw, lv))
        fh.write(np.ascontiguousarray(m, "<u4").tobytes())
    subprocess.run([exe, "cooc", str(src), str(dst)], check=True, timeout=300)
    out = np.fromfile(dst, dtype=np.uint32)
    rows, tw = int(out[0]), int(out[1])
    a, b = 2 + lv * rows * tw, 2 + lv * rows * tw + lv * n_kmers * n_kmers
    assert out.size == b + lv * nw
    return out[2:a].reshape(lv, rows, tw), out[a:b].reshape(lv, n_kmers, n_kmers), out[b:].reshape(lv, nw)


def bit_transpose(hit, rows, tw):
    """numpy's bit transpose of bool (levels, n_windows, n): uint32 (levels, rows, tw), bit w % 32 of word
    w // 32 of row c = hit[w][c]; zero rows and bits past the matrix."""
    lv, nw, n = hit.shape
    t = np.zeros((lv, rows, tw * 32), np.uint8)
    t[:, :n, :nw] = hit.transpose(0, 2, 1)
    return np.packbits(t, axis=-1, bitorder="little").view("<u4").reshape(lv, rows, tw).astype(np.uint32)


@pytest.mark.parametrize("n_windows", [1, 31, 32, 33, 63, 64, 65, 257])
def test_core_against_numpy(tool, tmp_path, n_windows):
    """The transposed planes, the product and the window counts of the program over four planes (densities 0.5
    and 0.03, all ones, all zero) with stray bits past n_kmers set, at 1, 32, 33 and 70 candidates (one word,
    a full word, a partial second and third; 70: two product tiles, so an off-diagonal tile and its mirror)."""
    rng = np.random.default_rng(n_windows)
    for n_kmers in (1, 32, 33, 70):
        hit = planes(rng, n_windows, n_kmers)
        T, cooc, wc = run_cooc(tool, tmp_path, stray(pack_hits(hit), n_kmers), n_kmers)
        assert T.shape[1] == (n_kmers + 31) // 32 * 32 and T.shape[2] == 32 * -(-n_windows // SLAB_WINDOWS)
        np.testing.assert_array_equal(T, bit_transpose(hit, T.shape[1], T.shape[2]), err_msg=f"T {n_kmers}")
        np.testing.assert_array_equal(cooc, gram(hit), err_msg=f"cooc {n_kmers}")
        np.testing.assert_array_equal(wc, hit.sum(axis=2), err_msg=f"window counts {n_kmers}")
        assert (cooc[2] == n_windows).all() and not cooc[3].any()


def test_core_on_the_split_path(tool, tmp_path):
    """3 slabs of windows (2049): the launch rule splits the window axis in two, the partial sums add up."""
    rng = np.random.default_rng(5)
    hit = np.stack([rng.random((2049, 70)) < 0.5, np.ones((2049, 70), bool)])
    assert rule(tool, 70, 2049, 2)[:2] == (2, 2)
    _, cooc, _ = run_cooc(tool, tmp_path, stray(pack_hits(hit), 70), 70)
    np.testing.assert_array_equal(cooc, gram(hit))


def rule(exe, n_kmers, n_windows, levels):
    r = subprocess.run([exe, "rule", str(n_kmers), str(n_windows), str(levels)], check=True, capture_output=True,
                       text=True, timeout=60)
    return tuple(int(x) for x in r.stdout.split())


def test_launch_rule(tool):
    """(splits, slabs a workgroup, slabs, tile pairs).  One or two slabs: never split.  From three on the
    window axis is cut, two slabs a workgroup at least, until the launch has 4096 workgroups; 4096 tile pairs
    x planes and more are never split.  These are the thresholds tests/test_gpu_cooc.py straddles."""
    assert rule(tool, 70, 1024, 3) == (1, 1, 1, 3)
    assert rule(tool, 70, 1025, 3) == (1, 2, 2, 3)
    assert rule(tool, 70, 2048, 3) == (1, 2, 2, 3)
    assert rule(tool, 70, 2049, 3) == (2, 2, 3, 3)
    assert rule(tool, 300, 5000, 3) == (3, 2, 5, 15)
    assert rule(tool, 300, 70001, 3) == (35, 2, 69, 15)
    assert rule(tool, 2000, 100000, 1) == (8, 13, 98, 528)      # 4224 workgroups
    assert rule(tool, 3264, 2049, 3) == (2, 2, 3, 1326)         # 3978 tile pairs x planes: split
    assert rule(tool, 3265, 2049, 3) == (1, 3, 3, 1378)         # 4134: not
    assert rule(tool, 0, 9, 3)[0] == 1 and rule(tool, 9, 0, 3)[0] == 1


# ---- C ABI ------------------------------------------------------------------------------------------

NAMES = {"ac_hit_cooccurrence_words", "ac_hit_cooccurrence_device", "ac_hit_cooccurrence", "ac_hit_window_counts_device"}


def test_abi_symbols_and_null_arguments():
    L = _lib.load()
    assert NAMES <= set(_lib.header_functions())
    assert all(hasattr(L, n) for n in NAMES)
    assert L.ac_abi_version() == 8
    assert L.ac_hit_cooccurrence_words(33, 3) == 3267 == ac.cooccurrence_words(33, 3)
    assert L.ac_hit_cooccurrence_words(0, 3) == 0 and L.ac_hit_cooccurrence_words(0, 0) == 0
    assert L.ac_hit_cooccurrence_words(2 ** 20, 4) == 2 ** 42  # (no 32-bit wrap)
    assert L.ac_hit_cooccurrence_device(None, None, 1, 1, 1, None, None) == _lib.AC_ERR_INVALID
    assert L.ac_hit_cooccurrence(None, None, 1, 1, 1, None) == _lib.AC_ERR_INVALID
    assert L.ac_hit_window_counts_device(None, None, 1, 1, 1, None, None) == _lib.AC_ERR_INVALID
    assert b"ctx is NULL" in L.ac_last_error(None)


# ---- Python surface ---------------------------------------------------------------------------------

def test_python_surface():
    assert {"cooccurrence_words", "WindowHits", "ApproxCounter"} <= set(ac.__all__)
    for name in ("hit_cooccurrence", "hit_window_counts"):
        assert callable(getattr(ac.ApproxCounter, name))
    assert ac.cooccurrence_words(33) == 1089 and ac.cooccurrence_words(0, 3) == 0


@pytest.mark.parametrize("n_kmers", [1, 33, 70])
def test_window_hits_without_a_counter_uses_numpy(n_kmers):
    """A hand-built WindowHits (no counter attached): cooccurrence() of every plane, the default being the top
    one, and window_counts() equal the numpy product and the row sums; stray bits are ignored; a level past
    E is rejected."""
    rng = np.random.default_rng(n_kmers)
    hit = np.stack([rng.random((50, n_kmers)) < p for p in (0.05, 0.3, 0.6)])
    wh = ac.WindowHits(None, stray(pack_hits(hit), n_kmers), n_kmers)
    want = gram(hit)
    for e in range(3):
        got = wh.cooccurrence(e)
        assert got.dtype == np.uint32 and got.shape == (n_kmers, n_kmers)
        np.testing.assert_array_equal(got, want[e])
        np.testing.assert_array_equal(np.diag(got), wh.level_counts()[e])
    np.testing.assert_array_equal(wh.cooccurrence(), want[2])
    np.testing.assert_array_equal(wh.window_counts(), hit.sum(axis=2))
    assert wh.window_counts().shape == (3, 50)
    for e in (3, -1):
        with pytest.raises(ValueError):
            wh.cooccurrence(e)


# ---- command line -----------------------------------------------------------------------------------

def cli(*args):
    return subprocess.run([CLI] + list(args) + [os.path.join(ROOT, "no_such_input.fasta")], capture_output=True,
                          text=True, timeout=60)


def test_cli_cooccurrence_is_refused_before_anything_is_opened():
    """--cooccurrence where the hits kernels cannot run: refused with the constraint named before the input is
    parsed (the file does not exist: parsing it would throw) or a device opened (none here)."""
    for k in ("17", "15"):
        r = cli("--cooccurrence", "-k", k)
        assert r.returncode == 1 and "--cooccurrence needs a kmer size (-k) of 16 or 18 to 32" in r.stderr, r.stderr
        assert "Parsing FASTA" not in r.stdout
    r = cli("--cooccurrence", "-k", "22", "-sl", "300")
    assert r.returncode == 1 and "--cooccurrence needs a sampling length (-sl) of at most 255" in r.stderr
    r = cli("--cooccurrence", "-g", "2")
    assert r.returncode == 1 and "--cooccurrence needs one GPU" in r.stderr
    r = cli("--cooccurrence", "--host-exact")
    assert r.returncode == 1 and "--cooccurrence cannot be combined with --host-exact" in r.stderr
    for r in (cli("--cooccurrence", "--host-exact"), cli("--cooccurrence", "-g", "2")):
        assert "Parsing FASTA" not in r.stdout
    # (combined with --levels the first flag of the loop names itself)
    r = cli("--cooccurrence", "--levels", "-k", "17")
    assert r.returncode == 1 and "--levels needs a kmer size" in r.stderr


def test_cli_help_lists_cooccurrence():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "    --cooccurrence\n" in r.stdout and ".cooc" in r.stdout
