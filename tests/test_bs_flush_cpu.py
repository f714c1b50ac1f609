"""The bit-sliced count kernel's flush by plane merge and its ~Eq table masks (bs_nfa.h: planes_add,
planes_get, merged_first / merged_per_lane, neq_mask) on the CPU: the helpers the kernel
runs, through tools/bs_flush_check.cpp, built with g++ under the address and undefined-behaviour
sanitizers and run as a child process.  Expected values are plain integer sums and the mask's definition."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from tests.test_bs_nfa_k import LISTED_K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approx_counter_amd", "csrc")
SANITIZE = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
M = 0xFFFFFFFF
VC_PLANES = 5


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bsflush") / "bs_flush_check")
    subprocess.run(["g++"] + SANITIZE + ["-I" + CSRC, os.path.join(ROOT, "tools", "bs_flush_check.cpp"), "-o", exe],
                   check=True)
    return exe


# ---- the plane merge and the extraction -----------------------------------------------------------

def levels(R, s):
    """The hit words a0 .. a3 (bit clear = level hit) of a window that adds s[j] (0..R) to candidate j:
    the levels nest, so s hits are levels R - s .. R - 1."""
    return [M & ~sum(1 << j for j in range(32) if r >= R - s[j]) for r in range(R)] + [M] * (4 - R)


def run_merge(exe, tmp_path, R, lwsh, lanes):
    """lanes: 64 lists of n (a0, a1, a2, a3, live).  -> (planes, [(lane, slot, value)])"""
    n = len(lanes[0])
    assert len(lanes) == 64 and all(len(x) == n for x in lanes)
    src, dst = tmp_path / "merge.bin", tmp_path / "merge.out"
    with open(src, "wb") as fh:
        fh.write(struct.pack("<I", n))
        for lane in lanes:
            for add in lane:
                fh.write(struct.pack("<5I", *add))
    subprocess.run([exe, "merge", str(R), str(lwsh), str(src), str(dst)], check=True, timeout=60)
    out = np.fromfile(dst, dtype=np.uint32)
    per = 32 >> (6 - lwsh)
    assert len(out) == 1 + 64 * per * 2
    rec = out[1:].reshape(64, per, 2)
    return int(out[0]), [(lane, int(s), int(v)) for lane in range(64) for s, v in rec[lane]]


def check_merge(exe, tmp_path, R, lwsh, lanes, sums):
    """sums[lane][j]: what lane's windows add to candidate j of its block -- the adds must be the blocks'
    plain sums over their lanes, each slot added once, by a lane of its own block."""
    LW = 1 << lwsh
    planes, adds = run_merge(exe, tmp_path, R, lwsh, lanes)
    assert planes == VC_PLANES + (6 - lwsh)
    want = np.zeros(32 * LW, np.int64)
    for lane in range(64):
        want[(lane % LW) * 32:(lane % LW) * 32 + 32] += sums[lane]
    assert sorted(s for _, s, _ in adds) == list(range(32 * LW)), "every slot once: no two lanes on one word"
    for lane, s, v in adds:
        assert s // 32 == lane % LW, "a lane adds candidates of its own block"
        assert v == want[s], f"R {R} LW {LW} slot {s}"
    return want


def vc_windows(R):
    return (2 ** VC_PLANES - 1) // R


@pytest.mark.parametrize("lwsh", [1, 2, 3])
@pytest.mark.parametrize("R", [1, 3, 4])
def test_merge_at_the_threshold(tool, tmp_path, R, lwsh):
    """Every lane's counters at the flush threshold -- vc_windows(R) windows that hit every level, for
    every candidate: 30 per lane at R = 3, 28 at R = 4, 31 at R = 1 -- merged over the 64 / LW lanes of a
    block: 30 x 32 = 960 at LW = 2, past nine planes."""
    n = vc_windows(R)
    add = tuple(levels(R, [R] * 32)) + (M,)
    want = check_merge(tool, tmp_path, R, lwsh, [[add] * n] * 64, [np.full(32, R * n)] * 64)
    assert (want == R * n * (64 >> lwsh)).all()
    if (R, lwsh) == (3, 1):
        assert want[0] == 960 and 960 >= 1 << 9


@pytest.mark.parametrize("lwsh", [1, 2, 3])
@pytest.mark.parametrize("R", [3, 4])
def test_merge_against_plain_sums(tool, tmp_path, R, lwsh):
    """Mixed adds of 0..R per candidate, lanes without a window (live = 0), candidates that only some lanes
    count, and a different number of hits in every lane."""
    rng = random.Random(10 * R + lwsh)
    n = vc_windows(R)
    lanes, sums = [], []
    for lane in range(64):
        adds, tot = [], np.zeros(32, np.int64)
        for _ in range(n):
            s = [rng.randint(0, R) if rng.random() < lane / 63 or lane == 63 else 0 for _ in range(32)]
            live = 0 if lane % 7 == 3 else rng.getrandbits(32) | (M if rng.random() < 0.5 else 0)
            adds.append(tuple(levels(R, s)) + (live,))
            tot += np.array([s[j] if live >> j & 1 else 0 for j in range(32)])
        lanes.append(adds)
        sums.append(tot)
    want = check_merge(tool, tmp_path, R, lwsh, lanes, sums)
    assert want.any() and len(set(want.tolist())) > 8


def test_merge_of_single_lanes(tool, tmp_path):
    """One lane of a block holds a count and the others none, for each lane in turn: the sum reaches the
    lane that extracts that candidate whichever lane it started in."""
    for lwsh in (1, 3):
        for src in (0, 1, 31, 32, 62, 63):
            s = [(j * 5 + src) % 4 for j in range(32)]
            lanes = [[tuple(levels(3, s if lane == src else [0] * 32)) + (M,)] for lane in range(64)]
            sums = [np.array(s if lane == src else [0] * 32) for lane in range(64)]
            check_merge(tool, tmp_path, 3, lwsh, lanes, sums)


# ---- the ~Eq mask ---------------------------------------------------------------------------------

def run_neq(exe, tmp_path, k, n, slots):
    src, dst = tmp_path / "neq.bin", tmp_path / "neq.out"
    src.write_bytes(struct.pack("<I64Q", n, *slots))
    subprocess.run([exe, "neq", str(k), str(src), str(dst)], check=True, timeout=60)
    out = np.fromfile(dst, dtype=np.uint64)
    assert len(out) == 4 * k
    return out.reshape(k, 4)


@pytest.mark.parametrize("k", LISTED_K)
def test_neq_mask_is_its_definition(tool, tmp_path, k):
    """Bit j of the mask of (position i, character c): candidate j's base i differs from c, or j is past
    the n candidates present -- whatever those slots hold.  Position 0 is the k-mer's first base, its
    highest two bits (k = 32 fills the word)."""
    rng = random.Random(k)
    for n in (1, 31, 32, 33, 63, 64):
        slots = [rng.getrandbits(2 * k) for _ in range(64)]
        slots[0] = 0                   # all A
        slots[n - 1] = 4 ** k - 1      # all T, in the last slot present
        got = run_neq(tool, tmp_path, k, n, slots)
        for i in range(k):
            for c in range(4):
                want = 0
                for j in range(64):
                    if j >= n or (slots[j] >> (2 * (k - 1 - i))) & 3 != c:
                        want |= 1 << j
                assert int(got[i, c]) == want, f"k {k} n {n} position {i} character {c}"
        for i in range(k):  # (each present candidate matches exactly one character per position)
            hit = [~int(got[i, c]) & (2 ** 64 - 1) for c in range(4)]
            assert hit[0] | hit[1] | hit[2] | hit[3] == (1 << n) - 1 and sum(bin(h).count("1") for h in hit) == n


def test_neq_mask_of_an_empty_block_and_unlisted_k(tool, tmp_path):
    """No candidate present (a block that LW rounds up to): all ones; k = 17 is not instantiated."""
    got = run_neq(tool, tmp_path, 16, 0, [0] * 64)
    assert (got == np.uint64(2 ** 64 - 1)).all()
    src, dst = tmp_path / "neq.bin", tmp_path / "neq.out"
    src.write_bytes(struct.pack("<I64Q", 1, *([0] * 64)))
    assert subprocess.run([tool, "neq", "17", str(src), str(dst)], timeout=60).returncode == 3
