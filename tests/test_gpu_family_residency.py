"""A bit-sliced launch's waves do not depend on what the context launched before.

launch() sizes a launch as one round of its kernel's resident waves and keeps that number, once queried, in a
cache with one slot per kernel family (counting, hits, hits and positions; plain and staged; three NFA rows
and four) and k.  A launch that read another family's slot would be sized by another kernel's residency -- for
a staged launch, whose copier workgroups must all be resident, a hang rather than a wrong count.

24 cases: K in (16, 32) -- at 32 the families' declared residencies differ most -- x edit budget E in (2, 3) x
six kinds, three on resident images (the plain kernels) and three through the jobs stage (the staged ones).
Each runs 3 candidates over 64 windows of K + 4 bases without N: two row items, well under one round, so
ac_last_launch's waves is exactly the family's cached resident-wave count.  Each case's waves on a fresh
context is the reference; one context then runs all 24 in that order and another in reverse order, and every
launch must count what the oracle counts, on the bit-sliced kernel, with the waves of its fresh context."""
import functools
import os

import numpy as np
import pytest

import approx_counter_amd as ac
from tests.hits_cases import equal_case
from tests.test_budget_cpu import count_e
from tests.test_gpu_bitslice import BITSLICE, kernel_of
from tests.test_gpu_jobs_hits import EARLY, sample_of

pytestmark = pytest.mark.gpu
# (AC_BITSLICE=0 refuses the hits calls and every budget but 2; AC_BS_WAVES_PCT rescales every launch)
GEOMETRY = bool(BITSLICE) and "AC_BS_WAVES_PCT" not in os.environ
KINDS = ("device", "device_hits", "device_positions", "jobs", "jobs_hits", "jobs_positions")
CASES = [(K, E, kind) for K in (16, 32) for E in (2, 3) for kind in KINDS
         if BITSLICE or (E == 2 and kind in ("device", "jobs"))]


@functools.lru_cache(maxsize=None)
def inputs(K, E):
    """(kmers, windows, the oracle's counts at budget E), built once per (K, E)."""
    km, w = equal_case(7300 + K, 3, 64, K + 4, p_n=0.0, k=K)
    assert not any("N" in x for x in w)
    return np.asarray(km, np.uint64), w, count_e(E, K, km, w)


def launch(c, case):
    """One launch of the case on context c, its counts compared with the oracle's; returns its waves."""
    import torch

    K, E, kind = case
    km, w, want = inputs(K, E)
    c.set_max_errors(E)
    if kind.startswith("device"):
        seg = ac.DeviceSegment.upload(km, ac.pack_windows(w))
        mk = lambda n: torch.full((n,), -1, dtype=torch.int32, device="cuda")  # noqa: E731
        hits = [mk(ac.hits_words(len(km), len(w), E))] if kind != "device" else None
        pos = [mk(ac.positions_words(len(km), len(w)))] if kind == "device_positions" else None
        c.count_device(K, [seg], window_len=[K + 4], hits=hits, positions=pos)
        torch.cuda.synchronize()
        c.check()
        got = seg.counts_numpy()
    else:
        jobs = ac.Jobs([(km, sample_of(w))])
        if kind == "jobs":
            got = c.count_jobs(K, jobs)[0]
        else:
            got = c.window_hits_jobs(K, jobs, positions=kind == "jobs_positions")[0].counts
        if EARLY:
            assert c.stage_mode() == 2, case
    np.testing.assert_array_equal(got, want, err_msg=str(case))
    assert kernel_of(c) == BITSLICE, case
    return int(c.last_launch()["waves"])


def test_waves_do_not_depend_on_the_launches_before():
    fresh = {}
    for case in CASES:
        with ac.ApproxCounter(0) as c:
            fresh[case] = launch(c, case)
        print(f"K {case[0]} E {case[1]} {case[2]}: {fresh[case]} waves on a fresh context", flush=True)
        assert fresh[case] > 0
    for order in (CASES, CASES[::-1]):
        with ac.ApproxCounter(0) as c:
            for case in order:
                waves = launch(c, case)
                if GEOMETRY:
                    assert waves == fresh[case], (case, waves, fresh[case])
