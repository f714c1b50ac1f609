"""The mixed-call schedule (tests/sequence_cases.py; DESIGN.md §4e "Call sequences") on the CPU: every property
the GPU walk of tests/test_gpu_call_sequence.py relies on is asserted here from the schedule data, so that
"every transition", "between two group sizes" and "groups rise and fall" are facts about the schedule.

The last three tests run a small Python model of the count scratch over the schedule -- two banks of queue
counters with their `dirty` note, and hand-off slots indexed by group x group size -- with one defect each, and
require that the model then reads a non-zero counter or slot somewhere in the walk.  That checks the SCHEDULE:
a launch frame with such a defect could not pass the walk unnoticed.  It says nothing about the kernels, which only
the GPU tests run."""
import collections

import numpy as np
import pytest

from tests import sequence_cases as sc
from tests.sequence_cases import KINDS, SEGMENTS, SIDES, WALK

# (group size, groups) of every table's shapes, written out: the arithmetic of launch_groups() is pinned to them
GROUPS = {
    "wm": [(192, 1), (64, 3), (256, 6)],
    "wm_jobs": [(256, 1), (128, 3), (192, 6)],
    "bs": [(256, 1), (256, 3), (256, 5), (256, 4), (256, 2)],
    "hits": [(256, 1), (256, 3), (256, 5), (256, 2), (256, 2)],
    "samples": [(256, 2), (256, 2), (256, 2), (256, 1), (256, 6), (256, 2)],
}
GROUPS.update({"bs_jobs": GROUPS["bs"], "dp_jobs": GROUPS["bs"], "pos": GROUPS["hits"], "hits_jobs": GROUPS["hits"],
               "pos_jobs": GROUPS["hits"]})


def launches(seg):
    return [op[1] for op in seg if op[0] == "launch"]


def gaps():
    """(previous launch, the operations between, launch) of every gap inside a segment."""
    out = []
    for seg in SEGMENTS:
        prev, between = None, []
        for op in seg:
            if op[0] != "launch":
                between.append(op)
                continue
            if prev is not None:
                out.append((prev, between, op[1]))
            prev, between = op[1], []
    return out


def test_segments_are_the_walk():
    assert [v for seg in SEGMENTS for v in launches(seg)] == list(WALK)
    assert [v.n for v in WALK] == list(range(len(WALK)))
    for i, seg in enumerate(SEGMENTS):
        ls = launches(seg)
        assert 10 <= len(ls) <= 15, (i, len(ls))
        assert all(v.segment == i for v in ls)
        assert seg[0] == ("set_max_errors", ls[0].E) and seg[1][0] == "launch"
        if i:
            assert ls[0].kind == launches(SEGMENTS[i - 1])[-1].kind
    # the budget every launch runs at is the one the operations before it set, on one context and on a fresh one
    for fresh in (False, True):
        cur = 2
        for seg in SEGMENTS:
            cur = 2 if fresh else cur
            for op in seg:
                if op[0] == "set_max_errors":
                    cur = op[1]
                elif op[0] == "launch":
                    assert op[1].E == cur
                    assert op[1].E == 2 or sc.is_bs(op[1].kind, op[1].shape)


def test_every_transition():
    pairs = collections.Counter((a.kind, b.kind) for a, b in zip(WALK, WALK[1:]))
    assert set(pairs) == {(a, b) for a in KINDS for b in KINDS}
    inside = {(a.kind, b.kind) for a, _, b in gaps()}
    assert len(inside) >= 110 and {(a, b) for a in KINDS for b in KINDS if a != b} <= inside
    print(f"transitions: {len(pairs)} ordered pairs in {len(WALK)} launches, {len(SEGMENTS)} segments")


def test_side_operations_before_every_kind():
    had = collections.defaultdict(set)
    for _, between, v in gaps():
        had[v.kind] |= {op[1] if op[0] == "side" else op[0] for op in between}
    for kind in KINDS:
        assert had[kind] >= set(SIDES) | {"set_max_errors"}, (kind, set(SIDES) - had[kind])
    between_sizes = set()
    for a, between, b in gaps():
        if sc.launch_groups(a.kind, a.shape)[0] != sc.launch_groups(b.kind, b.shape)[0]:
            between_sizes |= {op[1] for op in between if op[0] == "side"}
    assert between_sizes >= set(sc.BETWEEN_GROUP_SIZES)
    # a budget refusal needs a context whose budget is not 2
    for a, between, _ in gaps():
        assert a.E != 2 or all(op[:2] != ("side", "refuse_budget_k") for op in between)
    print(f"side operations: {sum(len(b) for _, b, _ in gaps())} in {len(gaps())} gaps")


def test_edit_budgets():
    at = collections.defaultdict(set)
    for v in WALK:
        at[v.kind].add(v.E)
    for kind in KINDS:
        assert at[kind] == ({2} if kind in ("wm", "wm_jobs") else {0, 1, 2, 3}), kind
    changes = collections.Counter((a.E, b.E) for a, _, b in gaps() if a.E != b.E)
    assert set(changes) == {(a, b) for a in range(4) for b in range(4) if a != b}
    same = [(a, b) for a, _, b in gaps() if a.kind == b.kind and a.shape == b.shape and a.E != b.E]
    assert same and any(3 in (a.E, b.E) for a, b in same)  # (the [E == 3][k] occupancy caches)
    print(f"budget changes: {sum(changes.values())} between launches, all 12 ordered ones; "
          f"{len(same)} between two launches of one kind and k")


def test_slot_reuploads():
    import approx_counter_amd as ac

    visits = [v for v in WALK if v.kind == "samples"]
    n = len(sc.SAMPLE_STATES)
    assert len(visits) >= n and [v.shape for v in visits] == [sc.SAMPLE_STATES[i % n] for i in range(len(visits))]
    img = [[ac.pack_windows(sc.case(s, j)[1]) for j in range(2)] for s in sc.SAMPLE_STATES]
    has_n = lambda s: any("N" in w for j in range(2) for w in sc.case(s, j)[1])  # noqa: E731
    st = sc.SAMPLE_STATES
    assert [img[0][j].equal_window_len() for j in range(2)] == [100, 101] and not has_n(st[0])
    assert [img[1][j].equal_window_len() for j in range(2)] == [100, 101] and has_n(st[1])
    for j in range(2):
        assert img[1][j].n_bases == img[0][j].n_bases == img[2][j].n_bases
        assert img[2][j].equal_window_len() is None and img[2][j].n_windows == img[0][j].n_windows
        assert img[3][j].n_bases < img[0][j].n_bases < img[4][j].n_bases
        assert max(x[j].n_bases for x in img) == img[4][j].n_bases
    assert st[5] == st[0]
    for i in (0, 1, 3, 4, 5):  # window_hits where it is legal, at every such state
        assert any(v.wh for v in visits if v.nth % n == i), i
    assert not any(v.wh for v in visits if v.nth % n == 2)
    print(f"re-uploads: {len(visits)} visits of both slots, {len(visits) // n} whole cycles of {n} states; "
          f"{sum(op[:2] == ('side', 'reupload') for seg in SEGMENTS for op in seg)} re-uploads of a slot in use")


def t_size(levels, rows, n_windows):
    """Words of the transposed planes (hit_cooc.h co_t_rows x co_t_words): what the shared scratch block holds."""
    return levels * sum(-(-r // 32) * 32 for r in rows) * -(-n_windows // 1024) * 32


def test_cooccurrence_and_cross_alternate_in_size():
    """Each of the two families reads the shared transposition scratch after the other filled it at a larger and
    at a smaller size."""
    seq = []
    for seg in SEGMENTS:
        done = []
        for op in seg:
            if op[0] == "launch":
                done.append(op[1])
            elif op[0] == "side" and op[1] in ("cooc", "cross", "cooc_host", "cross_host"):
                before = [v for v in WALK if v.n <= done[-1].n]
                shape, j, E = sc.matrix_after(before)
                nk, nw = shape.jobs[j][:2]
                size = {"cooc": lambda: t_size(E + 1, [nk], nw), "cross": lambda: t_size(1, [nk, nk], nw),
                        "cooc_host": lambda: t_size(3, sc.COOC_HOST[op[2] % 3][:1], sc.COOC_HOST[op[2] % 3][1]),
                        "cross_host": lambda: t_size(3, sc.CROSS_HOST[op[2] % 3][:2], sc.CROSS_HOST[op[2] % 3][2])}[op[1]]()
                seq.append((op[1].split("_")[0], size))
    seen = set()
    for (fa, sa), (fb, sb) in zip(seq, seq[1:]):
        if fa != fb and sa != sb:
            seen.add((fb, "after larger" if sa > sb else "after smaller"))
    assert seen == {(f, w) for f in ("cooc", "cross") for w in ("after larger", "after smaller")}, seen


def test_groups_of_every_shape():
    for kind, want in GROUPS.items():
        table = sc.TABLES[kind]
        assert [sc.launch_groups(kind, s) for s in table] == want, kind
        counts = [g for _, g in want]
        assert 1 in counts and ({2, 3} & set(counts)) and max(counts) >= 5, kind
    assert sc.launch_groups("wm", sc.ACC_GROW) == (64, 32) and sc.launch_groups("wm", sc.QUEUE_GROW) == (64, 260)
    assert sc.launch_groups("wm_jobs", sc.WM_JOBS_SHAPES[1], early=False) == (64, 5)   # (the DMA route is not staged)
    assert sc.launch_groups("bs_jobs", sc.BS_SHAPES[1], bs_on=False) == (128, 4)       # (AC_BITSLICE=0: k = 22, P = 1)
    for kind in KINDS:  # every kind's visits rotate through its whole table, so its groups rise and fall
        g = [sc.launch_groups(v.kind, v.shape)[1] for v in WALK if v.kind == kind]
        assert any(a < b for a, b in zip(g, g[1:])) and any(a > b for a, b in zip(g, g[1:])), kind
        if kind != "submit":
            assert {v.shape for v in WALK if v.kind == kind} >= set(sc.TABLES[kind]), kind
        jobs = {len(v.shape.jobs) for v in WALK if v.kind == kind}
        dead = any(not sc.live(j) for v in WALK if v.kind == kind for j in v.shape.jobs)
        assert dead and (len(jobs) >= 2 or kind == "samples"), kind  # (samples: always both upload slots)
    sizes = {sc.launch_groups(v.kind, v.shape)[0] for v in WALK}
    assert sizes == {64, 128, 192, 256}
    assert {len(v.shape.jobs) for v in WALK} == {1, 2, 3, 4}


def test_the_two_growth_visits():
    """The hand-off slots grow after smaller launches used them, and the queue block grows past its first 1,024
    counters, each on one context and on a segment's fresh one."""
    acc = next(v for v in WALK if v.shape == sc.ACC_GROW)
    queue = next(v for v in WALK if v.shape == sc.QUEUE_GROW)
    assert acc.kind == queue.kind == "wm" and acc.n < queue.n
    for v in (acc, queue):
        assert any(u.segment == v.segment and u.kind != "submit" for u in WALK[:v.n]), "the segment's first launch"
    before = [sc.acc_slots(u.kind, u.shape) for u in WALK[:acc.n] if u.kind != "submit"]
    assert before and max(before) < sc.acc_slots("wm", sc.ACC_GROW) == 2048
    assert sc.min_counters("wm", sc.QUEUE_GROW) == 1040 > 1024
    # no other launch can pass 1,024 counters: at most 32 sub-queues per group and resident / 64 + 4 per job in all
    for v in WALK:
        if v.shape != sc.QUEUE_GROW:
            assert sc.launch_groups(v.kind, v.shape)[1] <= 32


def test_expected_values_are_not_trivial():
    """Every launch visit counts something, and every hits visit holds pairs at each distance 0..E."""
    for v in WALK:
        counts = [sc.expected_counts(v.shape, j, v.E) for j in range(len(v.shape.jobs))]
        assert any(c.any() for c in counts), v
        for j, job in enumerate(v.shape.jobs):
            assert len(counts[j]) == job[0]
        if v.kind in sc.HIT_KINDS or v.with_hits or v.wh:
            at = set()
            for j, job in enumerate(v.shape.jobs):
                if sc.live(job):
                    hit, pos, c = sc.expected_matrices(v.shape, j, v.E)
                    np.testing.assert_array_equal(c, counts[j])
                    at |= {d for d in range(v.E + 1) if (hit[d] & ~(hit[d - 1] if d else False)).any()}
            assert at == set(range(v.E + 1)), (v, at)


# ---- the schedule can show carry-over: a model of the scratch with one defect ------------------------------------

RESIDENT = 8192  # a nominal resident wave count for the sub-queue rule; the model needs the rule's shape only


class Scratch:
    """count_launch.cpp's bookkeeping of one scratch set, with the kernel's part reduced to: the launch reads its
    bank's first `used` counters and its hand-off slots (they must be zero), leaves the counters non-zero, zeroes
    the other bank's first dirty counters, and leaves its slots zero again."""

    def __init__(self, defect):
        self.defect = defect
        self.qcap, self.bank, self.dirty = 1024, 0, [0, 0]
        self.queue = np.zeros((2, 1024), np.uint8)
        self.acc = np.zeros(0, np.uint8)

    def launch(self, group_size, groups_per_job, staged):
        """One launch; returns what it read that was not zero, or None."""
        live = [g for g in groups_per_job if g]
        if not live:  # an empty call: nothing runs
            if self.defect == "flip_on_empty":
                self.dirty[self.bank], self.dirty[self.bank ^ 1] = 0, 0
                self.bank ^= 1
            return None
        s_base = max(1, min(32, RESIDENT // (64 * sum(live))))
        used = sum(g * (-(-s_base // 4) * 4) for g in live) + (9 if staged else 0)
        slots = group_size * sum(live)
        if slots > len(self.acc):
            self.acc = np.zeros(slots, np.uint8)
        if used > self.qcap:
            self.qcap, self.bank, self.dirty = used, 0, [0, 0]
            self.queue = np.zeros((2, used), np.uint8)
        bad = "counter" if self.queue[self.bank, :used].any() else "slot" if self.acc[:slots].any() else None
        self.queue[self.bank, :used] = 1
        other = self.bank ^ 1
        self.queue[other, :(used if self.defect == "zero_by_this_launch" else self.dirty[other])] = 0
        if self.defect == "slots_left":  # the slots are reset as if every group held 64 candidates
            self.acc[:slots] = 1
            self.acc[:64 * sum(live)] = 0
        self.dirty[self.bank], self.dirty[other] = used, 0
        self.bank = other
        return bad


def model_walk(defect, segments=SEGMENTS):
    """The operations that read a non-zero counter or slot when the walk runs on one context with `defect`."""
    sets = {False: Scratch(defect), True: Scratch(defect)}  # (a submit counts on a scratch set of its own)
    found = []
    for seg in segments:
        for op in seg:
            if op[0] == "launch":
                v = op[1]
                gs = sc.launch_groups(v.kind, v.shape)[0]
                per_job = [-(-j[0] // gs) if sc.live(j) else 0 for j in v.shape.jobs]
                bad = sets[v.kind == "submit"].launch(gs, per_job, v.kind in sc.JOBS_KINDS)
                if bad:
                    found.append((v.n, v.kind, bad))
            elif op[:2] == ("side", "empty"):
                sets[False].launch(256, [0], False)
    return found


def test_the_model_without_a_defect_reads_zeros():
    assert model_walk(None) == []


@pytest.mark.parametrize("defect,reads", [("zero_by_this_launch", "counter"), ("flip_on_empty", "counter"),
                                          ("slots_left", "slot")])
def test_the_walk_shows_a_defect_in_the_scratch(defect, reads):
    """zero_by_this_launch: the other bank is zeroed by this launch's counter count instead of the previous one's.
    flip_on_empty: the bank flips on a call that launched nothing.  slots_left: hand-off slots beyond a layout of
    64-candidate groups are left non-zero.  This checks the schedule, not the kernels."""
    found = model_walk(defect)
    assert found and all(f[2] == reads for f in found[:1]), found[:3]
    # ... and most single segments on a fresh context show it too (the per-segment GPU test)
    alone = sum(bool(model_walk(defect, [seg])) for seg in SEGMENTS)
    assert alone >= len(SEGMENTS) // 2, alone
    print(f"{defect}: first read of a non-zero {reads} at launch {found[0][0]} ({found[0][1]}); "
          f"{len(found)} launches in the walk, {alone} of {len(SEGMENTS)} segments alone")
