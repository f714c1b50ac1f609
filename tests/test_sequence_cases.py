"""The mixed-call schedule (tests/sequence_cases.py; DESIGN.md §4e "Call sequences") on the CPU: every property
the GPU walk of tests/test_gpu_call_sequence.py relies on is asserted here from the schedule data, so that
"every transition", "between two group sizes" and "groups rise and fall" are facts about the schedule.

The last tests run a small Python model of the count scratch over the schedule -- two banks of queue counters
with their `dirty` note, and hand-off slots indexed by group x group size -- and one of the context's matrix blocks
(the hit, position, start, flank and edit blocks, carved per job at 256-byte offsets by the samples route and by
the jobs stage) with one defect each, and require that the model then reads a non-zero counter or slot, or words
of a block the call did not write, somewhere in the walk.  That checks the SCHEDULE:
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
               "pos_jobs": GROUPS["hits"], "profiles": GROUPS["hits"]})


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
    n = len(KINDS)
    assert n == 12 and len(pairs) == n * n and len(inside) >= n * (n - 1) == 132 and {(a, b) for a in KINDS for b in KINDS if a != b} <= inside
    print(f"transitions: {n * (n - 1)} ordered pairs of different kinds and {n} self-pairs in {len(WALK)} launches, "
          f"{len(SEGMENTS)} segments")


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
    assert all(len(between) - sum(op[0] == "set_max_errors" for op in between) == sc.PER_GAP for _, between, _ in gaps())
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


def test_dma_route_segments_hold_jobs_calls():
    """The child process of the DMA route runs the first two segments and cuts every other jobs call in two: they
    hold the eight jobs calls it asserts, of every jobs kind."""
    kinds = [v.kind for seg in SEGMENTS[:2] for v in launches(seg) if v.kind in sc.JOBS_KINDS]
    assert len(kinds) >= 8 and set(kinds) == set(sc.JOBS_KINDS), kinds
    print(f"DMA route: {len(kinds)} jobs calls in the first two segments")


def test_profiles_visits_and_side_operations():
    """Every variant of the profiles kind, the flank ones at both depths, the kind at every budget; every other pos
    visit with spans=; the device passes' side operations through all their forms."""
    visits = [v for v in WALK if v.kind == "profiles"]
    args = collections.Counter(sc.profile_args(v) for v in visits)
    assert set(args) == ({(True, 0, False), (False, 0, True)} | {(False, D, e) for D in (8, 32) for e in (False, True)})
    assert [v.nth for v in visits] == list(range(len(visits))) and len(visits) >= 8  # (in turn, two rounds or more)
    assert {v.E for v in visits} == {0, 1, 2, 3}
    by_variant = collections.defaultdict(set)
    for v in visits:
        by_variant[sc.PROFILE_VARIANTS[v.nth % 4]].add(v.E)
    assert all(len(by_variant[name]) >= 2 for name in sc.PROFILE_VARIANTS), by_variant
    assert {v.shape for v in visits} >= set(sc.HIT_SHAPES)
    pos = [v for v in WALK if v.kind == "pos"]
    assert any(sc.pos_spans(v) for v in pos) and not all(sc.pos_spans(v) for v in pos)
    assert {len(v.shape.jobs) for v in pos if sc.pos_spans(v)} >= {1, 2}
    assert any(not sc.live(j) for v in pos if sc.pos_spans(v) for j in v.shape.jobs)  # (a dead segment's buffer)
    uses = collections.Counter(op[1] for seg in SEGMENTS for op in seg if op[0] == "side")
    assert {sc.flanks_side(i) for i in range(uses["flanks_device"])} == \
        {(s, t, D) for s in (False, True) for t in (False, True) for D in (8, 32)}
    assert {sc.edits_side(i) for i in range(uses["edits_device"])} == {False, True}
    assert uses["spans_device"] >= 2 and uses["refuse_profiles"] >= 3  # (each use takes the next of three cases)
    # the matrices the device passes read: three shapes or more, two k, three budgets
    read = set()
    for seg in SEGMENTS:
        done = []
        for op in seg:
            if op[0] == "launch":
                done.append(op[1])
            elif op[0] == "side" and op[1] in ("spans_device", "flanks_device", "edits_device"):
                shape, j, E = sc.matrix_after([v for v in WALK if v.n <= done[-1].n])
                read.add((op[1], shape, E))
    for name in ("spans_device", "flanks_device", "edits_device"):
        shapes = {s for n, s, _ in read if n == name}
        assert len(shapes) >= 3 and len({s.k for s in shapes}) >= 2, (name, shapes)
        assert len({E for n, _, E in read if n == name}) >= 3, name
    print(f"profiles: {len(visits)} visits, variants {dict(args)}; {sum(map(sc.pos_spans, pos))} of {len(pos)} pos "
          f"visits with spans=; device passes {uses['spans_device']} / {uses['flanks_device']} / {uses['edits_device']}, "
          f"{uses['refuse_profiles']} refusals")


def test_matrix_blocks_grow_and_are_reused():
    """Along the walk on one context each of the start, flank and edit blocks is grown by a visit that needs more
    than any before it (after smaller ones used it), reused by a later visit that needs less, and carved for a
    second job at a nonzero offset; and a jobs call lays out d_pos between two profiles visits of different
    position bytes, so that d_start's offsets are not those d_pos had last."""
    blocks = Blocks()
    assert model_walk(None, blocks=blocks) == []
    for name in ("start", "flank", "edit"):
        log = [e for e in blocks.log if e[1] == name]
        grown = [i for i, e in enumerate(log) if 0 < e[3] < e[2]]
        assert grown, name
        reuse = [e for e in log[grown[0] + 1:] if 0 < e[2] < e[3]]
        assert reuse, name
        second = [e for e in log if any(o and u for o, u in zip(e[4][1:], e[5][1:]))]
        assert second and any(e[2] < e[3] for e in second), name  # (... also inside a larger block)
        print(f"{name} block: {len(log)} carves; grown at launch {log[grown[0]][0]} ({log[grown[0]][3] * 256} -> "
              f"{log[grown[0]][2] * 256} bytes), reused smaller at launch {reuse[0][0]} ({reuse[0][2] * 256} of "
              f"{reuse[0][3] * 256}); a second job at a nonzero offset in {len(second)} carves")
    # the start block's growth is the one visit chosen for it, after the jobs call that grew d_pos to that size
    grow_pos, grow_start = (next(v for v in WALK if v.kind == kind and v.nth == sc.START_GROW_AT[kind])
                            for kind in ("pos_jobs", "profiles"))
    assert grow_pos.shape == grow_start.shape == sc.START_GROW and grow_pos.n < grow_start.n
    assert sc.profile_args(grow_start)[2] and grow_start.E >= 1  # (its inserted N shows in an edit profile)
    start = {e[0]: e for e in blocks.log if e[1] == "start"}
    pos = {e[0]: e for e in blocks.log if e[1] == "pos"}
    assert start[grow_start.n][2] > start[grow_start.n][3] > 0 and pos[grow_start.n][2] == pos[grow_start.n][3]
    assert pos[grow_pos.n][2] > pos[grow_pos.n][3] > 0
    assert [n for n, e in start.items() if 0 < e[3] < e[2]] == [grow_start.n]
    # a hits_jobs or pos_jobs launch between two profiles visits of different position bytes
    between = []
    visits = [v for v in WALK if v.kind == "profiles"]
    for a, b in zip(visits, visits[1:]):
        jobs = [v for v in WALK[a.n + 1:b.n] if v.kind in ("hits_jobs", "pos_jobs")]
        if jobs and start[a.n][2] != start[b.n][2]:
            between.append((a.n, [v.n for v in jobs], b.n))
    assert between and any(any(WALK[n].kind == "pos_jobs" for n in mid) for _, mid, _ in between)
    # ... and a profiles visit of several jobs for which the last layout of d_pos was a pos_jobs launch's that gave
    # a later live job another offset, or had no such job (where the model's start_prev_offsets defect shows)
    differ = []
    for b in visits:
        last = max((n for n in pos if n < b.n), default=None)
        if last is not None and WALK[last].kind == "pos_jobs":
            prev, (off, units) = pos[last][4], start[b.n][4:6]
            if any(u and o != (prev[j] if j < len(prev) else 0) for j, (o, u) in enumerate(zip(off, units)) if j):
                differ.append((last, b.n))
    assert differ
    print(f"pos_jobs layouts of d_pos with other offsets than the next profiles visit's: {differ}")
    print(f"jobs launches between two profiles visits of different position bytes: {between}")


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
    # the profiles visits: every edit operation occurs, and on both flank sides pairs are cut by the window's edge
    ops, cut, columns = np.zeros(12, np.uint64), collections.Counter(), {}
    for v in WALK:
        if v.kind != "profiles":
            continue
        _, D, edits = sc.profile_args(v)
        for j, job in enumerate(v.shape.jobs):
            if not sc.live(job):
                continue
            hit, pos, _ = sc.expected_matrices(v.shape, j, v.E)
            start, top, L = sc.expected_starts(v.shape, j, v.E), hit[v.E], job[2]
            assert ((start >= 0) == top).all() and (start[top] < pos[top]).all() and top.any()
            if edits:
                prof = sc.expected_edits(v.shape, j, v.E)
                assert prof.shape == (job[0], v.shape.k, 12) and prof.any()
                ops += prof.sum(axis=(0, 1), dtype=np.uint64)
            if D:
                prof = sc.expected_flanks(v.shape, j, v.E, D)
                assert prof.shape == (2, job[0], D, 5) and prof.any()
                cut["right", D] += int((pos[top].astype(int) + D > L).sum())
                cut["left", D] += int((start[top] < D).sum())
                columns[D] = columns.get(D, 0) + prof.sum(axis=(1, 3), dtype=np.uint64)
    assert (ops > 0).all(), ops
    assert all(cut[side, D] > 0 for side in ("right", "left") for D in (8, 32)), cut
    # (a cut pair is counted in fewer columns: on both sides the columns' totals fall with the distance, and none is 0)
    assert all((columns[D][:, 0] > columns[D][:, -1]).all() and columns[D].all() for D in (8, 32)), columns
    print(f"profiles visits: edit operations {ops.tolist()}; pairs cut by the window's edge {dict(cut)}")


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


class Blocks:
    """The context's grow-only matrix blocks (ctx.h d_hits, d_pos, d_start, d_flank, d_edit) in units of 256 bytes,
    as capi.cpp count_samples and jobs_stage.cpp count_jobs carve them per job (sc.block_needs): a unit holds the
    (launch, job) tag of what wrote it last, 0 when fresh or zeroed.  The span pass writes a job's start matrix, and
    the copy to the host and the flank and edit passes read it; the flank and the edit pass zero their profile
    on the stream and then add into it, so they must find zeros.  `log` keeps (launch, block, units needed, capacity
    before, job offsets, job units) of every carve."""

    NAMES = ("hits", "pos", "start", "flank", "edit")

    def __init__(self, defect=None):
        self.defect = defect
        self.mem = {name: np.zeros(0, np.int64) for name in self.NAMES}
        self.pos_offsets = None  # of the last call that laid out d_pos, whichever stage it was
        self.log = []

    def carve(self, n, need):
        """Launch n; returns the block in which it read what it had not written (or stored outside), or None."""
        bad, pos_grew, layout = None, False, {}
        for name in self.NAMES:
            if name not in need:
                continue
            units = [-(-b // 256) for b in need[name]]
            off = [sum(units[:j]) for j in range(len(units))]
            self.log.append((n, name, sum(units), len(self.mem[name]), off, units))
            grow = sum(units) > len(self.mem[name])
            if name == "start" and self.defect == "start_grown_with_pos":
                grow = pos_grew
            if name == "pos":
                pos_grew = grow
            if grow:
                self.mem[name] = np.zeros(sum(units), np.int64)
            layout[name] = (off, units)
        for name, (off, units) in layout.items():
            mem = self.mem[name]
            for j, (o, u) in enumerate(zip(off, units)):
                if not u:
                    continue
                tag = 8 * n + j + 1
                if name in ("flank", "edit"):
                    if self.defect != name + "_not_zeroed":
                        mem[o:o + u] = 0
                    bad = bad or (name if mem[o:o + u].any() else None)
                    mem[o:o + u] = tag
                    continue
                at = o
                if name == "start" and self.defect == "start_prev_offsets" and self.pos_offsets is not None:
                    at = self.pos_offsets[j] if j < len(self.pos_offsets) else 0
                if at + u > len(mem):
                    bad = bad or name  # a store outside the block
                mem[at:at + u] = tag
                if not (len(mem) >= o + u and (mem[o:o + u] == tag).all()):
                    bad = bad or name
        if "pos" in layout:
            self.pos_offsets = layout["pos"][0]
        return bad


def model_walk(defect, segments=SEGMENTS, blocks=None):
    """The operations that read a non-zero counter or slot, or a matrix block's words that the call did not write,
    when the walk runs on one context with `defect`."""
    sets = {False: Scratch(defect), True: Scratch(defect)}  # (a submit counts on a scratch set of its own)
    blocks = blocks or Blocks(defect)
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
                need = sc.block_needs(v)
                bad = blocks.carve(v.n, need) if need else None
                if bad:
                    found.append((v.n, v.kind, bad))
            elif op[:2] == ("side", "empty"):
                sets[False].launch(256, [0], False)
    return found


def test_the_model_without_a_defect_reads_zeros():
    assert model_walk(None) == []


@pytest.mark.parametrize("defect,reads", [
    ("zero_by_this_launch", "counter"), ("flip_on_empty", "counter"), ("slots_left", "slot"),
    ("start_prev_offsets", "start"), ("start_grown_with_pos", "start"), ("flank_not_zeroed", "flank"),
    ("edit_not_zeroed", "edit")])
def test_the_walk_shows_a_defect_in_the_scratch(defect, reads):
    """zero_by_this_launch: the other bank is zeroed by this launch's counter count instead of the previous one's.
    flip_on_empty: the bank flips on a call that launched nothing.  slots_left: hand-off slots beyond a layout of
    64-candidate groups are left non-zero.  start_prev_offsets: the span pass writes a job's start matrix at the
    offset the previous call that laid out d_pos gave that job (a jobs call's, too).  start_grown_with_pos: d_start
    is grown only when d_pos had to grow in the same call.  flank_not_zeroed, edit_not_zeroed: the pass adds into
    what an earlier call left in its block.  This checks the schedule, not the kernels."""
    history = reads in Blocks.NAMES  # (a defect of the matrix blocks, not of the count scratch)
    found = model_walk(defect)
    assert found and all(f[2] == reads for f in found[:1]), found[:3]
    alone = sum(bool(model_walk(defect, [seg])) for seg in SEGMENTS)
    if history:
        # a defect of the matrix blocks needs a history: the walk on one context is what shows it
        assert all(f[1:] == ("profiles", reads) for f in found), found
    else:
        # ... and most single segments on a fresh context show it too (the per-segment GPU test)
        assert alone >= len(SEGMENTS) // 2, alone
    what = f"words it did not write in the {reads} block" if history else f"a non-zero {reads}"
    print(f"{defect}: first read of {what} at launch {found[0][0]} ({found[0][1]}); "
          f"{len(found)} launches in the walk, {alone} of {len(SEGMENTS)} segments alone")
