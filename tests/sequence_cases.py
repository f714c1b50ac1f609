"""The mixed-call schedule of tests/test_gpu_call_sequence.py and its expected values (DESIGN.md §4e "Call
sequences"); tests/test_sequence_cases.py asserts the schedule's properties on the CPU.  Nothing here needs a GPU.

One context carries state from call to call (ctx.h): two banks of queue counters and the `dirty` note, the count
hand-off slots, a staged launch's device lines, generation flags, three sets of staging slots, grow-only blocks,
notes about uploaded samples, the sticky edit budget, occupancy caches.  The WALK below is one deterministic
sequence of calls that puts every launch kind directly after every launch kind (itself included) on one context,
with the side operations, refusals, empty calls, budget changes and slot re-uploads in the gaps between them.

Launch kinds (each one call that reaches count_launch.cpp launch()):
  wm         count() / count_device() without window_len: ragged windows, or k = 10 / 17   word-parallel
  bs         count_device(window_len=...), k in 16, 22, 32                                  bit-sliced
  hits       count_device(..., hits=)                                                       bsh
  pos        count_device(..., hits=, positions=)                                           bsp
  samples    upload_sample(slot) + count_samples, and window_hits over uploads              the CLI's route
  wm_jobs    count_jobs over ragged Dna5 windows                                            staged word-parallel
  bs_jobs    count_jobs over equal windows in ordinary memory                               staged bit-sliced
  dp_jobs    count_jobs over .pinned() samples under AC_TESTING_DEVICE_PACK                 device packing
  hits_jobs  window_hits_jobs                                                               bshs
  pos_jobs   window_hits_jobs(positions=True)                                               bsps
  submit     submit_jobs into a device tensor, alternately with and without hits=           submit scratch, slot sets
  profiles   window_hits(spans= / flanks= / edits=) over uploads: the count launch, then     bsp, then hit_span,
             the span, flank and edit passes per job on the context's stream                hit_flank, hit_edit

The walk: an Eulerian circuit of the complete digraph on the 12 kinds (132 transitions, a fixed seed orders the
edges), cut into segments of 12 transitions.  A segment begins with a launch of the kind the previous one ended
with, so the cut itself is a self-pair; kinds that got no self-pair that way get one inside a segment.  A segment
run alone on a fresh context is a valid sequence: it starts by setting the budget of its first launch, and the
reductions before its first hits launch read matrices uploaded from the host.

"Directly before a launch" means: in the gap between the previous launch and this one, no launch between them.

Expected values are the existing ones, cached per shape: oracle.count_myers (E = 2), tests.test_budget_cpu.count_e
(other budgets), tests.hits_cases.expected_hits, tests.positions_cases.expected_positions / profile_of, numpy's
H^T H, oracle.host_ref for the exact count, tests.span_cases.starts_of, tests.flank_cases.flank_profile_of and
tests.edit_cases.edit_profile_of.

The span, flank and edit passes added three grow-only blocks to the context (d_start, d_flank, d_edit), carved
per job at 256-byte offsets like the hit and position blocks, which the jobs stage carves too.  block_needs()
below says what each launch takes of them; tests/test_sequence_cases.py runs a model of the blocks over the walk."""
import collections
import functools
import random

import numpy as np

KINDS = ("wm", "bs", "hits", "pos", "samples", "wm_jobs", "bs_jobs", "dp_jobs", "hits_jobs", "pos_jobs", "submit",
         "profiles")
HIT_KINDS = ("hits", "pos", "hits_jobs", "pos_jobs", "profiles")
JOBS_KINDS = ("wm_jobs", "bs_jobs", "dp_jobs", "hits_jobs", "pos_jobs", "submit")  # the jobs stage: staged when early
BS_K = (16,) + tuple(range(18, 33))  # the bit-sliced kernel's pattern lengths
SEED = 20240611

# Side operations: no count kernel, but they use or change context state.  set_max_errors is placed by the
# budget plan, the others by place_sides().
REFUSALS = ("refuse_ragged_hits", "refuse_pos_without_hits", "refuse_budget_k", "refuse_levels5", "refuse_profiles")
SIDES = ("exact_packed", "exact_uploaded", "level_counts", "position_profile", "window_counts", "cooc", "cross",
         "cooc_host", "cross_host", "reupload", "empty", "spans_device", "flanks_device", "edits_device") + REFUSALS
BETWEEN_GROUP_SIZES = REFUSALS + ("empty",)  # each at least once between two launches of different group size
PER_GAP = 2  # side operations per gap: enough to put all 19 before every one of the 12 kinds (asserted on the CPU)
# The profiles kind's variants, in turn: window_hits(spans=True), (flanks=D), (edits=True), (flanks=D, edits=True);
# D is 8 and, at every other round of the four, 32: the depth at which hit_flank.h fl_run takes three code words.
PROFILE_VARIANTS = ("spans", "flanks", "edits", "flanks_edits")
DEPTHS = (8, 32)

Shape = collections.namedtuple("Shape", "k jobs")
# a job: (n_kmers, n_windows, L, n) -- L an int (equal windows) or (lo, hi) (ragged ones); n the share of N
# bases, or "records": tests.test_gpu_bitslice.n_windows_case with 0..7 N per window, so that inline N records
# (nrec.h: up to 4 positions) are empty, full and overflowed; or "planted_n" (START_GROW below).  A job without
# k-mers or without windows is dead.

# word-parallel, resident: group sizes 192 (k = 10), 64 (k = 17), 256 (k = 16); 1, 3 and 6 groups; windows on
# both sides of 32 and 128 bases
WM_SHAPES = (
    Shape(10, ((100, 40, (20, 60), 0.01),)),
    Shape(17, ((130, 30, (90, 140), 0.02),)),
    Shape(16, ((1100, 9, (100, 130), 0.0), (5, 0, (100, 130), 0.0), (40, 33, (28, 36), 0.05))),
)
# The two plain-count visits that make the count scratch grow (count_launch.cpp).  k = 17 has groups of 64.
# ACC_GROW: acc_slots = groups x group size = 32 x 64 = 2048 slots, more than any launch before it (the largest
# other shape, 1100 + 33 candidates in groups of 256, takes 6 x 256 = 1536).  QUEUE_GROW: the sub-queue rule gives a
# segment s_base = min(32, resident / (64 x groups)) >= 1 sub-queues per group, rounded up to a multiple of 4
# (AC_WAVES_PER_BLOCK), so 260 groups take at least 260 x 4 = 1040 counters > qcap's first 1024 -- whatever the
# resident wave count is -- while every other shape stays below it (at most 6 groups x 32 sub-queues, or 32 x 8).
ACC_GROW = Shape(17, ((2000, 3, (60, 90), 0.01),))
QUEUE_GROW = Shape(17, ((16640, 3, (60, 90), 0.01),))
# The start block's growth (capi.cpp count_samples grows d_start by the position matrices' bytes, apart from d_pos).
# By rotation the first profiles visit is the largest (HIT_SHAPES[1]: 13,120 + 576 bytes of positions in two jobs,
# 14,080 at 256-byte offsets), so no later one would grow the block.  START_GROW takes 16,000 + 1,280 bytes (17,408):
# the pos_jobs visit START_GROW_AT["pos_jobs"] grows d_pos with it, and the next profiles visit,
# START_GROW_AT["profiles"] (an edits variant), then needs a start block larger than any before while d_pos is large
# enough already.  Its first job's last 8 windows are tests.edit_cases.planted_windows -- a k-mer with an N in place
# of, or inserted before, its middle base -- since no other shape of the walk holds an inserted N.
START_GROW = Shape(16, ((300, 50, 100, "planted_n"), (40, 20, 100, 0.0)))
START_GROW_AT = {"pos_jobs": 9, "profiles": 10}  # the kind's nth visit
WM_JOBS_SHAPES = (  # staged group sizes 256 (k = 16), 128 (k = 17), 192 (k = 10); job regions below and above
    Shape(16, ((120, 60, (90, 110), 0.01),)),                                              # a 4096-byte chunk
    Shape(17, ((200, 30, (20, 40), 0.02), (40, 0, (20, 40), 0.0), (10, 5, (130, 200), 0.0))),
    Shape(10, ((1000, 9, (100, 140), 0.01),)),
)
BS_SHAPES = (  # groups of 256: 1, 2 + 1, 5, and 2 + 1 + 1 in four jobs; L = 31 | 33, 127 | 128 | 129, 256
    Shape(16, ((40, 37, 100, 0.01),)),
    Shape(22, ((300, 70, 31, 0.02), (0, 20, 31, 0.0), (33, 9, 129, 0.0))),
    Shape(32, ((1100, 9, 256, 0.01),)),
    Shape(16, ((257, 65, 33, 0.01), (1, 1, 127, 0.0), (64, 33, 128, 0.02), (5, 0, 100, 0.0))),
    Shape(16, ((60, 37, 100, "records"), (40, 20, 100, 0.0))),
)
HIT_SHAPES = (  # small enough for the numpy DP of tests/positions_cases.py
    Shape(16, ((40, 37, 100, 0.01),)),
    Shape(22, ((300, 41, 33, 0.02), (33, 9, 129, 0.0))),
    Shape(16, ((1100, 7, 31, 0.01),)),
    Shape(32, ((70, 20, 127, 0.02), (5, 0, 127, 0.0), (0, 8, 127, 0.0), (9, 33, 256, 0.01))),
    Shape(16, ((60, 37, 100, "records"), (40, 20, 100, 0.0))),
)
# The samples kind's states, in this order per visit, both upload slots each time: equal windows without N, the
# same shape with N, ragged windows of the same n_bases (97..128 bases take the 128-base stride of 100 and 101),
# a smaller sample (one group: slot 1 is uploaded but has no k-mers), a larger one (the block grows; 5 + 1 groups),
# the first again.
SAMPLE_STATES = (
    Shape(16, ((70, 60, 100, 0.0), (33, 60, 101, 0.0))),
    Shape(16, ((70, 60, 100, 0.02), (33, 60, 101, 0.02))),
    Shape(16, ((70, 60, (97, 128), 0.02), (33, 60, (97, 128), 0.02))),
    Shape(22, ((40, 24, 100, 0.01), (0, 24, 101, 0.01))),
    Shape(16, ((1100, 80, 100, 0.01), (40, 80, 101, 0.01))),
    Shape(16, ((70, 60, 100, 0.0), (33, 60, 101, 0.0))),
)
TABLES = {"wm": WM_SHAPES, "bs": BS_SHAPES, "hits": HIT_SHAPES, "pos": HIT_SHAPES, "samples": SAMPLE_STATES,
          "wm_jobs": WM_JOBS_SHAPES, "bs_jobs": BS_SHAPES, "dp_jobs": BS_SHAPES, "hits_jobs": HIT_SHAPES,
          "pos_jobs": HIT_SHAPES, "submit": None,  # submit: HIT_SHAPES with hits=, BS_SHAPES without, alternately
          "profiles": HIT_SHAPES}
FIRST = {kind: i for i, kind in enumerate(KINDS)}  # where in its table a kind starts, so that no two run in step
# host-buffer co-occurrence shapes (n_kmers, n_windows) and cross ones (n_a, n_b, n_windows): small, larger, small
COOC_HOST = ((130, 257), (600, 1100), (33, 64))
CROSS_HOST = ((70, 33, 257), (300, 200, 1100), (9, 40, 31))


def live(job):
    return bool(job[0] and job[1])


def is_bs(kind, shape, bs_on=True):
    """stage_plan.cpp bs_launch: the launch is bit-sliced."""
    if not bs_on or kind == "wm" or shape.k not in BS_K:
        return False
    return all(isinstance(j[2], int) and 1 <= j[2] <= 256 for j in shape.jobs if live(j))


def group_size(k, staged, bs):
    """stage_plan.cpp launch_group_size: BS_GROUP, else wm_count.h cands_per_wave(pack_factor(k), staged)."""
    if bs:
        return 256
    P = min(32 // k, 4)
    return 64 * P * (2 if P == 2 else 2 if (P == 1 and staged) else 1)


def launch_groups(kind, shape, early=True, bs_on=True):
    """(group size, candidate groups) of the visit's count launch, as ac_last_launch reports them: the arithmetic
    of count_launch.cpp (groups_total) and of tests/test_gpu_bs_routes.py bs_rows."""
    gs = group_size(shape.k, kind in JOBS_KINDS and early, is_bs(kind, shape, bs_on))
    return gs, sum(-(-j[0] // gs) for j in shape.jobs if live(j))


def acc_slots(kind, shape):
    gs, groups = launch_groups(kind, shape)
    return gs * groups


def min_counters(kind, shape):
    """A lower bound of the launch's queue counters: 4 sub-queues per group."""
    return 4 * launch_groups(kind, shape)[1]


Visit = collections.namedtuple("Visit", "n kind nth shape E with_hits wh segment")
# n: the launch's index in the walk; nth: of its kind; with_hits: a submit with hits= / positions (odd nth of those);
# wh: a samples visit that also calls window_hits


def profile_args(v):
    """(spans, flanks, edits) of a profiles visit's window_hits call: the variants in turn by the kind's nth visit,
    D = 8 in the first round of four, 32 in the second, and so on."""
    variant = PROFILE_VARIANTS[v.nth % 4]
    D = DEPTHS[v.nth // 4 % 2] if "flanks" in variant else 0
    return variant == "spans", D, "edits" in variant


def pos_spans(v):
    """A pos visit that also passes spans= (every other one)."""
    return v.kind == "pos" and v.nth % 2 == 1


def euler_circuit(n, seed):
    """An Eulerian circuit of the complete digraph on n nodes without loops (Hierholzer; the seed orders every
    node's out-edges): n (n - 1) + 1 nodes, the first again at the end."""
    rng = random.Random(seed)
    out = {}
    for a in range(n):
        out[a] = [b for b in range(n) if b != a]
        rng.shuffle(out[a])
    stack, circuit = [0], []
    while stack:
        a = stack[-1]
        if out[a]:
            stack.append(out[a].pop())
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


def build_segments():
    """Lists of kinds: the circuit in runs of len(KINDS) transitions, each run beginning with the previous one's
    last kind again; then a self-pair inside a segment for every kind without one, and for two bit-sliced kinds in
    any case (the budget changes between two launches of one kind and k)."""
    n = len(KINDS)
    nodes = [KINDS[i] for i in euler_circuit(n, SEED)]
    segs = [nodes[i:i + n + 1] for i in range(0, len(nodes) - 1, n)]
    have = {segs[i][0] for i in range(1, len(segs))}
    need = [k for k in KINDS if k not in have]
    need += [k for k in ("bs", "hits_jobs") if k not in need]
    for kind in need:
        seg = min((s for s in segs if kind in s[1:]), key=len)
        at = seg.index(kind, 1)
        seg.insert(at, kind)
    return segs


def shape_of(kind, nth, with_hits):
    if kind == "submit":
        table = HIT_SHAPES if with_hits else BS_SHAPES
        return table[(nth // 2 + FIRST[kind]) % len(table)]
    if kind == "samples":
        return SAMPLE_STATES[nth % len(SAMPLE_STATES)]
    table = TABLES[kind]
    return table[(nth + FIRST[kind]) % len(table)]


def build_walk():
    """The launch visits, segment by segment: shapes by rotation, the growth visits, then the budget of every
    visit -- greedily the one that adds an uncovered change E -> E' or an uncovered (kind, E)."""
    segs = build_segments()
    nth = collections.Counter()
    visits = []
    grow = [ACC_GROW, QUEUE_GROW]
    for s, seg in enumerate(segs):
        for i, kind in enumerate(seg):
            v = nth[kind]
            nth[kind] += 1
            with_hits = kind == "submit" and v % 2 == 1
            shape = shape_of(kind, v, with_hits)
            same = i > 0 and seg[i - 1] == kind
            if same and kind != "samples":  # a self-pair inside a segment: the same shape, so the same k
                shape, with_hits = visits[-1].shape, visits[-1].with_hits
            elif kind == "wm" and grow and i > 0 and v >= 3 and (len(grow) == 2 or v >= 7):
                shape = grow.pop(0)
            elif START_GROW_AT.get(kind) == v:
                shape = START_GROW
            wh = kind == "samples" and is_bs(kind, shape)  # window_hits too, wherever it is legal
            visits.append(Visit(len(visits), kind, v, shape, None, with_hits, wh, s))
    assert not grow
    # budgets
    seen_change, seen_at = set(), set()
    cur, out = 2, []
    for v in visits:
        first = not out or out[-1].segment != v.segment
        if not is_bs(v.kind, v.shape):
            e = 2
        else:
            prev_same = not first and out[-1].kind == v.kind

            def score(e):
                return (4 * ((cur, e) not in seen_change and e != cur) + 2 * ((v.kind, e) not in seen_at) + (e != cur)
                        - 100 * (prev_same and e == cur), -((e - cur - 1) % 4))
            e = max(range(4), key=score)
        if not first and e != cur:
            seen_change.add((cur, e))
        seen_at.add((v.kind, e))
        cur = e
        out.append(v._replace(E=e))
    return out


def place_sides(visits):
    """sides[n]: the side operations in the gap before launch n (none before a segment's first launch) -- PER_GAP
    per gap, those the following kind has not had yet first; refuse_budget_k only where the context's budget is not 2;
    in a gap between two group sizes, the operations that still need such a gap first."""
    had = collections.defaultdict(set)
    total = collections.Counter()
    need_diff = set(BETWEEN_GROUP_SIZES)
    sides = {}
    for prev, v in zip(visits, visits[1:]):
        if prev.segment != v.segment:
            continue
        diff = launch_groups(prev.kind, prev.shape)[0] != launch_groups(v.kind, v.shape)[0]
        ok = [s for s in SIDES if s != "refuse_budget_k" or prev.E != 2]
        ok.sort(key=lambda s: (not (diff and s in need_diff), s in had[v.kind], total[s], SIDES.index(s)))
        pick = ok[:PER_GAP]
        for s in pick:
            had[v.kind].add(s)
            total[s] += 1
            if diff:
                need_diff.discard(s)
        sides[v.n] = tuple(pick)
    return sides


def build_ops(visits, sides):
    """The operations, segment by segment: ("set_max_errors", E), ("side", name, i) -- i counts the operation's
    uses, which rotates its shapes -- and ("launch", Visit)."""
    segs, uses, cur = [], collections.Counter(), None
    for v in visits:
        if v.segment == len(segs):
            segs.append([("set_max_errors", v.E)])  # (a fresh context starts at 2: the segment says its own)
            cur = v.E
        ops = segs[-1]
        for s in sides.get(v.n, ()):
            ops.append(("side", s, uses[s]))
            uses[s] += 1
        if v.E != cur:
            ops.append(("set_max_errors", v.E))
            cur = v.E
        ops.append(("launch", v))
    return segs


WALK = build_walk()
SIDES_AT = place_sides(WALK)
SEGMENTS = build_ops(WALK, SIDES_AT)


def upload_state_before(n):
    """The samples state whose slot 0 is on the device before launch n of the walk (the first one before any)."""
    last = [v for v in WALK[:n] if v.kind == "samples"]
    return last[-1].shape if last else SAMPLE_STATES[0]


# ---- cases and expected values, built once per shape -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(shape, j):
    """(kmers uint64, windows) of job j: budget_case (equal windows, windows at exactly 3 edits), planted_case
    (ragged ones) or n_windows_case ("records")."""
    from tests import cases
    from tests.test_gpu_bitslice import n_windows_case
    from tests.test_gpu_budget import budget_case

    nk, nw, L, n = shape.jobs[j]
    seed = 1000 * (sum(x if isinstance(x, int) else sum(x) for x in (nk, nw, L)) + shape.k) + j
    if n == "records":
        km, w = n_windows_case(seed, nw, L, [0, 1, 5, 0, 6, 4, 7], (0, 15, 16, 31, 32, 99))
        assert shape.k == 16 and nk == len(km)
        return np.asarray(km, np.uint64), w
    if n == "planted_n":
        from tests.edit_cases import planted_windows

        km, w = budget_case(seed, shape.k, nk, nw - 8, L, p_n=0.01)
        km = np.asarray(km[:nk], np.uint64)
        return km, list(w) + planted_windows(seed + 1, shape.k, [int(x) for x in km], 8, L)
    if not nw:
        return np.asarray(cases.planted_case(seed, shape.k, nk, 0)[0], np.uint64), []
    if isinstance(L, int):
        km, w = budget_case(seed, shape.k, max(nk, 1), nw, L, p_n=n)
        return np.asarray(km[:nk], np.uint64), w
    km, w = cases.planted_case(seed, shape.k, nk, nw, win_len=L, p_n=n)
    return np.asarray(km, np.uint64), [x[:L[1]] for x in w]  # (a planted occurrence may grow a window)


@functools.lru_cache(maxsize=None)
def expected_counts(shape, j, E):
    import oracle
    from tests.test_budget_cpu import count_e

    km, w = case(shape, j)
    if not (len(km) and len(w)):
        return np.zeros(len(km), np.uint64)
    if all(isinstance(x[2], int) for x in shape.jobs if live(x)) and shape in HIT_SHAPES:
        return expected_matrices(shape, j, E)[2]
    return oracle.count_myers(shape.k, km, w) if E == 2 else count_e(E, shape.k, km, w)


@functools.lru_cache(maxsize=None)
def expected_matrices(shape, j, E):
    """(hit bool (E + 1, n_windows, n_kmers), pos int16, counts) of job j."""
    from tests.positions_cases import expected_positions

    km, w = case(shape, j)
    return expected_positions(shape.k, km, w, E)


@functools.lru_cache(maxsize=None)
def expected_starts(shape, j, E):
    """int16 (n_windows, n_kmers) of job j: where each pair's best occurrence starts (tests.span_cases.starts_of),
    -1 where there is no hit."""
    from tests.span_cases import starts_of

    km, w = case(shape, j)
    hit, pos, _ = expected_matrices(shape, j, E)
    start = starts_of(shape.k, km, w, hit, pos)[0]
    start.setflags(write=False)
    return start


def packed_starts(shape, j, E):
    """The start matrix of job j in the matrix layout, uint32 (8, n_windows, words)."""
    from tests.span_cases import pack_starts

    return pack_starts(expected_starts(shape, j, E), expected_matrices(shape, j, E)[0][E])


@functools.lru_cache(maxsize=None)
def expected_flanks(shape, j, E, D, plane=None, with_start=True):
    """uint32 (2, n_kmers, D, 5) of job j over level plane `plane` (None: the top one, E), with the expected
    starts or with start = None (the left half zeros): tests.flank_cases.flank_profile_of."""
    from tests.flank_cases import flank_profile_of

    hit, pos, _ = expected_matrices(shape, j, E)
    start = expected_starts(shape, j, E) if with_start else None
    return flank_profile_of(case(shape, j)[1], hit[E if plane is None else plane], pos, start, D)


@functools.lru_cache(maxsize=None)
def expected_edits(shape, j, E, plane=None):
    """uint32 (n_kmers, k, 12) of job j over level plane `plane` (None: the top one): tests.edit_cases.edit_profile_of."""
    from tests.edit_cases import edit_profile_of

    km, w = case(shape, j)
    hit, pos, _ = expected_matrices(shape, j, E)
    return edit_profile_of(shape.k, km, w, hit[E if plane is None else plane], pos, expected_starts(shape, j, E))


@functools.lru_cache(maxsize=None)
def expected_exact(shape, j, limit=50):
    from oracle import host_ref

    _, w = case(shape, j)
    w = [x if isinstance(x, str) else "".join("ACGTN"[int(b)] for b in x) for x in w]
    counter, had_n = host_ref.count_kmers(w, shape.k, float(host_ref.adjust_threshold(1.0, 16, shape.k)), frozenset())
    return host_ref.get_most_frequent(counter, limit, shape.k), len(counter), had_n


@functools.lru_cache(maxsize=None)
def random_hits(n_kmers, n_windows, levels, seed):
    """(hit bool (levels, n_windows, n_kmers), the packed matrix with stray bits past n_kmers) of densities 0.5,
    0.1 and 0.03, for the host-buffer reductions."""
    from tests.hits_cases import pack_hits

    rng = np.random.default_rng(1000 * n_kmers + n_windows + seed)
    hit = np.stack([rng.random((n_windows, n_kmers)) < p for p in (0.5, 0.1, 0.03, 0.2)[:levels]])
    m = pack_hits(hit)
    if n_kmers % 32:
        m[:, :, -1] |= np.uint32((0xFFFFFFFF << (n_kmers % 32)) & 0xFFFFFFFF)
    return hit, m


def product(hit_a, hit_b):
    """numpy's H_a^T H_b per plane, as tests/test_gpu_cooc.py gram (float32 is exact below 2^24)."""
    assert hit_a.shape[1] < 1 << 24
    return np.stack([a.T @ b for a, b in zip(hit_a.astype(np.float32), hit_b.astype(np.float32))]).astype(np.uint32)


def matrix_after(visits):
    """(shape, job, E) of the hit matrix the reductions read after `visits` ran on one context at default
    settings: the first live job of the last hits or positions launch; before any, HIT_SHAPES[0] at E = 2,
    uploaded from the host."""
    m = (HIT_SHAPES[0], 0, 2)
    for v in visits:
        if v.kind in HIT_KINDS or (v.kind == "submit" and v.with_hits) or v.wh:
            m = (v.shape, next(j for j, x in enumerate(v.shape.jobs) if live(x)), v.E)
    return m


def flanks_side(i):
    """(with the start matrix, over the top plane, D) of the flanks_device operation's i-th use."""
    return i % 2 == 0, i // 2 % 2 == 0, DEPTHS[i // 4 % 2]


def edits_side(i):
    """Whether the edits_device operation's i-th use reads the top plane (else plane 0)."""
    return i % 2 == 0


# ---- the context's matrix blocks -----------------------------------------------------------------------------------

def align256(n):
    return (n + 255) // 256 * 256


def block_needs(v):
    """What launch v carves out of the context's grow-only matrix blocks at default settings, or None where it
    uses none: {block: bytes per job}.  capi.cpp count_samples (profiles, and a samples visit's window_hits) and
    jobs_stage.cpp count_jobs (hits_jobs, pos_jobs) carve `hits` and `pos` -- every job's matrix, a dead job's
    being empty; count_samples alone `start` (the position matrices' sizes and offsets, but a block of its own),
    `flank` and `edit` (live jobs only).  hits, pos and submit visits write the caller's tensors."""
    if v.kind == "profiles":
        spans, D, edits = profile_args(v)
        with_pos = True
    elif v.kind == "samples" and v.wh:
        spans, D, edits, with_pos = False, 0, False, v.nth % 2 == 1
    elif v.kind in ("hits_jobs", "pos_jobs"):
        spans, D, edits, with_pos = False, 0, False, v.kind == "pos_jobs"
    else:
        return None
    jobs, k = v.shape.jobs, v.shape.k
    words = [j[1] * ((j[0] + 31) // 32) for j in jobs]
    need = {"hits": [4 * (v.E + 1) * w for w in words]}
    if with_pos:
        need["pos"] = [4 * 8 * w for w in words]
    if v.kind == "profiles":
        need["start"] = need["pos"]
        if D:
            need["flank"] = [4 * 2 * j[0] * D * 5 if live(j) else 0 for j in jobs]
        if edits:
            need["edit"] = [4 * j[0] * k * 12 if live(j) else 0 for j in jobs]
    return need
