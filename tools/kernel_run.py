#!/usr/bin/env python3
"""Device-resident count-kernel launches of one BASELINE configuration, for
rocprofv3 PMC passes and kernel traces that must see only the kernel (the
bench's stage reads its inputs from pinned host memory, which changes the
memory counters).  Same workload and launch as bench.py's kernel leg.

    rocprofv3 --pmc SQ_INSTS_VALU -d gpurun_out/pmc_valu -o run -- \
        python3 tools/kernel_run.py --config cfg2 --launches 20

--k and --max-errors run the configuration's shape at another pattern length and edit budget
(ac_set_max_errors: the bit-sliced kernels); --time prints the launches' mean kernel time
from HIP events around them (back-to-back launches on resident input), for E = 3 against E = 2:

    python3 tools/kernel_run.py --config cfg5 --k 24 --max-errors 3 --warmup 20 --launches 100 --time

--hits runs the hits-writing kernels (ac_window_hits_device: the same launch also stores every window's hit
levels, DESIGN.md 4e "Hit levels") and prints the bytes of the matrices beside the time; --level-counts then
times ac_hit_level_counts_device over the first segment's matrix and prints the rate its bytes were read at.
--positions runs the hits-and-positions kernels instead (ac_window_positions_device, DESIGN.md 4e "Match end
positions"); --profile then times ac_hit_position_profile_device over the first segment's two matrices.
--spans (with --positions) then times the span pass (ac_hit_start_positions_device, DESIGN.md 4e "Match spans") over
every segment's matrices on resident input, in rounds interleaved with the hits-and-positions launch that produces
its input, and prints the top level plane's hit density; --random-windows replaces every window by random bases (no
planted occurrence: a density near 0, to see whether the pass's time follows the hits or the pairs).
--flanks D (with --positions --spans) also times the flank pass (ac_hit_flank_profile_device, DESIGN.md 4e "Flank
profiles") at depth D over every segment's top level plane, position matrix and start matrix, in the same interleaved
rounds, beside the floor of reading the 17 planes once at the measured HBM rate.
--edits (with --positions --spans) also times the edit pass (ac_hit_edit_profile_device, DESIGN.md 4e "Edit
profiles") over the same plane and matrices, in the same interleaved rounds, and prints its observations.
--cooc (with --hits or --positions) then times the co-occurrence of the first segment's top level plane on the
resident matrix (ac_hit_cooccurrence_device, DESIGN.md 4e "Co-occurrence"): the transposition and the product on
their own (ac_testing_hit_cooccurrence_stages) and the whole call, beside the level counter on the same plane and
the op model n (n + 1) / 2 x ceil(W / 32) x 2 lane-ops against bench.py's VALU peak.
--cross (with --hits or --positions) times the cross co-occurrence of the first two segments' top level planes
(ac_hit_cross_cooccurrence_device, DESIGN.md 4e "Cross co-occurrence"; the segments must hold the same number of
windows): the two transpositions and the cross product on their own (ac_testing_hit_cross_stages) and the whole
call, beside the Gram call's stages on the first segment in the same session, and the product times per tile.
--staged --hits / --positions run the staged hits kernels (ac_window_hits_jobs_submit, DESIGN.md 4e "Hits from the
jobs stage") on input sent ahead; --staged --time the staged counting kernel the same way, to set them against.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=0,
                    help="launches before the counted ones (a cold GPU runs its first ~10 ms below the "
                         "sustained clock; kernel traces then leave them out: prof_summary.py --skip)")
    ap.add_argument("--descriptors", action="store_true",
                    help="load every window's start / length (ac_error_count_device) even for equal windows")
    ap.add_argument("--staged", action="store_true",
                    help="the early launch's staged instantiation on resident input instead: ac_error_count_jobs "
                         "with every job sent ahead of the launch (AC_TESTING_ALL_AHEAD), so a kernel trace shows "
                         "its own cost against the plain kernel's")
    ap.add_argument("--k", type=int, help="pattern length instead of the configuration's")
    ap.add_argument("--max-errors", type=int, default=2, help="edit budget of the count (0..3; default 2)")
    ap.add_argument("--time", action="store_true", help="print the mean time of a launch (HIP events)")
    ap.add_argument("--hits", action="store_true", help="the hits-writing kernels (ac_window_hits_device)")
    ap.add_argument("--level-counts", action="store_true",
                    help="with --hits: also time ac_hit_level_counts_device over the first segment's matrix")
    ap.add_argument("--positions", action="store_true",
                    help="the hits-and-positions kernels (ac_window_positions_device); implies --hits")
    ap.add_argument("--profile", action="store_true",
                    help="with --positions: also time ac_hit_position_profile_device over the first segment's matrices")
    ap.add_argument("--spans", action="store_true",
                    help="with --positions: also time ac_hit_start_positions_device over every segment's matrices, "
                         "interleaved with the launch, and print the top plane's hit density")
    ap.add_argument("--flanks", default="", metavar="D[,D..]",
                    help="with --positions --spans: also time ac_hit_flank_profile_device at depth D (1..32; several: "
                         "each in turn) over every segment's matrices, in the same interleaved rounds")
    ap.add_argument("--edits", action="store_true",
                    help="with --positions --spans: also time ac_hit_edit_profile_device over every segment's matrices, in "
                         "the same interleaved rounds")
    ap.add_argument("--random-windows", action="store_true",
                    help="replace every window by random bases of the same length (no planted occurrence)")
    ap.add_argument("--cooc", action="store_true",
                    help="with --hits / --positions: also time ac_hit_cooccurrence_device over the first segment's top "
                         "level plane: transposition, product and the whole call")
    ap.add_argument("--cross", action="store_true",
                    help="with --hits / --positions: also time ac_hit_cross_cooccurrence_device over the first two "
                         "segments' top level planes: transpositions, product and the whole call, beside the Gram call")
    a = ap.parse_args()
    a.hits = a.hits or a.positions
    a.flanks = [int(x) for x in a.flanks.split(",") if x]
    import torch

    import approx_counter_amd as ac
    import bench

    sys.argv = ["bench.py", "--config", a.config] + (["--k", str(a.k)] if a.k else [])
    args = bench.parse()
    wl, _ = bench.build_workload(args, 0, 1)
    if a.random_windows:
        import numpy as np

        rng = np.random.default_rng(args.seed)
        for e in ("start", "end"):
            wl[e]["windows"] = [rng.integers(0, 4, size=len(w), dtype=np.uint8) for w in wl[e]["windows"]]
    if a.staged:
        from approx_counter_amd._lib import load

        L = load()
        jobs = [(wl[e]["kmers"], ac.Dna5Sample.from_windows(wl[e]["windows"])) for e in ("start", "end")]
        with ac.ApproxCounter(0, max_errors=a.max_errors) as c:
            prev = L.ac_testing_stage_hooks(2)  # AC_TESTING_ALL_AHEAD
            try:
                if a.hits or a.time:
                    # the submit forms: counts (and matrices) stay in device memory, so HIP events around the
                    # calls time the copy ahead and the staged kernel alone -- with --hits / --positions the
                    # staged hits kernels (ac_window_hits_jobs_submit / ac_window_positions_jobs_submit)
                    jb = ac.Jobs(jobs)
                    shapes = [(int(km.size), smp.n_windows) for km, smp in zip(jb.kmers, jb.samples)]
                    mk = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device="cuda")  # noqa: E731
                    hits = [mk(ac.hits_words(nk, nw, a.max_errors)) for nk, nw in shapes] if a.hits else None
                    pos = [mk(ac.positions_words(nk, nw)) for nk, nw in shapes] if a.positions else None
                    out = mk(jb.n_counts)
                    st = torch.cuda.current_stream()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    for i in range(a.warmup + a.launches):
                        if i == a.warmup:
                            t0.record()
                        c.submit_jobs(args.k, jb, out, stream=st.cuda_stream, hits=hits, positions=pos)
                    t1.record()
                    torch.cuda.synchronize()
                    c.check()
                    mb = sum(t.numel() for t in (hits or []) + (pos or [])) * 4 / 1e6
                    print(f"staged {'hits-and-positions' if a.positions else 'hits' if a.hits else 'counting'} kernel, "
                          f"k = {args.k}, E = {a.max_errors}: mean launch {t0.elapsed_time(t1) / a.launches * 1e3:.1f} us "
                          f"(copy ahead included), {mb:.1f} MB of matrices")
                else:
                    for _ in range(a.warmup + a.launches):
                        c.count_jobs(args.k, jobs)
            finally:
                L.ac_testing_stage_hooks(prev)
            print(f"{a.launches} staged launches of {a.config} on resident input (stage mode {c.stage_mode()}); "
                  f"geometry {c.last_launch()}")
        return
    packed = [ac.pack_windows(wl[e]["windows"]) for e in ("start", "end")]
    segs = [ac.DeviceSegment.upload(wl[e]["kmers"], packed[i]) for i, e in enumerate(("start", "end"))]
    arr = ac.ApproxCounter.segment_array(segs)
    eq = [p.equal_window_len() for p in packed]
    wlen = eq if all(x is not None for x in eq) and not a.descriptors else None
    with ac.ApproxCounter(0, max_errors=a.max_errors) as c:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hits = None
        if a.hits:
            words = [ac.hits_words(s.n_kmers, s.n_windows, a.max_errors) for s in segs]
            hits = [torch.empty(max(w, 1), dtype=torch.int32, device="cuda") for w in words]
        pos = None
        if a.positions:
            pwords = [ac.positions_words(s.n_kmers, s.n_windows) for s in segs]
            pos = [torch.empty(max(w, 1), dtype=torch.int32, device="cuda") for w in pwords]
        for i in range(a.warmup + a.launches):
            if i == a.warmup:
                t0.record()
            c.count_device(args.k, arr, window_len=wlen, hits=hits, positions=pos)
        t1.record()
        torch.cuda.synchronize()
        c.check()
        print(f"{a.launches} launches of {a.config} ({'equal windows' if wlen else 'descriptors'}); "
              f"geometry {c.last_launch()}")
        if a.time:
            print(f"k {args.k} max_errors {a.max_errors}: {t0.elapsed_time(t1) / a.launches:.4f} ms per launch "
                  f"({a.launches} launches after {a.warmup})"
                  + (f"; hits written per launch: {4 * sum(words)} bytes" if a.hits else "")
                  + (f"; positions written per launch: {4 * sum(pwords)} bytes" if a.positions else ""))
        if a.hits and a.level_counts:
            s0 = segs[0]
            for i in range(a.warmup + a.launches):
                if i == a.warmup:
                    t0.record()
                lc = c.hit_level_counts(hits[0], s0.n_kmers, s0.n_windows, a.max_errors + 1)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / a.launches
            assert (lc.sum(dim=0).cpu().numpy() == s0.counts_numpy()).all(), "level counts do not sum to the counts"
            print(f"level counts of {4 * words[0]} bytes ({s0.n_kmers} k-mers x {s0.n_windows} windows x "
                  f"{a.max_errors + 1} levels): {ms:.4f} ms per call (memset + kernel), "
                  f"{4 * words[0] / ms / 1e6:.1f} GB/s read")
        if a.hits and a.cooc:
            import ctypes

            from approx_counter_amd import _lib

            s0 = segs[0]
            n, nw, E = s0.n_kmers, s0.n_windows, a.max_errors
            top = hits[0][E * nw * ((n + 31) // 32):]  # (the single-plane idiom: plane E with levels = 1)
            out = torch.empty(max(n * n, 1), dtype=torch.int32, device="cuda")
            p = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), _lib.p32)  # noqa: E731
            ms = {}
            for name, stages in (("transposition", 1), ("product", 2), ("both", 3)):
                for i in range(a.warmup + a.launches):
                    if i == a.warmup:
                        t0.record()
                    _lib.check(c._L.ac_testing_hit_cooccurrence_stages(c.handle, p(top), n, nw, 1, p(out), stages, None), c.handle)
                t1.record()
                torch.cuda.synchronize()
                ms[name] = t0.elapsed_time(t1) / a.launches
            for i in range(a.warmup + a.launches):
                if i == a.warmup:
                    t0.record()
                lc = c.hit_level_counts(top, n, nw, 1)
            t1.record()
            torch.cuda.synchronize()
            ms["level counts"] = t0.elapsed_time(t1) / a.launches
            co = out[: n * n].view(n, n)
            assert (co.diagonal() == lc[0]).all(), "the diagonal is not the level counts"
            assert (co == co.t()).all(), "the co-occurrence is not symmetric"
            ops = n * (n + 1) // 2 * ((nw + 31) // 32) * 2
            print(f"co-occurrence of plane {E} ({n} k-mers x {nw} windows, {4 * nw * ((n + 31) // 32)} bytes in, {4 * n * n} out): "
                  + ", ".join(f"{k} {v:.4f} ms" for k, v in ms.items())
                  + f" per call; op model {ops:.3e} lane-ops = {ops / bench.VALU_PEAK_OPS * 1e3:.4f} ms at the VALU peak, "
                  f"{ops / bench.VALU_PEAK_OPS * 1e3 / ms['product'] * 100:.1f} % of the product's time")
        if a.hits and a.cross:
            import ctypes

            from approx_counter_amd import _lib

            sa, sb = segs[0], segs[1]
            na, nb, nw, E = sa.n_kmers, sb.n_kmers, sa.n_windows, a.max_errors
            if sb.n_windows != nw:
                sys.exit(f"--cross: the two segments hold {nw} and {sb.n_windows} windows; it needs equal counts")
            top_a = hits[0][E * nw * ((na + 31) // 32):]
            top_b = hits[1][E * nw * ((nb + 31) // 32):]
            out = torch.empty(max(na * nb, 1), dtype=torch.int32, device="cuda")
            gram = torch.empty(max(na * na, 1), dtype=torch.int32, device="cuda")
            p = lambda t: ctypes.cast(ctypes.c_void_p(t.data_ptr()), _lib.p32)  # noqa: E731
            L, h = c._L, c.handle
            legs = [(f"cross {name}", lambda st: L.ac_testing_hit_cross_stages(h, p(top_a), na, p(top_b), nb, nw, 1, p(out), st, None), st)
                    for name, st in (("transpositions", 1), ("product", 2), ("both", 3))]
            legs += [(f"gram {name}", lambda st: L.ac_testing_hit_cooccurrence_stages(h, p(top_a), na, nw, 1, p(gram), st, None), st)
                     for name, st in (("transposition", 1), ("product", 2), ("both", 3))]
            ms = {}
            for name, call, st in legs:  # (each leg's stage 2 reads the scratch its own stage 1 filled just before)
                for i in range(a.warmup + a.launches):
                    if i == a.warmup:
                        t0.record()
                    _lib.check(call(st), h)
                t1.record()
                torch.cuda.synchronize()
                ms[name] = t0.elapsed_time(t1) / a.launches
            g = gram[: na * na].view(na, na).clone()
            _lib.check(L.ac_hit_cross_cooccurrence_device(h, p(top_a), na, p(top_a), na, nw, 1, p(gram), None), h)
            torch.cuda.synchronize()
            assert (gram[: na * na].view(na, na) == g).all(), "cross(A, A) is not the Gram product"
            lc = c.hit_level_counts(top_b, nb, nw, 1)
            cx = out[: na * nb].view(na, nb)
            assert (cx <= lc[0][None, :]).all(), "a cross count exceeds its column's level count"
            ta, tb = (na + 63) // 64, (nb + 63) // 64
            tiles, pairs = ta * tb, ta * (ta + 1) // 2
            per_c, per_g = ms["cross product"] / tiles, ms["gram product"] / pairs
            print(f"cross co-occurrence of planes {E} ({na} x {nb} k-mers, {nw} windows, {4 * na * nb} bytes out): "
                  + ", ".join(f"{k} {v:.4f} ms" for k, v in ms.items())
                  + f" per call; cross product {per_c * 1e3:.4f} us per tile ({tiles} tiles), gram product "
                  f"{per_g * 1e3:.4f} us per tile pair ({pairs} pairs), ratio {per_c / per_g:.3f}")
        if a.positions and a.spans:
            if wlen is None:
                sys.exit("--spans needs equal windows")
            E, lv = a.max_errors, a.max_errors + 1
            starts = [torch.empty(max(w, 1), dtype=torch.int32, device="cuda") for w in pwords]
            live = [i for i, s in enumerate(segs) if s.n_kmers and s.n_windows]

            def the_pass():
                for i in live:
                    c.hit_start_positions(args.k, segs[i].kmers, segs[i].n_kmers, segs[i], wlen[i], hits[i], pos[i], lv,
                                          out=starts[i])

            flank_out = [torch.empty(max(ac.flank_words(s.n_kmers, 32), 1), dtype=torch.int32, device="cuda") for s in segs]
            tops = [hits[i][E * s.n_windows * ((s.n_kmers + 31) // 32):] for i, s in enumerate(segs)]

            def the_flank_pass(D):
                for i in live:
                    c.hit_flank_profile(segs[i], wlen[i], tops[i], pos[i], starts[i], segs[i].n_kmers, segs[i].n_windows,
                                        D, out=flank_out[i])

            edit_out = [torch.empty(max(ac.edit_words(s.n_kmers, args.k), 1) if a.edits else 1, dtype=torch.int32, device="cuda")
                        for s in segs]

            def the_edit_pass():
                for i in live:
                    c.hit_edit_profile(args.k, segs[i].kmers, segs[i].n_kmers, segs[i], wlen[i], tops[i], pos[i], starts[i],
                                       segs[i].n_windows, out=edit_out[i])

            rounds, t_launch, t_pass, t_flank, t_edit = 5, [], [], {D: [] for D in a.flanks}, []
            for r in range(rounds):  # a round: the launch's calls, then the pass's, on the same box minutes apart at most
                for call, into in ((lambda: c.count_device(args.k, arr, window_len=wlen, hits=hits, positions=pos), t_launch),
                                   (the_pass, t_pass)) + tuple((lambda D=D: the_flank_pass(D), t_flank[D]) for D in a.flanks) \
                        + (((the_edit_pass, t_edit),) if a.edits else ()):
                    for i in range(a.warmup + a.launches):
                        if i == a.warmup:
                            t0.record()
                        call()
                    t1.record()
                    torch.cuda.synchronize()
                    into.append(t0.elapsed_time(t1) / a.launches)
            c.check()
            pairs = hit_pairs = steps = 0
            j = torch.arange(32, device="cuda", dtype=torch.int32)[:, None]

            def values(planes):  # (8, words) plane words -> (32, words) values, bit j of a word its row j
                v = torch.zeros((32, planes.shape[1]), dtype=torch.int32, device="cuda")
                for b in range(8):
                    v |= ((planes[b][None, :] >> j) & 1) << b
                return v

            for i in live:
                s, words_i = segs[i], (segs[i].n_kmers + 31) // 32
                top = hits[i][E * s.n_windows * words_i: lv * s.n_windows * words_i]
                st, pl = starts[i][: pwords[i]].view(8, -1), pos[i][: pwords[i]].view(8, -1)
                assert not bool((st & ~top[None, :]).any()), "a start bit without a hit"
                mask = ((top[None, :] >> j) & 1).bool()
                ln = (values(pl) + 1 - values(st))[mask]
                # every hit has a span, of a length the budget allows
                assert bool(((ln >= args.k - E) & (ln <= args.k + E)).all()), "an occurrence length outside k - E .. k + E"
                hit_pairs += int(mask.sum())
                pairs += s.n_kmers * s.n_windows
                steps += int(ln.sum())
            ml, mp = sum(t_launch) / rounds, sum(t_pass) / rounds
            ops = steps * 30 + hit_pairs * 35  # (hit_span.h: about 30 integer ops a column, 35 to split the k-mer)
            print(f"span pass, k {args.k} E {E}: top plane density {hit_pairs / max(pairs, 1) * 100:.3f} % "
                  f"({hit_pairs} of {pairs} pairs); pass {mp:.4f} ms, launch {ml:.4f} ms, ratio {mp / ml:.3f} "
                  f"(rounds: pass {', '.join(f'{x:.4f}' for x in t_pass)}; launch {', '.join(f'{x:.4f}' for x in t_launch)}); "
                  f"op model {steps} columns = {ops:.3e} lane-ops = {ops / bench.VALU_PEAK_OPS * 1e3:.5f} ms at the VALU "
                  f"peak, {ops / bench.VALU_PEAK_OPS * 1e3 / mp * 100:.2f} % of the pass's time")
            for D in a.flanks:
                mf, obs = sum(t_flank[D]) / rounds, 0
                the_flank_pass(D)
                for i in live:
                    s = segs[i]
                    fl = flank_out[i][: ac.flank_words(s.n_kmers, D)].view(2, s.n_kmers, D, 5).to(torch.int64)
                    prof = c.hit_position_profile(tops[i], pos[i], s.n_kmers, s.n_windows, 1, wlen[i]).to(torch.int64)
                    # the right side's column j sums to the windows whose occurrence ends at or before L - j - 1
                    head = torch.cumsum(prof[0], dim=1)
                    for jj in range(D):
                        want = head[:, wlen[i] - jj - 2] if wlen[i] - jj - 2 >= 0 else torch.zeros_like(head[:, 0])
                        assert bool((fl[0, :, jj].sum(dim=1) == want).all()), "a right column is not the position profile's head"
                    obs += int(fl.sum())
                planes_b = 17 * 4 * sum(segs[i].n_windows * ((segs[i].n_kmers + 31) // 32) for i in live)
                floor = planes_b / 6.29e12 * 1e3  # (MI355X_MICROARCH.md: 6.29 TB/s measured of the 8.0 TB/s spec)
                print(f"flank pass, k {args.k} E {E} D {D}: {obs} observations of {hit_pairs} pairs; pass {mf:.4f} ms "
                      f"(rounds: {', '.join(f'{x:.4f}' for x in t_flank[D])}), launch {ml:.4f} ms, span pass {mp:.4f} ms, "
                      f"ratio to the launch {mf / ml:.3f}; 17 planes = {planes_b} bytes, {floor:.5f} ms at 6.29 TB/s, "
                      f"{floor / mf * 100:.2f} % of the pass's time")
            if a.edits:
                me, obs, edits_seen = sum(t_edit) / rounds, 0, 0
                the_edit_pass()
                for i in live:
                    s = segs[i]
                    ed = edit_out[i][: ac.edit_words(s.n_kmers, args.k)].view(s.n_kmers, args.k, 12).to(torch.int64)
                    lc = c.hit_level_counts(tops[i], s.n_kmers, s.n_windows, 1).to(torch.int64)
                    # every hit window aligns every base of the k-mer: match, substitution or deletion
                    assert bool((ed[:, :, :7].sum(dim=2) == lc[0][:, None]).all()), "a base's operations are not the level count"
                    obs += int(ed.sum())
                    edits_seen += int(ed[:, :, 1:].sum())
                print(f"edit pass, k {args.k} E {E}: {obs} observations ({edits_seen} edits) of {hit_pairs} pairs; pass {me:.4f} ms "
                      f"(rounds: {', '.join(f'{x:.4f}' for x in t_edit)}), launch {ml:.4f} ms, span pass {mp:.4f} ms"
                      + "".join(f", flank pass D {D} {sum(t_flank[D]) / rounds:.4f} ms" for D in a.flanks)
                      + f"; ratio to the span pass {me / mp:.3f}, to the launch {me / ml:.3f}; "
                      f"{obs / me / 1e6:.3f} G observations/s, {hit_pairs / me / 1e6:.3f} G pairs/s")
        if a.positions and a.profile:
            s0 = segs[0]
            for i in range(a.warmup + a.launches):
                if i == a.warmup:
                    t0.record()
                prof = c.hit_position_profile(hits[0], pos[0], s0.n_kmers, s0.n_windows, a.max_errors + 1, wlen[0])
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / a.launches
            lc = c.hit_level_counts(hits[0], s0.n_kmers, s0.n_windows, a.max_errors + 1)
            assert (prof.sum(dim=(0, 2)) == lc[-1]).all(), "the profile does not sum to the last level's counts"
            print(f"position profile of {4 * (words[0] + pwords[0])} bytes ({s0.n_kmers} k-mers x {s0.n_windows} windows x "
                  f"{a.max_errors + 1} levels + 8 planes, window_len {wlen[0]}): {ms:.4f} ms per call (memset + kernel), "
                  f"{4 * (words[0] + pwords[0]) / ms / 1e6:.1f} GB/s of the matrices' bytes")


if __name__ == "__main__":
    main()
