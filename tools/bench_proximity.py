#!/usr/bin/env python
"""Cost of the proximity graphs of a slide's nuclei (csrc/cellprox.hip) beside the cell graph, the spanning forest and scipy -- prints ONE
JSON line (profiles/cell_proximity.json).

    python tools/bench_proximity.py [--n 500000] [--extent 36000] [--radius 64] [--by any] [--classes 5] [--repeats 10] [--warmup 3]
                                    [--also LABEL=path/to/libnuhtc_hip.so ...] [--rounds 2]

Synthetic nucleus centres from the generator of tools/bench_points.py: `--n` points uniform on a square of `--extent` px, and one CLUSTERED
set of the same size (400 Gaussian clumps, sigma 300 px).  For each set:
  device_ms            nuhtc_cell_proximity alone, between two events, points and outputs resident on the device and room for 4 n + 64 edges
                       or, when there are more, for exactly that many (every stage, its own scratch allocation, the counts read back and
                       the final synchronisation included: it is one blocking call), `--repeats` after `--warmup`; the calls around the
                       timed ones are compared bitwise with the first (device_calls_repeat)
  m, m_rng             the Gabriel edges and how many of them are RNG edges
  device_stage_ms      one further call under the library's per-kernel profile: the cell_prox_* stages
  device_end_to_end_ms proximity.build from numpy to numpy: bounding box, upload, the call(s), download (wall clock)
  graph_ms, mst_ms     the yardsticks: nuhtc_cell_graph (k 8) and nuhtc_cell_mst on the same points at the same radius and mode in the same
                       process, timed the same way; forest_inside_rng says that every edge of the forest is an RNG edge of the device
  variants             with --also: other builds of the library (dev probes of csrc/cellprox.hip, see its -DNUHTC_PROX_* switches) timed in
                       `--rounds` alternating rounds with the shipped one, all in this process; each must return the shipped arrays
  scipy_ms             the host: cKDTree.query_pairs within the radius, then the two emptiness tests in numpy over the candidate's
                       neighbours; the edge sets and RNG flags must equal the device's.  Skipped with a note when scipy is not importable.
  checked_against_reference  a window of the points small enough for brute force, through the device again, against proximity_reference
bench.py is the project's headline benchmark and is not changed by this tool."""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_points as bp  # noqa: E402
from bench_points import med  # noqa: E402


def scipy_route(pts, lab, r, by):
    """-> (edges int64 (m, 2) ascending, rng bool (m,), ms for the pairs, ms for the tests).  query_pairs, then for every candidate the
    witnesses among the neighbours of its first end (a blocker is nearer to it than the other end is), padded to the widest list."""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    kd = cKDTree(pts.astype(np.float64))                      # half pixels as float64: integers, their squares exact
    pairs = kd.query_pairs(r + 0.5, output_type='ndarray').astype(np.int64)
    t1 = time.perf_counter()
    p = pts.astype(np.int64)
    i, j = pairs.min(1), pairs.max(1)
    dij = ((p[i] - p[j]) ** 2).sum(1)
    keep = dij <= r * r
    if by:
        keep &= lab[i] == lab[j]
    i, j, dij = i[keep], j[keep], dij[keep]
    n = len(p)
    both = np.concatenate([np.stack([i, j], 1), np.stack([j, i], 1)])          # the neighbour lists of every row, as a padded table
    both = both[np.argsort(both[:, 0], kind='stable')]
    count = np.bincount(both[:, 0], minlength=n)
    start = np.concatenate([[0], np.cumsum(count)])
    gab, rng = np.ones(len(i), bool), np.ones(len(i), bool)
    for c0 in range(0, len(i), 1 << 16):
        ic, jc, dc = i[c0:c0 + (1 << 16)], j[c0:c0 + (1 << 16)], dij[c0:c0 + (1 << 16), None]
        width = int(count[ic].max()) if len(ic) else 0
        slot = np.arange(width)[None, :]
        has = slot < count[ic, None]
        k = both[np.minimum(start[ic, None] + slot, len(both) - 1), 1]
        has &= k != jc[:, None]
        dik, djk = ((p[k] - p[ic, None]) ** 2).sum(2), ((p[k] - p[jc, None]) ** 2).sum(2)
        gab[c0:c0 + (1 << 16)] = ~((dik + djk < dc) & has).any(1)
        rng[c0:c0 + (1 << 16)] = ~((np.maximum(dik, djk) < dc) & has).any(1)
    e = np.stack([i[gab], j[gab]], 1)
    order = np.lexsort((e[:, 1], e[:, 0]))
    t2 = time.perf_counter()
    return e[order], rng[gab][order], 1e3 * (t1 - t0), 1e3 * (t2 - t1)


def measure(name, pts, lab, C, r, args, also):
    from nuhtc_amd import mst
    from nuhtc_amd import proximity as px
    n, by = len(pts), px.BY[args.by]
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    mout = mst.outputs(n, dev)
    cap, out, (_, m, m_rng) = bp.grown(lambda cap, out: px.call(p_d, l_d, C, r, by, cap, *out, bounds=bounds), lambda cap: px.outputs(n, cap, dev),
                                       px.first_edge_cap(n))
    found = dict(m=m, m_rng=m_rng)

    def prox_call():
        rc, found['m'], found['m_rng'] = px.call(p_d, l_d, C, r, by, cap, *out, bounds=bounds)
        return rc

    first, checked, repeated = bp.repeating(prox_call, out, lambda: (found['m'], found['m_rng']))
    timed = lambda fn, warmup=args.warmup: bp.timed(fn, args.repeats, warmup)
    checked()
    ms = timed(prox_call)
    checked()
    dev_out = [first[0][:m].cpu().numpy(), first[1][:m].cpu().numpy(), first[2][:m].cpu().numpy(), first[3].cpu().numpy()]
    gms = bp.graph_yardstick(p_d, l_d, C, r, bounds, args)
    mfound = {}

    def mst_call():
        rc, mfound['m'], _, _ = mst.call(p_d, l_d, C, r, by, *mout, bounds=bounds)
        return rc
    mms = timed(mst_call)
    forest = mout[0][:mfound['m']].cpu().numpy().astype(np.int64)
    code = lambda e: e[:, 0].astype(np.int64) * n + e[:, 1]
    inside = bool(np.isin(code(forest), code(dev_out[0][dev_out[2] == 1])).all())
    stages = bp.stage_split(prox_call, 'cell_prox')
    # ---- other builds of the library, alternating with the shipped one in this process
    vp, stream = bp.raw(dev)
    held = {label: (px.outputs(n, cap, dev), ctypes.c_int64(-1), ctypes.c_int64(-1)) for label in also}
    others = {label: (lambda fn=fn, vout=held[label][0], vm=held[label][1], vr=held[label][2]:
                      fn(0, vp(p_d), vp(l_d), n, C, r, by, cap, *bounds, *(vp(t) for t in vout), ctypes.byref(vm), ctypes.byref(vr), stream))
              for label, fn in also.items()}
    equals = lambda label: (held[label][1].value, held[label][2].value) == (m, m_rng) and bp.tensors_equal(held[label][0], first)
    variants = bp.variants(prox_call, others, equals, args)
    e2e, got = bp.end_to_end(lambda: px.build(pts, lab, C, r / 2, by))
    same = bool(all(np.array_equal(a, b) for a, b in zip(got[:4], dev_out)) and got[4:] == (m, m_rng))
    # ---- a window small enough for brute force, through the device again and against the definition
    win = bp.brute_window(pts, bounds, args.extent, args.check_n)
    sub, ref = px.build(pts[win], lab[win], C, r / 2, by), px.proximity_reference(pts[win], lab[win], C, r, by)
    exact = bool(all(np.array_equal(a, b) for a, b in zip(sub[:4], ref[:4])) and sub[4:] == ref[4:])
    line = dict(points=name, n=n, m=int(m), m_rng=int(m_rng), mean_gabriel_degree=round(2 * m / n, 3), mean_rng_degree=round(2 * m_rng / n, 3),
                mean_edge_px=round(float(np.sqrt(dev_out[1].astype(np.float64)).mean() / 2), 3) if m else 0.0,
                **bp.device_columns(ms, stages, e2e, same), device_calls_repeat=repeated(), **bp.graph_columns(gms, ms),
                mst_ms=[round(v, 3) for v in mms], mst_ms_median=round(med(mms), 3), device_over_mst=round(med(ms) / med(mms), 2),
                forest_edges=int(mfound['m']), forest_inside_rng=inside, variants=variants,
                checked_points=int(win.sum()), checked_against_reference=exact)
    # ---- the host: scipy on the same points
    try:
        import scipy.spatial  # noqa: F401
    except ImportError:
        line.update(scipy_ms=None, scipy_note='scipy is not importable')
        return line
    se, srng, pairs_ms, tests_ms = scipy_route(pts, lab, r, by)
    agree = bool(np.array_equal(se, dev_out[0].astype(np.int64)) and np.array_equal(srng, dev_out[2].astype(bool)))
    sk_ms = pairs_ms + tests_ms
    line.update(scipy_ms=round(sk_ms, 1), scipy_pairs_ms=round(pairs_ms, 1), scipy_tests_ms=round(tests_ms, 1),
                scipy_over_device_call=round(sk_ms / med(ms), 1), scipy_over_device_end_to_end=round(sk_ms / med(e2e), 1), scipy_edge_sets_agree=agree)
    return line


def main(argv=None):
    ap = bp.parser()
    ap.add_argument('--radius', type=float, default=64.0, help='px')
    ap.add_argument('--by', choices=('any', 'class'), default='any')
    bp.also_arguments(ap)
    args = ap.parse_args(argv)
    from nuhtc_amd import proximity as px
    bp.need_gpu('bench_proximity.py')
    C, r = args.classes, px.half_pixel_radius(args.radius)
    px.check_args(C, r, px.BY[args.by])
    also = bp.also_builds(args.also, 'nuhtc_cell_proximity')
    sets = [measure(name, p, lab, C, r, args, also) for name, (p, lab) in bp.point_sets(args.n, args.extent, C).items()]
    line = dict(what=f'tools/bench_proximity.py: Gabriel graph and relative neighbourhood graph of {args.n} synthetic nucleus centres on a {args.extent}-px square, '
                     f'radius {args.radius:g} px, by {args.by}, {C} classes, one MI355X; device: {args.repeats} calls after {args.warmup} warm-up calls; '
                     f'yardsticks: nuhtc_cell_graph k 8 and nuhtc_cell_mst at the same radius; host: scipy cKDTree.query_pairs + the two tests in numpy; '
                     f'variants: median ms of {args.repeats} calls per round, {args.rounds} alternating rounds',
                n=args.n, extent_px=args.extent, radius_px=args.radius, by=args.by, classes=C, sets=sets)
    bp.report(line, ('device_calls_agree', 'device_calls_repeat', 'checked_against_reference', 'forest_inside_rng', 'scipy_edge_sets_agree'),
              (('equals_shipped', bp.all_equal_shipped(sets)),))


if __name__ == '__main__':
    main()
