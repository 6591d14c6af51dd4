#!/usr/bin/env python
"""Cost of the proximity graphs of a slide's nuclei (csrc/cellprox.hip) beside the cell graph, the spanning forest and scipy -- prints ONE
JSON line (profiles/cell_proximity.json).

    python tools/bench_proximity.py [--n 500000] [--extent 36000] [--radius 64] [--by any] [--classes 5] [--repeats 10] [--warmup 3]
                                    [--also LABEL=path/to/libnuhtc_hip.so ...] [--rounds 2]

Synthetic nucleus centres from the generator of tools/bench_spatial.py: `--n` points uniform on a square of `--extent` px, and one CLUSTERED
set of the same size (400 Gaussian clumps, sigma 300 px).  For each set:
  device_ms            nuhtc_cell_proximity alone, between two events, points and outputs resident on the device and room for 4 n + 64 edges
                       (every stage, its own scratch allocation, the counts read back and the final synchronisation included: it is one
                       blocking call), `--repeats` after `--warmup`
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
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


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
    import torch
    from nuhtc_amd import cellgraph as cg
    from nuhtc_amd import cellpoints, hip, mst
    from nuhtc_amd import proximity as px
    n, by = len(pts), px.BY[args.by]
    dev = torch.device('cuda', 0)
    bounds = cellpoints.bounds_of(pts)
    p_d, l_d = torch.from_numpy(pts).to(dev), torch.from_numpy(lab).to(dev)
    cap = px.first_edge_cap(n)
    out = px.outputs(n, cap, dev)
    gout = [torch.full((n, w), -1, dtype=torch.int32, device=dev) for w in (8, 8, C)]
    mout = mst.outputs(n, dev)
    found = {}

    def prox_call():
        rc, found['m'], found['m_rng'] = px.call(p_d, l_d, C, r, by, cap, *out, bounds=bounds)
        return rc

    def timed(fn, repeats=args.repeats, warmup=args.warmup):
        ms = []
        for i in range(warmup + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn()
            e1.record()
            torch.cuda.synchronize()
            if rc:
                raise SystemExit(f'the device call failed ({rc})')
            if i >= warmup:
                ms.append(e0.elapsed_time(e1))
        return ms
    ms = timed(prox_call)
    m = found['m']
    if m > cap:
        raise SystemExit(f'{m} edges, more than the {cap} the benchmark has room for')
    dev_out = [out[0][:m].cpu().numpy(), out[1][:m].cpu().numpy(), out[2][:m].cpu().numpy(), out[3].cpu().numpy()]
    gms = timed(lambda: cg.call(p_d, l_d, C, r, 8, *gout, bounds=bounds))
    mfound = {}

    def mst_call():
        rc, mfound['m'], _, _ = mst.call(p_d, l_d, C, r, by, *mout, bounds=bounds)
        return rc
    mms = timed(mst_call)
    forest = mout[0][:mfound['m']].cpu().numpy().astype(np.int64)
    code = lambda e: e[:, 0].astype(np.int64) * n + e[:, 1]
    inside = bool(np.isin(code(forest), code(dev_out[0][dev_out[2] == 1])).all())
    hip.profile_enable(True)                                  # one more call for the split between the stages (events around each)
    prox_call()
    stages = {tag: round(v['ms'], 3) for tag, v in hip.profile_read().items() if tag.startswith('cell_prox')}
    hip.profile_enable(False)
    med = lambda v: float(np.median(v))
    # ---- other builds of the library, alternating with the shipped one in this process
    variants = {}
    if also:
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        calls = {'shipped': prox_call}
        for label, fn in also.items():
            vout = px.outputs(n, cap, dev)
            vm, vr = ctypes.c_int64(-1), ctypes.c_int64(-1)
            call = (lambda fn=fn, vout=vout, vm=vm, vr=vr: fn(0, vp(p_d), vp(l_d), n, C, r, by, cap, *bounds, *(vp(t) for t in vout),
                                                              ctypes.byref(vm), ctypes.byref(vr), stream))
            if call():
                raise SystemExit(f'{label}: the device call failed')
            same = bool(vm.value == m and vr.value == found['m_rng'] and all(np.array_equal(a[:m].cpu().numpy() if a.shape[0] == cap else a.cpu().numpy(), b)
                                                                          for a, b in zip(vout, dev_out)))
            variants[label] = dict(equals_shipped=same, ms=[])
            calls[label] = call
        variants['shipped'] = dict(ms=[])
        for _ in range(args.rounds):
            for label, call in calls.items():
                variants[label]['ms'].append(round(med(timed(call, warmup=1)), 3))
    e2e = []
    for i in range(3):
        t0 = time.perf_counter()
        got = px.build(pts, lab, C, r / 2, by)
        e2e.append(1e3 * (time.perf_counter() - t0))
    same = bool(all(np.array_equal(a, b) for a, b in zip(got[:4], dev_out)) and got[4:] == (m, found['m_rng']))
    # ---- a window small enough for brute force, through the device again and against the definition
    lo = np.array([bounds[0], bounds[1]])
    side = int(2 * args.extent * np.sqrt(min(1.0, args.check_n / max(n, 1))))
    win = ((pts - lo) < side).all(1)
    if win.sum() > 2 * args.check_n:                          # a dense corner of the clustered set
        win &= np.cumsum(win) <= 2 * args.check_n
    sub, ref = px.build(pts[win], lab[win], C, r / 2, by), px.proximity_reference(pts[win], lab[win], C, r, by)
    exact = bool(all(np.array_equal(a, b) for a, b in zip(sub[:4], ref[:4])) and sub[4:] == ref[4:])
    line = dict(points=name, n=n, m=int(m), m_rng=int(found['m_rng']), mean_gabriel_degree=round(2 * m / n, 3), mean_rng_degree=round(2 * found['m_rng'] / n, 3),
                mean_edge_px=round(float(np.sqrt(dev_out[1].astype(np.float64)).mean() / 2), 3) if m else 0.0,
                device_ms=[round(v, 3) for v in ms], device_ms_median=round(med(ms), 3), device_stage_ms=stages,
                device_end_to_end_ms=[round(v, 2) for v in e2e], device_end_to_end_ms_median=round(med(e2e), 2), device_calls_agree=same,
                graph_ms=[round(v, 3) for v in gms], graph_ms_median=round(med(gms), 3), device_over_graph=round(med(ms) / med(gms), 2),
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
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=500000)
    ap.add_argument('--extent', type=int, default=36000, help='side of the square the centres are drawn on, px')
    ap.add_argument('--radius', type=float, default=64.0, help='px')
    ap.add_argument('--by', choices=('any', 'class'), default='any')
    ap.add_argument('--classes', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--check-n', type=int, default=3000, dest='check_n', help='about how many points the brute-force check takes')
    ap.add_argument('--also', action='append', default=[], metavar='LABEL=LIB', help='another build of the library to time in alternating rounds')
    ap.add_argument('--rounds', type=int, default=2, help='alternating rounds of the shipped library and the --also builds')
    args = ap.parse_args(argv)
    import torch
    from bench_spatial import point_sets
    from nuhtc_amd import hip
    from nuhtc_amd import proximity as px
    if not torch.cuda.is_available():
        raise SystemExit('bench_proximity.py needs a GPU (there is no fallback)')
    C, r = args.classes, px.half_pixel_radius(args.radius)
    px.check_args(C, r, px.BY[args.by])
    shipped = hip.load().nuhtc_cell_proximity
    also = {}
    for spec in args.also:
        label, path = spec.split('=', 1)
        fn = ctypes.CDLL(os.path.abspath(path)).nuhtc_cell_proximity
        fn.argtypes, fn.restype = shipped.argtypes, shipped.restype
        also[label] = fn
    sets = [measure(name, p, lab, C, r, args, also) for name, (p, lab) in point_sets(args.n, args.extent, C).items()]
    line = dict(what=f'tools/bench_proximity.py: Gabriel graph and relative neighbourhood graph of {args.n} synthetic nucleus centres on a {args.extent}-px square, '
                     f'radius {args.radius:g} px, by {args.by}, {C} classes, one MI355X; device: {args.repeats} calls after {args.warmup} warm-up calls; '
                     f'yardsticks: nuhtc_cell_graph k 8 and nuhtc_cell_mst at the same radius; host: scipy cKDTree.query_pairs + the two tests in numpy; '
                     f'variants: median ms of {args.repeats} calls per round, {args.rounds} alternating rounds',
                n=args.n, extent_px=args.extent, radius_px=args.radius, by=args.by, classes=C, sets=sets)
    print(json.dumps(line))
    ok = all(s['device_calls_agree'] and s['checked_against_reference'] and s['forest_inside_rng'] and s.get('scipy_edge_sets_agree', True)
             and all(v.get('equals_shipped', True) for v in s['variants'].values()) for s in sets)
    if not ok:
        raise SystemExit('a check failed: see device_calls_agree / checked_against_reference / forest_inside_rng / scipy_edge_sets_agree / equals_shipped')


if __name__ == '__main__':
    main()
