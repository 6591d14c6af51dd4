#!/usr/bin/env python
"""Cost of the minimum spanning forest of a slide's nuclei (csrc/cellmst.hip) beside the cell graph and scipy -- prints ONE JSON line
(profiles/cell_mst.json).

    python tools/bench_mst.py [--n 500000] [--extent 36000] [--radius 64] [--by any] [--classes 5] [--repeats 10] [--warmup 3]
                              [--also LABEL=path/to/libnuhtc_hip.so ...] [--rounds 2]

Synthetic nucleus centres from the generator of tools/bench_points.py: `--n` points uniform on a square of `--extent` px, and one CLUSTERED
set of the same size (400 Gaussian clumps, sigma 300 px).  For each set:
  device_ms            nuhtc_cell_mst alone, between two events, points and outputs resident on the device (every stage, its own scratch
                       allocation, the one int read back per round and the final synchronisation included: it is one blocking call),
                       `--repeats` after `--warmup`
  rounds, m, T         the Boruvka rounds that added an edge, the edges and the trees
  device_stage_ms      one further call under the library's per-kernel profile: the cell_mst_* stages, summed over the rounds
  device_end_to_end_ms mst.build from numpy to numpy: bounding box, upload, the call, download (wall clock)
  graph_ms             the yardstick: nuhtc_cell_graph (k 8) on the same points at the same radius in the same run, timed the same way
  variants             with --also: other builds of the library timed in `--rounds` alternating rounds with the shipped one, all in this
                       process; each must return the shipped arrays
  scipy_ms             the host: cKDTree.sparse_distance_matrix within the radius, then csgraph.minimum_spanning_tree over the integer
                       weights d2 + 1 (scipy reads a weight of 0 as no edge).  Only m and the total of d2 are compared with the device's:
                       under ties scipy's forest may be another one of the same weight.  Skipped with a note when scipy is not importable.
  checked_against_reference  a window of the points small enough for brute force, through the device again, against mst.mst_reference
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


def measure(name, pts, lab, C, r, args, also):
    from nuhtc_amd import mst
    n, by = len(pts), mst.BY[args.by]
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    out = mst.outputs(n, dev)
    found = {}

    def mst_call():
        rc, found['m'], found['T'], found['rounds'] = mst.call(p_d, l_d, C, r, by, *out, bounds=bounds)
        return rc
    ms = bp.timed(mst_call, args.repeats, args.warmup)
    gms = bp.graph_yardstick(p_d, l_d, C, r, bounds, args)
    stages = bp.stage_split(mst_call, 'cell_mst')
    m = found['m']
    vp, stream = bp.raw(dev)
    held = {label: (mst.outputs(n, dev), [ctypes.c_int64(-1) for _ in range(3)]) for label in also}
    others = {label: (lambda fn=fn, vout=held[label][0], v=held[label][1]: fn(0, vp(p_d), vp(l_d), n, C, r, by, *bounds, *(vp(t) for t in vout),
                                                                             *(ctypes.byref(c) for c in v), stream)) for label, fn in also.items()}
    shipped_result = (found['m'], found['T'], found['rounds'])
    equals = lambda label: tuple(c.value for c in held[label][1]) == shipped_result and bp.tensors_equal(held[label][0], out)
    variants = bp.variants(mst_call, others, equals, args)
    dev_out = [out[0][:m].cpu().numpy(), out[1][:m].cpu().numpy(), out[2].cpu().numpy()]
    e2e, got = bp.end_to_end(lambda: mst.build(pts, lab, C, r / 2, by))
    same = bool(all(np.array_equal(a, b) for a, b in zip(got[:3], dev_out)) and got[3:] == (m, found['T']))
    # ---- a window small enough for brute force, through the device again and against the definition
    win = bp.brute_window(pts, bounds, args.extent, args.check_n)
    sub, ref = mst.build(pts[win], lab[win], C, r / 2, by), mst.mst_reference(pts[win], lab[win], C, r, by)
    exact = bool(all(np.array_equal(a, b) for a, b in zip(sub[:3], ref[:3])) and sub[3:] == ref[3:])
    total_d2 = int(dev_out[1].astype(np.int64).sum())
    line = dict(points=name, n=n, m=int(m), T=int(found['T']), rounds=int(found['rounds']), total_d2=total_d2,
                largest_tree=int(np.bincount(dev_out[2]).max()), mean_edge_px=round(float(np.sqrt(dev_out[1].astype(np.float64)).mean() / 2), 3) if m else 0.0,
                **bp.device_columns(ms, stages, e2e, same), **bp.graph_columns(gms, ms), variants=variants,
                checked_points=int(win.sum()), checked_against_reference=exact)
    # ---- the host: scipy on the same points
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import minimum_spanning_tree
        from scipy.spatial import cKDTree
    except ImportError:
        line.update(scipy_ms=None, scipy_note='scipy is not importable')
        return line
    t0 = time.perf_counter()
    kd = cKDTree(pts.astype(np.float64))                      # half pixels as float64: integers, their squares exact
    near = kd.sparse_distance_matrix(kd, r + 0.5, output_type='coo_matrix')
    t1 = time.perf_counter()
    i, j = near.row.astype(np.int64), near.col.astype(np.int64)
    d2 = ((pts[i].astype(np.int64) - pts[j].astype(np.int64)) ** 2).sum(1)
    keep = (i < j) & (d2 <= r * r)
    if by:
        keep &= lab[i] == lab[j]
    forest = minimum_spanning_tree(coo_matrix((d2[keep] + 1, (i[keep], j[keep])), shape=(n, n)).tocsr())
    t2 = time.perf_counter()
    sk_ms, sk_m = 1e3 * (t2 - t0), int(forest.nnz)
    sk_total = int(round(float(forest.sum()))) - sk_m
    line.update(scipy_ms=round(sk_ms, 1), scipy_pairs_ms=round(1e3 * (t1 - t0), 1), scipy_forest_ms=round(1e3 * (t2 - t1), 1), scipy_edges_within_radius=int(keep.sum()),
                scipy_over_device_call=round(sk_ms / med(ms), 1), scipy_over_device_end_to_end=round(sk_ms / med(e2e), 1),
                scipy_m_and_total_d2_agree=bool(sk_m == m and sk_total == total_d2))
    return line


def main(argv=None):
    ap = bp.parser()
    ap.add_argument('--radius', type=float, default=64.0, help='px')
    ap.add_argument('--by', choices=('any', 'class'), default='any')
    bp.also_arguments(ap)
    args = ap.parse_args(argv)
    from nuhtc_amd import mst
    bp.need_gpu('bench_mst.py')
    C, r = args.classes, mst.half_pixel_radius(args.radius)
    mst.check_args(C, r, mst.BY[args.by])
    also = bp.also_builds(args.also, 'nuhtc_cell_mst')
    sets = [measure(name, p, lab, C, r, args, also) for name, (p, lab) in bp.point_sets(args.n, args.extent, C).items()]
    line = dict(what=f'tools/bench_mst.py: minimum spanning forest of {args.n} synthetic nucleus centres on a {args.extent}-px square, radius {args.radius:g} px, '
                     f'by {args.by}, {C} classes, one MI355X; device: {args.repeats} calls after {args.warmup} warm-up calls; '
                     f'yardstick: nuhtc_cell_graph k 8 at the same radius; host: scipy cKDTree.sparse_distance_matrix + csgraph.minimum_spanning_tree',
                n=args.n, extent_px=args.extent, radius_px=args.radius, by=args.by, classes=C, sets=sets)
    bp.report(line, ('device_calls_agree', 'checked_against_reference', 'scipy_m_and_total_d2_agree'), (('equals_shipped', bp.all_equal_shipped(sets)),))


if __name__ == '__main__':
    main()
