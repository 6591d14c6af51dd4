#!/usr/bin/env python
"""Cost of the nucleus clusters of a slide (csrc/cellcluster.hip) beside the cell graph and scikit-learn's DBSCAN -- prints ONE JSON line
(profiles/cell_clusters.json).

    python tools/bench_clusters.py [--n 500000] [--extent 36000] [--radius 32] [--min-pts 5] [--by any] [--classes 5] [--repeats 10] [--warmup 3]

Synthetic nucleus centres from the generator of tools/bench_points.py: `--n` points uniform on a square of `--extent` px, and one CLUSTERED
set of the same size (400 Gaussian clumps, sigma 300 px).  For each set:
  device_ms            nuhtc_cell_clusters alone, between two events, points and outputs resident on the device (every stage, its own scratch
                       allocation and final synchronisation included: it is one blocking call), `--repeats` after `--warmup`
  device_stage_ms      one further call under the library's per-kernel profile: binning, degree, hook, resolve, number, tables
  device_end_to_end_ms clusters.build from numpy to numpy: bounding box, upload, the call, download (wall clock)
  graph_ms             the yardstick: nuhtc_cell_graph (k 8) on the same points at the same radius in the same run, timed the same way
  sklearn_ms           the host: sklearn.cluster.DBSCAN(eps = radius, min_samples = min_pts).fit on the same points in px (`--by any`
                       only; skipped with a note when scikit-learn is not importable), and whether its core set, noise set and core
                       partition are the device's
  checked_against_reference  a window of the points small enough for brute force, through the device again, against clusters.cluster_reference
bench.py is the project's headline benchmark and is not changed by this tool."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_points as bp  # noqa: E402
from bench_points import med  # noqa: E402


def measure(name, pts, lab, C, r, args):
    from nuhtc_amd import clusters as cl
    n, by = len(pts), cl.BY[args.by]
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    out = cl.outputs(n, C, dev)
    found = {}

    def clusters_call():
        rc, found['m'] = cl.call(p_d, l_d, C, r, args.min_pts, by, *out, bounds=bounds)
        return rc
    ms = bp.timed(clusters_call, args.repeats, args.warmup)
    gms = bp.graph_yardstick(p_d, l_d, C, r, bounds, args)
    stages = bp.stage_split(clusters_call, 'cell_clusters')
    m = found['m']
    dev_out = [t.cpu().numpy() for t in out[:3]] + [t[:m].cpu().numpy() for t in out[3:]]
    e2e, got = bp.end_to_end(lambda: cl.build(pts, lab, C, r / 2, args.min_pts, by))
    same = bool(all(np.array_equal(a, b) for a, b in zip(got, dev_out)))
    # ---- a window small enough for brute force, through the device again and against the definition
    win = bp.brute_window(pts, bounds, args.extent, args.check_n)
    sub = cl.build(pts[win], lab[win], C, r / 2, args.min_pts, by)
    exact = bool(all(np.array_equal(a, b) for a, b in zip(sub, cl.cluster_reference(pts[win], lab[win], C, r, args.min_pts, by))))
    cluster, core = dev_out[0], dev_out[1].astype(bool)
    line = dict(points=name, n=n, clusters=int(m), largest_cluster=int(dev_out[3].max()) if m else 0, core=int(core.sum()),
                border=int(((cluster >= 0) & ~core).sum()), noise=int((cluster < 0).sum()), mean_degree=round(float(dev_out[2].mean()), 2),
                **bp.device_columns(ms, stages, e2e, same), **bp.graph_columns(gms, ms),
                checked_points=int(win.sum()), checked_against_reference=exact)
    # ---- the host: scikit-learn on the same points in px
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        DBSCAN = None
    if DBSCAN is None or by:
        line.update(sklearn_ms=None, sklearn_note='scikit-learn is not importable' if DBSCAN is None else 'DBSCAN has no per-class mode')
        return line
    t0 = time.perf_counter()
    sk = DBSCAN(eps=r / 2, min_samples=args.min_pts).fit(pts.astype(np.float64) / 2)      # half-integers and their squares: exact in float64
    sk_ms = 1e3 * (time.perf_counter() - t0)
    sk_core = np.zeros(n, bool)
    sk_core[sk.core_sample_indices_] = True
    pairs = set(zip(cluster[sk_core].tolist(), sk.labels_[sk_core].tolist()))
    agrees = bool(np.array_equal(core, sk_core) and np.array_equal(cluster < 0, sk.labels_ < 0)
                  and len(pairs) == len(set(cluster[sk_core].tolist())) == len(set(sk.labels_[sk_core].tolist())))
    bm = ~sk_core & (cluster >= 0)                            # the border points: DBSCAN's to place, by its visiting order
    line.update(sklearn_ms=round(sk_ms, 1), sklearn_over_device_call=round(sk_ms / med(ms), 1), sklearn_over_device_end_to_end=round(sk_ms / med(e2e), 1),
                device_over_sklearn=round(med(ms) / sk_ms, 5), sklearn_core_noise_and_core_partition_agree=agrees,
                border_points_placed_differently=sum(1 for a, b in zip(cluster[bm].tolist(), sk.labels_[bm].tolist()) if (a, b) not in pairs) if agrees else None)
    return line


def main(argv=None):
    ap = bp.parser()
    ap.add_argument('--radius', type=float, default=32.0, help='px')
    ap.add_argument('--min-pts', type=int, default=5, dest='min_pts')
    ap.add_argument('--by', choices=('any', 'class'), default='any')
    args = ap.parse_args(argv)
    from nuhtc_amd import clusters as cl
    bp.need_gpu('bench_clusters.py')
    C, r = args.classes, cl.half_pixel_radius(args.radius)
    cl.check_args(C, r, args.min_pts, cl.BY[args.by])
    sets = [measure(name, p, lab, C, r, args) for name, (p, lab) in bp.point_sets(args.n, args.extent, C).items()]
    line = dict(what=f'tools/bench_clusters.py: DBSCAN clusters of {args.n} synthetic nucleus centres on a {args.extent}-px square, radius {args.radius:g} px, '
                     f'min_pts {args.min_pts}, by {args.by}, {C} classes, one MI355X; device: {args.repeats} calls after {args.warmup} warm-up calls; '
                     f'yardstick: nuhtc_cell_graph k 8 at the same radius; host: sklearn.cluster.DBSCAN',
                n=args.n, extent_px=args.extent, radius_px=args.radius, min_pts=args.min_pts, by=args.by, classes=C, sets=sets)
    bp.report(line, ('device_calls_agree', 'checked_against_reference', 'sklearn_core_noise_and_core_partition_agree'))


if __name__ == '__main__':
    main()
