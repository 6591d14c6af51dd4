#!/usr/bin/env python
"""Cost of the cellular neighbourhoods of a slide (csrc/cellhood.hip) beside the cell graph they are built on and scikit-learn's k-means on
the host -- prints ONE JSON line (profiles/cell_neighbourhoods.json).

    python tools/bench_neighbourhoods.py [--n 500000] [--extent 36000] [--radius 64] [--k 10] [--types 8] [--seed 0] [--iters 100]
                                         [--classes 5] [--repeats 10] [--warmup 3] [--host-threads 16]

Synthetic nucleus centres as in tools/bench_spatial.py (bench_points.point_sets): `--n` points uniform on a square of `--extent` px with
uniform labels, and one CLUSTERED set of the same size with skewed labels.  For each set:
  device_ms            nuhtc_cell_neighbourhoods alone, between two events, on the neighbour list nuhtc_cell_graph left on the device (the
                       windows, the seeding, every Lloyd iteration, the final pass, its own scratch allocation and its synchronisations
                       included: it is one blocking call), `--repeats` after `--warmup`
  device_stage_ms      one further call under the library's per-kernel profile: window, seeding, the iterations, the final pass;
                       per_iteration_ms is the iterations' time over n_iter launched in batches of 8 (so over the launched count)
  assign_gbytes_per_s  the packed 16 bytes per row the assign kernel must read, over the final pass's time (one assign kernel alone)
  graph_ms             the yardstick: nuhtc_cell_graph at the same k and radius on the same points, timed the same way
  device_end_to_end_ms neighbourhoods.build from numpy to numpy: upload, the graph, the call, download (wall clock)
  host_*               sklearn.cluster.KMeans(init=<the same seed rows' windows>, n_init=1, algorithm='lloyd', max_iter=--iters) on the same
                       windows in float64 with `--host-threads` threads: host_ms (the fit alone, wall clock), host_n_iter, and
                       host_label_agreement, the share of rows on which its labels equal the device's.  Agreement is reported, not
                       required: the host route is float and unquantised.  Without scikit-learn the columns are null.
  checked_against_reference  the timed result against neighbourhoods.cluster_reference on the device's own windows, and the windows of a
                       corner small enough for the brute-force graph against neighbourhoods_reference
bench.py is the project's headline benchmark and is not changed by this tool."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_points as bp  # noqa: E402
from bench_points import med  # noqa: E402


def host_route(window, seed_rows, hood, args):
    """-> dict of the host columns: scikit-learn's Lloyd from the same seeding rows."""
    try:
        from sklearn.cluster import KMeans
        from threadpoolctl import threadpool_limits
    except ImportError:
        return dict(host_route='none (no scikit-learn)', host_ms=None, host_n_iter=None, host_label_agreement=None)
    x = window.astype(np.float64)
    with threadpool_limits(limits=args.host_threads):
        t0 = time.perf_counter()
        km = KMeans(n_clusters=len(seed_rows), init=x[seed_rows], n_init=1, algorithm='lloyd', max_iter=args.iters).fit(x)
        ms = 1e3 * (time.perf_counter() - t0)
    return dict(host_route=f'sklearn.cluster.KMeans lloyd, float64, {args.host_threads} threads', host_ms=round(ms, 1), host_n_iter=int(km.n_iter_),
                host_label_agreement=round(float((km.labels_ == hood).mean()), 4))


def measure(name, pts, lab, C, r, args):
    import torch
    from nuhtc_amd import cellgraph
    from nuhtc_amd import neighbourhoods as nh
    n, k, K = len(pts), args.k, args.types
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    graph = [torch.full((n, w), -1, dtype=torch.int32, device=dev) for w in (k, k, C)]
    gms = bp.timed(lambda: cellgraph.call(p_d, l_d, C, r, k, *graph, bounds=bounds), args.repeats, args.warmup)
    out = nh.outputs(n, C, K, dev)
    last = []

    def full_call():
        rc, *more = nh.call(graph[0], l_d, n, k, C, K, args.seed, args.iters, False, *out)
        last[:] = more
        return rc
    ms = bp.timed(full_call, args.repeats, args.warmup)
    stages = bp.stage_split(full_call, 'cell_hood')
    n_iter, converged, inertia = last
    launched = min(-(-n_iter // 8) * 8, args.iters)
    dev_out = tuple(t.cpu().numpy() for t in out) + (inertia, n_iter, converged)
    e2e, got = bp.end_to_end(lambda: nh.build(pts, lab, C, r / 2, k, K, args.seed, args.iters))
    same = bool(all(np.array_equal(a, b) for a, b in zip(got[:6], dev_out[:6])) and got[6:] == dev_out[6:])
    exact = bool(all(np.array_equal(a, b) for a, b in zip(dev_out[1:6], nh.cluster_reference(dev_out[0], K, args.seed, args.iters)[:5]))
                 and dev_out[6:] == nh.cluster_reference(dev_out[0], K, args.seed, args.iters)[5:])
    win = bp.brute_window(pts, bounds, args.extent, args.check_n)
    sub = nh.build(pts[win], lab[win], C, r / 2, k, K, args.seed, args.iters)
    want = nh.neighbourhoods_reference(pts[win], lab[win], C, r, k, K, args.seed, args.iters)
    exact = exact and bool(all(np.array_equal(a, b) for a, b in zip(sub[:6], want[:6])) and sub[6:] == want[6:])
    final_ms = stages.get('cell_hood_final', 0.0)
    return dict(points=name, n=n, n_iter=n_iter, converged=converged, iterations_launched=launched, inertia_per_nucleus=round(inertia / 1024 ** 2 / n, 4),
                hood_size=dev_out[4].tolist(), **bp.device_columns(ms, stages, e2e, same),
                per_iteration_ms=round(stages.get('cell_hood_iterate', 0.0) / max(launched, 1), 4),
                assign_gbytes_per_s=round(16.0 * n / (final_ms * 1e6), 1) if final_ms else None,
                **bp.graph_columns(gms, ms), **host_route(dev_out[0], dev_out[5], dev_out[1], args),
                checked_points=int(win.sum()), checked_against_reference=exact)


def main(argv=None):
    ap = bp.parser()
    ap.add_argument('--radius', type=float, default=64.0, help='radius of the window, px (the default of the slide tool)')
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--types', type=int, default=8)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--host-threads', type=int, default=16, dest='host_threads')
    args = ap.parse_args(argv)
    from nuhtc_amd import cellpoints
    from nuhtc_amd import neighbourhoods as nh
    C, r = args.classes, cellpoints.half_pixel_radius(args.radius)
    nh.check_args(C, r, args.k, args.types, args.seed, args.iters)
    bp.need_gpu('bench_neighbourhoods.py')
    sets = [measure(name, p, lab, C, r, args) for name, (p, lab) in bp.point_sets(args.n, args.extent, C).items()]
    line = dict(what=f'tools/bench_neighbourhoods.py: cellular neighbourhoods of {args.n} synthetic nucleus centres on a {args.extent}-px square, windows of k '
                     f'{args.k} within {args.radius:g} px, {args.types} types (seed {args.seed}, at most {args.iters} iterations), {C} classes, one MI355X; '
                     f'device: {args.repeats} calls after {args.warmup} warm-up calls; yardstick: nuhtc_cell_graph at the same k and radius; host: '
                     f'scikit-learn KMeans (lloyd) from the same seeding rows on the same windows, {args.host_threads} threads',
                n=args.n, extent_px=args.extent, radius_px=args.radius, k=args.k, types=args.types, seed=args.seed, max_iter=args.iters, classes=C, sets=sets)
    bp.report(line, ('device_calls_agree', 'checked_against_reference'))


if __name__ == '__main__':
    main()
