#!/usr/bin/env python
"""Cost of the cell graph of a slide (csrc/cellgraph.hip) beside a host KD-tree -- prints ONE JSON line (profiles/cell_graph.json).

    python tools/bench_cellgraph.py [--n 500000] [--extent 36000] [--radius 64] [--k 8] [--classes 5] [--repeats 10] [--warmup 3] [--workers 16]

A synthetic slide's worth of nucleus centres: `--n` points uniform on a square of `--extent` px (the defaults: one nucleus per 2592 px^2, a
mean spacing of 51 px = 12.7 um at 40x, about 5 neighbours within 64 px), on the half-pixel lattice, labels uniform in 0..classes-1.
  device_ms            nuhtc_cell_graph alone, between two events, points and outputs resident on the device (binning + search, its own
                       scratch allocation and final synchronisation included: it is one blocking call), `--repeats` calls after `--warmup`
  device_stage_ms      one further call under the library's per-kernel profile: the binning launches and the search launch
  device_end_to_end_ms cellgraph.build from numpy to numpy: bounding box, upload, the call, download (wall clock)
  host_*               scipy.spatial.cKDTree on the same points: the build, then query(k + 1, distance_upper_bound = radius) with one worker
                       and with `--workers`
The two routes are not compared for equality here (a float KD-tree breaks distance ties its own way; tests/test_hip_cellgraph.py holds the
device to the integer definition); the edge counts of both are in the line.
bench.py is the project's headline benchmark and is not changed by this tool."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_points as bp  # noqa: E402
from bench_points import med  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=500000)
    ap.add_argument('--extent', type=int, default=36000, help='side of the square the centres are drawn on, px')
    ap.add_argument('--radius', type=float, default=64.0)
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--classes', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--workers', type=int, default=16)
    args = ap.parse_args(argv)
    import torch
    from scipy.spatial import cKDTree
    from nuhtc_amd import cellgraph as cg
    bp.need_gpu('bench_cellgraph.py')
    n, k, C = args.n, args.k, args.classes
    r = cg.half_pixel_radius(args.radius)
    rng = np.random.default_rng(0)
    pts = rng.integers(0, 2 * args.extent, (n, 2)).astype(np.int32)
    lab = rng.integers(0, C, n).astype(np.int32)
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    out = [torch.full((n, w), -1, dtype=torch.int32, device=dev) for w in (k, k, C)]
    graph_call = lambda: cg.call(p_d, l_d, C, r, k, *out, bounds=bounds)
    ms = bp.timed(graph_call, args.repeats, args.warmup)
    stages = bp.stage_split(graph_call, 'cell_graph')
    nb_dev = out[0].cpu().numpy()
    e2e, got = bp.end_to_end(lambda: cg.build(pts, lab, C, args.radius, k))
    same = bool(np.array_equal(got[0], nb_dev))
    # ---- the host route on the same points (px, float64)
    xy = pts.astype(np.float64) / 2
    t0 = time.perf_counter()
    tree = cKDTree(xy)
    t_build = time.perf_counter() - t0
    host = {}
    for w in sorted({1, max(1, args.workers)}):
        t0 = time.perf_counter()
        dist, idx = tree.query(xy, k=k + 1, distance_upper_bound=args.radius * (1 + 1e-12), workers=w)
        host[w] = time.perf_counter() - t0
    edges_host = int(np.isfinite(dist[:, 1:]).sum())
    w_hi = max(host)
    out_line = dict(what=f'tools/bench_cellgraph.py: cell graph of {n} synthetic nucleus centres uniform on a {args.extent}-px square '
                         f'(one per {args.extent ** 2 / n:.0f} px^2), radius {args.radius:g} px, k {k}, {C} classes, one MI355X; device: '
                         f'{args.repeats} calls after {args.warmup} warm-up calls; host: scipy cKDTree build + query(k + 1, distance_upper_bound)',
                    n=n, extent_px=args.extent, px2_per_nucleus=round(args.extent ** 2 / n, 1), radius_px=args.radius, k=k, classes=C,
                    mean_neighbours_within_radius=round(float(out[2].sum().item()) / n, 3), edges_device=int((nb_dev >= 0).sum()), edges_host=edges_host,
                    **bp.device_columns(ms, stages, e2e, same),
                    host_tree_build_ms=round(1e3 * t_build, 1), host_query_ms_1_worker=round(1e3 * host[1], 1),
                    **{f'host_query_ms_{w_hi}_workers': round(1e3 * host[w_hi], 1)},
                    host_total_ms_1_worker=round(1e3 * (t_build + host[1]), 1), host_total_ms_best=round(1e3 * (t_build + min(host.values())), 1),
                    host_best_over_device_end_to_end=round(1e3 * (t_build + min(host.values())) / med(e2e), 2),
                    host_best_over_device_call=round(1e3 * (t_build + min(host.values())) / med(ms), 2))
    print(json.dumps(out_line))
    if not same:
        raise SystemExit('two device builds of the same points differ')


if __name__ == '__main__':
    main()
