#!/usr/bin/env python
"""Cost of the spatial statistics of a slide (csrc/cellspatial.hip) beside the cell graph and a host KD-tree -- prints ONE JSON line
(profiles/cell_spatial.json).

    python tools/bench_spatial.py [--n 500000] [--extent 36000] [--step 8] [--bins 32] [--classes 5] [--repeats 10] [--warmup 3] [--workers 16]

Synthetic nucleus centres as in tools/bench_cellgraph.py: `--n` points uniform on a square of `--extent` px (the defaults: one nucleus per
2592 px^2, about 79 neighbours within 256 px), on the half-pixel lattice, labels uniform in 0..classes-1 -- and one CLUSTERED set of the
same size: 400 Gaussian clumps (sigma 300 px) on the same square, the labels skewed 60 / 25 / 10 / 4 / 1 %.  For each set:
  device_ms            nuhtc_cell_spatial alone, between two events, points and outputs resident on the device (binning, zeroing, search,
                       its own scratch allocation and final synchronisation included: it is one blocking call), `--repeats` after `--warmup`
  device_stage_ms      one further call under the library's per-kernel profile: the binning launches and the search launch
  device_end_to_end_ms spatial.build from numpy to numpy: bounding box, upload, the call, download (wall clock)
  graph_ms             the yardstick: nuhtc_cell_graph (k 8) on the same points at radius e_B in the same run, timed the same way
  host_count_ms        the host route: scipy.spatial.cKDTree.count_neighbors per ordered class pair (the cumulative counts at all edges) on
                       `--workers` threads, tree builds included; it yields pair_hist only, not nn_d2
  checked_against_reference  the timed result against spatial.spatial_reference on a window of the points small enough for brute force
                       (the points of a corner square, run through the device again), and the device's cumulative counts against the trees'
bench.py is the project's headline benchmark and is not changed by this tool."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_points as bp  # noqa: E402
from bench_points import med  # noqa: E402


def measure(name, pts, lab, C, edges, args):
    import torch
    from scipy.spatial import cKDTree
    from nuhtc_amd import spatial as sp
    n, B = len(pts), len(edges)
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    out = [torch.zeros((C, C, B), dtype=torch.int64, device=dev), torch.full((n, C), -1, dtype=torch.int32, device=dev),
           torch.zeros((C,), dtype=torch.int64, device=dev)]
    spatial_call = lambda: sp.call(p_d, l_d, C, edges, *out, bounds=bounds)
    ms = bp.timed(spatial_call, args.repeats, args.warmup)
    gms = bp.graph_yardstick(p_d, l_d, C, int(edges[-1]), bounds, args)
    stages = bp.stage_split(spatial_call, 'cell_spatial')
    ph_dev = out[0].cpu().numpy()
    e2e, got = bp.end_to_end(lambda: sp.build(pts, lab, C, edges))
    same = bool(np.array_equal(got[0], ph_dev) and np.array_equal(got[1], out[1].cpu().numpy()) and np.array_equal(got[2], out[2].cpu().numpy()))
    # ---- a window small enough for brute force, through the device again and against the definition
    win = bp.brute_window(pts, bounds, args.extent, args.check_n)
    sub = sp.build(pts[win], lab[win], C, edges)
    ref = sp.spatial_reference(pts[win], lab[win], C, edges)
    exact = bool(all(np.array_equal(a, b) for a, b in zip(sub, ref)))
    # ---- the host route: cumulative counts per ordered class pair (px, float64; radii a hair above the edge keep the inclusive compare)
    xy = pts.astype(np.float64) / 2
    radii = edges.astype(np.float64) / 2 * (1 + 1e-12)
    t0 = time.perf_counter()
    trees = [cKDTree(xy[lab == c]) for c in range(C)]
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max(1, args.workers)) as pool:
        cum = list(pool.map(lambda ab: trees[ab[0]].count_neighbors(trees[ab[1]], radii), [(a, b) for a in range(C) for b in range(C)]))
    t_count = time.perf_counter() - t0
    cum = np.array(cum, np.int64).reshape(C, C, B) - np.eye(C, dtype=np.int64)[:, :, None] * got[2][:, None, None]
    host_agrees = bool(np.array_equal(np.cumsum(ph_dev, 2), cum))
    return dict(points=name, n=n, ordered_pairs_within_reach=int(ph_dev.sum()), mean_neighbours_within_reach=round(float(ph_dev.sum()) / max(int(got[2].sum()), 1), 2),
                class_n=got[2].tolist(), **bp.device_columns(ms, stages, e2e, same), **bp.graph_columns(gms),
                host_tree_build_ms=round(1e3 * t_build, 1), host_count_ms=round(1e3 * t_count, 1), host_workers=args.workers,
                host_total_over_device_call=round(1e3 * (t_build + t_count) / med(ms), 2),
                host_total_over_device_end_to_end=round(1e3 * (t_build + t_count) / med(e2e), 2),
                host_cumulative_counts_agree=host_agrees, checked_points=int(win.sum()), checked_against_reference=exact)


def main(argv=None):
    ap = bp.parser()
    ap.add_argument('--step', type=float, default=8.0)
    ap.add_argument('--bins', type=int, default=32)
    ap.add_argument('--workers', type=int, default=16)
    args = ap.parse_args(argv)
    from nuhtc_amd import spatial as sp
    bp.need_gpu('bench_spatial.py')
    C = args.classes
    edges = sp.edges_from_step(args.step, args.bins)
    sets = [measure(name, p, lab, C, edges, args) for name, (p, lab) in bp.point_sets(args.n, args.extent, C).items()]
    line = dict(what=f'tools/bench_spatial.py: pair histograms of {args.n} synthetic nucleus centres on a {args.extent}-px square, {args.bins} bins of '
                     f'{args.step:g} px (reach {edges[-1] / 2:g} px), {C} classes, one MI355X; device: {args.repeats} calls after {args.warmup} warm-up calls; '
                     f'yardstick: nuhtc_cell_graph k 8 at the same reach; host: scipy cKDTree.count_neighbors per ordered class pair',
                n=args.n, extent_px=args.extent, step_px=args.step, bins=args.bins, reach_px=float(edges[-1]) / 2, classes=C, sets=sets)
    bp.report(line, ('device_calls_agree', 'checked_against_reference', 'host_cumulative_counts_agree'))


if __name__ == '__main__':
    main()
