#!/usr/bin/env python
"""Cost of the region census of a slide (csrc/cellregion.hip) beside matplotlib on the host -- prints ONE JSON line
(profiles/cell_regions.json).

    python tools/bench_regions.py [--n 500000] [--extent 36000] [--blobs 200] [--vertices 2000] [--classes 5] [--repeats 10] [--warmup 3]

Synthetic nucleus centres from the generator of tools/bench_points.py (`--n` points uniform on a square of `--extent` px, and one CLUSTERED
set of the same size), against synthetic regions: `--blobs` star-shaped blobs of `--vertices` vertices each scattered over the square, and
behind them one coarse outline with holes (region 0, so a blob is on top of it).  Two settings: the vertices as given, and ten times as
many.  For each setting and set:
  device_ms            nuhtc_cell_regions alone, between two events, points, edges and outputs resident on the device, the slab of
                       regions.choose_slab and the record cap of regions.slots_needed (every stage, its own scratch allocation and the final
                       synchronisation included: it is one blocking call), `--repeats` after `--warmup`
  device_stage_ms      one further call under the library's per-kernel profile: the points' binning, the edges' binning (check, count,
                       scan, emit, place) and the crossing kernel
  device_end_to_end_ms regions.build from numpy to numpy: bounding box, the records stated on the host, upload, the call, download
  graph_ms             the yardstick of the family: nuhtc_cell_graph (k 8, 64 px) on the same resident points, timed the same way
  host_ms              matplotlib.path.Path.contains_points ring by ring on the points of the ring's bounding box, float64; a region
                       holds a point when an odd number of its rings do
  host_depth_agrees    the host's and the device's `depth` are equal on every point whose on_boundary is 0
  checked_against_reference  a corner of the points small enough for brute force (--check-n of them, a tenth in the second setting)
                       against regions_reference on all edges
bench.py is the project's headline benchmark and is not changed by this tool."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_points as bp  # noqa: E402
from bench_points import med, timed  # noqa: E402


def synthetic_regions(extent, blobs, vertices, seed=1):
    """-> list of regions, each a list of rings of half-pixel vertices int64 (k, 2).  Region 0: a coarse outline of 256 vertices with 12 holes
    of 32; regions 1..: star-shaped blobs (radius about extent / 60 px, two harmonics) at random centres."""
    rng = np.random.default_rng(seed)

    def star(cx, cy, r, k, wobble):
        t = 2 * np.pi * np.arange(k) / k
        rad = r * (1 + wobble * np.sin(3 * t + rng.uniform(0, 6)) + 0.5 * wobble * np.sin(7 * t + rng.uniform(0, 6)))
        return np.rint(np.stack([cx + rad * np.cos(t), cy + rad * np.sin(t)], 1)).astype(np.int64)
    outline = [star(extent, extent, 0.96 * extent, 256, 0.03)] + [star(*rng.uniform(0.5 * extent, 1.5 * extent, 2), extent / 25, 32, 0.2) for _ in range(12)]
    return [outline] + [[star(*rng.uniform(0.1 * extent, 1.9 * extent, 2), extent / 30 * rng.uniform(0.6, 1.4), vertices, 0.25)] for _ in range(blobs)]


def edge_table(regions):
    edges = np.concatenate([np.concatenate([v, np.roll(v, -1, 0)], 1) for rings in regions for v in rings], 0)
    region = np.concatenate([np.full(len(v), g) for g, rings in enumerate(regions) for v in rings])
    return np.ascontiguousarray(edges, np.int32), np.ascontiguousarray(region, np.int32)


def host_route(pts, regions):
    """matplotlib, ring by ring on the points of the ring's bounding box -> (depth int64 (n,), ms)."""
    from matplotlib.path import Path
    t0 = time.perf_counter()
    p = pts.astype(np.float64)
    depth = np.zeros(len(p), np.int64)
    for rings in regions:
        held = np.zeros(len(p), np.int64)
        for v in rings:
            lo, hi = v.min(0), v.max(0)
            near = np.flatnonzero((pts >= lo).all(1) & (pts <= hi).all(1))
            if len(near):
                held[near] += Path(np.concatenate([v, v[:1]], 0).astype(np.float64), closed=True).contains_points(p[near])
        depth += held & 1
    return depth, 1e3 * (time.perf_counter() - t0)


def measure(name, pts, lab, C, regions, args, gms, check_n):
    import torch
    from nuhtc_amd import regions as rg
    edges, er = edge_table(regions)
    G, n = len(regions), len(pts)
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    e_d, er_d = torch.from_numpy(edges).to(dev), torch.from_numpy(er).to(dev)
    slab = rg.choose_slab(bounds)
    t0 = time.perf_counter()
    cap = rg.slots_needed(edges, bounds, slab)
    cap_ms = 1e3 * (time.perf_counter() - t0)
    out = rg.outputs(n, G, C, dev)
    needed = []

    def shipped():
        rc, m = rg.call(p_d, l_d, C, e_d, er_d, G, slab, cap, *out, bounds=bounds)
        needed.append(m)
        return rc
    ms = timed(shipped, args.repeats, args.warmup)
    got = [t.cpu().numpy() for t in out]
    stages = bp.stage_split(shipped, 'cell_regions')
    e2e, built = bp.end_to_end(lambda: rg.build(pts, lab, C, edges, er, G))
    same = bool(all(np.array_equal(a, b) for a, b in zip(built, got)) and set(needed) == {cap})
    win = bp.brute_window(pts, bounds, args.extent, check_n)
    ref = rg.regions_reference(pts[win], lab[win], C, edges, er, G, block=max(1, (1 << 24) // len(edges)))
    exact = bool(all(np.array_equal(got[k][win], ref[k]) for k in range(3)))
    depth, host_ms = host_route(pts, regions)
    off = got[2] == 0
    return dict(points=name, n=n, regions=G, edges=int(len(edges)), slab_half_px=slab, records=cap, records_on_host_ms=round(cap_ms, 1),
                n_inside=int((got[1] > 0).sum()), on_boundary=int(got[2].sum()), max_depth=int(got[1].max()),
                **bp.device_columns(ms, stages, e2e, same), **bp.graph_columns(gms, ms),
                checked_points=int(win.sum()), checked_against_reference=exact,
                host_ms=round(host_ms, 1), host_over_device_call=round(host_ms / med(ms), 1), host_over_device_end_to_end=round(host_ms / med(e2e), 1),
                host_depth_agrees=bool(np.array_equal(depth[off], got[1][off].astype(np.int64))), host_compared_points=int(off.sum()))


def main(argv=None):
    ap = bp.parser()
    ap.add_argument('--blobs', type=int, default=200)
    ap.add_argument('--vertices', type=int, default=2000, help='per blob in the first setting; the second has ten times as many')
    args = ap.parse_args(argv)
    from nuhtc_amd import regions as rg
    bp.need_gpu('bench_regions.py')
    C = args.classes
    rg.check_args(C, args.blobs + 1, args.blobs * args.vertices * 10 + 640)
    point = bp.point_sets(args.n, args.extent, C)
    sets = []
    for name, (p, lab) in point.items():
        dev, bounds, p_d, l_d = bp.resident(p, lab)
        gms = bp.graph_yardstick(p_d, l_d, C, 128, bounds, args)
        for vertices in (args.vertices, 10 * args.vertices):
            sets.append(dict(vertices_per_blob=vertices, **measure(name, p, lab, C, synthetic_regions(args.extent, args.blobs, vertices), args, gms,
                                                                       max(args.check_n * args.vertices // vertices, 1))))
    line = dict(what=f'tools/bench_regions.py: region census of {args.n} synthetic nucleus centres on a {args.extent}-px square against {args.blobs} star-shaped '
                     f'blobs of {args.vertices} and of {10 * args.vertices} vertices plus one outline with holes, {C} classes, one MI355X; device: {args.repeats} '
                     f'calls after {args.warmup} warm-up calls; host: matplotlib.path.Path.contains_points per ring on the points of its bounding box',
                n=args.n, extent_px=args.extent, blobs=args.blobs, classes=C, sets=sets)
    bp.report(line, ('device_calls_agree', 'checked_against_reference', 'host_depth_agrees'))


if __name__ == '__main__':
    main()
