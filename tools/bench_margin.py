#!/usr/bin/env python
"""Cost of the margin bands of a slide (csrc/cellmargin.hip) beside the region census on the same input and a numpy route on the host --
prints ONE JSON line (profiles/cell_margin.json).

    python tools/bench_margin.py [--n 500000] [--extent 36000] [--blobs 200] [--vertices 2000 20000] [--shapes 50x10 250x32]
                                 [--host-edges 500000] [--host-reach 1000] [--classes 5] [--repeats 10] [--warmup 3]

The synthetic nucleus centres of tools/bench_points.py (`--n` points uniform on a square of `--extent` px, and one CLUSTERED set of the same
size) against the synthetic regions of tools/bench_regions.py (`--blobs` star-shaped blobs and one outline with holes), once per entry of
`--vertices` (vertices per blob) and per entry of `--shapes` (band step in px x number of bands).  For each:
  device_ms            nuhtc_cell_margin alone, between two events, everything resident on the device, the slab of margin.choose_slab and
                       the record cap of margin.slots_needed (one blocking call), `--repeats` after `--warmup`
  device_stage_ms      one further call under the library's per-kernel profile: the points' binning, the edges' binning (check, count,
                       scan, emit, place) and the sweep
  device_end_to_end_ms margin.build from numpy to numpy
  regions_ms           the yardstick a reader can judge the sweep by: nuhtc_cell_regions on the same resident points and edges, timed
                       the same way in the same process (its own slab and cap); margin_over_regions is the ratio of the medians
  graph_ms             the yardstick of the family: nuhtc_cell_graph (k 8, 64 px) on the same resident points
  host_ms              settings of at most --host-edges edges and --host-reach px only: numpy in float64, ring by ring on the points of the ring's bounding box
                       grown by R -- the distance to every edge of the ring (projection clamped to the segment, hypot), its minimum placed
                       among the thresholds.  A float64 route: host_band_agrees compares its per-region bands with the device's
                       band_census (sides summed) after leaving out the points whose float distance lies within 1e-6 px of a threshold
  checked_against_reference  a corner of the points small enough for brute force against margin_reference on all edges
bench.py is the project's headline benchmark and is not changed by this tool."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_points as bp  # noqa: E402
from bench_points import med, timed  # noqa: E402
from bench_regions import edge_table, synthetic_regions  # noqa: E402


def host_route(pts, lab, C, regions, thr):
    """-> (near int64 (G, B, C): per region the points of each class by band, sides summed and points within 1e-6 px of a threshold left
    out; off int64 (G,): how many were left out; ms)."""
    t0 = time.perf_counter()
    p = pts.astype(np.float64)
    e = thr.astype(np.float64)
    near, left_out = np.zeros((len(regions), len(thr), C), np.int64), np.zeros(len(regions), np.int64)
    for g, rings in enumerate(regions):
        best = np.full(len(p), np.inf)
        for v in rings:
            lo, hi = v.min(0) - e[-1], v.max(0) + e[-1]
            rows = np.flatnonzero((p >= lo).all(1) & (p <= hi).all(1))
            a = v.astype(np.float64)
            d = np.roll(a, -1, 0) - a
            L2 = np.maximum((d * d).sum(1), 1e-300)
            for i0 in range(0, len(rows), max(1, (1 << 22) // len(a))):
                r = rows[i0:i0 + max(1, (1 << 22) // len(a))]
                w = p[r, None, :] - a[None]
                t = np.clip((w * d[None]).sum(2) / L2[None], 0, 1)
                best[r] = np.minimum(best[r], np.hypot(w[..., 0] - t * d[None, :, 0], w[..., 1] - t * d[None, :, 1]).min(1))
        rows = np.flatnonzero(best <= e[-1] + 1)
        sure = np.abs(best[rows, None] - e[None]).min(1) > 2e-6                        # half pixels: 1e-6 px
        left_out[g] = int((~sure).sum())
        rows = rows[sure & (best[rows] <= e[-1])]
        np.add.at(near[g], (np.searchsorted(e, best[rows], side='left'), lab[rows]), 1)
    return near, left_out, 1e3 * (time.perf_counter() - t0)


def measure(name, pts, lab, C, regions, thr, args, gms, check_n):
    import torch
    from nuhtc_amd import margin as mg
    from nuhtc_amd import regions as rg
    edges, er = edge_table(regions)
    G, n, B = len(regions), len(pts), len(thr)
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    e_d, er_d = torch.from_numpy(edges).to(dev), torch.from_numpy(er).to(dev)
    slab = mg.choose_slab(bounds, thr)
    t0 = time.perf_counter()
    cap = mg.slots_needed(edges, bounds, slab, thr)
    cap_ms = 1e3 * (time.perf_counter() - t0)
    out = mg.outputs(n, G, C, B, dev)
    needed = []

    def shipped():
        rc, m = mg.call(p_d, l_d, C, e_d, er_d, G, thr, slab, cap, *out, bounds=bounds)
        needed.append(m)
        return rc
    ms = timed(shipped, args.repeats, args.warmup)
    got = [t.cpu().numpy() for t in out]
    stages = bp.stage_split(shipped, 'cell_margin')
    e2e, built = bp.end_to_end(lambda: mg.build(pts, lab, C, edges, er, G, thr))
    same = bool(all(np.array_equal(a, b) for a, b in zip(built, got)) and set(needed) == {cap})
    r_slab = rg.choose_slab(bounds)
    r_cap, r_out = rg.slots_needed(edges, bounds, r_slab), rg.outputs(n, G, C, dev)
    rms = timed(lambda: rg.call(p_d, l_d, C, e_d, er_d, G, r_slab, r_cap, *r_out, bounds=bounds)[0], args.repeats, args.warmup)
    census_same = bool(np.array_equal(r_out[3].cpu().numpy(), got[1]))
    win = bp.brute_window(pts, bounds, args.extent, check_n)
    ref = mg.margin_reference(pts[win], lab[win], C, edges, er, G, thr, block=max(1, (1 << 22) // len(edges)))
    exact = bool(all(np.array_equal(got[k][win], ref[k]) for k in (2, 3, 4)))
    row = dict(points=name, n=n, regions=G, edges=int(len(edges)), band_step_px=float(thr[0]) / 2, bands=B, slab_half_px=slab, records=cap,
               records_on_host_ms=round(cap_ms, 1), n_near=int((got[2] < B).sum()), near_inside=int(got[4].sum()),
               **bp.device_columns(ms, stages, e2e, same), **bp.graph_columns(gms, ms),
               regions_ms=[round(v, 3) for v in rms], regions_ms_median=round(med(rms), 3), regions_records=r_cap, regions_slab_half_px=r_slab,
               margin_over_regions=round(med(ms) / med(rms), 2), census_equals_regions=census_same,
               checked_points=int(win.sum()), checked_against_reference=exact)
    if len(edges) <= args.host_edges and thr[-1] <= 2 * args.host_reach:
        near, left_out, host_ms = host_route(pts, lab, C, regions, thr)
        dev_near = got[0].sum(1)
        row.update(host_ms=round(host_ms, 1), host_over_device_call=round(host_ms / med(ms), 1), host_over_device_end_to_end=round(host_ms / med(e2e), 1),
                   host_left_out=int(left_out.sum()), host_band_differs=int(np.abs(dev_near - near).sum()),
                   host_band_agrees=bool((np.abs(dev_near - near).sum(axis=(1, 2)) <= left_out).all()))
    return row


def main(argv=None):
    ap = bp.parser()
    ap.add_argument('--blobs', type=int, default=200)
    ap.add_argument('--vertices', type=int, nargs='+', default=[2000, 20000], help='per blob, one setting each')
    ap.add_argument('--shapes', nargs='+', default=['50x10', '250x32'], help='band step in px x number of bands, one setting each')
    ap.add_argument('--sets', nargs='+', default=['uniform', 'clustered'])
    ap.add_argument('--host-edges', type=int, default=500000, dest='host_edges', help='the host route runs on settings of at most this many edges')
    ap.add_argument('--host-reach', type=float, default=1000.0, dest='host_reach', help='.. and of at most this reach (step x bands) in px')
    args = ap.parse_args(argv)
    from nuhtc_amd import margin as mg
    bp.need_gpu('bench_margin.py')
    C = args.classes
    shapes = [mg.thresholds_from_step(float(s.split('x')[0]), int(s.split('x')[1])) for s in args.shapes]
    mg.check_args(C, args.blobs + 1, args.blobs * max(args.vertices) + 640)
    point = bp.point_sets(args.n, args.extent, C)
    sets = []
    for name in args.sets:
        p, lab = point[name]
        dev, bounds, p_d, l_d = bp.resident(p, lab)
        gms = bp.graph_yardstick(p_d, l_d, C, 128, bounds, args)
        for vertices in args.vertices:
            regions = synthetic_regions(args.extent, args.blobs, vertices)
            for thr in shapes:
                sets.append(dict(vertices_per_blob=vertices, **measure(name, p, lab, C, regions, thr, args, gms, max(args.check_n * 2000 // vertices, 1))))
                print(f'# {name} {vertices} {thr[0] / 2:g}x{len(thr)}: {sets[-1]["device_ms_median"]} ms', file=sys.stderr, flush=True)
    line = dict(what=f'tools/bench_margin.py: margin bands of {args.n} synthetic nucleus centres on a {args.extent}-px square against {args.blobs} star-shaped blobs '
                     f'of {args.vertices} vertices plus one outline with holes, bands {args.shapes} (step px x bands), {C} classes, one MI355X; device: '
                     f'{args.repeats} calls after {args.warmup} warm-up calls; yardstick: nuhtc_cell_regions on the same input in the same process; host: numpy '
                     f'float64 distance to every edge of a ring on the points of its grown bounding box',
                n=args.n, extent_px=args.extent, blobs=args.blobs, classes=C, sets=sets)
    bp.report(line, ('device_calls_agree', 'checked_against_reference', 'census_equals_regions', 'host_band_agrees'))


if __name__ == '__main__':
    main()
