#!/usr/bin/env python
"""Cost of the alpha complex of a slide's nuclei (csrc/cellalpha.hip) beside the proximity graphs, the cell graph and scipy's Delaunay --
prints ONE JSON line (profiles/cell_alpha.json).

    python tools/bench_alpha.py [--n 500000] [--extent 36000] [--radii 32 64] [--by any] [--classes 5] [--repeats 10] [--warmup 3]
                                [--also LABEL=path/to/libnuhtc_hip.so ...] [--rounds 2]

Synthetic nucleus centres from the generator of tools/bench_points.py: `--n` points uniform on a square of `--extent` px, and one CLUSTERED
set of the same size (400 Gaussian clumps, sigma 300 px).  For each set and each radius r of `--radii` (px):
  device_ms            nuhtc_cell_alpha alone, between two events, points and outputs resident on the device and room for 4 n + 64 edges
                       or, when there are more, for exactly that many (every stage, its own scratch allocation, the counts read back and
                       the final synchronisation included: it is one blocking call), `--repeats` after `--warmup`; the calls around the
                       timed ones are compared bitwise with the first (device_calls_repeat)
  m, m_gabriel         the edges and how many of them are Gabriel edges; interior / outline / singular: the edges by their apexes
  device_stage_ms      one further call under the library's per-kernel profile: the cell_alpha_* stages
  device_end_to_end_ms alphacomplex.build from numpy to numpy: bounding box, upload, the call(s), download (wall clock)
  proximity_ms, graph_ms  the yardsticks: nuhtc_cell_proximity and nuhtc_cell_graph (k 8) on the same points at radius 2 r in the same process,
                       timed the same way; gabriel_equals_proximity says that the Gabriel-flagged edges ARE the proximity call's edges
  variants             with --also: other builds of the library (the routes of the witness loop, see csrc/cellalpha.hip's -DNUHTC_ALPHA_*
                       switches) timed in `--rounds` alternating rounds with the shipped one, all in this process; each must return the
                       shipped arrays
  scipy_ms             the host: scipy.spatial.Delaunay on the DISTINCT points of the set (once per set; the rows are mapped to their sites,
                       and the device's edges of length > 0 likewise: rows on one site never bind each other) plus the circumradius filter
                       and the Gabriel edges the triangles miss (taken from the device).  Where the device reports no degenerate edge (no
                       four cocircular points in reach) the edge counts must be equal (scipy_edge_counts_agree); otherwise the difference
                       is stated.  On every set the difference must be EXPLAINED (scipy_difference_explained): scipy has no edge the
                       device lacks, and every edge only the device has is a diagonal of cocircular sites (two apexes, lo == hi).
                       Skipped with a note without scipy.
  checked_against_reference  a window of the points small enough for brute force, through the device again, against alpha_reference
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


def scipy_triangulation(pts):
    """-> ((sites int (k, 2), site_of int64 (n,), simplices int64 (t, 3) over the sites), ms): scipy's Delaunay triangulation of the DISTINCT
    half-pixel points as float64 (qhull triangulates one of several coincident points and drops the others), and the site of every row."""
    from scipy.spatial import Delaunay
    t0 = time.perf_counter()
    sites, site_of = np.unique(pts, axis=0, return_inverse=True)
    tri = Delaunay(sites.astype(np.float64)).simplices.astype(np.int64)
    return (sites, site_of.reshape(-1).astype(np.int64), tri), 1e3 * (time.perf_counter() - t0)


def scipy_filter(pts, tri, r):
    """-> (edges int64 (m, 2) ascending and distinct: the sides of the simplices with circumradius <= r half pixels, in float64; ms)."""
    t0 = time.perf_counter()
    p = pts.astype(np.float64)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    cross = np.abs((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]))
    l2 = lambda u, v: ((u - v) ** 2).sum(1)
    lhs, rhs = l2(a, b) * l2(b, c) * l2(a, c), 4.0 * r * r * cross * cross
    keep = lhs <= rhs
    for k in np.flatnonzero(np.abs(lhs - rhs) <= 1e-9 * rhs):                # a circumradius at r to rounding: decided in Python integers
        (ax_, ay), (bx, by), (cx, cy) = ([int(v) for v in pts[row]] for row in tri[k])
        cr = (bx - ax_) * (cy - ay) - (by - ay) * (cx - ax_)
        sq = lambda ux, uy, vx, vy: (ux - vx) ** 2 + (uy - vy) ** 2
        keep[k] = sq(ax_, ay, bx, by) * sq(bx, by, cx, cy) * sq(ax_, ay, cx, cy) <= 4 * r * r * cr * cr
    t = tri[keep]
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [0, 2]]]), 1)
    e = np.unique(e, axis=0)
    return e, 1e3 * (time.perf_counter() - t0)


def measure(name, pts, lab, C, radius_px, args, also, tri):
    from nuhtc_amd import alphacomplex as ax
    from nuhtc_amd import proximity as px
    n, by, r = len(pts), ax.BY[args.by], ax.half_pixel_radius(radius_px)
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    cap, out, (_, m, m_gab) = bp.grown(lambda cap, out: ax.call(p_d, l_d, C, r, by, cap, *out, bounds=bounds), lambda cap: ax.outputs(n, cap, dev),
                                       ax.first_edge_cap(n))
    pout = px.outputs(n, cap, dev)
    found, pfound = dict(m=m, m_gab=m_gab), {}

    def alpha_call():
        rc, found['m'], found['m_gab'] = ax.call(p_d, l_d, C, r, by, cap, *out, bounds=bounds)
        return rc

    def prox_call():
        rc, pfound['m'], _ = px.call(p_d, l_d, C, 2 * r, by, cap, *pout, bounds=bounds)
        return rc

    timed = lambda fn, warmup=args.warmup: bp.timed(fn, args.repeats, warmup)
    first, checked, repeated = bp.repeating(alpha_call, out, lambda: (found['m'], found['m_gab']))
    checked()
    ms = timed(alpha_call)
    checked()
    dev_out = [t[:m].cpu().numpy() for t in first[:4]] + [first[4].cpu().numpy()]
    pms = timed(prox_call)
    gabriel = dev_out[3] == 1
    same_gabriel = bool(pfound['m'] == m_gab and np.array_equal(dev_out[0][gabriel], pout[0][:pfound['m']].cpu().numpy()))
    gms = bp.graph_yardstick(p_d, l_d, C, 2 * r, bounds, args)
    stages = bp.stage_split(alpha_call, 'cell_alpha')
    vp, stream = bp.raw(dev)
    held = {label: (ax.outputs(n, cap, dev), ctypes.c_int64(-1), ctypes.c_int64(-1)) for label in also}
    others = {label: (lambda fn=fn, vout=held[label][0], vm=held[label][1], vg=held[label][2]:
                      fn(0, vp(p_d), vp(l_d), n, C, r, by, cap, *bounds, *(vp(t) for t in vout), ctypes.byref(vm), ctypes.byref(vg), stream))
              for label, fn in also.items()}
    equals = lambda label: (held[label][1].value, held[label][2].value) == (m, m_gab) and bp.tensors_equal(held[label][0], first)
    variants = bp.variants(alpha_call, others, equals, args)
    e2e, got = bp.end_to_end(lambda: ax.build(pts, lab, C, r / 2, by))
    same = bool(all(np.array_equal(a, b) for a, b in zip(got[:5], dev_out)) and got[5:] == (m, m_gab))
    win = bp.brute_window(pts, bounds, args.extent, args.check_n)
    sub, ref = ax.build(pts[win], lab[win], C, r / 2, by), ax.alpha_reference(pts[win], lab[win], C, r, by)
    exact = bool(all(np.array_equal(a, b) for a, b in zip(sub[:5], ref[:5])) and sub[5:] == ref[5:])
    kind = (dev_out[2] >= 0).sum(1)
    d = ax.derive(*dev_out, pts, lab, C, r)
    line = dict(points=name, radius_px=radius_px, n=n, m=int(m), m_gabriel=int(m_gab), interior=int((kind == 2).sum()), outline=int((kind == 1).sum()),
                singular=int((kind == 0).sum()), triangles=int(d['n_triangles']), degenerate=int(d['n_degenerate']), mean_degree=round(2 * m / n, 3),
                **bp.device_columns(ms, stages, e2e, same), device_calls_repeat=repeated(), **bp.graph_columns(gms, ms),
                proximity_ms=[round(v, 3) for v in pms], proximity_ms_median=round(med(pms), 3), device_over_proximity=round(med(ms) / med(pms), 2),
                gabriel_equals_proximity=same_gabriel, variants=variants, checked_points=int(win.sum()), checked_against_reference=exact)
    if tri is None:
        line.update(scipy_ms=None, scipy_note='scipy is not importable' if by == 0 else 'scipy triangulates all labels at once: compared under --by any only')
        return line
    (sites, site_of, simplices), tri_ms = tri
    se, filter_ms = scipy_filter(sites, simplices, r)
    ns = len(sites)
    code = lambda e: e[:, 0].astype(np.int64) * ns + e[:, 1]
    # the device's edges between DISTINCT sites (rows that share a site never bind each other, so the complex of the rows is the complex
    # of the sites with every end repeated), and which of them are diagonals of cocircular sites: two apexes and lo == hi, in integers
    e = dev_out[0].astype(np.int64)
    s_ap, m_ap = ax._bounds_of_apexes(pts.astype(np.int64), e, dev_out[2].astype(np.int64))
    diagonal = (dev_out[2] >= 0).all(1) & (m_ap[:, 0] * s_ap[:, 1] - m_ap[:, 1] * s_ap[:, 0] == 0)
    apart = dev_out[1] > 0
    on_sites = np.sort(site_of[e], 1)
    dev_codes = np.unique(code(on_sites[apart]))
    union = np.union1d(code(se), code(on_sites[apart & gabriel]))                            # the triangles' sides plus the Gabriel edges
    scipy_only = np.setdiff1d(union, dev_codes)
    device_only = np.setdiff1d(dev_codes, union)
    explained = bool(len(scipy_only) == 0 and np.isin(device_only, code(on_sites[apart & diagonal])).all())
    sk_ms = tri_ms + filter_ms
    line.update(scipy_ms=round(sk_ms, 1), scipy_delaunay_ms=round(tri_ms, 1), scipy_filter_ms=round(filter_ms, 1), distinct_sites=int(ns),
                coincident_edges=int((~apart).sum()), device_site_edges=int(len(dev_codes)), scipy_edges=int(len(union)),
                scipy_only_edges=int(len(scipy_only)), device_only_edges=int(len(device_only)), scipy_over_device_call=round(sk_ms / med(ms), 1),
                scipy_over_device_end_to_end=round(sk_ms / med(e2e), 1), scipy_difference_explained=explained)
    if int(d['n_degenerate']) == 0:
        line['scipy_edge_counts_agree'] = bool(len(union) == len(dev_codes))
    else:
        line['scipy_note'] = (f"{int(d['n_degenerate'])} edges are diagonals of cocircular points, where scipy keeps one of two: the device has {len(device_only)} "
                              f"edges between distinct sites that scipy lacks, every one of them such a diagonal, and scipy none that the device lacks")
    return line


def main(argv=None):
    ap = bp.parser()
    ap.add_argument('--radii', type=float, nargs='+', default=[32.0, 64.0], help='px')
    ap.add_argument('--by', choices=('any', 'class'), default='any')
    bp.also_arguments(ap)
    args = ap.parse_args(argv)
    from nuhtc_amd import alphacomplex as ax
    bp.need_gpu('bench_alpha.py')
    C = args.classes
    for radius in args.radii:
        ax.check_args(C, ax.half_pixel_radius(radius), ax.BY[args.by])
    also = bp.also_builds(args.also, 'nuhtc_cell_alpha')
    try:
        import scipy.spatial  # noqa: F401
        have_scipy = args.by == 'any'
    except ImportError:
        have_scipy = False
    sets = []
    for name, (p, lab) in bp.point_sets(args.n, args.extent, C).items():
        tri = scipy_triangulation(p) if have_scipy else None
        sets += [measure(name, p, lab, C, radius, args, also, tri) for radius in args.radii]
    line = dict(what=f'tools/bench_alpha.py: alpha complex of {args.n} synthetic nucleus centres on a {args.extent}-px square, radii {args.radii} px, by {args.by}, '
                     f'{C} classes, one MI355X; device: {args.repeats} calls after {args.warmup} warm-up calls; yardsticks: nuhtc_cell_proximity and '
                     f'nuhtc_cell_graph k 8 at radius 2 r; host: scipy.spatial.Delaunay + the circumradius filter in float64; variants: median ms of '
                     f'{args.repeats} calls per round, {args.rounds} alternating rounds',
                n=args.n, extent_px=args.extent, radii_px=args.radii, by=args.by, classes=C, sets=sets)
    bp.report(line, ('device_calls_agree', 'device_calls_repeat', 'checked_against_reference', 'gabriel_equals_proximity', 'scipy_edge_counts_agree', 'scipy_difference_explained'),
              (('equals_shipped', bp.all_equal_shipped(sets)),))


if __name__ == '__main__':
    main()
