#!/usr/bin/env python
"""Cost of the alpha-shape outline of a slide's nuclei (csrc/celloutline.hip) beside the alpha complex it walks -- prints ONE JSON line
(profiles/cell_outline.json).

    python tools/bench_outline.py [--n 500000] [--extent 36000] [--radii 32 64] [--by any] [--classes 5] [--repeats 10] [--warmup 3]
                                  [--host-edges 200000]

Synthetic nucleus centres from the generator of tools/bench_points.py, the sets of tools/bench_alpha.py: `--n` points uniform on a square
of `--extent` px, and one CLUSTERED set of the same size.  For each set and each radius r of `--radii` (px):
  alpha_ms             nuhtc_cell_alpha on the resident points, between two events: the yardstick, in the same process
  device_ms            nuhtc_alpha_outline alone on the tensors that call left on the device, timed the same way (every stage, its own
                       scratch allocation, the two read-backs and synchronisations included: it is one blocking call)
  m, h, R, K, holes    the edges of the complex, the half-edges, the rings, the components, the rings of negative area
  rounds               the doubling rounds of either half of the rank stage: the smallest k with 2^k >= h
  device_stage_ms      one further call under the library's per-kernel profile: the cell_outline_* stages
  host_ms              the host route: `outline_reference`, the plain Python / numpy walk, on the same edges when there are at most
                       `--host-edges` of them; otherwise on the complex of a corner window of the points (host_subset_edges of them), with
                       host_ms_extrapolated = host_ms * m / host_subset_edges, marked as an extrapolation
  rings_equal_host     the device's nine results EQUAL the walk's, on the same edges or on the window's (the device runs the window too)
bench.py is the project's headline benchmark and is not changed by this tool."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_points as bp  # noqa: E402
from bench_points import med  # noqa: E402


def same_results(got, want):
    return all(np.array_equal(g, w) and np.asarray(g).dtype == np.asarray(w).dtype for g, w in zip(got[:6], want[:6])) and tuple(got[6:9]) == tuple(want[6:9])


def main():
    ap = bp.parser()
    ap.add_argument('--radii', type=float, nargs='+', default=[32.0, 64.0], help='alpha radii in px')
    ap.add_argument('--by', choices=('any', 'class'), default='any')
    ap.add_argument('--host-edges', type=int, default=200000, dest='host_edges', help='the most edges the plain walk takes whole')
    args = ap.parse_args()
    bp.need_gpu('bench_outline')
    import torch
    from nuhtc_amd import alphacomplex as ax
    from nuhtc_amd import outline as ol
    C, by = args.classes, ax.BY[args.by]
    sets = []
    for kind, (pts, lab) in bp.point_sets(args.n, args.extent, C).items():
        dev, bounds, p_d, l_d = bp.resident(pts, lab)
        n = len(pts)
        for radius in args.radii:
            r = ax.half_pixel_radius(radius)
            cap = ax.first_edge_cap(n)
            alpha = ax.outputs(n, cap, dev)
            rc, m, m_gab = ax.call(p_d, l_d, C, r, by, cap, *alpha, bounds=bounds)
            if rc or m > cap:
                cap = m
                alpha = ax.outputs(n, cap, dev)
            alpha_ms = bp.timed(lambda: ax.call(p_d, l_d, C, r, by, cap, *alpha, bounds=bounds)[0], args.repeats, args.warmup)
            m = ax.call(p_d, l_d, C, r, by, cap, *alpha, bounds=bounds)[1]
            out = ol.outputs(n, m, dev)
            run = lambda: ol.call(p_d, l_d, by, alpha[0], alpha[1], alpha[2], m, *out)
            ms = bp.timed(lambda: run()[0], args.repeats, args.warmup)
            rc, h, R, K = run()
            stages = bp.stage_split(run, 'cell_outline')
            got = tuple(t[:k].cpu().numpy() for t, k in zip(out, (h, R + 1, R, R, n, K))) + (h, R, K)
            row = dict(kind=kind, radius_px=radius, by=args.by, n=n, m=m, h=h, R=R, K=K, holes=int((got[2] < 0).sum()), rounds=int(np.ceil(np.log2(max(h, 1)))),
                       alpha_ms=[round(v, 3) for v in alpha_ms], alpha_ms_median=round(med(alpha_ms), 3), device_ms=[round(v, 3) for v in ms],
                       device_ms_median=round(med(ms), 3), device_over_alpha=round(med(ms) / med(alpha_ms), 3), device_stage_ms=stages)
            if m <= args.host_edges:
                e, d2, apex = (t[:m].cpu().numpy() for t in alpha[:3])
                t0 = time.perf_counter()
                want = ol.outline_reference(pts, lab, e, d2, apex, by)
                row.update(host_ms=round(1e3 * (time.perf_counter() - t0), 1), host_on='the same edges', rings_equal_host=same_results(got, want))
            else:                                       # a corner window with about host_edges edges: both routes on the window's own complex
                win = bp.brute_window(pts, bounds, args.extent, max(3, int(n * args.host_edges / m)))
                sub = ol.build(pts[win], lab[win], C, radius, by, with_alpha=True)
                t0 = time.perf_counter()
                want = ol.outline_reference(pts[win], lab[win], sub[9], sub[10], sub[11], by)
                host_ms = 1e3 * (time.perf_counter() - t0)
                row.update(host_ms=round(host_ms, 1), host_on='a corner window', host_subset_points=int(win.sum()), host_subset_edges=int(sub[14]),
                           host_ms_extrapolated=round(host_ms * m / max(int(sub[14]), 1), 1), host_is_extrapolated=True, rings_equal_host=same_results(sub[:9], want))
            row['host_over_device'] = round(row.get('host_ms_extrapolated', row['host_ms']) / med(ms), 1)
            sets.append(row)
            del alpha, out
            torch.cuda.empty_cache()
    bp.report(dict(tool='bench_outline', device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup, sets=sets), ('rings_equal_host',))


if __name__ == '__main__':
    main()
