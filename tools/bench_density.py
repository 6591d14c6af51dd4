#!/usr/bin/env python
"""Cost of the nucleus density maps of a slide (csrc/celldensity.hip) beside a numpy restatement on the host -- prints ONE JSON line
(profiles/cell_density.json).

    python tools/bench_density.py [--n 1000000] [--extent 50000] [--bandwidth 128] [--pitch 64] [--classes 5] [--repeats 10] [--warmup 3]
                                  [--also LABEL=path/to/libnuhtc_hip.so ...] [--rounds 2] [--more-shapes]

Synthetic nucleus centres from the generator of tools/bench_points.py: `--n` points uniform on a square of `--extent` px, and one CLUSTERED
set of the same size (400 Gaussian clumps, sigma 300 px), at the defaults of tools/infer_wsi.py --nuclei-density.  For each set:
  device_ms            nuhtc_cell_density alone, between two events, points and outputs resident on the device, the default window (every
                       stage, its own scratch allocation and the final synchronisation included: it is one blocking call), `--repeats`
                       after `--warmup`
  device_stage_ms      one further call under the library's per-kernel profile: the binning, and the kernel that took the sites
                       (cell_density_tile: staged through LDS; cell_density_site: every site on its own)
  device_end_to_end_ms density.build from numpy to numpy: bounding box, upload, the call, download (wall clock)
  variants             with --also: other builds of the library (NUHTC_EXTRA_CFLAGS_CELLDENSITY=-DNUHTC_SITE_ROUTE=1 forces the staged kernel, =2 the direct one) timed
                       in `--rounds` alternating rounds with the shipped one, all in this process; each must return the shipped arrays
  host_ms              the yardstick: numpy with a per-point scatter -- for every offset of a point's site footprint one np.add.at over all
                       points into the int64 rasters; must equal the device
  checked_against_reference  a sub-window small enough for brute force, through the device again, against density_reference on the points
                       within reach of it
With --more-shapes the shipped and the --also builds are timed at further (bandwidth, pitch) pairs on the uniform set: where the rule that
picks the kernel (site_route_staged of csrc/cellgrid_host.h) has to hold.  bench.py is the project's headline benchmark and is not changed
by this tool."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_points as bp  # noqa: E402
from bench_points import med, timed  # noqa: E402


def host_route(pts, lab, C, h, s, win):
    """numpy, a per-point scatter: -> (count int32, weight int64, ms).  A point at p reaches the sites floor(p / s) - k .. floor(p / s) + k + 1
    along each axis, k = h // s."""
    t0 = time.perf_counter()
    gx0, gy0, W, H = win
    p = pts.astype(np.int64)
    count, weight = np.zeros((C, H, W), np.int64), np.zeros((C, H, W), np.int64)
    known = (lab >= 0) & (lab < C)
    base, k = p // s, h // s
    for b in range(-k, k + 2):
        for a in range(-k, k + 2):
            gx, gy = base[:, 0] + a, base[:, 1] + b
            d2 = (gx * s - p[:, 0]) ** 2 + (gy * s - p[:, 1]) ** 2
            hit = known & (d2 <= h * h) & (gx >= gx0) & (gx < gx0 + W) & (gy >= gy0) & (gy < gy0 + H)
            at = (lab[hit], gy[hit] - gy0, gx[hit] - gx0)
            np.add.at(count, at, 1)
            np.add.at(weight, at, h * h - d2[hit])
    return count.astype(np.int32), weight, 1e3 * (time.perf_counter() - t0)


def variant_calls(also, p_d, l_d, n, C, h, s, win, bounds, dev):
    """-> {label: (call, outputs)} for the --also builds on the resident points."""
    from nuhtc_amd import density as dn
    vp, stream = bp.raw(dev)
    calls = {}
    for label, fn in also.items():
        vout = dn.outputs(C, win, dev)
        calls[label] = ((lambda fn=fn, vout=vout: fn(0, vp(p_d), vp(l_d), n, C, h, s, *win, *bounds, vp(vout[0]), vp(vout[1]), stream)), vout)
    return calls


def measure(name, pts, lab, C, h, s, args, also):
    import torch
    from nuhtc_amd import density as dn
    n = len(pts)
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    win = dn.window(bounds, h, s)
    out = dn.outputs(C, win, dev)
    shipped = lambda: dn.call(p_d, l_d, C, h, s, win, *out, bounds=bounds)
    ms = timed(shipped, args.repeats, args.warmup)
    count, weight = out[0].cpu().numpy(), out[1].cpu().numpy()
    stages = bp.stage_split(shipped, 'cell_density')
    held = variant_calls(also, p_d, l_d, n, C, h, s, win, bounds, dev)
    variants = bp.variants(shipped, {label: call for label, (call, _) in held.items()}, lambda label: bp.tensors_equal(held[label][1], out), args)
    del held
    e2e, got = bp.end_to_end(lambda: dn.build(pts, lab, C, h / 2, s / 2))
    same = bool(np.array_equal(got[0], count) and np.array_equal(got[1], weight) and got[2] == win)
    # ---- a sub-window small enough for brute force, through the device again and against the definition
    sub = (win[0] + win[2] // 3, win[1] + win[3] // 3, min(40, win[2]), min(30, win[3]))
    lo, hi = np.array(sub[:2]) * s - h, (np.array(sub[:2]) + np.array(sub[2:]) - 1) * s + h
    near = ((pts >= lo) & (pts <= hi)).all(1)                 # every point that can reach a site of the sub-window
    rc, sub_out = 0, dn.outputs(C, sub, dev)
    rc = dn.call(p_d, l_d, C, h, s, sub, *sub_out, bounds=bounds)
    torch.cuda.synchronize()
    ref = dn.density_reference(pts[near], lab[near], C, h, s, sub)
    exact = bool(rc == 0 and np.array_equal(sub_out[0].cpu().numpy(), ref[0]) and np.array_equal(sub_out[1].cpu().numpy(), ref[1]))
    hc, hw, host_ms = host_route(pts, lab, C, h, s, win)
    agree = bool(np.array_equal(hc, count) and np.array_equal(hw, weight))
    return dict(points=name, n=n, window=list(win), sites=int(win[2] * win[3]), class_total=count.reshape(C, -1).sum(1).tolist(),
                mean_count_per_site=round(float(count.sum()) / (win[2] * win[3]), 2),
                **bp.device_columns(ms, stages, e2e, same),
                variants=variants, checked_sites=int(sub[2] * sub[3]), checked_points=int(near.sum()), checked_against_reference=exact,
                host_ms=round(host_ms, 1), host_over_device_call=round(host_ms / med(ms), 1), host_over_device_end_to_end=round(host_ms / med(e2e), 1),
                host_rasters_agree=agree)


def more_shapes(pts, lab, C, args, also):
    """The shipped and the --also builds at further (bandwidth, pitch) pairs in px on one set: the rule against the measurement."""
    import torch
    from nuhtc_amd import density as dn
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    rows = []
    for bw, pitch in ((128, 32), (128, 16), (128, 8), (64, 64), (32, 4), (16, 64)):
        h, s = dn.half_pixel_radius(bw), dn.half_pixel_radius(pitch)
        win = dn.window(bounds, h, s)
        if win[2] * win[3] > dn.MAX_SITES:
            continue
        out = dn.outputs(C, win, dev)
        shipped = lambda: dn.call(p_d, l_d, C, h, s, win, *out, bounds=bounds)
        took = sorted(tag for tag in bp.stage_split(shipped, 'cell_density_') if tag in ('cell_density_tile', 'cell_density_site'))
        calls = {'shipped': shipped}
        same = {}
        for label, (call, vout) in variant_calls(also, p_d, l_d, len(pts), C, h, s, win, bounds, dev).items():
            call()
            torch.cuda.synchronize()
            same[label] = bool(torch.equal(vout[0], out[0]) and torch.equal(vout[1], out[1]))
            calls[label] = call
        rows.append(dict(bandwidth_px=bw, pitch_px=pitch, sites=int(win[2] * win[3]), shipped_kernel=took, ms=bp.alternating_rounds(calls, args.repeats, args.rounds), equals_shipped=same))
        del out
    return rows


def main(argv=None):
    ap = bp.parser(n=1000000, extent=50000, check_n=False)
    ap.add_argument('--bandwidth', type=float, default=128.0, help='px')
    ap.add_argument('--pitch', type=float, default=64.0, help='px')
    bp.also_arguments(ap)
    ap.add_argument('--more-shapes', action='store_true', dest='more_shapes', help='time further (bandwidth, pitch) pairs on the uniform set')
    args = ap.parse_args(argv)
    from nuhtc_amd import density as dn
    bp.need_gpu('bench_density.py')
    C, h, s = args.classes, dn.half_pixel_radius(args.bandwidth), dn.half_pixel_radius(args.pitch)
    dn.check_args(C, h, s)
    also = bp.also_builds(args.also, 'nuhtc_cell_density')
    point = bp.point_sets(args.n, args.extent, C)
    sets = [measure(name, p, lab, C, h, s, args, also) for name, (p, lab) in point.items()]
    line = dict(what=f'tools/bench_density.py: class-wise density maps of {args.n} synthetic nucleus centres on a {args.extent}-px square, bandwidth '
                     f'{args.bandwidth:g} px, pitch {args.pitch:g} px, {C} classes, one MI355X; device: {args.repeats} calls after {args.warmup} warm-up '
                     f'calls; host: numpy, one np.add.at per offset of a point\'s site footprint; variants: median ms of {args.repeats} calls per '
                     f'round, {args.rounds} alternating rounds',
                n=args.n, extent_px=args.extent, bandwidth_px=args.bandwidth, pitch_px=args.pitch, classes=C, sets=sets)
    if args.more_shapes:
        line['more_shapes_uniform'] = more_shapes(*point['uniform'], C, args, also)
    same = [v.get('equals_shipped', True) for s_ in sets for v in s_['variants'].values()]
    same += [ok for r in line.get('more_shapes_uniform', []) for ok in r['equals_shipped'].values()]
    bp.report(line, ('device_calls_agree', 'checked_against_reference', 'host_rasters_agree'), (('equals_shipped', all(same)),))


if __name__ == '__main__':
    main()
