#!/usr/bin/env python
"""Cost of the nucleus territories of a slide (csrc/cellterritory.hip) beside the density maps on the same lattice and scipy's cKDTree on
the host -- prints ONE JSON line (profiles/cell_territory.json).

    python tools/bench_territory.py [--n 500000] [--extent 36000] [--reach 64] [--pitch 4] [--coarse-pitch 32] [--classes 5] [--repeats 10]
                                    [--warmup 3] [--also LABEL=path/to/libnuhtc_hip.so ...] [--rounds 2]

Synthetic nucleus centres from the generator of tools/bench_points.py: `--n` points uniform on a square of `--extent` px, and one CLUSTERED
set of the same size, at the defaults of tools/infer_wsi.py --nuclei-territory and again at `--coarse-pitch`.  For each set and pitch:
  device_ms            nuhtc_cell_territory alone, between two events, points and outputs resident on the device, the default window (every
                       stage, its own scratch allocation and the final synchronisation included: it is one blocking call)
  device_stage_ms      one further call under the library's per-kernel profile: cell_territory_bin / _owner / _tally
  device_end_to_end_ms territory.build from numpy to numpy WITHOUT the maps: bounding box, upload, the call, the tallies' download
  with_maps_end_to_end_ms  the same with maps=True: the two rasters come off the device as well
  density_ms           the yardstick on the device: nuhtc_cell_density at the same reach and the same pitch where its cap of 2**24 sites
                       admits the window, else at the smallest multiple of the pitch that it admits (density_pitch_px says which)
  variants             with --also: other builds of the library (NUHTC_EXTRA_CFLAGS_CELLTERRITORY=-DNUHTC_SITE_ROUTE=1 forces the staged owner kernel, =2 the direct
                       one; -DNUHTC_TERRITORY_PER_SITE one atomic per site in the tally instead of one per run of a wave) timed in
                       `--rounds` alternating rounds with the shipped one, all in this process; each must return the shipped arrays
  host_ms              the yardstick on the host: scipy.spatial.cKDTree.query(k=1, distance_upper_bound=reach) over the sites of the
                       window's first rows, at most 2**22 of them (the owner and the distance alone, no tallies, float64, all cores);
                       the two are compared per million sites; host_agrees compares its owners with the device's: the same distance
                       everywhere, another owner only at that same distance
  checked_against_reference  a sub-window small enough for brute force, through the device again, against territory_reference on the
                       points within reach of it: every output
bench.py is the project's headline benchmark and is not changed by this tool."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_points as bp  # noqa: E402
from bench_points import med, timed  # noqa: E402


HOST_SITES = 1 << 22


def host_route(pts, lab, C, r, s, win, owner, nearest):
    """cKDTree over the competitors, the sites of the window's first rows (at most 2**22 of them) queried once -> (ms, agrees, owners that
    differ, sites queried): agrees compares owner and nearest_d2 wherever the device's
    owner is the only point at that distance (a tie is the tree's to break as it likes)."""
    from scipy.spatial import cKDTree
    gx0, gy0, W, H = win
    H = max(1, min(H, HOST_SITES // W))                                                    # the first rows of the window: at most HOST_SITES sites
    owner, nearest = owner[:H], nearest[:H]
    rows = np.flatnonzero((lab >= 0) & (lab < C))
    t0 = time.perf_counter()
    tree = cKDTree(pts[rows].astype(np.float64))
    gy, gx = np.mgrid[gy0:gy0 + H, gx0:gx0 + W]
    q = np.stack([gx.reshape(-1) * float(s), gy.reshape(-1) * float(s)], 1)
    dist, idx = tree.query(q, k=1, distance_upper_bound=float(r) * (1 + 1e-12), workers=-1)
    ms = 1e3 * (time.perf_counter() - t0)
    found = idx < len(rows)
    got = np.where(found, rows[np.minimum(idx, len(rows) - 1)], -1).reshape(H, W)
    d2 = np.where(found, np.rint(dist * dist), -1).astype(np.int64).reshape(H, W)
    same_d2 = bool(np.array_equal(d2, nearest))                                           # the distance has no tie to break
    differ = got != owner
    tie_only = True
    if differ.any():                                                                       # a different owner is fine only at the same distance
        v, u = np.nonzero(differ)
        other = pts[got[v, u]].astype(np.int64)
        qq = np.stack([(gx0 + u) * s, (gy0 + v) * s], 1)
        tie_only = bool((((qq - other) ** 2).sum(1) == nearest[v, u]).all())
    return ms, same_d2 and tie_only, int(differ.sum()), W * H


def variant_calls(also, p_d, l_d, n, C, r, s, win, bounds, dev):
    """-> {label: (call, outputs)} for the --also builds on the resident points."""
    from nuhtc_amd import territory as tr
    vp, stream = bp.raw(dev)
    calls = {}
    for label, fn in also.items():
        vout = tr.outputs(n, C, win, dev)
        calls[label] = ((lambda fn=fn, vout=vout: fn(0, vp(p_d), vp(l_d), n, C, r, s, *win, *bounds, *(vp(t) for t in vout), stream)), vout)
    return calls


def density_yardstick(p_d, l_d, C, r, s, bounds, args):
    """nuhtc_cell_density at the same reach, at the pitch itself or the smallest multiple of it whose default window density accepts."""
    from nuhtc_amd import density as dn
    m = 1
    while True:
        win = dn.window(bounds, r, m * s)
        if win[2] * win[3] <= dn.MAX_SITES:
            break
        m += 1
    out = dn.outputs(C, win, p_d.device)
    ms = timed(lambda: dn.call(p_d, l_d, C, r, m * s, win, *out, bounds=bounds), args.repeats, args.warmup)
    return dict(density_ms=[round(v, 3) for v in ms], density_ms_median=round(med(ms), 3), density_pitch_px=m * s / 2, density_sites=int(win[2] * win[3]))


def measure(name, pts, lab, C, r, s, args, also):
    import torch
    from nuhtc_amd import territory as tr
    n = len(pts)
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    win = tr.window(bounds, r, s)
    out = tr.outputs(n, C, win, dev)
    shipped = lambda: tr.call(p_d, l_d, C, r, s, win, *out, bounds=bounds)
    ms = timed(shipped, args.repeats, args.warmup)
    got = [t.cpu().numpy() for t in out]
    stages = bp.stage_split(shipped, 'cell_territory')
    held = variant_calls(also, p_d, l_d, n, C, r, s, win, bounds, dev)
    variants = bp.variants(shipped, {label: call for label, (call, _) in held.items()}, lambda label: bp.tensors_equal(held[label][1], out), args)
    del held
    dens = density_yardstick(p_d, l_d, C, r, s, bounds, args)
    e2e, built = bp.end_to_end(lambda: tr.build(pts, lab, C, r / 2, s / 2))
    e2e_maps, built_maps = bp.end_to_end(lambda: tr.build(pts, lab, C, r / 2, s / 2, maps=True))
    same = bool(built[1] == win and built[2] is None and all(np.array_equal(a, b.reshape(a.shape)) for a, b in zip(built[0], got[2:])) and
                np.array_equal(built_maps[2][0], got[0]) and np.array_equal(built_maps[2][1], got[1]))
    # ---- a sub-window small enough for brute force, through the device again and against the definition
    sub = (win[0] + win[2] // 3, win[1] + win[3] // 3, min(60, win[2]), min(45, win[3]))
    lo, hi = np.array(sub[:2]) * s - r, (np.array(sub[:2]) + np.array(sub[2:]) - 1) * s + r
    near = np.flatnonzero(((pts >= lo) & (pts <= hi)).all(1))                              # every point that can reach a site of the sub-window
    sub_out = tr.outputs(n, C, sub, dev)
    rc = tr.call(p_d, l_d, C, r, s, sub, *sub_out, bounds=bounds)
    torch.cuda.synchronize()
    ref = tr.territory_reference(pts[near], lab[near], C, r, s, sub)
    sg = [t.cpu().numpy() for t in sub_out]
    back = np.where(ref[0] >= 0, near[np.maximum(ref[0], 0)], -1)                          # the reference's rows are positions in `near`
    exact = bool(rc == 0 and np.array_equal(sg[0], back) and np.array_equal(sg[1], ref[1]) and np.array_equal(sg[2][near], ref[2]) and
                 np.array_equal(sg[3][near], ref[3]) and np.array_equal(sg[4][near], ref[4]) and int(sg[2].sum()) == int(ref[2].sum()) and
                 np.array_equal(sg[5], ref[5]) and np.array_equal(sg[6], ref[6]) and int(sg[7][0]) == int(ref[7]))
    host_ms, agree, ties, host_sites = host_route(pts, lab, C, r, s, win, got[0], got[1])
    per_m = lambda v, k: v * 1e6 / k
    d = tr.derive(got[2], got[4], got[5], got[6], got[7], lab, s)
    return dict(points=name, n=n, pitch_px=s / 2, window=list(win), sites=int(win[2] * win[3]), owned_share=round(1 - float(d['free_share']), 4),
                nuclei_with_sites=int((got[2] > 0).sum()), closed=int(d['closed'].sum()), class_area_share=[round(float(v), 4) for v in d['class_area_share']],
                **bp.device_columns(ms, stages, e2e, same), with_maps_end_to_end_ms=[round(v, 2) for v in e2e_maps],
                with_maps_end_to_end_ms_median=round(med(e2e_maps), 2), **dens, device_over_density=round(med(ms) / dens['density_ms_median'], 2),
                variants=variants, checked_sites=int(sub[2] * sub[3]), checked_points=int(len(near)), checked_against_reference=exact,
                host_ms=round(host_ms, 1), host_sites=host_sites, host_ms_per_million_sites=round(per_m(host_ms, host_sites), 1),
                device_ms_per_million_sites=round(per_m(med(ms), win[2] * win[3]), 4),
                host_over_device_call_per_site=round(per_m(host_ms, host_sites) / per_m(med(ms), win[2] * win[3]), 1),
                host_agrees=agree, host_ties_broken_otherwise=ties)


def main(argv=None):
    ap = bp.parser(check_n=False)
    ap.add_argument('--reach', type=float, default=64.0, help='px')
    ap.add_argument('--pitch', type=float, default=4.0, help='px')
    ap.add_argument('--coarse-pitch', type=float, default=32.0, dest='coarse_pitch', help='px; 0: the --pitch alone')
    bp.also_arguments(ap)
    args = ap.parse_args(argv)
    from nuhtc_amd import territory as tr
    bp.need_gpu('bench_territory.py')
    C, r = args.classes, tr.half_pixel_radius(args.reach)
    pitches = [tr.half_pixel_radius(v) for v in (args.pitch, args.coarse_pitch) if v]
    for s in pitches:
        tr.check_args(C, r, s)
    also = bp.also_builds(args.also, 'nuhtc_cell_territory')
    point = bp.point_sets(args.n, args.extent, C)
    sets = [measure(name, p, lab, C, r, s, args, also) for s in pitches for name, (p, lab) in point.items()]
    line = dict(what=f'tools/bench_territory.py: nearest-nucleus raster of {args.n} synthetic nucleus centres on a {args.extent}-px square, reach '
                     f'{args.reach:g} px, pitch {args.pitch:g} and {args.coarse_pitch:g} px, {C} classes, one MI355X; device: {args.repeats} calls after '
                     f'{args.warmup} warm-up calls; density: nuhtc_cell_density at the same reach; host: scipy cKDTree.query(k=1) over the sites, all '
                     f'cores; variants: median ms of {args.repeats} calls per round, {args.rounds} alternating rounds',
                n=args.n, extent_px=args.extent, reach_px=args.reach, classes=C, sets=sets,
                not_measured=['a whole slide with --nuclei-territory', '--gpus N', 'a window near 2**28 sites'])
    bp.report(line, ('device_calls_agree', 'checked_against_reference', 'host_agrees'), (('equals_shipped', bp.all_equal_shipped(sets)),))


if __name__ == '__main__':
    main()
