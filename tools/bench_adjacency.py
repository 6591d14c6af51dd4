#!/usr/bin/env python
"""Cost of the territory adjacency of a slide (csrc/celladjacency.hip) beside the territory call that writes the owner map it reads --
prints ONE JSON line (profiles/cell_adjacency.json).

    python tools/bench_adjacency.py [--n 500000] [--extent 36000] [--reach 64] [--pitch 4] [--coarse-pitch 32] [--classes 5] [--repeats 10]
                                    [--warmup 3] [--also LABEL=path/to/libnuhtc_hip.so ...] [--rounds 2]

Synthetic nucleus centres from the generator of tools/bench_points.py, the shapes of tools/bench_territory.py: `--n` points uniform on a
square of `--extent` px, and one CLUSTERED set of the same size, at the defaults of tools/infer_wsi.py --nuclei-adjacency and again at
`--coarse-pitch`.  For each set and pitch the owner map is written once by nuhtc_cell_territory and stays on the device:
  device_ms            nuhtc_territory_adjacency alone, between two events, map and outputs resident, room for first_edge_cap(n) edges
                       (every stage, its own scratch allocation and both synchronisations included: it is one blocking call); every one
                       of the timed calls is compared bitwise with the first (device_calls_repeat)
  device_stage_ms      one further call under the library's per-kernel profile: cell_adjacency_count / _insert / _place
  territory_ms         the territory call on the same points and window, timed the same way: what the graph costs on top of it
  device_end_to_end_ms adjacency.build from numpy to numpy: upload, the territory call, the adjacency call(s), the download
  variants             with --also: other builds of the library (-DNUHTC_ADJ_PER_PAIR inserts every site pair into the call's table
                       without the LDS tile table; -DNUHTC_ADJ_ROW_SORT sorts every row's segment with one thread instead of ranking
                       with one thread per edge) timed in `--rounds` alternating rounds with the shipped one, all in this process; each
                       must return the shipped arrays
  checked_against_reference  a sub-window small enough for numpy, through both device calls again, against adjacency_reference on the
                       device's own owner map of it, and the graph's shared against the device's contact table
bench.py is the project's headline benchmark and is not changed by this tool."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_points as bp  # noqa: E402
from bench_points import med, timed  # noqa: E402


def measure(name, pts, lab, C, r, s, args, also):
    import torch
    from nuhtc_amd import adjacency as adj
    from nuhtc_amd import territory as tr
    n = len(pts)
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    win = tr.window(bounds, r, s)
    terr = tr.outputs(n, C, win, dev)
    territory = lambda: tr.call(p_d, l_d, C, r, s, win, *terr, bounds=bounds)
    terr_ms = timed(territory, args.repeats, args.warmup)
    owner = terr[0]
    first_cap = adj.first_edge_cap(n)
    cap, out, (_, m) = bp.grown(lambda cap, out: adj.call(owner, n, cap, *out), lambda cap: adj.outputs(n, cap, dev), first_cap)
    found = dict(m=m)

    def shipped():
        rc, found['m'] = adj.call(owner, n, cap, *out)
        return rc
    first, checked, repeated = bp.repeating(shipped, out, lambda: found['m'])
    for _ in range(3):
        checked()
    ms = timed(shipped, args.repeats, args.warmup)
    checked()
    stages = bp.stage_split(shipped, 'cell_adjacency')
    vp, stream = bp.raw(dev)
    held = {label: (adj.outputs(n, cap, dev), ctypes.c_int64(-1)) for label in also}
    others = {label: (lambda fn=fn, vout=held[label][0], vm=held[label][1]: fn(0, vp(owner), win[2], win[3], n, cap, *(vp(t) for t in vout), ctypes.byref(vm), stream))
              for label, fn in also.items()}
    variants = bp.variants(shipped, others, lambda label: held[label][1].value == m and bp.tensors_equal(held[label][0], first), args)
    del others, held
    e2e, built = bp.end_to_end(lambda: adj.build(pts, lab, C, r / 2, s / 2))
    got = [t.cpu().numpy() for t in first]
    same = bool(built[2] == win and np.array_equal(built[0][0], got[0][:m]) and np.array_equal(built[0][1], got[1][:m]) and np.array_equal(built[0][2], got[2]))
    contact = terr[5].cpu().numpy()
    agrees = bool(np.array_equal(adj.contact_of(got[0][:m], got[1][:m], lab, C), contact))
    # ---- a sub-window small enough for numpy, through both device calls again and against the definition on the device's own map
    sub = (win[0] + win[2] // 3, win[1] + win[3] // 3, min(600, win[2]), min(450, win[3]))
    sub_terr = tr.outputs(n, C, sub, dev)
    rc = tr.call(p_d, l_d, C, r, s, sub, *sub_terr, bounds=bounds)
    sub_out = adj.outputs(n, cap, dev)
    rc2, sub_m = adj.call(sub_terr[0], n, cap, *sub_out)
    torch.cuda.synchronize()
    ref = adj.adjacency_reference(sub_terr[0].cpu().numpy(), n)
    sg = [t.cpu().numpy() for t in sub_out]
    exact = bool(rc == 0 and rc2 == 0 and sub_m == ref[3] and np.array_equal(sg[0][:sub_m], ref[0]) and np.array_equal(sg[1][:sub_m], ref[1]) and
                 np.array_equal(sg[2], ref[2]) and np.array_equal(adj.contact_of(ref[0], ref[1], lab, C), sub_terr[5].cpu().numpy()))
    degree = got[2]
    area, is_open = terr[2].cpu().numpy(), terr[4].cpu().numpy()
    closed = (is_open == 0) & (area > 0)
    return dict(points=name, n=n, pitch_px=s / 2, window=list(win), sites=int(win[2] * win[3]), edges=int(m), edge_cap=int(cap), first_edge_cap=int(first_cap),
                nuclei_with_neighbours=int((degree > 0).sum()), degree_max=int(degree.max()), closed=int(closed.sum()),
                closed_degree_mean=round(float(degree[closed].mean()), 3) if closed.any() else 0.0, shared_sum=int(got[1][:m].sum()),
                **bp.device_columns(ms, stages, e2e, same), device_calls_repeat=repeated(), contact_agrees=agrees,
                territory_ms=[round(v, 3) for v in terr_ms], territory_ms_median=round(med(terr_ms), 3),
                device_over_territory=round(med(ms) / med(terr_ms), 2), variants=variants, checked_sites=int(sub[2] * sub[3]),
                checked_edges=int(ref[3]), checked_against_reference=exact)


def main(argv=None):
    ap = bp.parser(check_n=False)
    ap.add_argument('--reach', type=float, default=64.0, help='px')
    ap.add_argument('--pitch', type=float, default=4.0, help='px')
    ap.add_argument('--coarse-pitch', type=float, default=32.0, dest='coarse_pitch', help='px; 0: the --pitch alone')
    bp.also_arguments(ap)
    args = ap.parse_args(argv)
    from nuhtc_amd import adjacency as adj
    bp.need_gpu('bench_adjacency.py')
    C, r = args.classes, adj.half_pixel_radius(args.reach)
    pitches = [adj.half_pixel_radius(v) for v in (args.pitch, args.coarse_pitch) if v]
    for s in pitches:
        adj.check_args(C, r, s)
    also = bp.also_builds(args.also, 'nuhtc_territory_adjacency')
    point = bp.point_sets(args.n, args.extent, C)
    sets = [measure(name, p, lab, C, r, s, args, also) for s in pitches for name, (p, lab) in point.items()]
    line = dict(what=f'tools/bench_adjacency.py: territory adjacency (the discrete Delaunay graph) of {args.n} synthetic nucleus centres on a '
                     f'{args.extent}-px square, reach {args.reach:g} px, pitch {args.pitch:g} and {args.coarse_pitch:g} px, {C} classes, one MI355X; device: '
                     f'{args.repeats} calls after {args.warmup} warm-up calls on the resident owner map; territory: nuhtc_cell_territory on the same '
                     f'window; variants: median ms of {args.repeats} calls per round, {args.rounds} alternating rounds',
                n=args.n, extent_px=args.extent, reach_px=args.reach, classes=C, sets=sets,
                not_measured=['a whole slide with --nuclei-adjacency', '--gpus N', 'a window near 2**28 sites', 'a host Delaunay triangulation beside it'])
    bp.report(line, ('device_calls_agree', 'device_calls_repeat', 'contact_agrees', 'checked_against_reference'), (('equals_shipped', bp.all_equal_shipped(sets)),))


if __name__ == '__main__':
    main()
