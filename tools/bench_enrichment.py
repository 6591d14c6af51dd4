#!/usr/bin/env python
"""Cost of the neighbourhood enrichment of a slide (csrc/cellenrich.hip) beside the spatial statistics' single sweep and a host KD-tree --
prints ONE JSON line (profiles/cell_enrichment.json).

    python tools/bench_enrichment.py [--n 500000] [--extent 36000] [--radius 64] [--perms 1000] [--seed 0] [--classes 5] [--repeats 10]
                                     [--warmup 3] [--host-n 50000] [--host-perms 50]

Synthetic nucleus centres as in tools/bench_spatial.py (bench_points.point_sets): `--n` points uniform on a square of `--extent` px with
uniform labels, and one CLUSTERED set of the same size with skewed labels.  For each set:
  device_ms            nuhtc_cell_enrichment alone at `--perms`, between two events, points and outputs resident on the device (binning,
                       zeroing, every batch's shuffle and sweep, its own scratch allocation and final synchronisation included: it is one
                       blocking call), `--repeats` after `--warmup`
  one_batch_ms         the same call at P = 16: the binning, ONE shuffle and ONE sweep (which also carries the observed labels)
  per_further_batch_ms (device_ms - one_batch_ms) / (batches - 1): what each batch of 16 permutations adds
  device_stage_ms      one further call at `--perms` under the library's per-kernel profile: the binning launches, the shuffles, the sweeps
  device_end_to_end_ms enrichment.build from numpy to numpy: bounding box, upload, the call, download (wall clock)
  spatial_ms           the yardstick: nuhtc_cell_spatial with the single edge r on the same points in the same run, timed the same way --
                       the same contacts swept once, without shuffling (it also writes nn_d2 and bins by (cell, class))
  host_*               the host route on the first `--host-n` points of the set (ALL of the square, thinned: fewer contacts per point): the
                       contacts from scipy.spatial.cKDTree.query_pairs (brute force without scipy) and one numpy bincount per
                       permutation for `--host-perms` permutations with numpy's own shuffle; host_extrapolated_ms scales the contact
                       search and each bincount by (n / host_n)^2 -- the number of contacts grows with the square of the density -- and
                       the permutations to `--perms`.  An estimate, labelled as one.
  checked_against_reference  the device on a window of the points small enough for brute force against enrichment.enrichment_reference
                       at `--perms`, and the timed `observed` against the spatial call's bin 0
bench.py is the project's headline benchmark and is not changed by this tool."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_points as bp  # noqa: E402
from bench_points import med  # noqa: E402


def host_route(pts, lab, C, r, perms):
    """-> (tree and contacts ms, ms per permutation, contacts, how the contacts were found) on the host."""
    from nuhtc_amd import enrichment as en
    t0 = time.perf_counter()
    try:
        from scipy.spatial import cKDTree
        pairs = cKDTree(pts.astype(np.float64)).query_pairs(r * (1 + 1e-12), output_type='ndarray')        # i < j, each once
        ci, cj, how = np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([pairs[:, 1], pairs[:, 0]]), 'scipy cKDTree.query_pairs'
    except ImportError:
        ci, cj = en.contacts(pts.astype(np.int64), r)
        how = 'brute force (no scipy)'
    t_contacts = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    cls = np.where((lab >= 0) & (lab < C), lab, C).astype(np.int64)
    t0 = time.perf_counter()
    for _ in range(perms):
        c = cls[rng.permutation(len(cls))]
        np.bincount(c[ci] * (C + 1) + c[cj], minlength=(C + 1) * (C + 1))
    t_perm = (time.perf_counter() - t0) / max(perms, 1)
    return 1e3 * t_contacts, 1e3 * t_perm, len(ci), how


def measure(name, pts, lab, C, r, args):
    import torch
    from nuhtc_amd import enrichment as en
    from nuhtc_amd import spatial as sp
    n, P = len(pts), args.perms
    dev, bounds, p_d, l_d = bp.resident(pts, lab)
    out = [torch.zeros(shape, dtype=torch.int64, device=dev) for shape in ((C, C), (P, C, C), (C,))]
    one = [torch.zeros(shape, dtype=torch.int64, device=dev) for shape in ((C, C), (16, C, C), (C,))]
    full_call = lambda: en.call(p_d, l_d, C, r, P, args.seed, *out, bounds=bounds)
    ms = bp.timed(full_call, args.repeats, args.warmup)
    ms16 = bp.timed(lambda: en.call(p_d, l_d, C, r, 16, args.seed, *one, bounds=bounds), args.repeats, args.warmup)
    sout = [torch.zeros((C, C, 1), dtype=torch.int64, device=dev), torch.full((n, C), -1, dtype=torch.int32, device=dev),
            torch.zeros((C,), dtype=torch.int64, device=dev)]
    sms = bp.timed(lambda: sp.call(p_d, l_d, C, [r], *sout, bounds=bounds), args.repeats, args.warmup)
    stages = bp.stage_split(full_call, 'cell_enrichment')
    dev_out = [t.cpu().numpy() for t in out]
    e2e, got = bp.end_to_end(lambda: en.build(pts, lab, C, r / 2, P, seed=args.seed))
    same = bool(all(np.array_equal(a, b) for a, b in zip(got, dev_out)) and np.array_equal(one[1].cpu().numpy(), dev_out[1][:16]))
    spatial_agrees = bool(np.array_equal(dev_out[0], sout[0].cpu().numpy()[:, :, 0]) and np.array_equal(dev_out[2], sout[2].cpu().numpy()))
    # ---- a window small enough for brute force, through the device again and against the definition
    win = bp.brute_window(pts, bounds, args.extent, args.check_n)
    sub = en.build(pts[win], lab[win], C, r / 2, P, seed=args.seed)
    exact = bool(all(np.array_equal(a, b) for a, b in zip(sub, en.enrichment_reference(pts[win], lab[win], C, r, P, args.seed))))
    # ---- the host route on a thinned set
    hn = min(args.host_n, n)
    t_contacts, t_perm, found, how = host_route(pts[:hn], lab[:hn], C, r, args.host_perms)
    scale = n / hn
    batches = (P + 15) // 16
    contacts = int(dev_out[0].sum())
    z = en.derive(dev_out[0], dev_out[1])['z']
    return dict(points=name, n=n, contacts=contacts, mean_contacts_per_point=round(contacts / max(int(dev_out[2].sum()), 1), 2), class_n=dev_out[2].tolist(),
                largest_abs_z=round(float(np.abs(z).max()), 2), **bp.device_columns(ms, stages, e2e, same),
                one_batch_ms=[round(v, 3) for v in ms16], one_batch_ms_median=round(med(ms16), 3),
                per_further_batch_ms=round((med(ms) - med(ms16)) / max(batches - 1, 1), 3), batches=batches,
                spatial_ms=[round(v, 3) for v in sms], spatial_ms_median=round(med(sms), 3), one_batch_over_spatial=round(med(ms16) / med(sms), 2),
                per_further_batch_over_spatial=round((med(ms) - med(ms16)) / max(batches - 1, 1) / med(sms), 2),
                host_route=how, host_n=hn, host_perms=args.host_perms, host_contacts=found, host_contacts_ms=round(t_contacts, 1),
                host_ms_per_permutation=round(t_perm, 2),
                host_extrapolated_ms=round(t_contacts * scale * scale + t_perm * scale * scale * P, 0),
                host_extrapolated_over_device_call=round((t_contacts * scale * scale + t_perm * scale * scale * P) / med(ms), 1),
                observed_equals_spatial_bin0=spatial_agrees, checked_points=int(win.sum()), checked_against_reference=exact)


def main(argv=None):
    ap = bp.parser()
    ap.add_argument('--radius', type=float, default=64.0, help='contact radius, px (the default of the slide tool)')
    ap.add_argument('--perms', type=int, default=1000)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--host-n', type=int, default=50000, dest='host_n')
    ap.add_argument('--host-perms', type=int, default=50, dest='host_perms')
    args = ap.parse_args(argv)
    from nuhtc_amd import cellpoints
    from nuhtc_amd import enrichment as en
    C, r = args.classes, cellpoints.half_pixel_radius(args.radius)
    en.check_args(C, r, args.perms, args.seed)
    bp.need_gpu('bench_enrichment.py')
    sets = [measure(name, p, lab, C, r, args) for name, (p, lab) in bp.point_sets(args.n, args.extent, C).items()]
    line = dict(what=f'tools/bench_enrichment.py: neighbourhood enrichment of {args.n} synthetic nucleus centres on a {args.extent}-px square, radius '
                     f'{args.radius:g} px, {args.perms} label permutations (seed {args.seed}), {C} classes, one MI355X; device: {args.repeats} calls after '
                     f'{args.warmup} warm-up calls; yardstick: nuhtc_cell_spatial with the single edge r; host: contacts once, one bincount per '
                     f'permutation, on {args.host_n} of the points, extrapolated',
                n=args.n, extent_px=args.extent, radius_px=args.radius, perms=args.perms, seed=args.seed, classes=C, sets=sets)
    bp.report(line, ('device_calls_agree', 'checked_against_reference', 'observed_equals_spatial_bin0'))


if __name__ == '__main__':
    main()
