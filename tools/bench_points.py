"""What the bench tools of the per-slide point analyses (bench_cellgraph, bench_spatial, bench_clusters, bench_mst, bench_proximity,
bench_density, bench_territory, bench_adjacency, bench_alpha, bench_enrichment, bench_regions, bench_margin) do in the same way: the synthetic point sets, the shared arguments, the event-timed loop, the stage split under the
library's profile, the wall-clock end-to-end loop, the window small enough for brute force, the cell-graph yardstick, the capacity protocol of
the edge-list calls with the check that every call repeats the first, the --also builds in alternating rounds and the one JSON line.
A helper, not a tool: each tool keeps its call, its summary columns and its host comparison."""
import argparse
import json
import os
import time

import numpy as np

med = lambda v: float(np.median(v))


def point_sets(n, extent, C, seed=0):
    """-> dict(uniform=(points, labels), clustered=(points, labels)): n half-pixel points uniform on a square of `extent` px with uniform
    labels, and n in 400 Gaussian clumps (sigma 300 px) on the same square with labels skewed 60 / 25 / 10 / 4 / 1 %."""
    rng = np.random.default_rng(seed)
    uniform = (rng.integers(0, 2 * extent, (n, 2)).astype(np.int32), rng.integers(0, C, n).astype(np.int32))
    centre = rng.uniform(0, 2 * extent, (400, 2))
    p = centre[rng.integers(0, 400, n)] + rng.normal(0, 2 * 300, (n, 2))
    p = np.clip(np.rint(p), 0, 2 * extent - 1).astype(np.int32)
    share = np.array([60, 25, 10, 4, 1][:C], np.float64) if C <= 5 else np.ones(C)
    lab = rng.choice(C, n, p=share / share.sum()).astype(np.int32)
    return dict(uniform=uniform, clustered=(p, lab))


def parser(n=500000, extent=36000, check_n=True):
    """The arguments every tool takes; the tool adds its own."""
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=n)
    ap.add_argument('--extent', type=int, default=extent, help='side of the square the centres are drawn on, px')
    ap.add_argument('--classes', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    if check_n:
        ap.add_argument('--check-n', type=int, default=3000, dest='check_n', help='about how many points the brute-force check takes')
    return ap


def need_gpu(tool):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f'{tool} needs a GPU (there is no fallback)')


def resident(pts, lab):
    """-> (device 0, the bounds of the points, the points and the labels on the device)."""
    import torch
    from nuhtc_amd import cellpoints
    dev = torch.device('cuda', 0)
    return dev, cellpoints.bounds_of(pts), torch.from_numpy(pts).to(dev), torch.from_numpy(lab).to(dev)


def timed(fn, repeats, warmup):
    """ms of `repeats` calls of fn, each between two events, after `warmup` calls; fn returns the library's code."""
    import torch
    ms = []
    for i in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        torch.cuda.synchronize()
        if rc:
            raise SystemExit(f'the device call failed ({rc})')
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms


def stage_split(fn, prefix):
    """One more call under the library's per-kernel profile (events around each stage) -> {tag: ms} of the tags that start with `prefix`."""
    from nuhtc_amd import hip
    hip.profile_enable(True)
    fn()
    stages = {tag: round(v['ms'], 3) for tag, v in hip.profile_read().items() if tag.startswith(prefix)}
    hip.profile_enable(False)
    return stages


def end_to_end(build):
    """Three calls of `build` (numpy to numpy) by the wall clock -> (ms, what the last one returned)."""
    e2e = []
    for i in range(3):
        t0 = time.perf_counter()
        got = build()
        e2e.append(1e3 * (time.perf_counter() - t0))
    return e2e, got


def brute_window(pts, bounds, extent, check_n):
    """-> bool (n,): the points of a corner square small enough for brute force, about check_n of them, at most twice that."""
    lo = np.array([bounds[0], bounds[1]])
    side = int(2 * extent * np.sqrt(min(1.0, check_n / max(len(pts), 1))))
    win = ((pts - lo) < side).all(1)
    if win.sum() > 2 * check_n:                               # a dense corner of the clustered set
        win &= np.cumsum(win) <= 2 * check_n
    return win


def graph_yardstick(p_d, l_d, C, r, bounds, args):
    """ms of nuhtc_cell_graph (k 8) on the same resident points at radius r half pixels, timed the same way."""
    import torch
    from nuhtc_amd import cellgraph
    gout = [torch.full((len(p_d), w), -1, dtype=torch.int32, device=p_d.device) for w in (8, 8, C)]
    return timed(lambda: cellgraph.call(p_d, l_d, C, r, 8, *gout, bounds=bounds), args.repeats, args.warmup)


def device_columns(ms, stages, e2e, same):
    return dict(device_ms=[round(v, 3) for v in ms], device_ms_median=round(med(ms), 3), device_stage_ms=stages,
                device_end_to_end_ms=[round(v, 2) for v in e2e], device_end_to_end_ms_median=round(med(e2e), 2), device_calls_agree=same)


def graph_columns(gms, ms=None):
    """The yardstick's columns, with the device call over it when `ms` is given."""
    over = dict(device_over_graph=round(med(ms) / med(gms), 2)) if ms is not None else {}
    return dict(graph_ms=[round(v, 3) for v in gms], graph_ms_median=round(med(gms), 3), **over)


def also_builds(specs, entry):
    """--also LABEL=LIB ... -> {label: the entry point `entry` of that build of the library, typed like the shipped one}."""
    import ctypes
    from nuhtc_amd import hip
    shipped = getattr(hip.load(), entry)
    also = {}
    for spec in specs:
        label, path = spec.split('=', 1)
        fn = getattr(ctypes.CDLL(os.path.abspath(path)), entry)
        fn.argtypes, fn.restype = shipped.argtypes, shipped.restype
        also[label] = fn
    return also


def also_arguments(ap):
    ap.add_argument('--also', action='append', default=[], metavar='LABEL=LIB', help='another build of the library to time in alternating rounds')
    ap.add_argument('--rounds', type=int, default=2, help='alternating rounds of the shipped library and the --also builds')


def raw(dev):
    """-> (vp, stream): a tensor as the void pointer, and the device's current stream, for a call into an --also build."""
    import ctypes
    import torch
    return (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def alternating_rounds(calls, repeats, rounds):
    """{label: call} -> {label: [median ms of `repeats` calls after one warm-up call, per round]}, the labels taking turns in every round."""
    out = {label: [] for label in calls}
    for _ in range(rounds):
        for label, call in calls.items():
            out[label].append(round(med(timed(call, repeats, 1)), 3))
    return out


def variants(shipped, others, equals, args):
    """The --also builds beside the shipped one: others = {label: call}, each called once and compared (equals(label) -> whether its outputs
    are the shipped ones), then `--rounds` alternating rounds of all of them -> {label: dict(equals_shipped, ms), 'shipped': dict(ms)}, or
    {} without --also."""
    import torch
    if not others:
        return {}
    out, calls = {}, {'shipped': shipped}
    for label, call in others.items():
        if call():
            raise SystemExit(f'{label}: the device call failed')
        torch.cuda.synchronize()
        out[label] = dict(equals_shipped=bool(equals(label)))
        calls[label] = call
    out['shipped'] = {}
    for label, ms in alternating_rounds(calls, args.repeats, args.rounds).items():
        out[label]['ms'] = ms
    return out


def tensors_equal(a, b):
    """Two lists of output tensors made with the same shapes and fill: bitwise the same (the rows no call writes included)."""
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


def all_equal_shipped(sets):
    return all(v.get('equals_shipped', True) for s in sets for v in s['variants'].values())


def grown(call, make_outputs, first_cap):
    """The capacity protocol of an edge-list call, for a tool: call(cap, out) -> (rc, m, ...) at first_cap, and when m > cap once more with
    room for exactly m -> (cap, out, what the last call returned)."""
    import torch
    cap, out = first_cap, make_outputs(first_cap)
    got = call(cap, out)
    if got[0]:
        raise SystemExit('the device call failed')
    torch.cuda.synchronize()
    if got[1] > cap:                                          # the first guess was too small: the timed calls have room for exactly m
        cap, out, m = got[1], make_outputs(got[1]), got[1]
        got = call(cap, out)
        if got[0] or got[1] != m:
            raise SystemExit('the second device call failed')
        torch.cuda.synchronize()
    return cap, out, got


def repeating(shipped, out, result):
    """Clones `out` as the FIRST result -> (first, checked, repeated): checked() is shipped() followed by a bitwise compare of `out` and
    result() with the first; repeated() says whether every checked call so far repeated it."""
    import torch
    first, first_result, ok = [t.clone() for t in out], result(), [True]

    def checked():
        rc = shipped()
        torch.cuda.synchronize()
        ok[0] = ok[0] and result() == first_result and tensors_equal(out, first)
        return rc
    return first, checked, lambda: ok[0]


def report(line, checks, more=()):
    """Prints the ONE JSON line; SystemExit when a set misses one of the `checks` it holds, or one of more = ((name, ok), ..) is not ok."""
    print(json.dumps(line))
    if not (all(s.get(c, True) for s in line['sets'] for c in checks) and all(ok for _, ok in more)):
        raise SystemExit('a check failed: see ' + ' / '.join(tuple(checks) + tuple(name for name, _ in more)))
