#!/usr/bin/env python
"""Cost of the per-nucleus table from a written GeoJSON (nuhtc_amd/ringfeat.py, csrc/ringfeat.hip) -- prints ONE JSON line
(profiles/ring_features.json).

    python tools/bench_ringfeat.py [--grid 11] [--nuclei 20000] [--block 2048] [--repeats 3] [--warmup 1]

A synthetic slide (nuhtc_amd.synth.nuclei_canvas, saved as a memory-mapped .npy so that the read is a read) and a slide's worth of
traced rings: ellipses with the canvas's own semi-axes (5 .. 12 px), traced by contours.trace_outer_contour and put at random places.
  stage_ms_*        ringfeat.measure() over the whole slide, `--repeats` times after `--warmup`, the median: the wall-clock time of each
                    stage of the block walk with the device synchronised behind it (read, upload, gather, fill, measure = the two
                    measurement ops), then derive (ringfeat.table) and write (write_db into a fresh file)
  kernel_ms_*       one chunk of 4096 frames of side 32 resident on the device, each step alone between two events, 10 times after 2:
                    nuhtc_op_frame_gather, nuhtc_op_ring_fill, the two measurement ops together
  host_fill_ms      contours.fill_rings (the host code that defines the pixel set) on the same rings, all threads it takes by default
bench.py (the detection path) is the project's headline benchmark and is not changed by this tool."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_rings(n, side, seed=0, shapes=48):
    """n traced rings (closed, slide pixels) inside a side x side slide: `shapes` distinct ellipses, each used at many places."""
    from nuhtc_amd import contours
    rng = np.random.default_rng(seed)
    base = []
    for _ in range(shapes):
        a, b, th = rng.uniform(5, 12), rng.uniform(5, 12), rng.uniform(0, np.pi)
        yy, xx = np.mgrid[-14:15, -14:15].astype(np.float64)
        u, v = xx * np.cos(th) + yy * np.sin(th), -xx * np.sin(th) + yy * np.cos(th)
        r = contours.trace_outer_contour((u / a) ** 2 + (v / b) ** 2 <= 1.0)
        base.append(r - r.min(0))
    rings = []
    for k in range(n):
        r = base[k % shapes]
        at = rng.integers(0, side - r.max(0) - 1)
        rings.append(np.concatenate([r, r[:1]], 0) + at)
    return rings


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, default=11, help='tiles per side of the synthetic canvas (192-px step, 256-px tiles)')
    ap.add_argument('--nuclei', type=int, default=20000)
    ap.add_argument('--block', type=int, default=2048)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    args = ap.parse_args(argv)
    import torch
    from nuhtc_amd import contours, ringfeat, synth
    if not torch.cuda.is_available():
        raise SystemExit('bench_ringfeat.py needs a GPU (there is no fallback)')
    canvas, _ = synth.nuclei_canvas(args.grid)
    side = canvas.shape[0]
    rings = synthetic_rings(args.nuclei, side)
    feats = [contours.feature(r, k % 5, 0.5, ('T', 'I', 'C', 'D', 'E')) for k, r in enumerate(rings)]
    med = lambda v: float(np.median(v))
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, 's.npy'), canvas)
        slide = np.load(os.path.join(tmp, 's.npy'), mmap_mode='r')
        t0 = time.perf_counter()
        parsed = ringfeat.parse(feats)
        parse_ms = 1e3 * (time.perf_counter() - t0)
        stages = {k: [] for k in ('read', 'upload', 'gather', 'fill', 'measure', 'derive', 'write', 'total')}
        for rep in range(args.warmup + args.repeats):
            tm = {}
            t0 = time.perf_counter()
            m = ringfeat.measure(slide, parsed, device=0, block=args.block, timings=tm)
            total = time.perf_counter() - t0
            t0 = time.perf_counter()
            _, values = ringfeat.table(m)
            tm['derive'] = time.perf_counter() - t0
            t0 = time.perf_counter()
            ringfeat.write_db(os.path.join(tmp, f'run{rep}', ringfeat.DB_NAME), values, m['score'], m['type'], m['label'], m['nuclei_id'], m['rect'])
            tm['write'] = time.perf_counter() - t0
            tm['total'] = total + tm['derive'] + tm['write']
            if rep >= args.warmup:
                for k in stages:
                    stages[k].append(1e3 * tm[k])
        blocks, _ = ringfeat.block_plan(parsed['rect'], slide.shape[:2], args.block)
    # ---- the kernels alone: one chunk of side 32
    S = 32
    idx = np.nonzero(ringfeat.frame_sides(parsed['rect']) == S)[0][:ringfeat.CHUNK]
    kernels = {}
    with ringfeat._Ops(0) as ops:
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)
        verts, off = ringfeat.pack_rings([parsed['rings'][i] for i in idx])
        block, origin, verts_d, off_d = dev(canvas), dev(parsed['rect'][idx, :2].astype(np.int32)), dev(verts), dev(off)
        frames = ops.gather(block, 0, 0, origin, S)
        masks, status = ops.fill(verts_d, off_d, origin, S)
        fams = ringfeat.select()        # the families that are always selected

        def measure():                  # as one chunk of ringfeat.measure(): the pairs, then every family of the selection
            pairs = ops.pairs(len(idx))
            return [ops.run(fam, pairs, frames, masks) for fam in fams]
        calls = {'gather': lambda: ops.gather(block, 0, 0, origin, S), 'fill': lambda: ops.fill(verts_d, off_d, origin, S), 'measure': measure}
        for name, call in calls.items():
            ms = []
            for i in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                if i >= 2:
                    ms.append(e0.elapsed_time(e1))
            kernels[name] = ms
        # a number for code that computes something else is no number: the chunk's masks against the host fill
        got = np.unpackbits(masks.cpu().numpy().view(np.uint8), axis=-1, bitorder='little').astype(bool)
        boxes, areas, bits, woff = contours.fill_rings([parsed['rings'][i] for i in idx])
        exact = bool((status.cpu().numpy() == 0).all() and np.array_equal(got.sum((1, 2)), areas))
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        contours.fill_rings(parsed['rings'])
        host.append(1e3 * (time.perf_counter() - t0))
    n = len(m['raw'])
    out = dict(what=f'tools/bench_ringfeat.py: per-nucleus table of {args.nuclei} synthetic traced rings on a {side} x {side} synthetic slide (memory-mapped .npy), '
                    f'one MI355X; measure() {args.repeats} times after {args.warmup}, medians; kernels on one resident chunk of {len(idx)} frames of side {S}, 10 times after 2',
               slide_side=side, nuclei=args.nuclei, measured=n, left_out=m['left_out'], block=args.block, blocks_read=len(blocks),
               mean_area_px=round(float(m['raw'][:, 0].mean()), 1), parse_ms=round(parse_ms, 2),
               **{f'stage_ms_{k}': round(med(v), 3) for k, v in stages.items()}, stage_ms_runs={k: [round(x, 3) for x in v] for k, v in stages.items()},
               **{f'kernel_ms_{k}': round(med(v), 4) for k, v in kernels.items()}, kernel_chunk=len(idx),
               kernel_us_per_nucleus_fill=round(1e3 * med(kernels['fill']) / max(len(idx), 1), 4),
               host_fill_ms=round(med(host), 2), host_fill_us_per_nucleus=round(1e3 * med(host) / max(len(parsed['rings']), 1), 3),
               dominant_stage=max(('read', 'upload', 'gather', 'fill', 'measure', 'derive', 'write'), key=lambda k: med(stages[k])),
               chunk_areas_equal_the_host_fill=exact,
               note='stage times are wall-clock with a device synchronisation behind every stage (the walk itself does not synchronise between gather and fill); '
                    'the measure stage includes the synchronisation the two measurement ops do themselves')
    print(json.dumps(out))
    if not exact:
        raise SystemExit('the device fill differs from the host fill')


if __name__ == '__main__':
    main()
