#!/usr/bin/env python
"""Benchmark of tissue segmentation and tile selection, host route against device route -- prints ONE JSON line.

    python tools/bench_tissue.py [--height 1200] [--width 1500] [--scale 64] [--step 192] [--patch 256] [--repeats 5] [--skip-host]

A synthetic segmentation level (noisy tissue blobs with holes on glass; `--scale` is its downsample, so the slide is height x scale by width x
scale pixels) goes through `segment_tissue` and, per tissue contour, `contour_coords`:
  host route    once (numpy / scipy: the code of nuhtc_amd/tissue.py without `device`)
  device route  `--repeats` times after one warm-up, upload and read-back included (csrc/tissue.hip)
and the two tile lists, contours and holes must be equal.  Stages: `mask` = saturation, median, threshold and close alone; `segment_tissue` = mask
+ border following + area filter (the latter two are host code on both routes); `contour_coords` = all contours' grids.
bench.py (the detection path) is the project's headline benchmark and is not changed by this tool."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def level_image(H, W, seed=0):
    """Glass with one large tissue region, two smaller ones and holes, ragged outlines, H&E-like colours with pixel noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    wob = np.kron(rng.normal(0, 0.05, (-(-H // 25), -(-W // 25))), np.ones((25, 25), np.float32))[:H, :W]
    ell = lambda cy, cx, ry, rx: ((yy - cy * H) / (ry * H)) ** 2 + ((xx - cx * W) / (rx * W)) ** 2 + wob <= 1
    tissue = ell(0.5, 0.42, 0.46, 0.38) | ell(0.3, 0.9, 0.2, 0.07) | ell(0.8, 0.9, 0.12, 0.06)
    for cy, cx, r in ((0.35, 0.3, 0.06), (0.6, 0.5, 0.09), (0.5, 0.2, 0.03), (0.75, 0.35, 0.04)):
        tissue &= ~ell(cy, cx, r, r * H / W)
    tissue ^= rng.random((H, W)) < 0.03                     # specks and pinholes for the median and the close
    img = np.where(tissue[..., None], np.array([200, 120, 180]), np.array([235, 233, 236])).astype(np.int64)
    return np.clip(img - rng.integers(0, 10, img.shape), 0, 255).astype(np.uint8)


def route(lv, args, device):
    """(seconds per stage, (coords, contours, holes)) of one pass."""
    from nuhtc_amd import tissue as T
    H, W = lv.shape[:2]
    wh = (W * args.scale, H * args.scale)
    t = {}
    t0 = time.perf_counter()
    if device is None:
        sat = T.saturation_u8(lv)
        binary = np.where(T.median_blur(sat, 7) > 8, np.uint8(255), np.uint8(0))
        T.morph_close(binary, 4)
    else:
        T.tissue_mask_device(lv, device=device)
    t['mask'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    conts, holes = T.segment_tissue(None, scale=float(args.scale), level_image=lv, device=device)
    t['segment_tissue'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    parts = [T.contour_coords(c, h, wh, args.patch, args.step, 'four_pt', True, device=device) for c, h in zip(conts, holes)]
    t['contour_coords'] = time.perf_counter() - t0
    coords = np.concatenate(parts, 0) if parts else np.zeros((0, 2), np.int64)
    return t, (coords, conts, holes)


def same(a, b):
    return (np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
            and [len(h) for h in a[2]] == [len(h) for h in b[2]] and all(np.array_equal(x, y) for p, q in zip(a[2], b[2]) for x, y in zip(p, q)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=1200)
    ap.add_argument('--width', type=int, default=1500)
    ap.add_argument('--scale', type=int, default=64)
    ap.add_argument('--step', type=int, default=192)
    ap.add_argument('--patch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--skip-host', action='store_true', help='device route only (no equality check, no ratios)')
    args = ap.parse_args(argv)
    import torch
    from nuhtc_amd import hip, tissue as T
    if not torch.cuda.is_available():
        raise SystemExit('bench_tissue.py needs a GPU (there is no fallback)')
    lv = level_image(args.height, args.width)
    probe = hip.ClockProbe(0)
    probe.start(20)
    clock = [probe.ghz()]
    route(lv, args, 0)                                       # warm-up: code objects, allocator
    runs = [route(lv, args, 0) for _ in range(args.repeats)]
    probe.start(20)
    clock.append(probe.ghz())
    dev_t = {k: [round(r[0][k], 5) for r in runs] for k in runs[0][0]}
    coords, conts, holes = runs[-1][1]
    out = dict(what='tools/bench_tissue.py: segment_tissue + contour_coords on a synthetic segmentation level, host route once, device route '
                    f'{args.repeats} times after one warm-up (upload and read-back included), one MI355X',
               level=[args.height, args.width], scale=args.scale, step=args.step, patch=args.patch,
               contours=len(conts), holes=int(sum(len(h) for h in holes)), contour_vertices=[int(len(c)) for c in conts],
               candidates=int(sum(len(np.arange(x, x + w, args.step)) * len(np.arange(y, y + h, args.step)) for x, y, w, h in map(T.bounding_rect, conts))),
               tiles=int(len(coords)), device_s=dev_t, device_s_median={k: float(np.median(v)) for k, v in dev_t.items()},
               shader_clock_ghz_one_wave_probe_before_after=[None if c is None else round(c, 3) for c in clock],
               clock_note='one-wave spin probe on an otherwise idle GPU before and after the device runs; no clock was set or pinned')
    if not args.skip_host:
        host_t, host_out = route(lv, args, None)
        out['host_s'] = {k: round(v, 4) for k, v in host_t.items()}
        out['host_over_device'] = {k: round(host_t[k] / out['device_s_median'][k], 1) for k in host_t}
        out['tile_lists_equal'] = bool(same(host_out, runs[-1][1]) and all(same(r[1], runs[-1][1]) for r in runs))
        if not out['tile_lists_equal']:
            print(json.dumps(out))
            raise SystemExit('device route differs from the host route')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
