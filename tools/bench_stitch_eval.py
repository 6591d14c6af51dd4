#!/usr/bin/env python
"""Benchmark of the stitched-tile evaluation (tools/eval_consep.py), host route against device route -- prints ONE JSON line.

    python tools/bench_stitch_eval.py [--images 2] [--grid 9] [--tile 256] [--stride 93] [--batch 16] [--gt 600]

Synthetic images (nuhtc_amd.synth.nuclei_canvas: a `grid` x `grid` tiling of `tile`-pixel tiles at `stride`, 1000 x 1000 by default like
CoNSeP) with a synthetic ground truth of `--gt` rectangles, four classes, the engine's default detection limits, seeded synthetic weights.
  host route    the loop of --eval-on host: per batch the inference, `Engine.results` (every mask to the host), the candidate rules and
                crops; then per image the mask-NMS, pair tables and label maps on crops (nuhtc_amd.stitch)
  device route  the loop of --eval-on gpu: inference and gather per batch without synchronising, then per image the records to the host,
                nuhtc_merge_overlap, pairs and render on the device
Both routes then finish with the same *_tables functions (timed as `metrics`).  Kept indices, tables and maps of the two routes must be
equal; the tool exits non-zero when they are not.  bench.py (the detection path) is the project's headline benchmark and is not changed
by this tool."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=2)
    ap.add_argument('--grid', type=int, default=9)
    ap.add_argument('--tile', type=int, default=256)
    ap.add_argument('--stride', type=int, default=93)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--gt', type=int, default=600, help='ground-truth rectangles per image')
    args = ap.parse_args(argv)
    import torch
    import eval_consep
    from nuhtc_amd import hip, synth, weights
    from nuhtc_amd import stitch as S
    from nuhtc_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit('bench_stitch_eval.py needs a GPU (there is no fallback)')
    P, side = args.tile, synth.canvas_side(args.grid, args.stride, args.tile)
    a = eval_consep.parse_args(['cfg', 'ck', '--data', 'x', '--tile', str(P), '--stride', str(args.stride), '--batch', str(args.batch), '--save'])
    eng = Engine(weights.bench_state_dict(0, num_classes=4, obj_bias=0.0), device=0, max_batch=args.batch, tile=(P, P), num_classes=4)
    grid = S.tile_grid(side, side, P, args.stride)
    images, gts = [], []
    for i in range(args.images):
        band = synth.nuclei_canvas(args.grid, step=args.stride, size=P, mean_count=60 + 7 * i)
        images.append(np.ascontiguousarray(np.asarray(band[0] if isinstance(band, tuple) else band)[:side, :side, :3]).astype(np.uint8))
        rng = np.random.RandomState(100 + i)
        inst = np.zeros((side, side), np.int32)
        for k in range(args.gt):
            y, x = rng.randint(0, side - 20, 2)
            inst[y:y + rng.randint(8, 20), x:x + rng.randint(8, 20)] = k + 1
        gts.append(S.gt_from_mat(inst, rng.randint(1, 8, args.gt)))
    store = eng.stitch_store(1, len(grid) * eng.cfg.max_per_img, a.pool_cap)
    eval_consep.device_image(eng, store, images[0], grid, gts[0], a, hip)          # warm-up of both loops' kernels
    t = dict(host=dict(infer_fetch_crop=0.0, nms_tables_maps=0.0), device=dict(infer_gather_nms_tables_maps=0.0), metrics=0.0)
    equal, n_cand, n_kept, fallback = True, [], [], 0
    for img, gt in zip(images, gts):
        t0 = time.perf_counter()
        c = eval_consep.host_image(eng, img, grid, a, hip)
        t1 = time.perf_counter()
        h = S.score_image_host(c, gt, side, side, a.mask_nms_thr, want_maps=True)
        t2 = time.perf_counter()
        d = eval_consep.device_image(eng, store, img, grid, gt, a, hip)
        t3 = time.perf_counter()
        t['host']['infer_fetch_crop'] += t1 - t0
        t['host']['nms_tables_maps'] += t2 - t1
        t['device']['infer_gather_nms_tables_maps'] += t3 - t2
        n_cand.append(len(c))
        n_kept.append(len(h['kept']))
        if d is None:
            fallback += 1
            equal = False
            continue
        equal &= all(np.array_equal(h[k], d[k]) for k in ('kept', 'labels', 'box', 'inter', 'area_t', 'area_p', 'inst_map', 'type_map'))
        t0 = time.perf_counter()
        fs = S.FoldScores(4)
        fs.add('x', d['inter'], d['area_t'], d['area_p'], gt[1], d['labels'])
        t['metrics'] += time.perf_counter() - t0
    host_s = sum(t['host'].values())
    dev_s = t['device']['infer_gather_nms_tables_maps']
    out = dict(what=f'tools/bench_stitch_eval.py: {args.images} synthetic {side} x {side} images, {len(grid)} tiles of {P} px at stride {args.stride} each, batch '
                    f'{args.batch}, seeded synthetic weights, {args.gt} ground-truth rectangles per image; each route once per image after one warm-up image, one MI355X',
               images=args.images, tiles_per_image=len(grid), candidates=n_cand, kept=n_kept,
               host_s={k: round(v, 4) for k, v in t['host'].items()}, device_s={k: round(v, 4) for k, v in t['device'].items()},
               metrics_s=round(t['metrics'], 4), host_s_per_image=round(host_s / args.images, 4), device_s_per_image=round(dev_s / args.images, 4),
               host_over_device=round(host_s / dev_s, 2), fallback=fallback, routes_equal=bool(equal))
    print(json.dumps(out))
    if not equal:
        raise SystemExit('device route differs from the host route')


if __name__ == '__main__':
    main()
