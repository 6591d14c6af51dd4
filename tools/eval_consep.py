#!/usr/bin/env python
"""Run the engine over a CoNSeP-format fold -- images larger than a tile -- and score it as the reference's
`CoNSePCocoDataset.evaluate` does (nuhtc/datasets/WSI_coco_CoNSeP.py:117-426).

    python tools/eval_consep.py <config> <checkpoint> --data <fold dir> [--out infer/consep] [--batch 16] [--tile 256] [--stride 93]
                                [--fg-thr 0.1] [--discard-offset 4] [--mask-nms-thr 0.02] [--save] [--eval-on host|gpu]
                                [--cand-cap N --pool-cap N --trip-cap N]

<fold dir>/Images/<name>.png and <fold dir>/Labels/<name>.mat (inst_map, inst_type); all images of a fold have one size and
(size - tile) / stride is a whole number on both axes (CoNSeP: 1000 x 1000, a 9 x 9 grid of 256-pixel tiles at stride 93).  Every image
is cut into its tiles, detections close to an inner tile edge are dropped, the rest are shifted into the image frame, one mask-NMS runs
over all candidates of the image and the survivors are scored against the ground truth: AJI, AJI+, DQ, SQ, PQ, Dice per image, the
multi-class PQ and the confusion matrix over the fold.  Written: summary.json, confusion_matrix.npy, a line per image on stdout and,
with --save, <out>/<name>.mat (inst_map, inst_type, inst_centroid, inst_uid).  The reference's overlay images and wandb logging are not
reproduced.

--eval-on host (default): the masks of every tile are fetched (`Engine.results`) and scored by nuhtc_amd.stitch on crops.
--eval-on gpu: candidates are gathered on the device right behind the inference (`Engine.stitch_gather_async`), the image-level
mask-NMS, the pair tables and the label maps are built there, and the host finishes from the integer tables: the same files, no mask
reaches the host.  An image whose tables outgrow --cand-cap / --pool-cap / --trip-cap (or that holds more than 8192 ground-truth
instances, or a prediction over more than 64 of them) is scored by the host route; stderr reports how many images went which way.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nuhtc_amd import evaluation as E  # noqa: E402
from nuhtc_amd import stitch as S  # noqa: E402
from nuhtc_amd.apis import init_detector  # noqa: E402

MAX_T_CAP = 8192          # ST_MAX_TCAP of csrc/stitch.hip


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('config')
    p.add_argument('checkpoint')
    p.add_argument('--data', required=True, help='fold directory holding Images/ and Labels/')
    p.add_argument('--out', default='infer/consep')
    p.add_argument('--batch', type=int, default=16)
    p.add_argument('--tile', type=int, default=256)
    p.add_argument('--stride', type=int, default=93)
    p.add_argument('--fg-thr', type=float, default=0.1, dest='fg_thr')
    p.add_argument('--discard-offset', type=float, default=4, dest='discard_offset')
    p.add_argument('--mask-nms-thr', type=float, default=0.02, dest='mask_nms_thr')
    p.add_argument('--save', action='store_true', help='write <out>/<name>.mat per image')
    p.add_argument('--eval-on', default='host', choices=['host', 'gpu'], dest='eval_on', help='where the images are scored (same outputs)')
    p.add_argument('--cand-cap', type=int, default=0, dest='cand_cap', help='gpu: candidates per image (default: tiles x max_per_img, the most there can be)')
    p.add_argument('--pool-cap', type=int, default=1 << 22, dest='pool_cap', help='gpu: 32-bit words of mask crops per image')
    p.add_argument('--trip-cap', type=int, default=1 << 16, dest='trip_cap', help='gpu: (ground truth, prediction) pairs per image')
    p.add_argument('--device', default='cuda:0')
    return p.parse_args(argv)


def tile_batches(image, grid, tile, batch):
    """-> (tile records, (n, tile, tile, 3) uint8) per batch of an image's tiles, row-major."""
    for i0 in range(0, len(grid), batch):
        ts = grid[i0:i0 + batch]
        yield ts, np.stack([image[t['oy']:t['oy'] + tile, t['ox']:t['ox'] + tile] for t in ts])


def host_image(eng, image, grid, a, hip):
    """The host route's candidates of one image: every tile's masks fetched."""
    import torch
    c = S.Candidates()
    for ts, tiles in tile_batches(image, grid, a.tile, a.batch):
        with torch.cuda.stream(eng.stream):
            B = eng.infer_async(eng.to_device(tiles), hip.CH_AS_IS)          # an RGB file: the network sees true RGB (tools/infer.py)
            for t, res in zip(ts, eng.results(B)):
                S.add_tile(c, res, t, a.tile, a.fg_thr, a.discard_offset)
    return c.freeze()


def device_image(eng, store, image, grid, gt, a, hip):
    """The device route for one image -> the dictionary of stitch.score_image_host, or None when a table outgrew its capacity."""
    import torch
    gt_map, _, n_t = gt
    H, W = gt_map.shape
    with torch.cuda.stream(eng.stream):
        eng.stitch_reset(store)
        for ts, tiles in tile_batches(image, grid, a.tile, a.batch):
            B = eng.infer_async(eng.to_device(tiles), hip.CH_AS_IS)
            meta = torch.tensor([S.tile_meta(0, t) for t in ts], dtype=torch.int32).to(eng.device, non_blocking=True)
            eng.stitch_gather_async(B, meta, store, a.fg_thr, a.discard_offset)
        eng.check()               # waits for the stream; raises when the connected-component proposals overflowed
        rec = eng.stitch_read(store, 0)
        if rec['overflow'] or n_t > MAX_T_CAP:
            return None
        kept = eng.stitch_nms(store, 0, rec, a.mask_nms_thr, H, W)
        r = eng.stitch_pairs(store, 0, rec, kept, torch.from_numpy(np.ascontiguousarray(gt_map)).to(eng.device), max(n_t, 1), a.trip_cap)
        if r['overflow']:
            return None
        out = dict(kept=kept, labels=rec['label'][kept], box=rec['box'][kept], inter=E.dense_pairs(n_t, len(kept), *r['pairs']),
                   area_t=r['area_t'][:n_t].astype(np.float64), area_p=rec['area'][kept].astype(np.float64))
        if a.save:
            inst, typ = eng.stitch_render(store, 0, rec, kept, H, W)
            out['inst_map'], out['type_map'] = inst.cpu().numpy(), typ.cpu().numpy()
    return out


def main(argv=None):
    a = parse_args(argv)
    from nuhtc_amd import hip
    names, images, gts = S.load_fold(a.data)
    if not names:
        raise SystemExit(f'eval_consep: no Labels/*.mat under {a.data}')
    H, W = images[names[0]].shape[:2]
    for n in names:
        if images[n].shape[:2] != (H, W) or gts[n][0].shape != (H, W):
            raise SystemExit(f'eval_consep: {n} is not {H} x {W} like the rest of the fold (or its inst_map is not)')
    try:
        grid = S.tile_grid(H, W, a.tile, a.stride)
    except ValueError as e:
        raise SystemExit(f'eval_consep: {e}')
    model = init_detector(a.config, a.checkpoint, device=a.device, max_batch=a.batch)
    nc = int(model.opts['num_classes'])
    eng = model.engine((a.tile, a.tile))
    os.makedirs(a.out, exist_ok=True)
    fs = S.FoldScores(nc)
    store = None
    if a.eval_on == 'gpu':
        store = eng.stitch_store(1, a.cand_cap or len(grid) * eng.cfg.max_per_img, a.pool_cap)
    on_device = fallback = 0
    for name in names:
        gt = gts[name]
        r = device_image(eng, store, images[name], grid, gt, a, hip) if store is not None else None
        if r is None:
            fallback += store is not None
            r = S.score_image_host(host_image(eng, images[name], grid, a, hip), gt, H, W, a.mask_nms_thr, want_maps=a.save)
        else:
            on_device += 1
        print(fs.add(name, r['inter'], r['area_t'], r['area_p'], gt[1], r['labels']))
        if a.save:
            import scipy.io as sio
            sio.savemat(os.path.join(a.out, f'{name}.mat'), S.pred_mat(r['inst_map'], r['labels'], r['box']))
    if store is not None:
        print(f'eval_consep: {on_device} of {len(names)} images scored from device tables, {fallback} through their masks'
              + (' (tables over capacity: raise --cand-cap / --pool-cap / --trip-cap)' if fallback else ''), file=sys.stderr)
    summary = fs.summary()
    np.save(os.path.join(a.out, 'confusion_matrix.npy'), fs.cm)
    with open(os.path.join(a.out, 'summary.json'), 'w') as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == '__main__':
    main()
