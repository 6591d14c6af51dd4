#!/usr/bin/env python
"""Run the engine over a PanNuke-format fold and score / export it, with the scoring on the device.

    python tools/eval_pannuke.py <config> <checkpoint> --images fold/images.npy [--masks fold/masks.npy --types fold/types.npy]
                                 [--out infer/pannuke] [--batch 16] [--format pannuke|conic|consep] [--eval-on host|gpu]
                                 [--t-cap N --trip-cap N --joint-cap N]

The arguments, the input format and the files written are those of tools/test_pannuke.py (preds_<format>.npy, confusion_matrix.npy,
summary.json, class_stats.csv, tissue_stats.csv): the same replacement of the reference's `tools/test.py --eval segm` +
analysis_tools/pannuke/compute_stats.py.

--eval-on host (default) IS tools/test_pannuke.py: every mask is fetched (`Engine.results`) and scored with the mask functions of
nuhtc_amd.evaluation.
--eval-on gpu scores each batch on the device right behind the inference (`Engine.eval_async`: score filter, mask-NMS, pair tables,
label maps, joint histograms) and finishes from the integer tables with the *_tables twins: the same files and numbers, no mask
reaches the host.  A batch whose tables outgrow their capacity is scored through its masks with the host functions; how many batches
went which way is reported on stderr.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_pannuke as host_tool  # noqa: E402
from nuhtc_amd import evaluation as E  # noqa: E402
from nuhtc_amd.apis import concat_results, init_detector  # noqa: E402


def parse_args(argv=None):
    """This tool's own options; every other argument is tools/test_pannuke.py's and is parsed by its parser.  -> (namespace, the rest)."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument('--eval-on', default='host', choices=['host', 'gpu'], help='where the batches are scored (same outputs)')
    p.add_argument('--t-cap', type=int, default=0, help='gpu: ground-truth instances per image the device tables hold (default: the most the fold has)')
    p.add_argument('--trip-cap', type=int, default=None, help='gpu: pair entries per batch (default: Engine.eval_async)')
    p.add_argument('--joint-cap', type=int, default=None, help='gpu: joint-histogram entries per batch (default: Engine.eval_async)')
    own, rest = p.parse_known_args(argv)
    return own, rest


def host_args(rest):
    """`rest` through the parser of tools/test_pannuke.py (which reads sys.argv)."""
    keep = sys.argv
    sys.argv = [keep[0]] + list(rest)
    try:
        return host_tool.parse_args()
    finally:
        sys.argv = keep


class Scores:
    """What the loop accumulates per image, from the device tables or -- for a batch over their capacity -- from the masks."""

    def __init__(self, nc):
        self.nc = nc
        self.preds, self.stats, self.mpq_info, self.joint = [], {}, [], []
        self.cm = np.zeros((nc + 1, nc + 1))

    def add_stat(self, s):
        if s:
            for key, v in s.items():
                self.stats.setdefault(key, []).append(v)

    def mask_image(self, res, mask, a, H, W):
        boxes, labels, pm = concat_results(res)
        sel = boxes[:, 4] >= a.fg_thr
        boxes, labels, pm = boxes[sel], labels[sel], (pm[sel] if len(pm) else np.zeros((0, H, W), bool))
        if len(pm):
            pm, keep = E.mask_nms(pm, boxes[:, 4], thr=a.mask_nms_thr)
            labels = labels[keep]
        self.preds.append(E.convert_format(pm, labels, H, W, self.nc, a.format))
        if mask is not None:
            tm, tl = host_tool.gt_instances(mask, self.nc)
            self.add_stat(E.stat_calc(tm, pm))
            self.mpq_info.append(E.multi_stat_calc(tm, pm, tl, labels, self.nc))
            E.update_confusion_matrix(self.cm, tm, pm, tl, labels)
            if a.format == 'pannuke':
                self.joint.append(E.joint_tables(mask, self.preds[-1], self.nc))

    def table_image(self, r, k, gt, a):
        """Image k of a batch Engine.eval_read returned; gt = (labels, n_t) of evaluation.gt_rows or None."""
        labels = r['labels'][k]
        if a.format == 'consep':         # (never written: the centroids of `convert_format` need the masks)
            self.preds.append({'inst_map': r['maps'][k, :, :, 0].astype(int), 'inst_type': r['maps'][k, :, :, 1].astype(int)})
        else:
            self.preds.append(r['maps'][k].astype(int))
        if gt is not None:
            tl, n_t = gt
            inter = E.dense_pairs(n_t, len(labels), *r['pairs'][k])
            at, ap = r['area_t'][k, :n_t], r['area_p'][k]
            self.add_stat(E.stat_calc_tables(inter, at, ap))
            self.mpq_info.append(E.multi_stat_calc_tables(inter, at, ap, tl, labels, self.nc))
            E.update_confusion_matrix_tables(self.cm, inter, at, ap, tl, labels)
            if a.format == 'pannuke':
                self.joint.append(r['joint'][k])


def main(argv=None):
    own, rest = parse_args(argv)
    if own.eval_on == 'host':          # tools/test_pannuke.py as it is
        keep = sys.argv
        sys.argv = [keep[0]] + rest
        try:
            return host_tool.main()
        finally:
            sys.argv = keep
    a = host_args(rest)
    import torch
    from nuhtc_amd import hip
    images = np.load(a.images)
    if images.dtype != np.uint8:
        images = np.clip(images, 0, 255).astype(np.uint8)
    masks = np.load(a.masks) if a.masks else None
    types = np.load(a.types) if a.types else None
    model = init_detector(a.config, a.checkpoint, device=a.device, max_batch=a.batch)
    nc = int(model.opts['num_classes'])
    os.makedirs(a.out, exist_ok=True)
    N, H, W = images.shape[:3]
    sc = Scores(nc)
    eng = model.engine((H, W))
    gt = [E.gt_rows(masks[i], nc) for i in range(N)] if masks is not None else None      # once per fold, independent of the model
    t_cap = max([own.t_cap, 1] + [g[2] for g in gt]) if gt else max(own.t_cap, 1)
    batches = fallback = 0
    pad = eng.cfg.tile_w - W
    for i0 in range(0, N, a.batch):
        # the channel handling of tools/test_pannuke.py: RGB arrays reversed, then the ndarray ("BGR") branch of inference_detector
        batch = np.stack([np.ascontiguousarray(images[i][..., ::-1]) for i in range(i0, min(N, i0 + a.batch))])
        with torch.cuda.stream(eng.stream):
            B = eng.infer_async(eng.to_device(batch), hip.CH_SWAP)
            g = None
            if gt is not None:
                g = np.stack([np.pad(gt[i0 + k][0], ((0, 0), (0, pad), (0, 0))) for k in range(B)])
                g = torch.from_numpy(g).to(eng.device, non_blocking=True)
            eng.eval_async(B, g, t_cap=t_cap, fg_thr=a.fg_thr, mask_nms_thr=a.mask_nms_thr, trip_cap=own.trip_cap, joint_cap=own.joint_cap,
                           data_format='pannuke' if a.format == 'pannuke' else 'conic')
            eng.check()               # waits for the stream; raises when the connected-component proposals overflowed
            r = eng.eval_read()
            batches += 1
            if r['overflow']:         # tables over their capacity: this batch through its masks (still on the device)
                fallback += 1
                for k, res in enumerate(eng.results(B)):
                    sc.mask_image(res, masks[i0 + k] if masks is not None else None, a, H, W)
                continue
        for k in range(B):
            sc.table_image(r, k, gt[i0 + k][1:] if gt is not None else None, a)
    print(f'eval_pannuke: {batches - fallback} of {batches} batches scored from device tables, {fallback} through their masks'
          + (' (tables over capacity: raise --t-cap / --trip-cap / --joint-cap)' if fallback else ''), file=sys.stderr)
    # from here on: the writers of tools/test_pannuke.py, fed from the tables
    if a.format != 'consep':
        np.save(os.path.join(a.out, f'preds_{a.format}.npy'), np.array(sc.preds))
    summary = {}
    if masks is not None:
        summary.update({k: float(np.mean(v)) for k, v in sc.stats.items() if k not in ('tp', 'fp', 'fn', 'iou')})
        summary.update({k: float(v) for k, v in E.aggregate_mpq(sc.mpq_info).items()})
        np.save(os.path.join(a.out, 'confusion_matrix.npy'), sc.cm)
        if a.format == 'pannuke' and types is not None:
            r = E.pannuke_stats_tables(sc.joint, list(types), num_classes=nc)
            summary['mPQ'], summary['bPQ'] = float(r['mPQ']), float(r['bPQ'])
            with open(os.path.join(a.out, 'class_stats.csv'), 'w', newline='') as f:
                w = csv.writer(f)
                w.writerow(['', 'Class Name', 'PQ'])
                for j, (n, v) in enumerate(zip(['Neoplastic', 'Inflam', 'Connective', 'Dead', 'Non-Neoplastic'], r['class_pq'])):
                    w.writerow([j, n, v])
            with open(os.path.join(a.out, 'tissue_stats.csv'), 'w', newline='') as f:
                w = csv.writer(f)
                w.writerow(['', 'Tissue name', 'PQ', 'PQ bin'])
                for j, n in enumerate(E.PANNUKE_TISSUES):
                    w.writerow([j, n, r['tissue_mpq'][n], r['tissue_bpq'][n]])
                w.writerow([len(E.PANNUKE_TISSUES), 'mean', r['mPQ'], r['bPQ']])
    with open(os.path.join(a.out, 'summary.json'), 'w') as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == '__main__':
    main()
