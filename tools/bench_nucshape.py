#!/usr/bin/env python
"""Cost of the per-nucleus shape integers (csrc/nucshape.hip) -- prints ONE JSON line (profiles/nucleus_shape.json).

    python tools/bench_nucshape.py [--tile 256] [--batch 16] [--rounds 12]

Synthetic tiles (nuhtc_amd.synth), one batch resident on the device; one engine infers it once and exports its kept detections, and the
four per-nucleus ops -- nuhtc_op_nucleus_shape, nuhtc_op_nucleus_morph, nuhtc_op_nucleus_texture, nuhtc_op_nucleus_gradient -- run on
those masks (the engine's own, K slots a tile, the kept (tile, slot) pairs), taken in turn `--rounds` times, each call between two
events; the first two rounds are dropped.  All four scan one mask per workgroup, so the other three are the yardsticks; the shape kernel
alone reads no tile.  There is no target time: the file records the four side by side.  Here the whole 256-px tile is the frame of every
nucleus, while the document route (tools/wsi_feat_extract.py --shape) gives every nucleus a frame of its own.  The timed rows are checked
against the numpy restatement (nuhtc_amd.nucshape.shape_reference).  bench.py (the detection path) launches none of this and is not
changed by this tool."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--tile', type=int, default=256)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=12)
    args = ap.parse_args(argv)
    import torch
    from nuhtc_amd import hip, nucfeat, nucshape, synth, weights
    from nuhtc_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit('bench_nucshape.py needs a GPU (there is no fallback)')
    P, B = args.tile, args.batch
    e = Engine(weights.bench_state_dict(0, obj_bias=0.0), device=0, max_batch=B, tile=(P, P))
    tiles = np.stack([synth.nuclei_tile(1000 + k, P) for k in range(B)])
    with torch.cuda.stream(e.stream):
        dev = e.to_device(tiles)
        e.infer_async(dev, hip.CH_SWAP)
        e.export_async(B)
        e.stream.synchronize()
        g = e.export_read()
        if g is None:
            raise SystemExit('the batch held more kept detections than the export buffers')
        n = int(g['n'])
        pairs_np = np.stack([np.asarray(g['tile'], np.int32), np.asarray(g['slot'], np.int32)], 1)
        pairs = torch.from_numpy(np.ascontiguousarray(pairs_np)).to(e.device)
        masks = e.masks[:B].contiguous()
        ops = {'shape': lambda: e.op_nucleus_shape(masks, pairs, W=P),
               'morph': lambda: e.op_nucleus_morph(dev, masks, pairs, hip.CH_SWAP),
               'tex': lambda: e.op_nucleus_texture(dev, masks, pairs, hip.CH_SWAP),
               'grad': lambda: e.op_nucleus_gradient(dev, masks, pairs, hip.CH_SWAP, 1)}
        ms = {k: [] for k in ops}
        last = {}
        for i in range(args.rounds):
            for k, call in ops.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(e.stream)
                last[k] = call()
                e1.record(e.stream)
                e.stream.synchronize()
                if i >= 2:
                    ms[k].append(e0.elapsed_time(e1))
        rows = last['shape'].cpu().numpy()
        mb = nucfeat.unpack_mask_words(masks.cpu().numpy())
    # the rows of the timed batch against the numpy restatement: a number for code that computes something else is no number
    exact = all(np.array_equal(nucshape.shape_reference(mb[t, s]), rows[i]) for i, (t, s) in enumerate(pairs_np.tolist()))
    med = lambda v: float(np.median(v))
    us = lambda k: round(1e3 * med(ms[k]) / max(n, 1), 4)
    side = np.minimum(rows[:, nucshape.I_X1] - rows[:, nucshape.I_X0], rows[:, nucshape.I_Y1] - rows[:, nucshape.I_Y0])
    out = dict(what=f'tools/bench_nucshape.py: per-nucleus shape integers on the kept masks of {B} synthetic {P}-px tiles resident on the device, one MI355X; '
                    f'the shape, morphometry, texture and gradient ops on the same masks in turn, {args.rounds} rounds, the first two dropped; each figure is '
                    'one synchronous op call between two events (launch and stream synchronisation included)',
               tile=P, batch=B, kept_nuclei_per_batch=n, mean_area_px=round(float(rows[:, nucshape.I_A].mean()), 1) if n else 0.0,
               mean_smaller_side_px=round(float(side.mean()), 1) if n else 0.0,
               op_ms_per_batch=[round(v, 4) for v in ms['shape']], op_ms_per_batch_median=round(med(ms['shape']), 4),
               nucmorph_op_ms_per_batch_median=round(med(ms['morph']), 4), nuctex_op_ms_per_batch_median=round(med(ms['tex']), 4),
               nucgrad_op_ms_per_batch_median=round(med(ms['grad']), 4),
               op_us_per_nucleus=us('shape'), nucmorph_op_us_per_nucleus=us('morph'), nuctex_op_us_per_nucleus=us('tex'), nucgrad_op_us_per_nucleus=us('grad'),
               rows_equal_the_restatement=bool(exact))
    print(json.dumps(out))
    if not exact:
        raise SystemExit('the shape rows differ from the restatement')


if __name__ == '__main__':
    main()
