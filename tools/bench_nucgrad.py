#!/usr/bin/env python
"""Cost of the per-nucleus gradient integers (csrc/nucgrad.hip) -- prints ONE JSON line (profiles/nucleus_gradient.json).

    python tools/bench_nucgrad.py [--tile 256] [--batch 16] [--rounds 12] [--edge-thr 1]

Synthetic tiles (nuhtc_amd.synth), one batch resident on the device; one engine infers it once and exports its kept detections, and the
three ops that read tile pixels under a mask -- nuhtc_op_nucleus_gradient, nuhtc_op_nucleus_morph, nuhtc_op_nucleus_texture -- run on
those masks (the engine's own, K slots a tile, the kept (tile, slot) pairs), taken in turn `--rounds` times, each call between two
events; the first two rounds are dropped.  The morphometry and texture kernels also scan one mask per workgroup and read the tile under
it, so they are the yardsticks; there is no target time.  The gradient kernel reads the frame ROUND a mask pixel as well -- here the
whole 256-px tile is the frame, while the document route (tools/wsi_feat_extract.py --gradient) gives every nucleus a frame of its own.
The timed rows are checked against the numpy restatement (nuhtc_amd.nucgrad.grad_reference).  bench.py (the detection path) launches
none of this and is not changed by this tool."""
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
    ap.add_argument('--edge-thr', type=int, default=1, help='T, quarter grey levels')
    args = ap.parse_args(argv)
    import torch
    from nuhtc_amd import hip, nucfeat, nucgrad, nucmorph, synth, weights
    from nuhtc_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit('bench_nucgrad.py needs a GPU (there is no fallback)')
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
        ops = {'grad': lambda: e.op_nucleus_gradient(dev, masks, pairs, hip.CH_SWAP, args.edge_thr),
               'morph': lambda: e.op_nucleus_morph(dev, masks, pairs, hip.CH_SWAP),
               'tex': lambda: e.op_nucleus_texture(dev, masks, pairs, hip.CH_SWAP)}
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
        rows = last['grad'].cpu().numpy()
        area = last['morph'][0].cpu().numpy()[:, nucmorph.I_A]
        mb = nucfeat.unpack_mask_words(masks.cpu().numpy())
    # the rows of the timed batch against the numpy restatement: a number for code that computes something else is no number
    rgb = tiles[..., ::-1]
    exact = all(np.array_equal(nucgrad.grad_reference(rgb[t], mb[t, s], args.edge_thr), rows[i]) for i, (t, s) in enumerate(pairs_np.tolist()))
    med = lambda v: float(np.median(v))
    out = dict(what=f'tools/bench_nucgrad.py: per-nucleus gradient integers on the kept masks of {B} synthetic {P}-px tiles resident on the device, one MI355X; '
                    f'the gradient, morphometry and texture ops on the same masks in turn, {args.rounds} rounds, the first two dropped; each figure is one '
                    'synchronous op call between two events (launch and stream synchronisation included)',
               tile=P, batch=B, kept_nuclei_per_batch=n, mean_area_px=round(float(area.mean()), 1) if n else 0.0, edge_thr=args.edge_thr,
               mean_edge_px=round(float(rows[:, nucgrad.I_EDGE].mean()), 1) if n else 0.0,
               op_ms_per_batch=[round(v, 4) for v in ms['grad']], op_ms_per_batch_median=round(med(ms['grad']), 4),
               op_us_per_nucleus=round(1e3 * med(ms['grad']) / max(n, 1), 4),
               nucmorph_op_ms_per_batch_median=round(med(ms['morph']), 4), nuctex_op_ms_per_batch_median=round(med(ms['tex']), 4),
               ratio_to_nucmorph=round(med(ms['grad']) / med(ms['morph']), 3), ratio_to_nuctex=round(med(ms['grad']) / med(ms['tex']), 3),
               rows_equal_the_restatement=bool(exact))
    print(json.dumps(out))
    if not exact:
        raise SystemExit('the gradient rows differ from the restatement')


if __name__ == '__main__':
    main()
