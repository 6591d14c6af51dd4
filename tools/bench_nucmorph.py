#!/usr/bin/env python
"""Cost of the per-nucleus morphometry of the slide path (csrc/nucmorph.hip) -- prints ONE JSON line (profiles/nucleus_morph.json).

    python tools/bench_nucmorph.py [--tile 256] [--batch 16] [--steps 30] [--warmup 5] [--repeats 3]

Synthetic tiles (nuhtc_amd.synth), one batch resident on the device, three engines of the same weights on their own streams: one exports
every step plainly, one with the morphometry integers (Engine.export_async(nucmorph=True)) and one with the embeddings (nucfeat=True:
the figures of tools/bench_nucfeat.py taken in the same run -- that kernel also scans one mask per workgroup, so it is the yardstick).
  kernel_*              nuhtc_nucleus_morph / nuhtc_nucleus_features alone, between two events, on the kept detections of the batch
  ms_per_batch_*        `--steps` steps of infer_async + export_async back to back, one synchronisation at the end, the three engines in
                        turn, `--repeats` times.  The copy to pinned memory is part of a step; the morphometry adds 1152 bytes per
                        detection of the export capacity, the embeddings 1024.
bench.py (the detection path without any export) is the project's headline benchmark and is not changed by this tool."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--tile', type=int, default=256)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args(argv)
    import torch
    from nuhtc_amd import hip, nuclei, nucmorph, synth, weights
    from nuhtc_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit('bench_nucmorph.py needs a GPU (there is no fallback)')
    P, B = args.tile, args.batch
    sd = weights.bench_state_dict(0, obj_bias=0.0)
    tiles = np.stack([synth.nuclei_tile(1000 + k, P) for k in range(B)])
    kinds = {'plain': {}, 'morph': dict(nucmorph=True), 'feat': dict(nucfeat=True)}
    engines = {k: Engine(sd, device=0, max_batch=B, tile=(P, P)) for k in kinds}
    devs = {}
    for k, e in engines.items():
        with torch.cuda.stream(e.stream):
            devs[k] = e.to_device(tiles)
            e.stream.synchronize()

    def steps(k, n):
        e = engines[k]
        with torch.cuda.stream(e.stream):
            t0 = time.perf_counter()
            for _ in range(n):
                e.infer_async(devs[k], hip.CH_SWAP)
                e.export_async(B, **kinds[k])
            e.stream.synchronize()
            return time.perf_counter() - t0

    for k in kinds:
        steps(k, args.warmup)
    ms = {k: [] for k in kinds}
    for _ in range(args.repeats):
        for k in kinds:
            ms[k].append(1e3 * steps(k, args.steps) / args.steps)
    # ---- the kernels alone, on the last export of the engine that carries their rows
    def alone(k, call):
        e = engines[k]
        out = []
        with torch.cuda.stream(e.stream):
            for i in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(e.stream)
                call(e, e._ex['dev'], e._ex['cap'])
                e1.record(e.stream)
                e.stream.synchronize()
                if i >= 2:
                    out.append(e0.elapsed_time(e1))
        return out

    def kernel(name, kind):
        return alone(name, lambda e, d, cap: e._nucleus_async(kind, B, d['idx'], d['nk'], cap, [d[f] for f, _, _ in kind.fields]))

    k_morph = kernel('morph', nuclei.MORPH)
    k_feat = kernel('feat', nuclei.FEAT)
    g = {k: engines[k].export_read() for k in kinds}
    if any(v is None for v in g.values()):
        raise SystemExit('the batch held more kept detections than the export buffers')
    same = all(np.array_equal(g['plain'][f], g[k][f]) for k in ('morph', 'feat') for f in ('tile', 'slot', 'boxes', 'labels'))
    # the rows of the timed batch against the numpy restatement: a number for code that computes something else is no number
    e = engines['morph']
    with torch.cuda.stream(e.stream):
        masks = e.masks[:B].cpu().numpy()
    from nuhtc_amd import nucfeat
    mb = nucfeat.unpack_mask_words(masks)
    rgb = tiles[..., ::-1]
    exact = all(np.array_equal(np.concatenate(nucmorph.morph_reference(rgb[t], mb[t, s])), np.concatenate([g['morph']['morph_raw'][i], g['morph']['morph_hist'][i]]))
                for i, (t, s) in enumerate(zip(g['morph']['tile'].tolist(), g['morph']['slot'].tolist())))
    n = int(g['morph']['n'])
    area = g['morph']['morph_raw'][:, nucmorph.I_A]
    med = lambda v: float(np.median(v))
    out = dict(what=f'tools/bench_nucmorph.py: per-nucleus morphometry on {B} synthetic {P}-px tiles resident on the device, one MI355X; {args.steps} steps of '
                    f'infer + export per run after {args.warmup} warm-up steps, three engines in turn, {args.repeats} runs each',
               tile=P, batch=B, kept_nuclei_per_batch=n, mean_area_px=round(float(area.mean()), 1) if n else 0.0, export_capacity=int(e._ex['cap']),
               kernel_ms_per_batch=[round(v, 4) for v in k_morph], kernel_ms_per_batch_median=round(med(k_morph), 4),
               kernel_us_per_nucleus=round(1e3 * med(k_morph) / max(n, 1), 4),
               nucfeat_kernel_ms_per_batch_median=round(med(k_feat), 4), nucfeat_kernel_us_per_nucleus=round(1e3 * med(k_feat) / max(n, 1), 4),
               ms_per_batch_without=[round(v, 4) for v in ms['plain']], ms_per_batch_with=[round(v, 4) for v in ms['morph']],
               ms_per_batch_with_nucfeat=[round(v, 4) for v in ms['feat']],
               ms_per_batch_without_median=round(med(ms['plain']), 4), ms_per_batch_with_median=round(med(ms['morph']), 4),
               ms_per_batch_with_nucfeat_median=round(med(ms['feat']), 4),
               export_copy_bytes={k: int(engines[k]._ex['blob_dev'].numel()) for k in kinds},
               other_fields_equal=bool(same), rows_equal_the_restatement=bool(exact),
               note='a step is one engine alone on its stream (latency schedule), not the four-engine slide loop of tools/bench_wsi.py')
    print(json.dumps(out))
    if not same or not exact:
        raise SystemExit('the export with the morphometry differs from the export without in its other fields, or its rows from the restatement')


if __name__ == '__main__':
    main()
