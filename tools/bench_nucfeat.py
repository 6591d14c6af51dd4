#!/usr/bin/env python
"""Cost of the per-nucleus embeddings of the slide path (csrc/nucfeat.hip) -- prints ONE JSON line (profiles/nucleus_features.json).

    python tools/bench_nucfeat.py [--tile 256] [--batch 16] [--steps 30] [--warmup 5] [--repeats 3]

Synthetic tiles (nuhtc_amd.synth), one batch resident on the device, two engines of the same weights on their own streams: one exports
every step without embeddings, the other with (Engine.export_async(nucfeat=True)).
  kernel_ms_per_batch   nuhtc_nucleus_features alone, between two events, on the kept detections of the batch (their number is in the line)
  tiles_per_s           `--steps` steps of infer_async + export_async back to back, one synchronisation at the end, the two engines in turn,
                        `--repeats` times: without and with the embeddings.  The copy to pinned memory is part of a step; it grows by
                        1 KB per detection of the export capacity.
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
    from nuhtc_amd import hip, nuclei, synth, weights
    from nuhtc_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit('bench_nucfeat.py needs a GPU (there is no fallback)')
    P, B = args.tile, args.batch
    sd = weights.bench_state_dict(0, obj_bias=0.0)
    tiles = np.stack([synth.nuclei_tile(1000 + k, P) for k in range(B)])
    engines = {False: Engine(sd, device=0, max_batch=B, tile=(P, P)), True: Engine(sd, device=0, max_batch=B, tile=(P, P))}
    devs = {}
    for nf, e in engines.items():
        with torch.cuda.stream(e.stream):
            devs[nf] = e.to_device(tiles)
            e.stream.synchronize()

    def steps(nf, n):
        e = engines[nf]
        with torch.cuda.stream(e.stream):
            t0 = time.perf_counter()
            for _ in range(n):
                e.infer_async(devs[nf], hip.CH_SWAP)
                e.export_async(B, nucfeat=True) if nf else e.export_async(B)
            e.stream.synchronize()
            return time.perf_counter() - t0

    for nf in (False, True):
        steps(nf, args.warmup)
    rates = {False: [], True: []}
    for _ in range(args.repeats):
        for nf in (False, True):
            rates[nf].append(B * args.steps / steps(nf, args.steps))
    # ---- the kernel alone, on the last export of the engine that carries the embeddings
    e = engines[True]
    g = e.export_read()
    if g is None:
        raise SystemExit('the batch held more kept detections than the export buffers')
    d, cap = e._ex['dev'], e._ex['cap']
    kms = []
    with torch.cuda.stream(e.stream):
        for i in range(12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(e.stream)
            e._nucleus_async(nuclei.FEAT, B, d['idx'], d['nk'], cap, [d['feat']])
            e1.record(e.stream)
            e.stream.synchronize()
            if i >= 2:
                kms.append(e0.elapsed_time(e1))
    plain = engines[False].export_read()
    same = all(np.array_equal(plain[k], g[k]) for k in ('tile', 'slot', 'boxes', 'labels'))
    blob = {nf: int(engines[nf]._ex['blob_dev'].numel()) for nf in (False, True)}
    med = lambda v: float(np.median(v))
    out = dict(what=f'tools/bench_nucfeat.py: per-nucleus embeddings on {B} synthetic {P}-px tiles resident on the device, one MI355X; {args.steps} steps of '
                    f'infer + export per run after {args.warmup} warm-up steps, two engines in turn, {args.repeats} runs each',
               tile=P, batch=B, kept_nuclei_per_batch=int(g['n']), export_capacity=int(cap),
               kernel_ms_per_batch=[round(k, 4) for k in kms], kernel_ms_per_batch_median=round(med(kms), 4),
               kernel_us_per_nucleus=round(1e3 * med(kms) / max(int(g['n']), 1), 4),
               tiles_per_s_without=[round(r, 1) for r in rates[False]], tiles_per_s_with=[round(r, 1) for r in rates[True]],
               tiles_per_s_without_median=round(med(rates[False]), 1), tiles_per_s_with_median=round(med(rates[True]), 1),
               with_over_without=round(med(rates[True]) / med(rates[False]), 4),
               ms_per_batch_without=round(1e3 * B / med(rates[False]), 4), ms_per_batch_with=round(1e3 * B / med(rates[True]), 4),
               export_copy_bytes_without=blob[False], export_copy_bytes_with=blob[True], other_fields_equal=bool(same),
               note='a step is one engine alone on its stream (latency schedule), not the four-engine slide loop of tools/bench_wsi.py')
    print(json.dumps(out))
    if not same:
        raise SystemExit('the export with embeddings differs from the export without in its other fields')


if __name__ == '__main__':
    main()
