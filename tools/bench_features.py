#!/usr/bin/env python
"""Benchmark of the tile feature step (nuhtc_features: Swin-T + FPN + fpn_mean_pool) -- prints ONE JSON line.

    python tools/bench_features.py [--steps 40] [--warmup 10] [--tile 256] [--in-flight 4]

For B = 16 and B = 64: synthetic 256x256 nuclei tiles resident in HBM, seeded weights, `--in-flight` features_only engines (throughput
schedule, one stream each) fed round robin without host waits -> `tiles_per_s_b<B>`; the same steps on one engine, one batch at a time
-> `ms_per_step_b<B>`.  bench.py (the detection path) is the project's headline benchmark and is not changed by this tool."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(B, steps, warmup, tile, depth):
    from nuhtc_amd import hip, synth, weights
    from nuhtc_amd.engine import Engine
    sd = weights.bench_state_dict(0, obj_bias=3.0)
    tiles = synth.nuclei_tiles(B, tile, start=0)
    engs = [Engine(sd, device=0, max_batch=B, tile=(tile, tile), features_only=1, schedule=hip.SCHED_THROUGHPUT if depth > 1 else hip.SCHED_LATENCY)
            for _ in range(max(1, depth))]
    devs = []
    for e in engs:
        with torch.cuda.stream(e.stream):
            devs.append(e.to_device(tiles))
        e.stream.synchronize()

    def go(n, k0=0):
        for i in range(n):
            e = engs[(k0 + i) % len(engs)]
            with torch.cuda.stream(e.stream):
                e.features_async(devs[(k0 + i) % len(engs)], hip.CH_SWAP)
        for e in engs:
            e.stream.synchronize()
    go(warmup)
    t0 = time.perf_counter()
    go(steps)
    t_flight = time.perf_counter() - t0
    # one batch at a time on one engine
    e, d = engs[0], devs[0]
    with torch.cuda.stream(e.stream):
        for _ in range(warmup):
            e.features_async(d, hip.CH_SWAP)
        e.stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            e.features_async(d, hip.CH_SWAP)
            e.stream.synchronize()
        t_seq = time.perf_counter() - t0
    feat = e.feat[:B].cpu()
    assert torch.isfinite(feat).all()
    for x in engs:
        x.close()
    return B * steps / t_flight, 1e3 * t_seq / steps


def main(argv=None):
    p = argparse.ArgumentParser(allow_abbrev=False)
    p.add_argument('--steps', type=int, default=40)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--tile', type=int, default=256)
    p.add_argument('--in-flight', type=int, default=4, dest='in_flight')
    p.add_argument('--batches', default='16,64', help='comma-separated batch sizes')
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_features needs a GPU')
    line = dict(metric='feature_step_tiles_per_s', tile=a.tile, in_flight=a.in_flight, steps=a.steps, warmup=a.warmup,
                device=torch.cuda.get_device_name(0))
    for B in (int(v) for v in a.batches.split(',')):
        tps, ms = run(B, a.steps, a.warmup, a.tile, a.in_flight)
        line[f'tiles_per_s_b{B}'] = round(tps, 1)
        line[f'ms_per_step_b{B}'] = round(ms, 3)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
