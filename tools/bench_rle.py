#!/usr/bin/env python
"""Benchmark of the COCO run-length masks of the slide path, host route against device route -- prints ONE JSON line.

    python tools/bench_rle.py [--instances 10000] [--tile 256] [--batch 1536] [--bytes-per-det 256] [--run-cap 1024] [--repeats 5] [--host-n N]

The kept detections of synthetic tiles (nuhtc_amd.synth, the engine's own per-tile filter + mask-NMS) are collected on the device until
there are `--instances` of them; their bit-packed full-tile masks stay resident there.
  host route    the loop of tools/infer_wsi.py run_slide with --rle-on host: per nucleus the crop out of PackedMasks, the paste into a P x P
                array, cocomask.encode, and cocomask.to_bbox on the string (rank 0's half); once over the first `--host-n` nuclei
  device route  nuhtc_rle_encode over batches of `--batch` masks (what one export of 16 tiles holds), each batch's lengths, offsets, boxes
                and strings leaving in ONE copy to pinned memory, then the host's gather of the strings into one blob; `--repeats` times
                after one warm-up.  kernel_ms_per_batch is the three launches alone, between two events.
Strings and boxes of the two routes must be equal.  bench.py (the detection path) is the project's headline benchmark and is not changed
by this tool."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--instances', type=int, default=10000)
    ap.add_argument('--tile', type=int, default=256)
    ap.add_argument('--batch', type=int, default=1536)
    ap.add_argument('--bytes-per-det', type=int, default=256, dest='bytes_per_det')
    ap.add_argument('--run-cap', type=int, default=1024, dest='run_cap')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-n', type=int, default=None, dest='host_n', help='nuclei the host route encodes (default: all)')
    args = ap.parse_args(argv)
    import torch
    from nuhtc_amd import cocomask, hip, synth, weights, wsi
    from nuhtc_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit('bench_rle.py needs a GPU (there is no fallback)')
    P = args.tile
    eng = Engine(weights.bench_state_dict(0, obj_bias=0.0), device=0, max_batch=16, tile=(P, P))
    lib, dev = eng.lib, eng.device
    # ---- the masks: kept detections of synthetic tiles, compacted on the device by the export
    words, boxes, seed = [], [], 0
    with torch.cuda.stream(eng.stream):
        while sum(len(w) for w in words) < args.instances:
            tiles = np.stack([synth.nuclei_tile(1000 + seed + k, P) for k in range(16)])
            seed += 16
            B = eng.infer_async(eng.to_device(tiles), hip.CH_SWAP)
            eng.export_async(B)
            eng.stream.synchronize()
            g = eng.export_read()
            if g is None:
                raise SystemExit('a batch held more kept detections than the export buffers')
            live = np.flatnonzero(g['crop_box'][:, 2] > g['crop_box'][:, 0])
            words.append(eng._ex['dev']['words'][torch.from_numpy(live).to(dev)].clone())
            boxes.append(g['crop_box'][live].copy())
            if seed > 16 * 400:
                raise SystemExit('the synthetic tiles do not yield enough detections')
    words = torch.cat(words)[:args.instances].contiguous()
    boxes = np.concatenate(boxes)[:args.instances]
    N, wpm = int(words.shape[0]), P * P // 32
    tiles_used = seed

    # ---- host route (records as run_slide sees them: PackedMasks crops in tile pixels, origin 0)
    full = np.unpackbits(words.cpu().numpy().view(np.uint8).reshape(N, P, P // 8), axis=-1, bitorder='little')
    pm = wsi.PackedMasks(*wsi.pack_masks([(full[i, y0:y1, x0:x1].astype(bool), int(x0), int(y0)) for i, (x0, y0, x1, y1) in enumerate(boxes)]))
    hn = N if args.host_n is None else min(N, args.host_n)
    t0 = time.perf_counter()
    host_rles = []
    for i in range(hn):
        crop, x0, y0 = pm[i]
        m = np.zeros((P, P), np.uint8)
        m[y0:y0 + crop.shape[0], x0:x0 + crop.shape[1]] = crop
        host_rles.append(cocomask.encode(m)['counts'].encode('ascii'))
    t_encode = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_boxes = [cocomask.to_bbox({'size': [P, P], 'counts': s.decode('ascii')}) for s in host_rles]
    t_bbox = time.perf_counter() - t0

    # ---- device route
    nb = args.batch
    pool = nb * args.bytes_per_det
    fields = dict(len=nb * 4, off=(nb + 1) * 4, bbox=nb * 16, bytes=pool)
    offs, total = {}, 0
    for k, sz in fields.items():
        offs[k] = total
        total += (sz + 255) // 256 * 256
    blob_dev = torch.zeros(total, dtype=torch.uint8, device=dev)
    blob_host = torch.zeros(total, dtype=torch.uint8).pin_memory()
    view = lambda blob, k, dt: blob[offs[k]:offs[k] + fields[k]].view(dt)
    d = dict(len=view(blob_dev, 'len', torch.int32), off=view(blob_dev, 'off', torch.int32), bbox=view(blob_dev, 'bbox', torch.int32), bytes=view(blob_dev, 'bytes', torch.uint8))
    h = dict(len=view(blob_host, 'len', torch.int32).numpy(), off=view(blob_host, 'off', torch.int32).numpy(),
             bbox=view(blob_host, 'bbox', torch.int32).numpy().reshape(nb, 4), bytes=view(blob_host, 'bytes', torch.uint8).numpy())
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)

    def device_pass(timed_kernel=False):
        blobs, lens, bbs, kms, fallback = [], [], [], [], 0
        for i0 in range(0, N, nb):
            n = min(nb, N - i0)
            if timed_kernel:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
            rc = lib.nuhtc_rle_encode(dev.index, vp(words[i0:i0 + n]), None, n, P, P, args.run_cap, vp(d['len']), vp(d['off']), vp(d['bytes']), pool, vp(d['bbox']), sp)
            if rc:
                raise SystemExit(f'nuhtc_rle_encode failed ({rc})')
            if timed_kernel:
                e1.record(stream)
            blob_host.copy_(blob_dev, non_blocking=True)
            stream.synchronize()
            if timed_kernel:
                kms.append(e0.elapsed_time(e1))
            ln, off = h['len'][:n].astype(np.int64), h['off'][:n].astype(np.int64)
            ok = (ln >= 0) & (off + np.maximum(ln, 0) <= pool)
            fallback += int((~ok).sum())
            dn = np.where(ok, ln, 0)
            start = np.cumsum(dn) - dn
            blobs.append(h['bytes'][np.arange(int(dn.sum()), dtype=np.int64) + np.repeat(off - start, dn)])
            lens.append(np.where(ok, ln, -1))
            bbs.append(h['bbox'][:n].copy())
        return np.concatenate(blobs), np.concatenate(lens), np.concatenate(bbs), kms, fallback

    probe = hip.ClockProbe(0)
    probe.start(20)
    clock = [probe.ghz()]
    device_pass()
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        blob, lens, bbs, _, fallback = device_pass()
        times.append(time.perf_counter() - t0)
    kms = device_pass(True)[3]
    probe.start(20)
    clock.append(probe.ghz())

    # ---- equality and the observed maxima
    pos = np.cumsum(np.maximum(lens, 0)) - np.maximum(lens, 0)
    dev_rles = [blob[pos[i]:pos[i] + lens[i]].tobytes() if lens[i] >= 0 else None for i in range(N)]
    equal = all(dev_rles[i] is None or (dev_rles[i] == host_rles[i] and bbs[i].tolist() == host_boxes[i]) for i in range(hn))
    runs = [len(cocomask.string_to_counts(s.decode('ascii'))) for s in host_rles]
    t_dev = float(np.median(times))
    out = dict(what=f'tools/bench_rle.py: COCO run-length masks of {N} kept detections of {tiles_used} synthetic {P}-px tiles, masks resident on the device; '
                    f'host route once over {hn}, device route {args.repeats} times after one warm-up (copy and host gather included), one MI355X',
               instances=N, tile=P, batch=nb, batches=-(-N // nb), rle_bytes_per_det=args.bytes_per_det, run_cap=args.run_cap,
               host_s=dict(encode=round(t_encode, 4), to_bbox=round(t_bbox, 4)), host_nuclei_per_s=round(hn / (t_encode + t_bbox), 1),
               device_s=[round(t, 5) for t in times], device_nuclei_per_s=round(N / t_dev, 1),
               device_over_host=round((N / t_dev) / (hn / (t_encode + t_bbox)), 1),
               kernel_ms_per_batch=[round(k, 4) for k in kms], kernel_ms_per_batch_median=round(float(np.median(kms)), 4),
               longest_string_bytes=int(max(len(s) for s in host_rles)), mean_string_bytes=round(float(np.mean([len(s) for s in host_rles])), 1),
               largest_run_count=int(max(runs)), fallback=int(fallback), strings_and_boxes_equal=bool(equal),
               shader_clock_ghz_one_wave_probe_before_after=[None if c is None else round(c, 3) for c in clock],
               clock_note='one-wave spin probe on an otherwise idle GPU before and after the device runs; no clock was set or pinned')
    print(json.dumps(out))
    if not equal:
        raise SystemExit('device route differs from the host route')


if __name__ == '__main__':
    main()
