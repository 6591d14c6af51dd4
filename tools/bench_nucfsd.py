#!/usr/bin/env python
"""Cost of the per-nucleus Fourier-descriptor integers (csrc/nucfsd.hip) -- prints ONE JSON line (profiles/nucleus_fsd.json).

    python tools/bench_nucfsd.py [--tile 256] [--batch 16] [--rounds 12]

Synthetic tiles (nuhtc_amd.synth), one batch resident on the device; one engine infers it once and exports its kept detections.  The
outer border of every kept mask is traced on the host (contours.mask_to_ring: the ring a detection run writes) and the rings are
uploaded once, as ringfeat.measure uploads them for the fill.  Then nuhtc_op_ring_fsd on those rings and the four per-nucleus ops on
the masks of the same nuclei -- nuhtc_op_nucleus_shape, nuhtc_op_nucleus_morph, nuhtc_op_nucleus_texture, nuhtc_op_nucleus_gradient --
run in turn `--rounds` times, each call between two events and followed by a stream synchronisation; the first two rounds are dropped.
The same rows by the numpy restatement on the host (nuhtc_amd.nucfsd.fsd_reference, one ring at a time) are timed with the host clock:
that is what the kernel replaces.  There is no target time: the file records the figures side by side.  The timed rows are checked
against the restatement.  bench.py (the detection path) launches none of this and is not changed by this tool."""
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
    ap.add_argument('--tile', type=int, default=256)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=12)
    args = ap.parse_args(argv)
    import torch
    from nuhtc_amd import contours, hip, nucfeat, nucfsd, ringfeat, synth, weights
    from nuhtc_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit('bench_nucfsd.py needs a GPU (there is no fallback)')
    P, B = args.tile, args.batch
    e = Engine(weights.bench_state_dict(0, obj_bias=0.0), device=0, max_batch=B, tile=(P, P))
    tiles = np.stack([synth.nuclei_tile(1000 + k, P) for k in range(B)])
    lib = hip.load()
    with torch.cuda.stream(e.stream):
        dev = e.to_device(tiles)
        e.infer_async(dev, hip.CH_SWAP)
        e.export_async(B)
        e.stream.synchronize()
        g = e.export_read()
        if g is None:
            raise SystemExit('the batch held more kept detections than the export buffers')
        n = int(g['n'])
        if not 1 <= n <= 4096:
            raise SystemExit(f'{n} kept nuclei: nuhtc_op_ring_fsd takes 1 .. 4096 rings a call')
        pairs_np = np.stack([np.asarray(g['tile'], np.int32), np.asarray(g['slot'], np.int32)], 1)
        pairs = torch.from_numpy(np.ascontiguousarray(pairs_np)).to(e.device)
        masks = e.masks[:B].contiguous()
        mb = nucfeat.unpack_mask_words(masks.cpu().numpy())
        rings = []
        for t, s in pairs_np.tolist():
            r = np.asarray(contours.mask_to_ring(mb[t, s]), np.int64).reshape(-1, 2)
            rings.append(r[:-1] if len(r) > 1 and (r[0] == r[-1]).all() else r)
        verts, ring_off = ringfeat.pack_rings(rings)
        if len(verts) == 0:
            raise SystemExit('no kept mask has a pixel')
        verts_d, off_d = torch.from_numpy(verts).to(e.device), torch.from_numpy(ring_off).to(e.device)
        rows_d = torch.empty(n, nucfsd.ROW, dtype=torch.int32, device=e.device)
        status_d = torch.empty(n, dtype=torch.int32, device=e.device)
        vp = lambda x: ctypes.c_void_p(x.data_ptr())

        def fsd():
            rc = lib.nuhtc_op_ring_fsd(0, vp(verts_d), len(verts), vp(off_d), n, vp(rows_d), vp(status_d), ctypes.c_void_p(e.stream.cuda_stream))
            if rc:
                raise SystemExit(f'nuhtc_op_ring_fsd failed ({rc})')
            e.stream.synchronize()                      # the four ops beside it synchronise too
            return rows_d

        ops = {'fsd': fsd,
               'shape': lambda: e.op_nucleus_shape(masks, pairs, W=P),
               'morph': lambda: e.op_nucleus_morph(dev, masks, pairs, hip.CH_SWAP),
               'tex': lambda: e.op_nucleus_texture(dev, masks, pairs, hip.CH_SWAP),
               'grad': lambda: e.op_nucleus_gradient(dev, masks, pairs, hip.CH_SWAP, 1)}
        ms = {k: [] for k in ops}
        for i in range(args.rounds):
            for k, call in ops.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(e.stream)
                call()
                e1.record(e.stream)
                e.stream.synchronize()
                if i >= 2:
                    ms[k].append(e0.elapsed_time(e1))
        rows = rows_d.cpu().numpy()
    # the same rows on the host, and the timed rows against them: a number for code that computes something else is no number
    host_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = np.stack([nucfsd.fsd_reference(r) for r in rings])
        host_s.append(time.perf_counter() - t0)
    exact = bool(np.array_equal(rows, want))
    med = lambda v: float(np.median(v))
    us = lambda k: round(1e3 * med(ms[k]) / n, 4)
    lens = np.diff(ring_off)
    out = dict(what=f'tools/bench_nucfsd.py: per-nucleus Fourier-descriptor integers on the traced rings of the kept masks of {B} synthetic {P}-px tiles, rings '
                    f'resident on the device, one MI355X; nuhtc_op_ring_fsd and the shape, morphometry, texture and gradient ops on the same nuclei in turn, '
                    f'{args.rounds} rounds, the first two dropped; each figure is one call and a stream synchronisation between two events (launch included); '
                    'host: numpy fsd_reference ring by ring, best of three, host clock',
               tile=P, batch=B, kept_nuclei_per_batch=n, mean_vertices_per_ring=round(float(lens.mean()), 1), max_vertices_per_ring=int(lens.max()),
               mean_perimeter_steps=round(float((want[:, 1] + want[:, 2]).mean()), 1), measured_rings=int((want[:, 0] == 0).sum()),
               op_ms_per_batch=[round(v, 4) for v in ms['fsd']], op_ms_per_batch_median=round(med(ms['fsd']), 4),
               nucshape_op_ms_per_batch_median=round(med(ms['shape']), 4), nucmorph_op_ms_per_batch_median=round(med(ms['morph']), 4),
               nuctex_op_ms_per_batch_median=round(med(ms['tex']), 4), nucgrad_op_ms_per_batch_median=round(med(ms['grad']), 4),
               op_us_per_nucleus=us('fsd'), nucshape_op_us_per_nucleus=us('shape'), nucmorph_op_us_per_nucleus=us('morph'), nuctex_op_us_per_nucleus=us('tex'),
               nucgrad_op_us_per_nucleus=us('grad'),
               host_reference_ms_per_batch=round(1e3 * min(host_s), 2), host_reference_us_per_nucleus=round(1e6 * min(host_s) / n, 2),
               rows_equal_the_restatement=exact)
    print(json.dumps(out))
    if not exact:
        raise SystemExit('the rows differ from the restatement')


if __name__ == '__main__':
    main()
