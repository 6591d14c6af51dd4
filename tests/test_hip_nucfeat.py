"""GPU tests of the per-nucleus embeddings (csrc/nucfeat.hip): nuhtc_op_nucleus_pool against the float64 restatement
(nuhtc_amd.nucfeat.pool_reference) on designed masks, within the derived bound (nucfeat.pool_bound: (n + 3) 2^-24 sum(w |x|) / A, n the
non-zero cells of the level); bitwise repeatability and independence of the batch split; Engine.export_async(nucfeat=True) against the
engine's own maps and masks; tools/infer_wsi.py --nuclei-feat end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nuhtc_amd import hip, nucfeat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'nuhtc', 'htc_lite_swin_pannuke_infer.py')
TOOL = os.path.join(ROOT, 'tools', 'infer_wsi.py')
STRIDES = (4, 8, 16, 32)


@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    return Engine(weights.bench_state_dict(0, obj_bias=3.0), device=0, max_batch=4, tile=(64, 64))


def _maps(rng, B, H, W, cancelling=None):
    """Random normal level maps (B, ceil(H / s), ceil(W / s), 64) float32; level `cancelling` alternates +-1e4 from cell to cell under the noise, so
    the terms of a sum are four orders of magnitude above the sum."""
    out = []
    for l, s in enumerate(STRIDES):
        h, w = -(-H // s), -(-W // s)
        x = rng.standard_normal((B, h, w, 64))
        if l == cancelling:
            x += 1e4 * (1 - 2 * ((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2))[None, :, :, None]
        out.append(x.astype(np.float32))
    return out


def _masks_64():
    def blank():
        return np.zeros((64, 64), bool)
    m = {}
    m['pixel at (0, 0)'] = blank(); m['pixel at (0, 0)'][0, 0] = True
    m['pixel at (H-1, W-1)'] = blank(); m['pixel at (H-1, W-1)'][63, 63] = True
    m['block x 30..34: crosses a word and cells'] = blank(); m['block x 30..34: crosses a word and cells'][6:13, 30:35] = True
    m['one level-3 cell'] = blank(); m['one level-3 cell'][32:64, 0:32] = True
    m['full tile'] = np.ones((64, 64), bool)
    two = blank(); two[3:9, 2:7] = True; two[40:52, 41:60] = True; two[45, 50] = False
    m['two disjoint blobs'] = two
    yy, xx = np.mgrid[0:64, 0:64]
    m['disc'] = (yy - 30) ** 2 + (xx - 33) ** 2 <= 11 ** 2
    return m


def _check(got, maps_np, strides, masks_bool, pairs, what):
    """Every row of `got` against pool_reference within pool_bound; returns the largest error / bound."""
    worst = 0.0
    for d, (b, s) in enumerate(pairs):
        lv = [m[b] for m in maps_np]
        ref, bound = nucfeat.pool_reference(lv, strides, masks_bool[b, s]), nucfeat.pool_bound(lv, strides, masks_bool[b, s])
        err = np.abs(got[d].astype(np.float64) - ref)
        if bound.any():
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert (err <= bound).all(), (what, d, b, s, float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def test_op_designed_masks_64(eng):
    rng = np.random.default_rng(0)
    names = list(_masks_64())
    masks = np.stack([np.stack(list(_masks_64().values()))] * 2)                     # (2, K, 64, 64): the same masks on both tiles
    maps = _maps(rng, 2, 64, 64, cancelling=0)
    pairs = np.array([(b, s) for s in range(len(names)) for b in range(2)], np.int32)
    out = eng.op_nucleus_pool([_dev(eng, m) for m in maps], STRIDES, _dev(eng, nucfeat.pack_mask_words(masks)), _dev(eng, pairs)).cpu().numpy()
    worst = _check(out, maps, STRIDES, masks, pairs, '64x64')
    print(f'64 x 64, maps 16 / 8 / 4 / 2, {len(pairs)} rows: largest error / bound {worst:.3f}')
    for s, name in enumerate(names):                                                  # the same mask on tile 0 and tile 1: different maps, different rows
        assert not np.array_equal(out[2 * s], out[2 * s + 1]), name
    assert np.array_equal(out[0], np.concatenate([m[0, 0, 0] for m in maps]))        # one pixel: the cell itself, exactly
    assert np.array_equal(out[3], np.concatenate([m[1, -1, -1] for m in maps]))
    # the cancelling level is what the bound is about: its terms are ~1e4, its sums ~1
    full = out[2 * names.index('full tile')]
    assert np.abs(full[:64]).max() < 10 and np.abs(maps[0][0]).mean() > 5e3


def test_op_width_not_a_multiple_of_32(eng):
    rng = np.random.default_rng(1)
    H, W = 48, 80
    maps = _maps(rng, 2, H, W, cancelling=1)
    assert [m.shape[1:3] for m in maps] == [(12, 20), (6, 10), (3, 5), (2, 3)]
    masks = np.zeros((2, 3, H, W), bool)
    masks[:, 0, 37:48, 66:80] = True                                                  # touches the right and the bottom edge
    masks[:, 2, 10:31, 58:70] = True                                                  # crosses the word boundary at x = 64
    masks[:, 2, 20, 61] = False                                                       # (slot 1 stays empty: A == 0)
    cap, n = 8, 5
    pairs = np.array([(0, 0), (0, 1), (1, 2), (1, 0), (0, 2), (1, 1), (0, 0), (1, 2)], np.int32)
    words = nucfeat.pack_mask_words(masks)
    assert words.shape == (2, 3, H, 3)
    out = torch.full((cap, 256), 7.5, dtype=torch.float32, device=eng.device)
    eng.op_nucleus_pool([_dev(eng, m) for m in maps], STRIDES, _dev(eng, words), _dev(eng, pairs), W=W,
                        n=torch.tensor([n], dtype=torch.int32, device=eng.device), out=out)
    got = out.cpu().numpy()
    worst = _check(got[:n], maps, STRIDES, masks, pairs[:n], '48x80')
    print(f'48 x 80, maps 12x20 / 6x10 / 3x5 / 2x3, {n} of {cap} rows: largest error / bound {worst:.3f}')
    assert not got[1].any()                                                           # A == 0: a zero row
    assert (got[n:] == 7.5).all()                                                     # rows past the count: untouched
    assert np.abs(got[0]).max() > 0 and np.abs(got[2]).max() > 0
    # the whole list, and an entry outside the batch
    all_rows = eng.op_nucleus_pool([_dev(eng, m) for m in maps], STRIDES, _dev(eng, words), _dev(eng, pairs), W=W).cpu().numpy()
    assert np.array_equal(all_rows[:n], got[:n]) and np.array_equal(all_rows[6], got[0]) and np.array_equal(all_rows[7], got[2])
    bad = eng.op_nucleus_pool([_dev(eng, m) for m in maps], STRIDES, _dev(eng, words), _dev(eng, np.array([(2, 0), (0, 3), (-1, 0), (0, 0)], np.int32)), W=W).cpu().numpy()
    assert not bad[:3].any() and np.array_equal(bad[3], got[0])


def test_op_out_of_range_pairs_count_and_sentinel(eng):
    """The pool's twin of the morphometry and texture tests of this name (the three kernels resolve a list entry through one helper,
    csrc/nucleus_list.h): entries outside the batch give exact zero rows, rows from the device count on keep what they held."""
    rng = np.random.default_rng(4)
    B, K, H, W, strides = 2, 3, 64, 64, (2, 4, 8, 16)
    maps = [rng.standard_normal((B, H // s, W // s, 64)).astype(np.float32) for s in strides]
    assert [m.shape[1] for m in maps] == [32, 16, 8, 4]
    masks = np.zeros((B, K, H, W), bool)
    masks[0, 1, 5:21, 28:37] = True                                                   # crosses the word boundary at x = 32
    masks[1, 2, 40:64, 50:64] = True                                                  # touches the right and the bottom edge
    masks[0, 0, 1:9, 1:9] = True
    masks[1, 0, 30:33, 2:60] = True
    pairs = np.array([(0, 1), (B, 0), (1, 2), (0, -1), (0, 0), (1, 0)], np.int32)
    n = 4
    out = torch.full((len(pairs), 256), -7.5, dtype=torch.float32, device=eng.device)
    eng.op_nucleus_pool([_dev(eng, m) for m in maps], strides, _dev(eng, nucfeat.pack_mask_words(masks)), _dev(eng, pairs),
                        n=torch.tensor([n], dtype=torch.int32, device=eng.device), out=out)
    got = out.cpu().numpy()
    assert (got[n:] == -7.5).all()                                                    # rows 4 and 5: past the count, untouched
    assert (got[[1, 3]] == 0).all()                                                   # tile = B, slot = -1: zero rows
    worst = _check(got[[0, 2]], maps, strides, masks, pairs[[0, 2]], '64x64 at strides 2 / 4 / 8 / 16')
    print(f'64 x 64, maps 32 / 16 / 8 / 4, rows 0 and 2 of {n}: largest error / bound {worst:.3f}')
    assert np.abs(got[0]).max() > 0 and np.abs(got[2]).max() > 0


def test_op_refuses_maps_that_do_not_cover_the_image(eng):
    from nuhtc_amd.engine import HipError
    rng = np.random.default_rng(2)
    maps = [_dev(eng, m) for m in _maps(rng, 1, 64, 64)]
    words = _dev(eng, nucfeat.pack_mask_words(np.ones((1, 1, 64, 64), bool)))
    pairs = _dev(eng, np.zeros((1, 2), np.int32))
    with pytest.raises(HipError):
        eng.op_nucleus_pool(maps, (2, 8, 16, 32), words, pairs)                       # a 16 x 16 map at stride 2 covers 32 x 32 pixels
    with pytest.raises(HipError):
        eng.op_nucleus_pool(maps, (4, 8, 16, 0), words, pairs)


def test_op_two_runs_are_bitwise_equal(eng):
    rng = np.random.default_rng(3)
    masks = np.stack([np.stack(list(_masks_64().values()))] * 2)
    maps = [_dev(eng, m) for m in _maps(rng, 2, 64, 64, cancelling=2)]
    pairs = _dev(eng, np.array([(b, s) for b in range(2) for s in range(masks.shape[1])], np.int32))
    words = _dev(eng, nucfeat.pack_mask_words(masks))
    a = eng.op_nucleus_pool(maps, STRIDES, words, pairs)
    b = eng.op_nucleus_pool(maps, STRIDES, words, pairs)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def _export(e, dev_tiles, **kw):
    """infer + export of one batch on the engine's stream -> a snapshot of export_read()."""
    with torch.cuda.stream(e.stream):
        B = e.infer_async(dev_tiles, hip.CH_SWAP)
        e.export_async(B, **kw)
        e.stream.synchronize()
        g = e.export_read()
    assert g is not None
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in g.items()}


@pytest.mark.parametrize('which', ['seeded', 'bench'])
def test_rows_are_bitwise_independent_of_the_batch_split(hip_device, which):
    """Ten synthetic 64-px tiles as one batch of 10, as 4 + 6 and as ten batches of 1: the same kept nuclei and the same rows, bit for bit."""
    from nuhtc_amd import synth, weights
    from nuhtc_amd.engine import Engine
    sd = weights.seeded_state_dict(0) if which == 'seeded' else weights.bench_state_dict(0, obj_bias=3.0)
    tiles = synth.nuclei_tiles(10, 64, start=0)
    e = Engine(sd, device=0, max_batch=10, tile=(64, 64))
    with torch.cuda.stream(e.stream):
        dev = e.to_device(tiles)
    runs = []
    for split in ([10], [4, 6], [1] * 10):
        rows, key, i0 = [], [], 0
        for bs in split:
            g = _export(e, dev[i0:i0 + bs], nucfeat=True)
            rows.append(g['feat']); key.append(np.stack([g['tile'] + i0, g['slot']], 1))
            i0 += bs
        runs.append((np.concatenate(key), np.concatenate(rows)))
    print(f'{which}: {len(runs[0][0])} kept nuclei on 10 tiles')
    for key, rows in runs[1:]:
        assert np.array_equal(key, runs[0][0]) and np.array_equal(rows.view(np.uint32), runs[0][1].view(np.uint32))
    assert np.isfinite(runs[0][1]).all()
    if which == 'bench':
        assert len(runs[0][0]) > 0


KEYS = {'n', 'tile', 'slot', 'boxes', 'labels', 'cn', 'xy', 'crop_box', 'crop_area', 'crop_off', 'crop_words', 'crop_total', 'pool'}


def test_engine_export_with_embeddings(eng):
    from nuhtc_amd import synth
    tiles = synth.nuclei_tiles(4, 64, start=0)
    with torch.cuda.stream(eng.stream):
        dev = eng.to_device(tiles)
    plain = _export(eng, dev)
    size_plain = eng._ex['blob_dev'].numel()
    g = _export(eng, dev, nucfeat=True)
    with torch.cuda.stream(eng.stream):
        maps_t = [eng.buffer(f'x{l}')[:4] for l in range(4)]
        masks = nucfeat.unpack_mask_words(eng.masks[:4].cpu().numpy())
        counts, keep = eng.counts[:4].cpu().numpy(), eng.keep[:4].cpu().numpy()
    n = g['n']
    assert n > 0 and n == int(sum(keep[b, :counts[b]].sum() for b in range(4))) and g['feat'].shape == (n, 256) and g['feat'].dtype == np.float32
    # every other field bit for bit as without the embeddings, and without them the layout and the keys as before
    assert set(plain) == KEYS and set(g) == KEYS | {'feat'}
    for k in KEYS:
        assert np.array_equal(plain[k], g[k]), k
    again = _export(eng, dev)
    assert eng._ex['blob_dev'].numel() == size_plain and set(again) == KEYS
    # the rows against the engine's own maps and masks: scale_factor 2, so a map cell of stride 4 << l covers (4 << l) / 2 mask pixels
    strides = (2, 4, 8, 16)
    maps = [m.cpu().numpy() for m in maps_t]
    assert [m.shape[1] for m in maps] == [32, 16, 8, 4]
    pairs = np.stack([g['tile'], g['slot']], 1)
    worst = _check(g['feat'], maps, strides, masks, pairs, 'engine')
    print(f'{n} kept nuclei on 4 tiles of 64 px: largest error / bound {worst:.3f}')
    assert np.array_equal(eng.nucleus_features(4, g['tile'], g['slot']), g['feat'])     # the synchronous route: the same bits
    # a mask of the whole tile through the op on those maps: the tile embedding of nuhtc_features (tolerance of tests/test_hip_features.py)
    full = _dev(eng, nucfeat.pack_mask_words(np.ones((4, 1, 64, 64), bool)))
    with torch.cuda.stream(eng.stream):
        rows = eng.op_nucleus_pool([m.contiguous() for m in maps_t], strides, full, _dev(eng, np.array([(b, 0) for b in range(4)], np.int32))).cpu().numpy()
        eng.features_async(dev, hip.CH_SWAP)
        eng.stream.synchronize()
        tile_feat = eng.feat[:4].cpu().numpy()
    err = np.abs(rows - tile_feat)
    print(f'full-tile mask against nuhtc_features: max |diff| {err.max():.3e}')
    assert (err <= 1e-5 + 1e-4 * np.abs(tile_feat)).all()


def _run(cmd, env=None, limit=300):
    p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, TOOL] + cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, p.returncode
    return p.stdout


def test_cli_nuclei_feat(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-feat on a synthetic .npy slide: one row per written nucleus in the order of <id>.geojson, only the merged
    file's nuclei with --merge, the documents the same bytes with and without the flag, two ranks on one device the same table."""
    from nuhtc_amd import synth, weights
    ck = tmp_path / 'w.pth'
    torch.save(dict(state_dict=weights.bench_state_dict(0, obj_bias=0.0)), ck)
    slide = np.concatenate([np.concatenate(list(synth.nuclei_tiles(5, 64, start=r * 5)), 1) for r in range(3)], 0)    # 192 x 320
    np.save(tmp_path / 's1.npy', slide)
    base = [str(tmp_path / 's1.npy'), CFG, str(ck), '--patch_size', '64', '--step_size', '48', '--batch_size', '8', '--mode', 'qupath']
    env = dict(os.environ, NUHTC_HOST_AFFINITY='0')
    docs = lambda d: {f: open(tmp_path / d / 'nuclei' / 's1' / f, 'rb').read() for f in sorted(os.listdir(tmp_path / d / 'nuclei' / 's1')) if f.endswith('.geojson')}
    table = lambda d: nucfeat.read_npz(str(tmp_path / d / 'nuclei' / 's1' / 's1_nuclei_feat.npz'))
    _run(base + ['--save_dir', str(tmp_path / 'plain'), '--merge'], env)
    assert not os.path.exists(tmp_path / 'plain' / 'nuclei' / 's1' / 's1_nuclei_feat.npz')
    _run(base + ['--save_dir', str(tmp_path / 'feat'), '--nuclei-feat'], env)
    _run(base + ['--save_dir', str(tmp_path / 'featm'), '--nuclei-feat', '--merge'], env)
    plain, feat, featm = docs('plain'), docs('feat'), docs('featm')
    assert set(plain) == {'s1.geojson', 's1_point.geojson', 's1_merged.geojson'} and featm == plain
    assert feat == {k: v for k, v in plain.items() if k != 's1_merged.geojson'}
    every, merged = json.loads(plain['s1.geojson']), json.loads(plain['s1_merged.geojson'])
    t = table('feat')
    n = len(every)
    print(f'{n} nuclei written, {len(merged)} after the merge')
    assert n > 10 and 0 < len(merged) < n
    assert t['nuclei_id'].tolist() == list(range(n)) and t['features'].shape == (n, 256) and t['features'].dtype == np.float32
    assert t['label'].tolist() == [f['properties']['label'] for f in every] and t['score'].tolist() == [f['properties']['score'] for f in every]
    assert np.isfinite(t['features']).all() and (np.abs(t['features']).sum(1) > 0).all()
    tm = table('featm')
    assert len(tm['nuclei_id']) == len(merged) and [every[i] for i in tm['nuclei_id']] == merged
    assert np.array_equal(tm['features'], t['features'][tm['nuclei_id']]) and tm['score'].tolist() == [f['properties']['score'] for f in merged]
    two = dict(env, NUHTC_ONE_DEVICE='1', NUHTC_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='4')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        two.pop(k, None)
    _run(base + ['--save_dir', str(tmp_path / 'two'), '--nuclei-feat', '--merge', '--gpus', '2'], two)
    t2 = table('two')
    assert docs('two') == plain
    for k in ('nuclei_id', 'features', 'label', 'score'):
        assert np.array_equal(t2[k], tm[k]), k
