"""GPU tests of the per-nucleus morphometry (csrc/nucmorph.hip): the device produces integers only, so every check is EQUALITY with the
numpy restatement (nuhtc_amd.nucmorph.morph_reference) -- nuhtc_op_nucleus_morph on the designed masks of tests/nucmorph_cases.py,
Engine.export_async(nucmorph=True) against the engine's own masks and tiles, tools/infer_wsi.py --nuclei-morph end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nuhtc_amd import hip, nucfeat
from nuhtc_amd import nucmorph as nm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucmorph_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'nuhtc', 'htc_lite_swin_pannuke_infer.py')
TOOL = os.path.join(ROOT, 'tools', 'infer_wsi.py')


@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    return Engine(weights.bench_state_dict(0, obj_bias=3.0), device=0, max_batch=4, tile=(64, 64))


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _reference(tiles_rgb, masks, pairs):
    """(raw (n, 16), hist (n, 256)) of the pairs (tile, slot); a pair outside the arrays gives zeros."""
    raw, hist = np.zeros((len(pairs), 16), np.int64), np.zeros((len(pairs), 256), np.int64)
    for d, (b, s) in enumerate(pairs):
        if 0 <= b < len(tiles_rgb) and 0 <= s < masks.shape[1]:
            raw[d], hist[d] = nm.morph_reference(tiles_rgb[b], masks[b, s])
    return raw, hist


def _run_op(eng, tiles, masks, pairs, mode=hip.CH_AS_IS, **kw):
    raw, hist = eng.op_nucleus_morph(_dev(eng, tiles), _dev(eng, nucfeat.pack_mask_words(masks)), _dev(eng, np.asarray(pairs, np.int32)), mode, **kw)
    return raw.cpu().numpy(), hist.cpu().numpy()


@pytest.fixture(scope='module')
def small():
    """The designed 64 x 40 masks on each of the four tiles: tiles (4, 64, 40, 3), masks (4, K, 64, 40), names, tile names."""
    t, m = cases.tiles(cases.H_SMALL, cases.W_SMALL), cases.small_masks()
    return np.stack(list(t.values())), np.stack([np.stack(list(m.values()))] * len(t)), list(m), list(t)


def test_op_designed_masks_64x40(eng, small):
    tiles, masks, names, tnames = small
    pairs = [(b, s) for b in range(len(tnames)) for s in range(len(names))]
    raw, hist = _run_op(eng, tiles, masks, pairs)
    want_raw, want_hist = _reference(tiles, masks, pairs)
    for d, (b, s) in enumerate(pairs):
        assert np.array_equal(raw[d], want_raw[d]), (tnames[b], names[s], raw[d], want_raw[d])
        assert np.array_equal(hist[d], want_hist[d]), (tnames[b], names[s])
    assert raw.dtype == np.int64 and hist.dtype == np.int32
    k = {n: i for i, n in enumerate(names)}
    assert not raw[k['empty']].any() and not hist[k['empty']].any()
    assert raw[k['annulus'], nm.I_HULL2] > 2 * raw[k['annulus'], nm.I_A] and raw[k['two blobs'], nm.I_HULL2] > 4 * raw[k['two blobs'], nm.I_A]
    assert hist[k['disc r=7']].sum() == raw[k['disc r=7'], nm.I_A] and np.count_nonzero(hist[k['disc r=7']]) > 20        # the random tile
    z = len(names) * tnames.index('zeros') + k['disc r=7']
    assert np.count_nonzero(hist[z]) == 1 and np.count_nonzero(hist[len(names) * tnames.index('full') + k['disc r=7']]) == 1


def test_op_channel_modes(eng, small):
    """Three distinct constant planes: CH_AS_IS reads byte 0 as red, CH_SWAP byte 2 -- the histograms of the tile and of the tile reversed."""
    tiles, masks, names, tnames = small
    b = tnames.index('planes')
    pairs = [(b, s) for s in range(len(names))]
    as_is = _run_op(eng, tiles, masks, pairs, hip.CH_AS_IS)
    swap = _run_op(eng, tiles, masks, pairs, hip.CH_SWAP)
    rgb, bgr = _reference(tiles, masks, pairs), _reference(tiles[..., ::-1], masks, pairs)
    assert np.array_equal(as_is[1], rgb[1]) and np.array_equal(swap[1], bgr[1]) and np.array_equal(as_is[0], swap[0]) and np.array_equal(as_is[0], rgb[0])
    s = names.index('disc r=7')
    assert np.argmax(rgb[1][s]) != np.argmax(bgr[1][s])                       # the two readings give different values
    from nuhtc_amd.engine import HipError
    with pytest.raises(HipError):
        _run_op(eng, tiles, masks, pairs, 2)


@pytest.mark.parametrize('side', [256, 1024])
def test_op_large_frames(eng, side):
    """256: the full frame (E runs along the frame) and an annulus over many words; 1024: the largest frame the op takes, full -- Sxx needs
    more than 32 bits, the rows are staged in 19 bands, the hull stack holds 1025 points."""
    if side == 256:
        m = cases.big_masks()
        masks = np.stack(list(m.values()))[None]
        tiles = np.stack([cases.tiles(side, side)['random']])
    else:
        masks = np.ones((1, 2, side, side), bool)
        masks[0, 1, :, : side // 2 + 7] = False
        masks[0, 1, 5::97] = False                                            # empty rows inside the rectangle
        tiles = np.stack([cases.tiles(side, side, seed=1)['random']])
    pairs = [(0, 0), (0, 1)]
    raw, hist = _run_op(eng, tiles, masks, pairs)
    want_raw, want_hist = _reference(tiles, masks, pairs)
    assert np.array_equal(raw, want_raw), (raw, want_raw)
    assert np.array_equal(hist, want_hist)
    assert raw[0, nm.I_E] == 4 * side and raw[0, nm.I_HULL2] == 2 * side * side
    if side == 1024:
        assert raw[0, nm.I_SXX] > 2 ** 32


def test_op_out_of_range_pairs_count_and_sentinel(eng, small):
    tiles, masks, names, tnames = small
    K = len(names)
    pairs = [(0, names.index('annulus')), (4, 0), (0, K), (-1, 0), (0, -1), (3, names.index('two blobs')), (1, 2), (2, 3)]
    want = _reference(tiles, masks, pairs)
    raw, hist = _run_op(eng, tiles, masks, pairs)
    assert np.array_equal(raw, want[0]) and np.array_equal(hist, want[1])
    assert not raw[1:5].any() and not hist[1:5].any() and raw[0].any() and raw[5].any()
    # n_dev smaller than n_max: the later rows keep the sentinel
    n = 3
    out = (torch.full((len(pairs), 16), -7, dtype=torch.int64, device=eng.device), torch.full((len(pairs), 256), -7, dtype=torch.int32, device=eng.device))
    raw2, hist2 = _run_op(eng, tiles, masks, pairs, n=torch.tensor([n], dtype=torch.int32, device=eng.device), out=out)
    assert np.array_equal(raw2[:n], want[0][:n]) and np.array_equal(hist2[:n], want[1][:n])
    assert (raw2[n:] == -7).all() and (hist2[n:] == -7).all()
    from nuhtc_amd.engine import HipError
    with pytest.raises(HipError):
        eng.op_nucleus_morph(torch.zeros(1, 1025, 8, 3, dtype=torch.uint8, device=eng.device), torch.zeros(1, 1, 1025, 1, dtype=torch.int32, device=eng.device),
                             torch.zeros(1, 2, dtype=torch.int32, device=eng.device))


def test_op_same_nucleus_in_a_batch_of_1_and_of_8(eng, small):
    tiles, masks, names, tnames = small
    s = names.index('L across x=31|32')
    one = _run_op(eng, tiles[:1], masks[:1, s:s + 1], [(0, 0)])
    rng = np.random.default_rng(5)
    t8 = rng.integers(0, 256, (8,) + tiles.shape[1:], dtype=np.uint8)
    m8 = rng.random((8, 3) + masks.shape[2:]) < 0.4
    t8[5], m8[5, 1] = tiles[0], masks[0, s]
    pairs = [(b, k) for b in range(8) for k in range(3)]
    many = _run_op(eng, t8, m8, pairs)
    d = pairs.index((5, 1))
    assert many[0][d].tobytes() == one[0][0].tobytes() and many[1][d].tobytes() == one[1][0].tobytes()
    want = _reference(t8, m8, pairs)                                          # and random 40 % masks: many components, holes, both words
    assert np.array_equal(many[0], want[0]) and np.array_equal(many[1], want[1])


def _export(e, dev_tiles, **kw):
    """infer + export of one batch on the engine's stream -> a snapshot of export_read()."""
    with torch.cuda.stream(e.stream):
        B = e.infer_async(dev_tiles, hip.CH_SWAP)
        e.export_async(B, **kw)
        e.stream.synchronize()
        g = e.export_read()
    assert g is not None
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in g.items()}


KEYS = {'n', 'tile', 'slot', 'boxes', 'labels', 'cn', 'xy', 'crop_box', 'crop_area', 'crop_off', 'crop_words', 'crop_total', 'pool'}


def test_engine_export_with_morphometry(eng):
    from nuhtc_amd import synth
    tiles = synth.nuclei_tiles(4, 64, start=0)
    with torch.cuda.stream(eng.stream):
        dev = eng.to_device(tiles)
    plain = _export(eng, dev)
    size_plain = eng._ex['blob_dev'].numel()
    g = _export(eng, dev, nucmorph=True)
    with torch.cuda.stream(eng.stream):
        masks = nucfeat.unpack_mask_words(eng.masks[:4].cpu().numpy())
        sync = eng.nucleus_morph(4, g['tile'], g['slot'])
    n = g['n']
    assert n > 0 and g['morph_raw'].shape == (n, 16) and g['morph_raw'].dtype == np.int64 and g['morph_hist'].shape == (n, 256) and g['morph_hist'].dtype == np.int32
    # every other field bit for bit as without the flag, and without it the layout and the keys as before
    assert set(plain) == KEYS and set(g) == KEYS | {'morph_raw', 'morph_hist'}
    for k in KEYS:
        assert np.array_equal(plain[k], g[k]), k
    again = _export(eng, dev)
    assert eng._ex['blob_dev'].numel() == size_plain and set(again) == KEYS
    both = _export(eng, dev, nucmorph=True, nucfeat=True)
    assert set(both) == KEYS | {'morph_raw', 'morph_hist', 'feat'} and np.array_equal(both['morph_raw'], g['morph_raw']) and np.array_equal(both['morph_hist'], g['morph_hist'])
    # the rows against the engine's own masks and the tiles it was given: CH_SWAP, so red is byte 2
    rgb = np.asarray(tiles)[..., ::-1]
    want_raw, want_hist = _reference(rgb, masks, list(zip(g['tile'].tolist(), g['slot'].tolist())))
    assert np.array_equal(g['morph_raw'], want_raw) and np.array_equal(g['morph_hist'], want_hist)
    some = g['morph_raw'][:, nm.I_A] > 0
    assert (g['morph_raw'][:, nm.I_A] == g['crop_area']).all() and np.array_equal(g['morph_raw'][some, nm.I_X0:nm.I_Y1 + 1], g['crop_box'][some])
    assert np.array_equal(sync[0], g['morph_raw']) and np.array_equal(sync[1], g['morph_hist'])      # the synchronous route: the same bytes
    cols, val = nm.derive(g['morph_raw'], g['morph_hist'])
    print(f'{n} kept nuclei on 4 tiles of 64 px; mean area {val[:, 0].mean():.1f}, mean solidity {val[:, cols.index("Shape.Solidity")].mean():.3f}')
    assert np.isfinite(val).all()


def test_infer_tiles_redo_route_carries_the_rows(hip_device, tmp_path, monkeypatch):
    """A batch with more kept nuclei than the export capacity is run again alone and read from the engine's own tensors (wsi._unpack,
    _gather_sync, Engine.nucleus_morph / nucleus_features, one pack_rows per record): the same records and the same rows as the packed route."""
    from nuhtc_amd import synth, weights, wsi
    from nuhtc_amd.apis import init_detector
    from nuhtc_amd.engine import Engine
    ck = str(tmp_path / 'w.pth')
    torch.save(dict(meta={}, state_dict=weights.bench_state_dict(0, obj_bias=0.0)), ck)
    model = init_detector(CFG, ck, device='cuda:0', max_batch=4)
    img = np.concatenate([np.concatenate([synth.nuclei_tile(10 + 2 * r + c, 128) for c in range(2)], 1) for r in range(2)], 0)
    tiles, coords = wsi.tile_grid(img, 64, 48)
    packed = wsi.infer_tiles(model, tiles, coords, batch_size=4, nucfeat=True, nucmorph=True)
    whole = Engine.export_async
    forced = []

    def two_rows(self, B, *a, **kw):
        forced.append(B)
        return whole(self, B, *a, **dict(kw, cap=2))
    monkeypatch.setattr(Engine, 'export_async', two_rows)
    redone = wsi.infer_tiles(model, tiles, coords, batch_size=4, nucfeat=True, nucmorph=True)
    monkeypatch.undo()
    n = len(packed['score'])
    print(f'{n} records on {len(tiles)} tiles, {len(forced)} batches exported into two rows')
    assert n > 10 and forced and packed['morph'].shape == (n, nm.ROW) and np.asarray(redone['morph']).shape == (n, nm.ROW)
    assert list(redone['tile']) == list(packed['tile']) and list(redone['label']) == list(packed['label']) and list(redone['score']) == list(packed['score'])
    assert np.array_equal(np.asarray(redone['box']), np.asarray(packed['box']))
    assert np.array_equal(np.asarray(redone['morph'], np.int64), packed['morph'])
    assert np.array_equal(np.asarray(redone['feat'], np.float32).view(np.uint32), np.asarray(packed['feat'], np.float32).view(np.uint32))
    raw, hist, origin = nm.unpack_rows(packed['morph'])
    assert np.array_equal(origin, np.asarray(coords)[np.asarray(packed['tile'])]) and (raw[:, nm.I_A] > 0).all() and (hist.sum(1) == raw[:, nm.I_A]).all()
    # and the packed rows themselves against the restatement on the slide's pixels (tile_grid cuts RGB tiles, infer_tiles reads them CH_SWAP)
    for k in range(0, n, 7):
        crop, x0, y0 = packed['mask'][k]
        t = int(packed['tile'][k])
        full = np.zeros((64, 64), bool)
        full[y0 - origin[k, 1]:y0 - origin[k, 1] + crop.shape[0], x0 - origin[k, 0]:x0 - origin[k, 0] + crop.shape[1]] = crop
        want = nm.morph_reference(np.asarray(tiles[t])[..., ::-1], full)
        assert np.array_equal(raw[k], want[0]) and np.array_equal(hist[k], want[1]), k


def _run(cmd, env=None, limit=300):
    p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, TOOL] + cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, p.returncode
    return p.stdout


def test_cli_nuclei_morph(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-morph on a synthetic .npy slide, alone and with --merge --nuclei-feat --nuclei-graph: row-aligned files,
    the documents the same bytes as without the flag, two ranks on one device the same table; the position columns against the polygons of the GeoJSON document."""
    from nuhtc_amd import cellgraph, synth, weights
    ck = tmp_path / 'w.pth'
    torch.save(dict(state_dict=weights.bench_state_dict(0, obj_bias=0.0)), ck)
    slide = np.concatenate([np.concatenate(list(synth.nuclei_tiles(5, 64, start=r * 5)), 1) for r in range(3)], 0)    # 192 x 320
    np.save(tmp_path / 's1.npy', slide)
    base = [str(tmp_path / 's1.npy'), CFG, str(ck), '--patch_size', '64', '--step_size', '48', '--batch_size', '8', '--mode', 'qupath']
    env = dict(os.environ, NUHTC_HOST_AFFINITY='0')
    where = lambda d: tmp_path / d / 'nuclei' / 's1'
    docs = lambda d: {f: open(where(d) / f, 'rb').read() for f in sorted(os.listdir(where(d))) if f.endswith('.geojson')}
    _run(base + ['--save_dir', str(tmp_path / 'plain'), '--merge'], env)
    assert not os.path.exists(where('plain') / 's1_nuclei_morph.npz')
    _run(base + ['--save_dir', str(tmp_path / 'morph'), '--nuclei-morph'], env)
    _run(base + ['--save_dir', str(tmp_path / 'all'), '--nuclei-morph', '--merge', '--nuclei-feat', '--nuclei-graph'], env)
    plain, alone, every_flag = docs('plain'), docs('morph'), docs('all')
    assert set(plain) == {'s1.geojson', 's1_point.geojson', 's1_merged.geojson'} and every_flag == plain
    assert alone == {k: v for k, v in plain.items() if k != 's1_merged.geojson'}
    every, merged = json.loads(plain['s1.geojson']), json.loads(plain['s1_merged.geojson'])
    t = nm.read_npz(str(where('morph') / 's1_nuclei_morph.npz'))
    n = len(every)
    print(f'{n} nuclei written, {len(merged)} after the merge')
    assert n > 10 and 0 < len(merged) < n
    assert t['nuclei_id'].tolist() == list(range(n)) and t['values'].shape == (n, len(nm.COLUMNS)) and t['columns'].tolist() == list(nm.COLUMNS)
    assert t['label'].tolist() == [f['properties']['label'] for f in every] and t['score'].tolist() == [f['properties']['score'] for f in every]
    assert np.isfinite(t['values']).all() and (t['raw'][:, nm.I_A] > 0).all() and (t['hist'].sum(1) == t['raw'][:, nm.I_A]).all()
    assert np.array_equal(t['values'], nm.derive(t['raw'], t['hist'], t['origin'])[1])
    col = {c: i for i, c in enumerate(nm.COLUMNS)}
    for k, f in enumerate(every):                                  # the slide-pixel rectangle of row k holds the polygon of feature k
        ring = np.array(f['geometry']['coordinates'][0])
        v = t['values'][k]
        assert v[col['Identifier.Xmin']] <= ring[:, 0].min() and ring[:, 0].max() <= v[col['Identifier.Xmax']], k
        assert v[col['Identifier.Ymin']] <= ring[:, 1].min() and ring[:, 1].max() <= v[col['Identifier.Ymax']], k
    tm = nm.read_npz(str(where('all') / 's1_nuclei_morph.npz'))
    assert len(tm['nuclei_id']) == len(merged) and [every[i] for i in tm['nuclei_id']] == merged
    for k in ('values', 'raw', 'hist', 'origin', 'label', 'score'):
        assert np.array_equal(tm[k], t[k][tm['nuclei_id']]), k
    tf = nucfeat.read_npz(str(where('all') / 's1_nuclei_feat.npz'))
    tg = cellgraph.read_npz(str(where('all') / 's1_nuclei_graph.npz'))
    assert np.array_equal(tf['nuclei_id'], tm['nuclei_id']) and np.array_equal(tg['nuclei_id'], tm['nuclei_id']) and np.array_equal(tf['label'], tm['label'])
    two = dict(env, NUHTC_ONE_DEVICE='1', NUHTC_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='4')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        two.pop(k, None)
    _run(base + ['--save_dir', str(tmp_path / 'two'), '--nuclei-morph', '--merge', '--nuclei-feat', '--nuclei-graph', '--gpus', '2'], two)
    t2 = nm.read_npz(str(where('two') / 's1_nuclei_morph.npz'))
    assert docs('two') == plain
    for k in ('nuclei_id', 'values', 'raw', 'hist', 'origin', 'label', 'score'):
        assert np.array_equal(t2[k], tm[k]), k
