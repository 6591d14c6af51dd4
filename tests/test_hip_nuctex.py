"""GPU tests of the per-nucleus texture counts (csrc/nuctex.hip): the device produces integers only, so every check is EQUALITY with the
numpy restatement (nuhtc_amd.nuctex.glcm_reference) -- nuhtc_op_nucleus_texture on the designed masks and tiles of tests/nuctex_cases.py,
Engine.export_async(nuctex=True) against the engine's own masks and tiles, the per-detection route of infer_tiles, tools/infer_wsi.py
--nuclei-texture end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nuhtc_amd import hip, nucfeat
from nuhtc_amd import nuctex as nt

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucmorph_cases as morph_cases  # noqa: E402
import nuctex_cases as cases  # noqa: E402

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
    """int64 (n, 2, 136) of the pairs (tile, slot); a pair outside the arrays gives zeros."""
    T = np.zeros((len(pairs), 2, nt.CELLS), np.int64)
    for d, (b, s) in enumerate(pairs):
        if 0 <= b < len(tiles_rgb) and 0 <= s < masks.shape[1]:
            T[d] = nt.glcm_reference(tiles_rgb[b], masks[b, s])
    return T


def _run_op(eng, tiles, masks, pairs, mode=hip.CH_AS_IS, **kw):
    return eng.op_nucleus_texture(_dev(eng, tiles), _dev(eng, nucfeat.pack_mask_words(masks)), _dev(eng, np.asarray(pairs, np.int32)), mode, **kw).cpu().numpy()


@pytest.fixture(scope='module')
def small():
    """The designed 64 x 40 masks on each of the five tiles: tiles (5, 64, 40, 3), masks (5, K, 64, 40), names, tile names, and the
    restatement of every (tile, mask), computed once."""
    t, m = cases.tiles(cases.H_SMALL, cases.W_SMALL), cases.small_masks()
    tiles, masks = np.stack(list(t.values())), np.stack([np.stack(list(m.values()))] * len(t))
    pairs = [(b, s) for b in range(len(t)) for s in range(len(m))]
    want = _reference(tiles, masks, pairs)
    want.setflags(write=False)
    return tiles, masks, list(m), list(t), pairs, want


def test_op_designed_masks_64x40(eng, small):
    tiles, masks, names, tnames, pairs, want = small
    got = _run_op(eng, tiles, masks, pairs)
    assert got.dtype == np.int32 and got.shape == (len(pairs), 2, nt.CELLS)
    for d, (b, s) in enumerate(pairs):
        assert np.array_equal(got[d], want[d]), (tnames[b], names[s], np.nonzero(got[d] != want[d]))
    k = {n: i for i, n in enumerate(names)}
    at = lambda t, n: got[len(names) * tnames.index(t) + k[n]]
    # what the cases were designed to hold, on the restatement's side and so on the device's
    assert np.unique(nt.levels(tiles[tnames.index('random')])).tolist() == list(range(16))
    assert np.unique(nt.levels(tiles[tnames.index('ramp')])).tolist() == list(range(10))
    for t in tnames:
        for n in ('empty', 'pixel', 'corner top left', 'corner bottom right', 'checkerboard', 'diagonal line'):
            assert not at(t, n).any(), (t, n)                                                 # no 4-neighbour pair: a zero row
        assert at(t, '1x2 pair').sum(1).tolist() == [1, 0] and at(t, '2x1 pair').sum(1).tolist() == [0, 1]
        assert at(t, 'pair across x=31|32').sum(1).tolist() == [1, 0]
        assert at(t, 'pair in the last row').sum(1).tolist() == [1, 0] and at(t, 'pair in the last column').sum(1).tolist() == [0, 1]
        assert at(t, '2x2 in the last corner').sum(1).tolist() == [2, 2]
        assert at(t, 'full frame').sum(1).tolist() == [64 * 39, 63 * 40]
    for t, level in (('zeros', 15), ('full', 0), ('planes', 7)):                              # one level: every pair in one diagonal cell
        row = at(t, 'full frame')
        assert row[0, nt.tri(level, level)] == 64 * 39 and row[1, nt.tri(level, level)] == 63 * 40 and np.count_nonzero(row) == 2
    G = nt.full_matrix(at('ramp', 'full frame'))
    i, j = np.mgrid[0:16, 0:16]
    assert not G[:, np.abs(i - j) > 1].any() and G[:, np.abs(i - j) == 1].any()              # the ramp: the diagonal and its neighbours
    assert np.count_nonzero(at('random', 'full frame')) > 250                                 # the random tile: 262 of the 272 cells


def test_op_channel_modes(eng, small):
    """CH_AS_IS reads byte 0 as red, CH_SWAP byte 2: the counts of the tile and of the tile with its bytes reversed."""
    tiles, masks, names, tnames, _, _ = small
    for t in ('planes', 'ramp', 'random'):
        b = tnames.index(t)
        pairs = [(b, s) for s in range(len(names))]
        as_is, swap = _run_op(eng, tiles, masks, pairs, hip.CH_AS_IS), _run_op(eng, tiles, masks, pairs, hip.CH_SWAP)
        rgb, bgr = _reference(tiles, masks, pairs), _reference(tiles[..., ::-1], masks, pairs)
        assert np.array_equal(as_is, rgb) and np.array_equal(swap, bgr), t
        assert not np.array_equal(rgb, bgr), t                                                # the two readings give different counts
    from nuhtc_amd.engine import HipError
    with pytest.raises(HipError):
        _run_op(eng, tiles, masks, [(0, 0)], 2)


@pytest.mark.parametrize('side', [256, 1024])
def test_op_large_frames(eng, side):
    """256: the full frame on a constant tile (65 280 pairs an offset in ONE cell: every add of the workgroup would meet at one address)
    and on a random one, and an annulus over many words; 1024: the largest frame the op takes, full, 1 047 552 pairs an offset -- on a
    constant tile the largest count a record can hold -- and half a frame with empty rows."""
    if side == 256:
        m = morph_cases.big_masks()
        masks = np.stack([np.stack(list(m.values()))] * 3)
        t = cases.tiles(side, side)
        tiles = np.stack([t['random'], t['planes'], t['ramp']])
        pairs = [(b, s) for b in range(3) for s in range(2)]
    else:
        masks = np.ones((2, 2, side, side), bool)
        masks[:, 1, :, : side // 2 + 7] = False
        masks[:, 1, 5::97] = False                                            # empty rows inside the rectangle
        t = cases.tiles(side, side, seed=1)
        tiles = np.stack([t['random'], t['zeros']])
        pairs = [(0, 0), (0, 1), (1, 0)]
    got = _run_op(eng, tiles, masks, pairs)
    want = _reference(tiles, masks, pairs)
    assert np.array_equal(got, want), np.nonzero(got != want)
    full = side * (side - 1)
    assert got[0].sum(1).tolist() == [full, full]
    one = got[pairs.index((1, 0))]                                            # the constant tile: one cell an offset
    assert np.count_nonzero(one) == 2 and one.max() == full and (full == 65280 or full == 1047552)


def test_op_out_of_range_pairs_count_and_sentinel(eng, small):
    tiles, masks, names, tnames, _, _ = small
    K = len(names)
    pairs = [(0, names.index('annulus')), (5, 0), (0, K), (-1, 0), (0, -1), (4, names.index('two blobs')), (1, 2), (2, names.index('disc r=7'))]
    want = _reference(tiles, masks, pairs)
    got = _run_op(eng, tiles, masks, pairs)
    assert np.array_equal(got, want)
    assert not got[1:5].any() and got[0].any() and got[5].any()
    n = 3                                                                     # n_dev smaller than n_max: the later rows keep the sentinel
    out = torch.full((len(pairs), 2, nt.CELLS), -7, dtype=torch.int32, device=eng.device)
    got2 = _run_op(eng, tiles, masks, pairs, n=torch.tensor([n], dtype=torch.int32, device=eng.device), out=out)
    assert np.array_equal(got2[:n], want[:n]) and (got2[n:] == -7).all()
    from nuhtc_amd.engine import HipError
    with pytest.raises(HipError):
        eng.op_nucleus_texture(torch.zeros(1, 1025, 8, 3, dtype=torch.uint8, device=eng.device), torch.zeros(1, 1, 1025, 1, dtype=torch.int32, device=eng.device),
                               torch.zeros(1, 2, dtype=torch.int32, device=eng.device))


def test_op_batch_of_1_and_of_8_and_two_runs(eng, small):
    tiles, masks, names, tnames, _, _ = small
    s, b = names.index('L across x=31|32'), tnames.index('ramp')
    one = _run_op(eng, tiles[b:b + 1], masks[:1, s:s + 1], [(0, 0)])
    rng = np.random.default_rng(5)
    t8 = rng.integers(0, 256, (8,) + tiles.shape[1:], dtype=np.uint8)
    m8 = rng.random((8, 3) + masks.shape[2:]) < 0.6
    t8[5], m8[5, 1] = tiles[b], masks[0, s]
    pairs = [(i, k) for i in range(8) for k in range(3)]
    many = _run_op(eng, t8, m8, pairs)
    assert many[pairs.index((5, 1))].tobytes() == one[0].tobytes() and one.any()
    assert np.array_equal(many, _reference(t8, m8, pairs))                    # and random 60 % masks: many components, holes, both words
    assert _run_op(eng, t8, m8, pairs).tobytes() == many.tobytes()            # two runs: the same bytes


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


def test_engine_export_with_texture(eng):
    from nuhtc_amd import synth
    tiles = synth.nuclei_tiles(4, 64, start=0)
    with torch.cuda.stream(eng.stream):
        dev = eng.to_device(tiles)
    plain = _export(eng, dev)
    size_plain = eng._ex['blob_dev'].numel()
    morph = _export(eng, dev, nucmorph=True)
    g = _export(eng, dev, nuctex=True)
    with torch.cuda.stream(eng.stream):
        masks = nucfeat.unpack_mask_words(eng.masks[:4].cpu().numpy())
        sync = eng.nucleus_texture(4, g['tile'], g['slot'])
    n = g['n']
    assert n > 0 and g['tex'].shape == (n, 2, nt.CELLS) and g['tex'].dtype == np.int32
    # every other field bit for bit as without the flag, and without it the layout and the keys as before
    assert set(plain) == KEYS and set(g) == KEYS | {'tex'} and set(morph) == KEYS | {'morph_raw', 'morph_hist'}
    for k in KEYS:
        assert np.array_equal(plain[k], g[k]), k
    again = _export(eng, dev)
    assert eng._ex['blob_dev'].numel() == size_plain and set(again) == KEYS
    both = _export(eng, dev, nuctex=True, nucmorph=True, nucfeat=True)
    assert set(both) == KEYS | {'tex', 'morph_raw', 'morph_hist', 'feat'} and np.array_equal(both['tex'], g['tex'])
    assert np.array_equal(both['morph_raw'], morph['morph_raw']) and np.array_equal(both['morph_hist'], morph['morph_hist'])
    # the rows against the engine's own masks and the tiles it was given: CH_SWAP, so red is byte 2
    rgb = np.asarray(tiles)[..., ::-1]
    want = _reference(rgb, masks, list(zip(g['tile'].tolist(), g['slot'].tolist())))
    assert np.array_equal(g['tex'], want)
    assert np.array_equal(sync, g['tex'])                                     # the synchronous route: the same bytes
    # a nucleus's pairs against its morphometry: 4 A = E + 2 (pairs of both offsets)
    assert np.array_equal(4 * morph['morph_raw'][:, 0], morph['morph_raw'][:, 10] + 2 * g['tex'].sum((1, 2)))
    cols, val = nt.derive(g['tex'])
    print(f'{n} kept nuclei on 4 tiles of 64 px; {g["tex"].sum() / n:.1f} pairs a nucleus, mean entropy {val[:, cols.index("Haralick.Entropy.Mean")].mean():.3f}')
    assert np.isfinite(val).all() and g['tex'].sum() > 0


def test_infer_tiles_redo_route_carries_the_rows(hip_device, tmp_path, monkeypatch):
    """A batch with more kept nuclei than the export capacity is run again alone and read from the engine's own tensors (wsi._unpack,
    _gather_sync, Engine.nucleus_texture, one pack_rows per record): the same records and the same rows as the packed route."""
    from nuhtc_amd import nucmorph as nm
    from nuhtc_amd import synth, weights, wsi
    from nuhtc_amd.apis import init_detector
    from nuhtc_amd.engine import Engine
    ck = str(tmp_path / 'w.pth')
    torch.save(dict(meta={}, state_dict=weights.bench_state_dict(0, obj_bias=0.0)), ck)
    model = init_detector(CFG, ck, device='cuda:0', max_batch=4)
    img = np.concatenate([np.concatenate([synth.nuclei_tile(10 + 2 * r + c, 128) for c in range(2)], 1) for r in range(2)], 0)
    tiles, coords = wsi.tile_grid(img, 64, 48)
    packed = wsi.infer_tiles(model, tiles, coords, batch_size=4, nucmorph=True, nuctex=True)
    without = wsi.infer_tiles(model, tiles, coords, batch_size=4)
    whole = Engine.export_async
    forced = []

    def two_rows(self, B, *a, **kw):
        forced.append(B)
        return whole(self, B, *a, **dict(kw, cap=2))
    monkeypatch.setattr(Engine, 'export_async', two_rows)
    redone = wsi.infer_tiles(model, tiles, coords, batch_size=4, nucmorph=True, nuctex=True)
    monkeypatch.undo()
    n = len(packed['score'])
    print(f'{n} records on {len(tiles)} tiles, {len(forced)} batches exported into two rows')
    assert n > 10 and forced and packed['tex'].shape == (n, nt.ROW) and np.asarray(redone['tex']).shape == (n, nt.ROW)
    assert 'tex' not in without and 'morph' not in without and list(without['score']) == list(packed['score'])
    assert list(redone['tile']) == list(packed['tile']) and list(redone['label']) == list(packed['label']) and list(redone['score']) == list(packed['score'])
    assert np.array_equal(np.asarray(redone['tex'], np.int64), packed['tex'])
    assert np.array_equal(np.asarray(redone['morph'], np.int64), packed['morph'])
    glcm = nt.unpack_rows(packed['tex'])
    raw, _, origin = nm.unpack_rows(packed['morph'])
    assert np.array_equal(4 * raw[:, nm.I_A], raw[:, nm.I_E] + 2 * glcm.sum((1, 2)))
    # and the packed rows themselves against the restatement on the slide's pixels (tile_grid cuts RGB tiles, infer_tiles reads them CH_SWAP)
    for k in range(0, n, 7):
        crop, x0, y0 = packed['mask'][k]
        t = int(packed['tile'][k])
        full = np.zeros((64, 64), bool)
        full[y0 - origin[k, 1]:y0 - origin[k, 1] + crop.shape[0], x0 - origin[k, 0]:x0 - origin[k, 0] + crop.shape[1]] = crop
        assert np.array_equal(glcm[k], nt.glcm_reference(np.asarray(tiles[t])[..., ::-1], full)), k


def _run(cmd, env=None, limit=300):
    p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, TOOL] + cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, p.returncode
    return p.stdout


def test_cli_nuclei_texture(hip_device, tmp_path):
    """tools/infer_wsi.py on a synthetic .npy slide, three starts: without the flag; with --nuclei-texture --nuclei-feat --nuclei-morph
    (row-aligned files, values == derive(glcm), every other file the same bytes); with --merge on two ranks of one device (the survivors'
    rows of the same table)."""
    from nuhtc_amd import nucmorph as nm
    from nuhtc_amd import synth, weights
    ck = tmp_path / 'w.pth'
    torch.save(dict(state_dict=weights.bench_state_dict(0, obj_bias=0.0)), ck)
    slide = np.concatenate([np.concatenate(list(synth.nuclei_tiles(5, 64, start=r * 5)), 1) for r in range(3)], 0)    # 192 x 320
    np.save(tmp_path / 's1.npy', slide)
    base = [str(tmp_path / 's1.npy'), CFG, str(ck), '--patch_size', '64', '--step_size', '48', '--batch_size', '8', '--mode', 'qupath']
    env = dict(os.environ, NUHTC_HOST_AFFINITY='0')
    where = lambda d: tmp_path / d / 'nuclei' / 's1'
    files = lambda d: {f: open(where(d) / f, 'rb').read() for f in sorted(os.listdir(where(d)))}
    _run(base + ['--save_dir', str(tmp_path / 'plain'), '--nuclei-feat', '--nuclei-morph'], env)
    _run(base + ['--save_dir', str(tmp_path / 'tex'), '--nuclei-texture', '--nuclei-feat', '--nuclei-morph'], env)
    plain, tex = files('plain'), files('tex')
    assert 's1_nuclei_texture.npz' not in plain and {'s1.geojson', 's1_point.geojson', 's1_nuclei_feat.npz', 's1_nuclei_morph.npz'} <= set(plain)
    assert set(tex) == set(plain) | {'s1_nuclei_texture.npz'}
    for f in plain:                                                            # every other file: the same bytes (of an .npz the same arrays:
        if f.endswith('.npz'):                                                 # the zip directory carries the time of writing)
            with np.load(where('plain') / f) as za, np.load(where('tex') / f) as zb:
                assert za.files == zb.files and all(za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes() for k in za.files), f
        else:
            assert tex[f] == plain[f], f
    every = json.loads(plain['s1.geojson'])
    t = nt.read_npz(str(where('tex') / 's1_nuclei_texture.npz'))
    tm = nm.read_npz(str(where('tex') / 's1_nuclei_morph.npz'))
    tf = nucfeat.read_npz(str(where('tex') / 's1_nuclei_feat.npz'))
    n = len(every)
    assert n > 10 and t['nuclei_id'].tolist() == list(range(n)) and t['values'].shape == (n, 26) and t['columns'].tolist() == list(nt.COLUMNS)
    assert t['glcm'].shape == (n, 2, nt.CELLS) and t['glcm'].dtype == np.int32
    assert np.array_equal(t['nuclei_id'], tm['nuclei_id']) and np.array_equal(t['nuclei_id'], tf['nuclei_id'])
    assert np.array_equal(t['label'], tm['label']) and np.array_equal(t['score'], tm['score'])
    assert t['label'].tolist() == [f['properties']['label'] for f in every] and t['score'].tolist() == [f['properties']['score'] for f in every]
    assert np.array_equal(t['values'], nt.derive(t['glcm'])[1]) and np.isfinite(t['values']).all()
    # row k of the texture file and row k of the morphometry file measure the same mask: 4 A = E + 2 pairs
    assert np.array_equal(4 * tm['raw'][:, nm.I_A], tm['raw'][:, nm.I_E] + 2 * t['glcm'].sum((1, 2)).astype(np.int64))
    two = dict(env, NUHTC_ONE_DEVICE='1', NUHTC_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='4')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        two.pop(k, None)
    _run(base + ['--save_dir', str(tmp_path / 'two'), '--nuclei-texture', '--nuclei-morph', '--merge', '--gpus', '2'], two)
    merged = json.loads(open(where('two') / 's1_merged.geojson').read())
    assert open(where('two') / 's1.geojson', 'rb').read() == plain['s1.geojson']
    t2 = nt.read_npz(str(where('two') / 's1_nuclei_texture.npz'))
    tm2 = nm.read_npz(str(where('two') / 's1_nuclei_morph.npz'))
    print(f'{n} nuclei written, {len(merged)} after the merge')
    assert 0 < len(merged) < n and len(t2['nuclei_id']) == len(merged) and [every[i] for i in t2['nuclei_id']] == merged
    assert np.array_equal(t2['nuclei_id'], tm2['nuclei_id'])
    for k in ('values', 'glcm', 'label', 'score'):
        assert np.array_equal(t2[k], t[k][t2['nuclei_id']]), k
