"""GPU tests of tile feature extraction: nuhtc_features (backbone + FPN + csrc/pool.hip) against the oracle and the reference goldens,
against the maps of the detection path, its determinism, the features_only engine, and tools/extract_features_nuhtc.py end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, 'configs', 'nuhtc', 'htc_lite_swin_pannuke_infer.py')
TOOL = os.path.join(ROOT, 'tools', 'extract_features_nuhtc.py')
# Tolerance against the oracle's maps averaged in float64.  The existing tests hold each element of x0..x3 to 2e-4 absolute
# (test_hip_dense.py / test_hip_edges.py); a mean of H*W such elements carries at most that error and in practice far less (the
# elementwise errors are rounding noise of both signs); the pooling itself adds ~1e-7 relative (fp64 sums, one fp32 rounding).
ATOL, RTOL = 1e-5, 1e-4


def _detector(sd, max_batch=16):
    from nuhtc_amd.apis import init_detector
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = init_detector(CONFIG, None, device='cuda:0', max_batch=max_batch)
    model.state_dict = sd
    return model


def _feat(model, tiles, mode):
    """model_feat for the ndarray convention (CH_SWAP); the same engine with the file convention for channel_mode 0."""
    from nuhtc_amd import apis
    if mode == 1:
        return apis.model_feat(model, list(tiles))
    return model.feature_engine(tiles.shape[1:3]).features(tiles, mode)


def _f64_means(maps):
    return np.concatenate([m.double().mean(dim=(2, 3)).numpy() for m in maps], 1)


@pytest.mark.parametrize('case', ['small_b2', 'pad_b2', 'five_b2'])
def test_features_vs_oracle_and_reference_golden(hip_device, case):
    from oracle import model as O
    g = G.load(case)
    sd = G.seeded_sd(g)
    tiles, mode = g['tiles'], int(g['channel_mode'])
    got = _feat(_detector(sd), tiles, mode)
    assert got.shape == (len(tiles), 256) and got.dtype == np.float32
    with torch.no_grad():
        x = O.fpn(sd, O.backbone(sd, O.preprocess(tiles, mode)))
    ref = _f64_means(x)
    err = np.abs(got - ref)
    print(f'{case}: max |feat - oracle mean| {err.max():.3e}, max rel {(err / np.maximum(np.abs(ref), 1e-12)).max():.3e}')
    assert (err <= ATOL + RTOL * np.abs(ref)).all(), err.max()
    for l in range(4):     # the reference's own maps: sum over tiles and channels of mean * H*W = the golden sum of x_l
        H, W = (int(v) for v in g[f'x{l}.shape'][2:])
        s = float(got[:, 64 * l:64 * (l + 1)].astype(np.float64).sum() * H * W)
        want, asum = float(g[f'x{l}.sum']), float(g[f'x{l}.asum'])
        print(f'  x{l}: sum {s:.6e} golden {want:.6e} (asum {asum:.3e})')
        assert abs(s - want) <= RTOL * asum, (l, s, want)


def test_features_equal_the_detection_maps(hip_device):
    """nuhtc_features pools the maps the detection path computes: the float64 mean of Engine.buffer('x{l}') after nuhtc_infer on a full
    engine equals the features within 1e-6 relative; the buffers stay readable after nuhtc_features."""
    from nuhtc_amd.engine import Engine
    g = G.load('five_b2')
    sd = G.seeded_sd(g)
    tiles, mode = g['tiles'], int(g['channel_mode'])
    eng = Engine(sd, device=0, max_batch=len(tiles), tile=tiles.shape[1:3])
    dev = eng.to_device(tiles)
    eng.infer_async(dev, mode)
    eng.check()
    maps = [eng.buffer(f'x{l}')[:len(tiles)].cpu().permute(0, 3, 1, 2) for l in range(4)]
    ref = _f64_means(maps)
    eng.features_async(dev, mode)
    got = eng.feat[:len(tiles)].cpu().numpy()
    err = np.abs(got - ref)
    print(f'max |feat - mean(x after infer)| {err.max():.3e}, max rel {(err / np.maximum(np.abs(ref), 1e-30)).max():.3e}')
    assert (err <= 1e-6 * np.abs(ref) + 1e-12).all()
    after = [eng.buffer(f'x{l}')[:len(tiles)].cpu().permute(0, 3, 1, 2) for l in range(4)]
    err2 = np.abs(got - _f64_means(after))
    assert (err2 <= 1e-6 * np.abs(_f64_means(after)) + 1e-12).all()
    print('x maps after nuhtc_features bitwise those after nuhtc_infer:', all(torch.equal(a, b) for a, b in zip(maps, after)))


def test_features_are_bitwise_independent_of_the_batch_split(hip_device):
    from nuhtc_amd import synth, weights
    from nuhtc_amd.engine import Engine
    sd = weights.seeded_state_dict(0)
    tiles = synth.nuclei_tiles(40, 64, start=3)
    eng = Engine(sd, device=0, max_batch=16, tile=(64, 64), features_only=1)
    dev = eng.to_device(tiles)
    runs = []
    for bs in (1, 7, 16):
        out = torch.empty(40, 256, dtype=torch.float32, device=eng.device)
        for i in range(0, 40, bs):
            eng.features_async(dev[i:i + bs], 1, out=out[i:i + bs])
        runs.append(out.cpu())
    runs.append(torch.from_numpy(eng.features(tiles, 1)))
    runs.append(torch.from_numpy(eng.features(tiles, 1)))
    for r in runs[1:]:
        assert torch.equal(r, runs[0])
    assert torch.isfinite(runs[0]).all() and float(runs[0].abs().sum()) > 0


def test_features_only_engine(hip_device):
    """Finalizes with the backbone and neck tensors alone, returns the full engine's features bit for bit, refuses nuhtc_infer."""
    import ctypes
    from nuhtc_amd import hip, synth, weights
    from nuhtc_amd.engine import Engine, HipError
    sd = weights.seeded_state_dict(1)
    bb = {k: v for k, v in sd.items() if k.startswith(('backbone.', 'neck.'))}
    assert len(bb) < len(sd)
    tiles = synth.nuclei_tiles(5, 96, start=0)
    fo = Engine(bb, device=0, max_batch=5, tile=(96, 96), features_only=1)
    with pytest.raises(HipError, match='missing weight'):
        Engine(bb, device=0, max_batch=5, tile=(96, 96))
    fo_all = Engine(sd, device=0, max_batch=5, tile=(96, 96), features_only=1)      # the heads' tensors accepted and dropped
    full = Engine(sd, device=0, max_batch=5, tile=(96, 96))
    a, b, c = fo.features(tiles, 1), fo_all.features(tiles, 1), full.features(tiles, 1)
    assert np.array_equal(a, c) and np.array_equal(b, c)
    dev = fo.to_device(tiles)
    rc = fo.lib.nuhtc_infer(fo.h, ctypes.c_void_p(dev.data_ptr()), 5, 1, None, ctypes.byref(hip.Dets()))
    assert rc == hip.E_STATE
    with pytest.raises(HipError, match='features_only'):
        fo.infer_async(dev, 1)
    fo.features_async(dev, 1)          # the engine is still usable
    for l in range(4):
        assert fo.buffer(f'x{l}').shape[-1] == 64
    assert np.array_equal(fo.feat[:5].cpu().numpy(), c)


def _run(cmd, env=None, limit=600):
    p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, TOOL] + cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    print(p.stdout[-3000:], p.stderr[-3000:])
    assert p.returncode == 0, p.returncode
    return p.stdout


def test_cli_end_to_end(hip_device, tmp_path):
    """tools/extract_features_nuhtc.py on a synthetic .npy slide with a reference-layout patches/<id>.h5: --gpus 1, a second run that
    skips, two ranks on one device, --target_patch_size; rows in coordinate order and equal to model_feat of the same tiles."""
    from nuhtc_amd import features, h5coords, synth, tilestore, weights
    if not h5coords.available():
        pytest.skip('no HDF5 back end')
    sd = weights.seeded_state_dict(0)
    ck = tmp_path / 'w.pth'
    torch.save(dict(state_dict=sd), ck)
    (tmp_path / 'h5' / 'patches').mkdir(parents=True)
    (tmp_path / 'wsi').mkdir()
    slide = np.concatenate([np.concatenate(list(synth.nuclei_tiles(5, 64, start=r * 5)), 1) for r in range(3)], 0)    # 192 x 320
    np.save(tmp_path / 'wsi' / 's1.npy', slide)
    coords = np.array([[64 * i, 64 * j] for j in range(3) for i in range(5)][::-1] + [[290, 170], [-10, 5]], np.int64)     # edge tiles pad
    h5coords.write_coords(str(tmp_path / 'h5' / 'patches' / 's1.h5'), coords, dict(patch_size=64, patch_level=0, name='s1'))
    (tmp_path / 'list.csv').write_text('slide_id\ns1.npy\n')
    base = ['--config', CONFIG, '--checkpoint', str(ck), '--data_h5_dir', str(tmp_path / 'h5'), '--data_slide_dir', str(tmp_path / 'wsi'),
            '--slide_ext', '.npy', '--csv_path', str(tmp_path / 'list.csv')]
    env = dict(os.environ, NUHTC_HOST_AFFINITY='0')
    _run(base + ['--feat_dir', str(tmp_path / 'f1'), '--gpus', '1', '--batch_size', '8'], env)
    r = h5coords.read_features(str(tmp_path / 'f1' / 'h5_files' / 's1.h5'))
    pt = torch.load(tmp_path / 'f1' / 'pt_files' / 's1.pt')
    assert np.array_equal(r['coords'], coords) and np.array_equal(r['features'], pt.numpy()) and pt.shape == (len(coords), 256)
    bag = tilestore.TileBag(np.load(tmp_path / 'wsi' / 's1.npy'), coords, 64)
    tiles = bag.read(0, len(bag))
    model = _detector(sd)
    from nuhtc_amd.apis import model_feat
    want = model_feat(model, list(tiles))
    print('CLI rows == model_feat bitwise:', np.array_equal(r['features'], want), 'max diff', float(np.abs(r['features'] - want).max()))
    np.testing.assert_allclose(r['features'], want, rtol=1e-6, atol=1e-7)
    out = _run(base + ['--feat_dir', str(tmp_path / 'f1')], env)
    assert 'skipped s1' in out
    two = dict(env, NUHTC_ONE_DEVICE='1', NUHTC_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='4')
    _run(base + ['--feat_dir', str(tmp_path / 'f2'), '--gpus', '2', '--batch_size', '8'], two)
    r2 = h5coords.read_features(str(tmp_path / 'f2' / 'h5_files' / 's1.h5'))
    assert np.array_equal(r2['features'], r['features']) and np.array_equal(r2['coords'], coords)
    _run(base + ['--feat_dir', str(tmp_path / 'f3'), '--target_patch_size', '48'], env)
    r3 = h5coords.read_features(str(tmp_path / 'f3' / 'h5_files' / 's1.h5'))
    want3 = model_feat(model, list(features.resize_tiles(tiles, (48, 48))))
    np.testing.assert_allclose(r3['features'], want3, rtol=1e-6, atol=1e-7)
    assert not np.allclose(r3['features'], r['features'])
