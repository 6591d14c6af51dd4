"""CPU tests of bench.py's host-side helpers (no GPU): the 10 Hz power / clock sampler against a fake sysfs tree, the argument parser, and
the output dump on a stand-in engine."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_card(root, idx, bdf, power_uw, sclk_hz, busy):
    dev = os.path.join(root, 'devices', bdf)
    hm = os.path.join(dev, 'hwmon', 'hwmon3')
    os.makedirs(hm)
    os.makedirs(os.path.join(root, 'class/drm'), exist_ok=True)
    os.makedirs(os.path.join(root, 'class/drm', f'card{idx}'))
    os.symlink(dev, os.path.join(root, 'class/drm', f'card{idx}', 'device'))
    w = lambda p, v: open(p, 'w').write(v)
    w(os.path.join(hm, 'power1_input'), f'{power_uw}\n')
    w(os.path.join(hm, 'power1_cap'), '1400000000\n')
    w(os.path.join(hm, 'freq1_input'), f'{sclk_hz}\n')
    w(os.path.join(hm, 'temp2_label'), 'junction\n'); w(os.path.join(hm, 'temp2_input'), '55000\n')
    w(os.path.join(hm, 'temp3_label'), 'mem\n'); w(os.path.join(hm, 'temp3_input'), '48000\n')
    w(os.path.join(dev, 'gpu_busy_percent'), f'{busy}\n')
    w(os.path.join(dev, 'pp_dpm_fclk'), '0: 1250Mhz *\n')
    w(os.path.join(dev, 'pp_dpm_mclk'), '0: 900Mhz\n1: 2000Mhz *\n')
    return dev


def test_power_log_phases_and_card_choice(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    root = str(tmp_path / 'sys')
    _fake_card(root, 0, '0000:05:00.0', 300_000_000, 1_400_000_000, 100)       # somebody else's GPU: busier
    _fake_card(root, 8, '0000:0a:00.0', 1_300_000_000, 2_000_000_000, 90)       # ours
    pl = bench.PowerLog(sysfs=root)
    assert len(pl.cards) == 2
    pl.mark('_setup')
    time.sleep(0.25)
    pl.mark('timed_in_flight')
    time.sleep(0.45)
    pl.mark('_after')
    time.sleep(0.15)
    csv = str(tmp_path / 'p.csv')
    out = pl.summary(csv, pci_bdf='0000:0a:00.0')
    assert out['available'] and out['device'].endswith('0000:0a:00.0') and out['device_chosen_by'].startswith('pci bus id') and out['power_cap_w'] == 1400.0
    assert list(out['phases']) == ['timed_in_flight']                          # phases whose name starts with '_' are not reported
    ph = out['phases']['timed_in_flight']
    assert 2 <= ph["samples"] <= 7 and ph['power_w_mean'] == 1300.0 and ph['sclk_mhz_mean'] == 2000.0
    assert ph['temp_junction_c_max'] == 55.0 and ph['temp_mem_c_max'] == 48.0 and ph['fclk_mhz_mean'] == 1250.0 and ph['mclk_mhz_mean'] == 2000.0
    lines = open(csv).read().splitlines()
    assert lines[0].startswith('t_s,power_w,sclk_mhz') and lines[-1].endswith('_after') and any(l.endswith('timed_in_flight') for l in lines)
    # without a bus id (or without a match) the busiest card is taken, and the line says so
    pl2 = bench.PowerLog(sysfs=root)
    pl2.mark('x')
    time.sleep(0.25)
    out2 = pl2.summary(None, pci_bdf='0000:ff:00.0')
    assert out2['device'].endswith('0000:05:00.0') and out2['device_chosen_by'] == 'busiest card in sysfs'
    # a box without readable hwmon files
    assert bench.PowerLog(sysfs=str(tmp_path / 'none')).summary() == {'available': False, 'note': 'no amdgpu hwmon files readable on this box'}


def test_bench_help_lists_the_contract_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True, check=True).stdout
    for flag in ('--gpus', '--steps', '--warmup', '--in-flight', '--cpu-full', '--power-csv', '--fixed-load', '--full', '--dump-outputs'):
        assert flag in out
    # the options of the --full figures are refused on a plain run instead of being ignored
    err = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gemm-shapes'], capture_output=True, text=True)
    assert err.returncode == 2 and '--gemm-shapes belongs to --full' in err.stderr


def test_dump_outputs_unpacks_what_the_engine_returns(tmp_path):
    """bench.dump_outputs on a stand-in engine (host tensors in the Engine's buffer layout, image width 200 in rows padded to 224): every array
    float32 / float64, the detections in (tile, slot) order, the masks unpacked and cropped exactly as Engine.results does it (bit j of word
    w = column 32 w + j), and the seeded tile / record samples taking what they name."""
    import types
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    B, K, H, W, TW = 3, 7, 40, 200, 224
    g = torch.Generator().manual_seed(1)
    e = types.SimpleNamespace(image_hw=(H, W), cfg=types.SimpleNamespace(tile_h=H, tile_w=TW), counts=torch.tensor([5, 0, 7], dtype=torch.int32),
                              boxes=torch.rand(B, K, 5, generator=g), labels=torch.randint(0, 5, (B, K), dtype=torch.int32, generator=g),
                              keep=torch.randint(0, 2, (B, K), dtype=torch.uint8, generator=g),
                              masks=torch.randint(-2 ** 31, 2 ** 31 - 1, (B, K, H, TW // 32), dtype=torch.int32, generator=g))
    head = torch.rand(4, 9, dtype=torch.float64)
    head[:, 6] = torch.tensor([2., 3., 1., 4.])            # ring lengths
    verts = torch.randint(0, 99, (10, 2), dtype=torch.int32)
    crops = torch.randint(0, 99, (4, 6))
    gathered = [[head, verts, crops, torch.zeros(3, dtype=torch.int32), torch.zeros(0, dtype=torch.uint8), torch.tensor([0])]]
    names = bench.dump_outputs(str(tmp_path), e, B, gathered, sample=6)
    a = {n: np.load(tmp_path / (n + '.npy')) for n in names}
    assert sorted(os.listdir(tmp_path)) == sorted(n + '.npy' for n in names)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    ref = np.concatenate([np.unpackbits(e.masks[b, :int(e.counts[b])].numpy().view(np.uint8).reshape(-1, H, TW // 8), axis=-1,
                                        bitorder='little')[..., :W] for b in range(B)])
    assert np.array_equal(a['tile_index'], [0, 1, 2]) and np.array_equal(a['det_tile'], [0] * 5 + [2] * 7)
    assert np.array_equal(a['det_boxes'][5:], e.boxes[2].numpy()) and np.array_equal(a['det_labels'][:5], e.labels[0, :5].numpy())
    assert np.array_equal(a['det_keep'][5:], e.keep[2].numpy())
    assert np.array_equal(a['det_mask_area'], ref.sum((1, 2)))
    assert a['mask_sample'].shape == (6, H, W) and np.array_equal(a['mask_sample'], ref[a['mask_sample_index'].astype(int)])
    assert np.array_equal(a['mask_coverage'], np.stack([ref[:5].sum(0), np.zeros((H, W)), ref[5:].sum(0)]))
    assert np.array_equal(a['records_index'], [0, 1, 2, 3]) and np.array_equal(a['records_head'], head.numpy())
    assert np.array_equal(a['records_rings'], verts.numpy()) and np.array_equal(a['records_crops'], crops.numpy())
    # samples: 2 of the 3 tiles, 2 of the 4 records (each with its own ring)
    names = bench.dump_outputs(str(tmp_path / 's'), e, B, gathered, sample=3, max_tiles=2, max_records=2)
    s = {n: np.load(tmp_path / 's' / (n + '.npy')) for n in names}
    tiles, rec = s['tile_index'].astype(int), s['records_index'].astype(int)
    assert len(tiles) == 2 and len(rec) == 2
    first = np.concatenate([[0], np.cumsum(e.counts.numpy())])
    rows = np.concatenate([np.arange(first[t], first[t + 1]) for t in tiles])
    assert np.array_equal(s['det_tile'], np.repeat(tiles, e.counts.numpy()[tiles])) and np.array_equal(s['det_mask_area'], ref[rows].sum((1, 2)))
    assert np.array_equal(s['mask_sample'], ref[rows][s['mask_sample_index'].astype(int)])
    off = [0, 2, 5, 6, 10]
    assert np.array_equal(s['records_head'], head.numpy()[rec])
    assert np.array_equal(s['records_rings'], np.concatenate([verts.numpy()[off[i]:off[i + 1]] for i in rec]))
