"""The device encoder of COCO run-length masks (csrc/rle.hip: nuhtc_rle_encode) against the host encoder (nuhtc_amd/cocomask.py) on the
designed masks of tests/rle_cases.py, then through Engine.export_async(rle=True) and tools/infer_wsi.py --rle-on gpu.  Integer work on
both sides: every comparison is exact equality."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from nuhtc_amd import cocomask, hip
import rle_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs/nuhtc/htc_lite_swin_pannuke_infer.py')
FILL, MARK = 0xAA, -7            # what the output buffers hold before a call
SMALL = (RC.H, RC.W)


@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    return Engine(weights.bench_state_dict(0, obj_bias=0.0), device=0, max_batch=4, tile=(128, 128))


def run(eng, names, pool_cap=None, n=None, pool_bytes=None, run_cap=RC.RUN_CAP):
    """One call of Engine.rle_encode on the named cases (one frame size) with marked output buffers -> numpy (len, off, bytes, bbox)."""
    masks = [RC.cases()[k] for k in names]
    H, W = masks[0].shape
    dev = eng.device
    words = torch.from_numpy(RC.pack(masks).view(np.int32)).to(dev)
    total = sum(len(RC.expected()[k][0]) for k in names)
    pool_bytes = pool_bytes or total + 64
    out = (torch.full((len(names),), MARK, dtype=torch.int32, device=dev), torch.full((len(names) + 1,), MARK, dtype=torch.int32, device=dev),
           torch.full((pool_bytes,), FILL, dtype=torch.uint8, device=dev), torch.full((len(names), 4), MARK, dtype=torch.int32, device=dev))
    n_dev = torch.tensor([n], dtype=torch.int32, device=dev) if n is not None else None
    got = eng.rle_encode(words, H, W, run_cap=run_cap, n=n_dev, pool_cap=pool_bytes if pool_cap is None else pool_cap, out=out)
    return [t.cpu().numpy() for t in got]


def check_strings(names, ln, off, data, bbox, limit=None):
    """Every named case's string and box against the host encoder; strings that end past `limit` are not looked at.  -> names checked."""
    seen = []
    for i, name in enumerate(names):
        want, box, ncounts = RC.expected()[name]
        if ncounts > RC.RUN_CAP:
            assert ln[i] == -1 and bbox[i].tolist() == [0, 0, 0, 0], name
            continue
        assert ln[i] == len(want), (name, ln[i], len(want))
        assert bbox[i].tolist() == box, (name, bbox[i].tolist(), box)
        if limit is None or off[i] + ln[i] <= limit:
            assert data[off[i]:off[i] + ln[i]].tobytes() == want, name
            seen.append(name)
    return seen


def test_rle_op_designed_masks(eng):
    for shape, names in RC.frames().items():          # all cases of a frame size in one call
        ln, off, data, bbox = run(eng, names)
        check_strings(names, ln, off, data, bbox)
        assert [k for k, v in zip(names, ln) if v == -1] == (['big_checkerboard'] if shape == (128, 128) else [])
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.maximum(ln, 0))]))          # the exclusive scan, total in off[n]
        assert off[-1] == sum(len(RC.expected()[k][0]) for k in names if k != 'big_checkerboard')
        assert len(data) > off[-1] and (data[off[-1]:] == FILL).all()                             # nothing past the total


def test_rle_op_pool_overflow(eng):
    names = RC.frames()[SMALL]
    total = sum(len(RC.expected()[k][0]) for k in names)
    pool_cap = total // 2 + 3
    ln, off, data, bbox = run(eng, names, pool_cap=pool_cap, pool_bytes=total + 64)
    assert off[-1] == total and np.array_equal(off, np.concatenate([[0], np.cumsum(ln)]))        # the needed total, not the written one
    seen = check_strings(names, ln, off, data, bbox, limit=pool_cap)
    assert 0 < len(seen) < len(names) and seen == names[:len(seen)]
    end = off[len(seen)]                           # the strings that fit are a prefix; the first that does not is left out whole
    assert end <= pool_cap and (data[end:] == FILL).all()


def test_rle_op_n_from_device(eng):
    names = RC.frames()[SMALL]
    n = 7
    ln, off, data, bbox = run(eng, names, n=n)
    check_strings(names[:n], ln[:n], off, data, bbox[:n])
    assert (ln[n:] == MARK).all() and (bbox[n:] == MARK).all() and (off[n + 1:] == MARK).all()
    assert off[n] == ln[:n].sum() and (data[off[n]:] == FILL).all()
    over = run(eng, names[:5], n=9)                # a count past n_max is clamped
    check_strings(names[:5], *over)
    zero = run(eng, names[:5], n=0)
    assert (zero[0] == MARK).all() and zero[1].tolist() == [0] + [MARK] * 5 and (zero[2] == FILL).all()


def test_rle_op_deterministic(eng):
    names = RC.frames()[SMALL]
    a, b = run(eng, names), run(eng, names)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_rle_op_run_cap_and_refusals(eng):
    """run_cap is the number of counts a mask may have: a mask with exactly that many is encoded, one more is given up on."""
    names = ['word_seam_row', 'pixel_mid', 'empty']          # 73, 3 and 1 counts
    for cap, gave_up in ((73, []), (72, [0]), (2, [0, 1]), (1, [0, 1])):
        ln = run(eng, names, run_cap=cap)[0]
        assert np.flatnonzero(ln == -1).tolist() == gave_up, cap
    lib = hip.load()
    w = torch.zeros(4, 64 * 96 // 32, dtype=torch.int32, device=eng.device)
    o = [torch.full((k,), MARK, dtype=torch.int32, device=eng.device) for k in (4, 5, 16)]
    data = torch.full((64,), FILL, dtype=torch.uint8, device=eng.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda H, W, run_cap: lib.nuhtc_rle_encode(0, vp(w), None, 4, H, W, run_cap, vp(o[0]), vp(o[1]), vp(data), 64, vp(o[2]), None)
    assert [call(64, 95, 1024), call(2048, 1024, 1024), call(64, 96, 0)] == [hip.E_INVALID] * 3
    torch.cuda.synchronize()
    assert all((t == MARK).all() for t in o) and (data == FILL).all()


def test_rle_op_full_capacity_encodes_the_checkerboard(eng):
    """With the kernel's largest run_cap (hip.RLE_MAX_RUNS, what Engine.export_async passes) the 4097 counts of the checkerboard are
    encoded on the device: more counts than threads of a workgroup, so the count loop and its scan take several rounds."""
    names = RC.frames()[(RC.BIG, RC.BIG)]
    ln, off, data, bbox = run(eng, names, run_cap=hip.RLE_MAX_RUNS)
    for i, name in enumerate(names):
        want, box, ncounts = RC.expected()[name]
        assert ln[i] == len(want) and data[off[i]:off[i] + ln[i]].tobytes() == want and bbox[i].tolist() == box, name
    assert off[-1] == ln.sum() and (data[off[-1]:] == FILL).all()
    assert (run(eng, names, run_cap=1 << 20)[0] == ln).all()          # a larger request is taken as the ceiling


KEYS = {'n', 'tile', 'slot', 'boxes', 'labels', 'cn', 'xy', 'crop_box', 'crop_area', 'crop_off', 'crop_words', 'crop_total', 'pool'}


def test_export_rle_matches_host_encoder(eng):
    from nuhtc_amd import synth
    tiles = np.stack([synth.nuclei_tile(60 + k, 128) for k in range(4)])
    snap = lambda g: {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in g.items()}
    with torch.cuda.stream(eng.stream):
        B = eng.infer_async(eng.to_device(tiles), hip.CH_SWAP)
        eng.export_async(B)
        eng.stream.synchronize()
        before = snap(eng.export_read())
        size_before = eng._ex['blob_dev'].numel()
        eng.export_async(B, rle=True)
        eng.stream.synchronize()
        g = snap(eng.export_read())
        masks = [eng.export_full_mask(k) for k in range(g['n'])]
        eng.export_async(B)
        eng.stream.synchronize()
        after = snap(eng.export_read())
        size_after = eng._ex['blob_dev'].numel()
    assert g['n'] > 20 and g['rle_total'] <= g['rle_pool'] and (g['rle_len'] > 0).all()
    assert np.array_equal(g['rle_off'], np.cumsum(g['rle_len']) - g['rle_len']) and g['rle_total'] == g['rle_len'].sum()
    for k, m in enumerate(masks):
        r = cocomask.encode(m)
        assert g['rle_bytes'][g['rle_off'][k]:g['rle_off'][k] + g['rle_len'][k]].tobytes() == r['counts'].encode('ascii'), k
        assert g['rle_bbox'][k].tolist() == cocomask.to_bbox(r), k
    print('longest string', int(g['rle_len'].max()), 'bytes over', g['n'], 'kept detections of 128-px tiles')
    # rle=False: the layout, the size and every returned key as without the feature
    assert set(before) == KEYS and set(after) == KEYS and set(g) == KEYS | {'rle_len', 'rle_off', 'rle_bbox', 'rle_bytes', 'rle_total', 'rle_pool'}
    assert size_after == size_before
    for k in KEYS:
        assert np.array_equal(before[k], after[k]) and np.array_equal(before[k], g[k]), k


def test_infer_wsi_rle_on_gpu_writes_the_same_coco_json(hip_device, tmp_path):
    from nuhtc_amd import synth, weights
    H, W = 768, 1024
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    blob = ((yy - 380) / 300.0) ** 2 + ((xx - 500) / 420.0) ** 2 <= 1
    tex = np.concatenate([np.concatenate([synth.nuclei_tile(40 + 4 * r + c, 256) for c in range(W // 256)], 1) for r in range(H // 256)], 0)
    img = np.full((H, W, 3), 235, np.uint8)
    img[blob] = tex[blob]
    np.save(tmp_path / 'slide.npy', img)
    ck = tmp_path / 'w.pth'
    torch.save(dict(state_dict=weights.bench_state_dict(0, obj_bias=0.0)), ck)
    docs = {}
    for where in ('host', 'gpu'):
        cmd = ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'tools/infer_wsi.py'), str(tmp_path / 'slide.npy'), CFG, str(ck), '--seg', '--patch',
               '--patch_size', '128', '--step_size', '96', '--batch_size', '16', '--seg_downsample', '4', '--save_dir', str(tmp_path / where), '--mode', 'coco',
               '--rle-on', where]
        done = subprocess.run(cmd, check=True, capture_output=True, text=True)
        docs[where] = open(tmp_path / where / 'nuclei/slide/coco_nuclei.json', 'rb').read()
        fell = re.findall(r'--rle-on gpu: (\d+) of (\d+) run-length masks fell back to the host encoder', done.stderr)
        assert fell == ([] if where == 'host' else [('0', str(len(json.loads(docs[where])['annotations'])))])
    assert docs['gpu'] == docs['host'] and len(json.loads(docs['host'])['annotations']) > 20
    assert sorted(os.listdir(tmp_path / 'gpu/imgs/slide')) == sorted(os.listdir(tmp_path / 'host/imgs/slide'))
