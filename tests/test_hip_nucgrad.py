"""GPU tests of the per-nucleus gradient integers (csrc/nucgrad.hip): the device produces integers only, so every check is EQUALITY with the
numpy restatement (nuhtc_amd.nucgrad.grad_reference) -- nuhtc_op_nucleus_gradient on the designed masks and tiles of
tests/nucgrad_cases.py, the threshold, the list and frame handling, the largest frames, repeatability, the document route
(ringfeat.measure(gradient=True)) and tools/wsi_feat_extract.py --gradient end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nuhtc_amd import contours, hip, nucfeat, ringfeat
from nuhtc_amd import nucgrad as ng

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucgrad_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'wsi_feat_extract.py')
CLASSES = ('T', 'I', 'C', 'D', 'E')


@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    return Engine(weights.bench_state_dict(0, obj_bias=3.0), device=0, max_batch=4, tile=(64, 64))


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _reference(tiles_rgb, masks, pairs, T=1):
    """int64 (n, 18) of the pairs (tile, slot); a pair outside the arrays gives zeros."""
    out = np.zeros((len(pairs), ng.ROW), np.int64)
    for d, (b, s) in enumerate(pairs):
        if 0 <= b < len(tiles_rgb) and 0 <= s < masks.shape[1]:
            out[d] = ng.grad_reference(tiles_rgb[b], masks[b, s], T)
    return out


def _run_op(eng, tiles, masks, pairs, mode=hip.CH_AS_IS, T=1, **kw):
    return eng.op_nucleus_gradient(_dev(eng, tiles), _dev(eng, nucfeat.pack_mask_words(masks)), _dev(eng, np.asarray(pairs, np.int32)), mode, T, **kw).cpu().numpy()


@pytest.fixture(scope='module')
def small():
    """Every designed 64 x 40 mask on five tiles: tiles (5, 64, 40, 3), masks (5, K, 64, 40), mask names, tile names, the pairs and the
    restatement of every (tile, mask) at T = 1, computed once."""
    every, m = cases.tiles(cases.H_SMALL, cases.W_SMALL), cases.small_masks()
    t = {k: every[k] for k in cases.GPU_TILES}
    tiles, masks = np.stack(list(t.values())), np.stack([np.stack(list(m.values()))] * len(t))
    pairs = [(b, s) for b in range(len(t)) for s in range(len(m))]
    want = _reference(tiles, masks, pairs)
    want.setflags(write=False)
    return tiles, masks, list(m), list(t), pairs, want


def test_op_designed_masks_64x40(eng, small):
    tiles, masks, names, tnames, pairs, want = small
    got = _run_op(eng, tiles, masks, pairs)
    assert got.dtype == np.int64 and got.shape == (len(pairs), ng.ROW) and len(tnames) == 5
    for d, (b, s) in enumerate(pairs):
        assert np.array_equal(got[d], want[d]), (tnames[b], names[s], got[d], want[d])
    at = lambda t, n: got[len(names) * tnames.index(t) + names.index(n)]
    # what the cases were designed to hold, on the restatement's side and so on the device's
    for t in tnames:
        assert not at(t, 'empty').any()
        assert at(t, 'full frame')[ng.I_A] == 64 * 40 and at(t, 'full frame')[ng.I_HIST:].sum() == 64 * 40
    assert at('planes', 'full frame').tolist() == [2560, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2560, 0, 0, 0, 0]
    assert at('vertical step', 'full frame').tolist() == [2560, 128 * 510, 128 * 510 ** 2, 128 * 510 ** 3, 128 * 510 ** 4, 0, 510, 64, 2432, 0, 0, 0, 0, 0, 0, 0, 0, 128]
    assert at('ridge', 'full frame')[ng.I_EDGE] == 64                                            # the plateau two pixels wide counts once a row
    assert at('random', 'pixel at x=31')[ng.I_A] == 1 and at('random', 'pixel at x=32')[ng.I_A] == 1
    assert at('random', 'full frame')[ng.I_EDGE] > 300 and np.count_nonzero(at('random', 'full frame')[ng.I_HIST:]) == 10


def test_op_channel_modes(eng, small):
    """CH_AS_IS reads byte 0 as red, CH_SWAP byte 2: the rows of the tile and of the tile with its bytes reversed; on a coloured tile the
    two readings differ."""
    tiles, masks, names, tnames, _, _ = small
    for t in ('ramp', 'random'):
        b = tnames.index(t)
        pairs = [(b, s) for s in range(len(names))]
        as_is, swap = _run_op(eng, tiles, masks, pairs, hip.CH_AS_IS), _run_op(eng, tiles, masks, pairs, hip.CH_SWAP)
        rgb, bgr = _reference(tiles, masks, pairs), _reference(tiles[..., ::-1], masks, pairs)
        assert np.array_equal(as_is, rgb) and np.array_equal(swap, bgr), t
        assert not np.array_equal(rgb, bgr), t


def test_op_edge_threshold(eng, small):
    from nuhtc_amd.engine import HipError
    tiles, masks, names, tnames, _, want1 = small
    b = tnames.index('random')
    pairs = [(b, s) for s in range(len(names))]
    edges = []
    for T in (1, 400, 1442):
        got = _run_op(eng, tiles, masks, pairs, T=T)
        assert np.array_equal(got, _reference(tiles, masks, pairs, T)), T
        edges.append(got[:, ng.I_EDGE])
        keep = [i for i in range(ng.ROW) if i != ng.I_EDGE]
        assert np.array_equal(got[:, keep], want1[b * len(names):(b + 1) * len(names)][:, keep])    # the threshold moves the edge count alone
    assert (edges[0] >= edges[1]).all() and (edges[1] >= edges[2]).all()                        # monotone non-increasing
    k = names.index('full frame')
    assert edges[0][k] > edges[1][k] > 0
    for T in (0, 1443):
        with pytest.raises(HipError):
            _run_op(eng, tiles, masks, [(0, 0)], T=T)
    with pytest.raises(HipError):
        _run_op(eng, tiles, masks, [(0, 0)], 2)                                                  # a bad channel_mode


def test_op_list_and_frame_handling(eng, small):
    tiles, masks, names, tnames, _, _ = small
    K = len(names)
    pairs = [(0, names.index('annulus')), (5, 0), (0, K), (-1, 0), (0, -1), (4, names.index('two blobs')), (1, 2), (2, names.index('disc r=7'))]
    want = _reference(tiles, masks, pairs)
    got = _run_op(eng, tiles, masks, pairs)
    assert np.array_equal(got, want)
    assert not got[1:5].any() and got[0].any() and got[5].any()                                 # an entry outside the batch: a zero row
    n = 3                                                                                       # n_dev below n_max: the later rows keep the poison
    out = torch.full((len(pairs), ng.ROW), -7, dtype=torch.int64, device=eng.device)
    got2 = _run_op(eng, tiles, masks, pairs, n=torch.tensor([n], dtype=torch.int32, device=eng.device), out=out)
    assert np.array_equal(got2[:n], want[:n]) and (got2[n:] == -7).all()
    rng = np.random.default_rng(9)
    for H, W in ((7, 33), (9, 1), (1, 1), (1, 40)):                                             # a bit in the second word; frames of one column, one pixel, one row
        t = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        m = np.stack([np.ones((2, H, W), bool), rng.random((2, H, W)) < 0.6], 1)
        pairs = [(0, 0), (0, 1), (1, 0), (1, 1)]
        got = _run_op(eng, t, m, pairs)
        assert np.array_equal(got, _reference(t, m, pairs)), (H, W)
        assert got[0, ng.I_A] == H * W
        if W & 31:                                                                              # the padding bits of a row's last word set: ignored
            words = nucfeat.pack_mask_words(m)
            words[..., -1] |= np.int32(-1 << (W & 31))
            dirty = eng.op_nucleus_gradient(_dev(eng, t), _dev(eng, words), _dev(eng, np.asarray(pairs, np.int32))).cpu().numpy()
            assert dirty.tobytes() == got.tobytes(), (H, W)
    from nuhtc_amd.engine import HipError
    with pytest.raises(HipError):
        eng.op_nucleus_gradient(torch.zeros(1, 1025, 8, 3, dtype=torch.uint8, device=eng.device), torch.zeros(1, 1, 1025, 1, dtype=torch.int32, device=eng.device),
                                torch.zeros(1, 2, dtype=torch.int32, device=eng.device))


@pytest.mark.parametrize('side', [256, 1024])
def test_op_large_frames(eng, side):
    """256: the full frame on the random tile and on a constant one (every pixel in bin 5).  1024, the largest frame the op takes, full,
    on alternating black and white columns: inside, the central difference spans two columns of the same colour and is 0; the first and
    last column hold the one-sided difference, m = isqrt(4 x 510^2) = 1020, so S4 = 2048 x 1020^4 = 2.2e15 -- the sums of a frame this
    size in int64 and its addressing.  (The bound S4 < 2^63 for 2^20 pixels at m = 1442 is arithmetic, tests/test_nucgrad_host.py; the
    largest m itself is reached in the corners of a checkerboard, which the second 1024-px row measures.)"""
    if side == 256:
        t = cases.tiles(side, side)
        tiles = np.stack([t['random'], t['planes']])
        masks = np.ones((2, 1, side, side), bool)
        pairs = [(0, 0), (1, 0)]
    else:
        tiles = np.stack([cases.columns(side, side), cases.checker(side, side)])
        masks = np.ones((2, 1, side, side), bool)
        pairs = [(0, 0), (1, 0)]
    got = _run_op(eng, tiles, masks, pairs)
    want = _reference(tiles, masks, pairs)
    assert np.array_equal(got, want), (got, want)
    assert got[0, ng.I_A] == side * side
    if side == 256:
        assert got[1].tolist() == [side * side, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, side * side, 0, 0, 0, 0]
    else:
        assert got[0, ng.I_MX] == 1020 and got[0, ng.I_S4] == 2 * side * 1020 ** 4 and got[0, ng.I_EDGE] == 2 * side
        assert got[1, ng.I_MX] == 1442 and got[1, ng.I_S4] == 4 * 1442 ** 4 + 4 * (side - 2) * 1020 ** 4


def test_op_repeatable_across_calls_and_batch_splits(eng):
    rng = np.random.default_rng(5)
    t = rng.integers(0, 256, (10, 64, 40, 3), dtype=np.uint8)
    m = rng.random((10, 1, 64, 40)) < 0.6
    pairs = [(i, 0) for i in range(10)]
    whole = _run_op(eng, t, m, pairs)
    assert np.array_equal(whole, _reference(t, m, pairs))
    assert _run_op(eng, t, m, pairs).tobytes() == whole.tobytes()                               # two calls
    split = np.concatenate([_run_op(eng, t[:4], m[:4], pairs[:4]), _run_op(eng, t[4:], m[4:], pairs[:6])])
    assert split.tobytes() == whole.tobytes()                                                   # 4 + 6
    ones = np.concatenate([_run_op(eng, t[i:i + 1], m[i:i + 1], [(0, 0)]) for i in range(10)])
    assert ones.tobytes() == whole.tobytes()                                                    # ten of 1


# ---------------------------------------------------------------------------------------------------------------- the document route
SLIDE_H, SLIDE_W = 300, 280


def _slide():
    s = np.zeros((SLIDE_H, SLIDE_W, 3), np.uint8)
    s[:, :SLIDE_W // 2] = np.random.default_rng(23).integers(0, 256, (SLIDE_H, SLIDE_W // 2, 3), dtype=np.uint8)
    s[:, SLIDE_W // 2:] = cases.tex.ramp(SLIDE_H, SLIDE_W - SLIDE_W // 2)
    return s


def _placed():
    """[(name, bool mask cropped to its rectangle, slide (x, y) of the rectangle)]: nuclei in the slide's corners and at its edges (the
    clamped origin, the margin beyond the slide), across the block boundary at 128, one whose margin needs the next side (28 + 4 = 32 fits,
    29 + 4 does not) and one of 254 px, whose rectangle plus margin exceeds 256."""
    yy, xx = np.mgrid[0:64, 0:64]
    disc = (yy[:15, :15] - 7) ** 2 + (xx[:15, :15] - 7) ** 2 <= 49
    sq = lambda n: np.ones((n, n), bool)
    long254 = np.ones((6, 254), bool)
    out = [('corner 0 0', disc, (0, 0)), ('one px from the corner', disc, (1, 1)), ('right edge', disc, (SLIDE_W - 15, 100)),
           ('bottom edge', disc, (60, SLIDE_H - 15)), ('last corner', sq(3), (SLIDE_W - 3, SLIDE_H - 3)), ('inside', disc, (40, 40)),
           ('at the block corner', disc, (128, 128)), ('across the block corner', disc, (121, 122)), ('side 28', sq(28), (70, 200)),
           ('side 29', sq(29), (150, 30)), ('side 124', sq(124), (140, 160)), ('254 px', long254, (10, 280))]
    for n, m, (x, y) in out:
        assert x + m.shape[1] <= SLIDE_W and y + m.shape[0] <= SLIDE_H, n
    return out


def _features(placed):
    return [contours.feature(contours.mask_to_ring(m, (x, y)), k % 5, 0.5 + k / 100.0, CLASSES) for k, (n, m, (x, y)) in enumerate(placed)]


def _host_frame(slide, ring, origin, S):
    """(frame uint8 (S, S, 3), mask bool (S, S)): the slide's pixels at `origin`, zeros beyond the slide, and contours.fill_rings's pixel
    set of the ring (nuhtc_fill_rings) pasted into the frame."""
    ox, oy = origin
    frame = np.zeros((S, S, 3), np.uint8)
    part = slide[oy:oy + S, ox:ox + S]
    frame[:part.shape[0], :part.shape[1]] = part
    boxes, areas, bits, woff = contours.fill_rings([np.asarray(ring)])
    x0, y0, x1, y1 = (int(v) for v in boxes[0])
    w, h = x1 - x0, y1 - y0
    wpr = (w + 31) // 32
    crop = np.unpackbits(np.ascontiguousarray(bits[woff[0]:woff[0] + h * wpr].reshape(h, wpr)).view(np.uint8), axis=-1, bitorder='little').astype(bool)[:, :w]
    mask = np.zeros((S, S), bool)
    mask[y0 - oy:y1 - oy, x0 - ox:x1 - ox] = crop
    return frame, mask


def test_measure_with_gradient_equals_the_restatement(hip_device):
    slide, placed = _slide(), _placed()
    feats = _features(placed)
    T = 6
    m = ringfeat.measure(slide, feats, device=0, block=128, gradient=True, edge_thr=T)
    plain = ringfeat.measure(slide, feats, device=0, block=128)
    n = len(placed)
    assert len(m['raw']) == n and m['grad'].shape == (n, ng.ROW) and m['grad'].dtype == np.int64 and sum(m['left_out'].values()) == 0
    assert set(m) == set(plain) | {'grad', 'grad_ok', 'grad_origin'}
    for k in ('raw', 'hist', 'glcm', 'origin', 'nuclei_id', 'rect', 'score', 'label'):            # the other measurements: the same bytes
        assert m[k].dtype == plain[k].dtype and m[k].tobytes() == plain[k].tobytes(), k
    sides = {}
    for i, (name, mask, (x, y)) in enumerate(placed):
        origin, side = ringfeat.gradient_frames(m['rect'][i:i + 1])
        sides[name] = int(side[0])
        assert m['grad_origin'][i].tolist() == origin[0].tolist() == [max(x - 2, 0), max(y - 2, 0)], name
        if name == '254 px':
            assert side[0] == 0 and not m['grad_ok'][i] and not m['grad'][i].any()
            continue
        assert m['grad_ok'][i], name
        ring = contours.trace_outer_contour(mask) + np.array([x, y])
        frame, filled = _host_frame(slide, ring, origin[0].tolist(), int(side[0]))
        assert filled.sum() == mask.sum()
        want = ng.grad_reference(frame, filled, T)
        assert np.array_equal(m['grad'][i], want), (name, m['grad'][i], want)
        assert m['grad'][i][ng.I_A] == m['raw'][i][0]                                            # the same pixels as the morphometry's
    assert sides['corner 0 0'] == 32 and sides['side 28'] == 32 and sides['side 29'] == 64 and sides['side 124'] == 128 and sides['254 px'] == 0
    one = ringfeat.measure(slide, feats, device=0, block=2048, gradient=True, edge_thr=T)       # the block size changes nothing
    assert one['grad'].tobytes() == m['grad'].tobytes() and one['grad_ok'].tobytes() == m['grad_ok'].tobytes()
    cols, val = ringfeat.table(m, gradient=True)
    assert cols == ringfeat.table_columns(gradient=True) and val.shape == (n, 63)
    bad = [i for i in range(n) if not m['grad_ok'][i]]
    assert len(bad) == 1 and np.isnan(val[bad[0], 55:]).all() and np.isfinite(np.delete(val, bad[0], 0)).all() and np.isfinite(val[:, :55]).all()
    assert np.array_equal(val[:, :55], ringfeat.table(plain)[1])


def _run_tool(cmd, limit=120):
    p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, TOOL] + cmd, cwd=ROOT, capture_output=True, text=True)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, p.returncode
    return p.stdout, p.stderr


def test_tool_with_and_without_gradient(hip_device, tmp_path):
    slide, placed = _slide(), _placed()
    feats = _features(placed)
    data = tmp_path / 'wsi'
    data.mkdir()
    np.save(data / 's1.npy', slide)
    segs = {}
    for d in ('plain', 'grad'):
        segs[d] = tmp_path / d
        (segs[d] / 's1').mkdir(parents=True)
        with open(segs[d] / 's1' / 's1_merged.geojson', 'w') as f:
            json.dump(feats, f)
    db = lambda d: str(segs[d] / 's1' / 'nuclei_feat.db')
    base = lambda d: [str(data), '--segdir', str(segs[d]), '--slide_ext', '.npy']
    _, err = _run_tool(base('plain'))
    assert f's1: {len(feats)} rows written, left out none' in err and 'without gradient columns' not in err
    _, err = _run_tool(base('grad') + ['--gradient', '--edge-thr', '1.5'])
    assert f's1: {len(feats)} rows written, left out none, 1 without gradient columns' in err
    a, b = ringfeat.read_db(db('plain')), ringfeat.read_db(db('grad'))
    assert a['columns'] == ringfeat.db_columns() and b['columns'] == ringfeat.db_columns(gradient=True) and len(b['columns']) == len(a['columns']) + 8
    assert [c for c, _ in b['columns'][56:64]] == [c.replace('.', '_') for c in ng.COLUMNS]
    m = ringfeat.measure(slide, feats, device=0, gradient=True, edge_thr=6)
    _, val = ringfeat.table(m, gradient=True)
    raw = lambda path: sqlite3_rows(path)
    for i, (ra, rb) in enumerate(zip(raw(db('plain')), raw(db('grad')))):
        assert rb[:56] == ra[:56] and rb[64:] == ra[56:], i                                      # the 55 shared columns and the trailing ones: equal bytes
        if placed[i][0] == '254 px':
            assert list(rb[56:64]) == [None] * 8
        else:
            assert all(isinstance(v, float) and np.isfinite(v) for v in rb[56:64]) and list(rb[56:64]) == val[i, 55:].tolist(), i
    # again: the table holds every nucleus, the slide resumes to no work and the file stays as it is
    before = {d: open(db(d), 'rb').read() for d in segs}
    out, err = _run_tool(base('grad') + ['--gradient', '--edge-thr', '1.5'])
    assert 'skipped:s1\n' in out and 'no slide measured' in err
    # --gradient onto the table written without it: skipped with the message, which names the file and the difference; the bytes unchanged
    # (the other direction: column_mismatch in tests/test_nucgrad_host.py)
    out, err = _run_tool(base('plain') + ['--gradient'])
    assert 'skipped:s1' in out and db('plain') in out and 'Nucleus_Gradient_Mag_Mean' in out and db('plain') in err
    assert {d: open(db(d), 'rb').read() for d in segs} == before


def sqlite3_rows(path):
    """The rows of the table as SQLite returns them (a REAL comes back as the float64 that was stored: equal values are equal bytes)."""
    import sqlite3
    con = sqlite3.connect(path)
    try:
        return con.execute(f'SELECT * FROM {ringfeat.TABLE} ORDER BY rowid').fetchall()
    finally:
        con.close()
