"""GPU tests of the per-nucleus shape integers (csrc/nucshape.hip): the device produces integers only, so every check is EQUALITY with the
numpy restatement (nuhtc_amd.nucshape.shape_reference) -- nuhtc_op_nucleus_shape on the designed masks of tests/nucshape_cases.py, the
list and frame handling, the largest frames, repeatability, the document route (ringfeat.measure(shape=True)) and
tools/wsi_feat_extract.py --shape end to end."""
import json
import os
import sqlite3
import subprocess
import sys

import numpy as np
import pytest
import torch

from nuhtc_amd import contours, nucfeat, ringfeat
from nuhtc_amd import nucgrad as ng
from nuhtc_amd import nucshape as ns

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucshape_cases as cases  # noqa: E402

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


def _reference(masks, pairs):
    """int64 (n, 24) of the pairs (tile, slot); a pair outside the arrays gives zeros."""
    out = np.zeros((len(pairs), ns.ROW), np.int64)
    for d, (b, s) in enumerate(pairs):
        if 0 <= b < masks.shape[0] and 0 <= s < masks.shape[1]:
            out[d] = ns.shape_reference(masks[b, s])
    return out


def _run_op(eng, masks, pairs, **kw):
    """masks bool (B, K, H, W)"""
    return eng.op_nucleus_shape(_dev(eng, nucfeat.pack_mask_words(masks)), _dev(eng, np.asarray(pairs, np.int32)), W=masks.shape[-1], **kw).cpu().numpy()


@pytest.fixture(scope='module')
def small():
    """The sixteen designed 64 x 40 masks as two batches of B = 2, K = 4: masks (2, 2, 4, 64, 40), names, the pairs of a batch and the
    restatement (2, 8, 24), computed once."""
    m = cases.small_masks()
    names = list(m)
    assert len(names) == 16
    masks = np.stack(list(m.values())).reshape(2, 2, 4, cases.H_SMALL, cases.W_SMALL)
    pairs = [(b, s) for b in range(2) for s in range(4)]
    want = np.stack([_reference(masks[c], pairs) for c in range(2)])
    want.setflags(write=False)
    return masks, names, pairs, want


def test_op_designed_masks_64x40(eng, small):
    masks, names, pairs, want = small
    got = np.stack([_run_op(eng, masks[c], pairs) for c in range(2)])
    assert got.dtype == np.int64 and got.shape == (2, 8, ns.ROW)
    for k, name in enumerate(names):
        assert np.array_equal(got.reshape(16, -1)[k], want.reshape(16, -1)[k]), (name, got.reshape(16, -1)[k], want.reshape(16, -1)[k])
    at = lambda n: got.reshape(16, -1)[names.index(n)].tolist()
    # what the cases were designed to hold, on the restatement's side and so on the device's
    assert at('empty') == [0] * 24
    assert at('pixel at (0, 0)') == [1, 0, 0, 1, 1] + [0] * 9 + [1] * 10
    assert at('pixel at (39, 63)') == [1, 39, 63, 40, 64, 39, 63, 39 * 39, 39 * 63, 63 * 63, 39 ** 3, 39 * 39 * 63, 39 * 63 * 63, 63 ** 3] + [1] * 10
    for n in ('solid 8x8 at x0=0', 'solid 8x8 at x0=29'):
        assert at(n)[0] == 64 and at(n)[ns.I_BOX:] == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1], n
    assert at('solid 7x5 in the last corner')[:5] == [35, 33, 59, 40, 64] and at('solid 7x5 in the last corner')[ns.I_BOX:ns.I_BOX + 3] == [6, 3, 1]
    assert at('checkerboard 16x16 at x0=3')[ns.I_BOX:] == [64, 16, 4, 1, 1, 1, 1, 1, 1, 1]
    assert at('full frame')[:5] == [64 * 40, 0, 0, 40, 64] and at('full frame')[ns.I_BOX:] == [0, 0, 0, 4, 2, 1, 1, 1, 1, 1]
    assert at('disc r=12 at x=32')[3] == 40                                                     # cut by the frame's right edge


def test_op_list_and_frame_handling(eng, small):
    from nuhtc_amd.engine import HipError
    masks, names, _, _ = small
    masks = masks[0]                                                                            # B = 2, K = 4
    pairs = [(1, 2), (2, 0), (0, 4), (-1, 0), (0, -1), (1, 3), (0, 1), (1, 0)]
    want = _reference(masks, pairs)
    got = _run_op(eng, masks, pairs)
    assert np.array_equal(got, want)
    assert not got[1:5].any() and got[0].any() and got[5].any()                                 # an entry outside the batch: a zero row
    n = 3                                                                                       # n_dev below n_max: the later rows keep the poison
    out = torch.full((len(pairs), ns.ROW), -7, dtype=torch.int64, device=eng.device)
    got2 = _run_op(eng, masks, pairs, n=torch.tensor([n], dtype=torch.int32, device=eng.device), out=out)
    assert np.array_equal(got2[:n], want[:n]) and (got2[n:] == -7).all()
    rng = np.random.default_rng(9)
    for H, W in ((64, 40), (7, 33), (9, 1), (1, 1), (1, 40), (5, 64), (3, 95)):                 # garbage in the padding bits of a row's last word: ignored
        m = np.stack([np.ones((2, H, W), bool), rng.random((2, H, W)) < 0.6], 1)
        pairs = [(0, 0), (0, 1), (1, 0), (1, 1)]
        got = _run_op(eng, m, pairs)
        assert np.array_equal(got, _reference(m, pairs)), (H, W)
        assert got[0, ns.I_A] == H * W
        if W & 31:
            words = nucfeat.pack_mask_words(m)
            words[..., -1] |= np.int32(-1 << (W & 31))
            dirty = eng.op_nucleus_shape(_dev(eng, words), _dev(eng, np.asarray(pairs, np.int32)), W=W).cpu().numpy()
            assert dirty.tobytes() == got.tobytes(), (H, W)
    with pytest.raises(HipError):
        eng.op_nucleus_shape(torch.zeros(1, 1, 1025, 1, dtype=torch.int32, device=eng.device), torch.zeros(1, 2, dtype=torch.int32, device=eng.device))
    with pytest.raises(HipError):
        eng.op_nucleus_shape(torch.zeros(1, 1, 8, 33, dtype=torch.int32, device=eng.device), torch.zeros(1, 2, dtype=torch.int32, device=eng.device))


@pytest.mark.parametrize('side', [256, 1024])
def test_op_large_frames(eng, side):
    """One nucleus in a frame of 256 and of 1024 pixels a side, the largest the op takes: a holed ellipse whose rectangle starts at x0 = 33
    (off the word grid) and spans the rest of the frame -- the third-order sums in int64 (1e14 at 1024) and every level of the planes."""
    m = cases.holed_ellipse(side)[None, None]
    got = _run_op(eng, m, [(0, 0)])
    want = _reference(m, [(0, 0)])
    assert np.array_equal(got, want), (got, want)
    assert got[0, 1:5].tolist() == [33, 0, side, side] and got[0, ns.I_A] > side * side // 2
    assert (got[0, ns.I_BOX:] > 0).all() and got[0, ns.I_BOX + 9] == 1
    if side == 1024:
        assert got[0, ns.I_SXXX] > 10 ** 14 and got[0, ns.I_BOX] > 1000


def test_op_repeatable_across_calls_and_batch_splits(eng):
    rng = np.random.default_rng(5)
    m = np.stack([np.pad(cases.blob(int(h), int(w), rng), ((3, 61 - h), (2, 38 - w))) for h, w in rng.integers(3, 38, (10, 2))])[:, None]
    assert m.shape == (10, 1, 64, 40)
    pairs = [(i, 0) for i in range(10)]
    whole = _run_op(eng, m, pairs)
    assert np.array_equal(whole, _reference(m, pairs))
    assert _run_op(eng, m, pairs).tobytes() == whole.tobytes()                                  # two calls
    split = np.concatenate([_run_op(eng, m[:4], pairs[:4]), _run_op(eng, m[4:], pairs[:6])])
    assert split.tobytes() == whole.tobytes()                                                   # 4 + 6
    ones = np.concatenate([_run_op(eng, m[i:i + 1], [(0, 0)]) for i in range(10)])
    assert ones.tobytes() == whole.tobytes()                                                    # ten of 1


# ---------------------------------------------------------------------------------------------------------------- the document route
SLIDE_H, SLIDE_W = 300, 280


def _slide():
    return np.random.default_rng(23).integers(0, 256, (SLIDE_H, SLIDE_W, 3), dtype=np.uint8)


def _ellipse(h, w, hole=-1.0):
    """bool (h, w): the ellipse inscribed in the rectangle (it touches all four sides), without its part inside `hole` of the radius."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = ((yy - (h - 1) / 2.0) / (h / 2.0)) ** 2 + ((xx - (w - 1) / 2.0) / (w / 2.0)) ** 2
    return (d <= 1.0) & (d > hole * abs(hole))


def _placed():
    """[(name, bool mask cropped to its rectangle, slide (x, y) of the rectangle)]: nuclei in the slide's corners, across the block
    boundary at 128, of every frame side (32, 64, 128, 256) and two with a hole, which the ring fills."""
    disc = cases.disc(15, 15, 7, 7, 7)
    ring = cases.disc(31, 31, 15, 15, 15, 6)
    sq = lambda h, w: np.ones((h, w), bool)
    out = [('corner 0 0', disc, (0, 0)), ('last corner', sq(3, 3), (SLIDE_W - 3, SLIDE_H - 3)), ('across the block corner', disc, (121, 122)),
           ('annulus', ring, (40, 40)), ('side 33', sq(33, 20), (70, 200)), ('ellipse 50x90', _ellipse(50, 90), (150, 30)),
           ('holed ellipse 130x100', _ellipse(130, 100, 0.2), (140, 160)), ('one pixel', sq(1, 1), (200, 10)), ('254 px', sq(6, 254), (10, 290))]
    for n, m, (x, y) in out:
        assert x + m.shape[1] <= SLIDE_W and y + m.shape[0] <= SLIDE_H, n
    return out


def _features(placed):
    return [contours.feature(contours.mask_to_ring(m, (x, y)), k % 5, 0.5 + k / 100.0, CLASSES) for k, (n, m, (x, y)) in enumerate(placed)]


def _host_mask(ring, origin, S):
    """bool (S, S): contours.fill_rings's pixel set of the ring (nuhtc_fill_rings) pasted into the frame at `origin`."""
    ox, oy = origin
    boxes, areas, bits, woff = contours.fill_rings([np.asarray(ring)])
    x0, y0, x1, y1 = (int(v) for v in boxes[0])
    w, h = x1 - x0, y1 - y0
    wpr = (w + 31) // 32
    crop = np.unpackbits(np.ascontiguousarray(bits[woff[0]:woff[0] + h * wpr].reshape(h, wpr)).view(np.uint8), axis=-1, bitorder='little').astype(bool)[:, :w]
    mask = np.zeros((S, S), bool)
    mask[y0 - oy:y1 - oy, x0 - ox:x1 - ox] = crop
    return mask


def _want_rows(placed, m):
    """The restatement on host-filled masks in the frames measure() uses (the rectangle's corner, frame_sides)."""
    sides = ringfeat.frame_sides(m['rect'])
    want = np.zeros((len(placed), ns.ROW), np.int64)
    for i, (name, mask, (x, y)) in enumerate(placed):
        assert m['origin'][i].tolist() == [x, y], name
        ring = contours.trace_outer_contour(mask) + np.array([x, y])
        want[i] = ns.shape_reference(_host_mask(ring, (x, y), int(sides[i])))
    return want, sides


def test_measure_with_shape_equals_the_restatement(hip_device):
    slide, placed = _slide(), _placed()
    feats = _features(placed)
    m = ringfeat.measure(slide, feats, device=0, block=128, shape=True)
    plain = ringfeat.measure(slide, feats, device=0, block=128)
    n = len(placed)
    assert len(m['raw']) == n and m['shape'].shape == (n, ns.ROW) and m['shape'].dtype == np.int64 and sum(m['left_out'].values()) == 0
    assert set(m) == set(plain) | {'shape'}
    for k in ('raw', 'hist', 'glcm', 'origin', 'nuclei_id', 'rect', 'score', 'label'):            # the other measurements: the same bytes
        assert m[k].dtype == plain[k].dtype and m[k].tobytes() == plain[k].tobytes(), k
    want, sides = _want_rows(placed, m)
    for i, (name, mask, _) in enumerate(placed):
        assert np.array_equal(m['shape'][i], want[i]), (name, m['shape'][i], want[i])
        assert m['shape'][i][ns.I_A] == m['raw'][i][0]                                           # the same pixels as the morphometry's
        assert m['shape'][i][1:5].tolist() == [0, 0, mask.shape[1], mask.shape[0]], name        # the frame's corner is the rectangle's
    assert sorted(set(sides.tolist())) == [32, 64, 128, 256]
    assert m['shape'][[p[0] for p in placed].index('annulus')][ns.I_A] == cases.disc(31, 31, 15, 15, 15).sum()      # the hole is filled
    one = ringfeat.measure(slide, feats, device=0, block=2048, shape=True)                      # the block size changes nothing
    assert one['shape'].tobytes() == m['shape'].tobytes()
    cols, val = ringfeat.table(m, shape=True)
    assert cols == ringfeat.table_columns(shape=True) and val.shape == (n, 63) and np.isfinite(val).all()
    assert np.array_equal(val[:, :55], ringfeat.table(plain)[1]) and np.array_equal(val[:, 55:], ns.derive(want)[1])
    both = ringfeat.measure(slide, feats, device=0, block=128, gradient=True, shape=True)
    cols, val2 = ringfeat.table(both, gradient=True, shape=True)
    assert cols == ringfeat.table_columns(gradient=True, shape=True) and val2.shape == (n, 71) and both['shape'].tobytes() == m['shape'].tobytes()
    assert np.array_equal(val2[:, 63:], val[:, 55:]) and np.array_equal(val2[:, :55], val[:, :55])


def _run_tool(cmd, limit=120):
    p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, TOOL] + cmd, cwd=ROOT, capture_output=True, text=True)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, p.returncode
    return p.stdout, p.stderr


def _rows(path):
    """The rows of the table as SQLite returns them (a REAL comes back as the float64 that was stored: equal values are equal bytes)."""
    con = sqlite3.connect(path)
    try:
        return con.execute(f'SELECT * FROM {ringfeat.TABLE} ORDER BY rowid').fetchall()
    finally:
        con.close()


def test_tool_with_and_without_shape(hip_device, tmp_path):
    slide, placed = _slide(), _placed()
    feats = _features(placed)
    data = tmp_path / 'wsi'
    data.mkdir()
    np.save(data / 's1.npy', slide)
    segs = {}
    for d in ('plain', 'shape', 'both'):
        segs[d] = tmp_path / d
        (segs[d] / 's1').mkdir(parents=True)
        with open(segs[d] / 's1' / 's1_merged.geojson', 'w') as f:
            json.dump(feats, f)
    db = lambda d: str(segs[d] / 's1' / 'nuclei_feat.db')
    base = lambda d: [str(data), '--segdir', str(segs[d]), '--slide_ext', '.npy']
    flags = {'plain': [], 'shape': ['--shape'], 'both': ['--gradient', '--shape']}
    for d in segs:
        _, err = _run_tool(base(d) + flags[d])
        assert f's1: {len(feats)} rows written, left out none' in err
    a, b, c = (ringfeat.read_db(db(d)) for d in ('plain', 'shape', 'both'))
    assert a['columns'] == ringfeat.db_columns() and b['columns'] == ringfeat.db_columns(shape=True) and c['columns'] == ringfeat.db_columns(gradient=True, shape=True)
    assert [x for x, _ in b['columns'][56:64]] == [x.replace('.', '_') for x in ns.COLUMNS] == [x for x, _ in c['columns'][64:72]]
    assert [x for x, _ in c['columns'][56:64]] == [x.replace('.', '_') for x in ng.COLUMNS]
    m = ringfeat.measure(slide, feats, device=0)
    val = ns.derive(_want_rows(placed, m)[0])[1]                                                # derive of the restatement on host-filled masks
    for i, (ra, rb, rc) in enumerate(zip(_rows(db('plain')), _rows(db('shape')), _rows(db('both')))):
        assert rb[:56] == ra[:56] and rb[64:] == ra[56:], i                                      # the common columns: equal bytes
        assert rc[:56] == ra[:56] and rc[72:] == ra[56:], i
        assert all(isinstance(v, float) and np.isfinite(v) for v in rb[56:64]) and list(rb[56:64]) == val[i].tolist() == list(rc[64:72]), i
    # --shape onto the table written without it: skipped with the message, which names the file and the difference; the bytes unchanged
    before = {d: open(db(d), 'rb').read() for d in segs}
    out, err = _run_tool(base('plain') + ['--shape'])
    assert 'skipped:s1' in out and db('plain') in out and 'Shape_HuMoments1' in out and db('plain') in err
    assert 'Shape_HuMoments1' in ringfeat.column_mismatch(db('both'), gradient=True) and ringfeat.column_mismatch(db('both'), gradient=True, shape=True) is None
    assert {d: open(db(d), 'rb').read() for d in segs} == before
