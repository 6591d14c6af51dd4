"""GPU tests of the per-nucleus table from a written GeoJSON (csrc/ringfeat.hip, nuhtc_amd/ringfeat.py, tools/wsi_feat_extract.py).
Everything the device produces is an integer or a bit, so every check is EQUALITY: the ring fill with contours.fill_rings (the host code
that defines which pixels a written ring stands for), the gather with numpy slicing, measure() with morph_reference / glcm_reference on
(frame crop of the slide, filled ring), the tool with table(measure()) of this process, and the whole route with the rows the engine
measures under its own masks during a detection run."""
import json
import os
import sqlite3
import subprocess
import sys

import numpy as np
import pytest
import torch

from nuhtc_amd import contours, nucmorph, nuctex, ringfeat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nuctex_cases as tex_cases  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs', 'nuhtc', 'htc_lite_swin_pannuke_infer.py')
TOOL = os.path.join(ROOT, 'tools', 'wsi_feat_extract.py')
CLASSES = ('T', 'I', 'C', 'D', 'E')


@pytest.fixture(scope='module')
def ops(hip_device):
    with ringfeat._Ops(0) as o:
        yield o


def _bits(words, S):
    """int32 / uint32 (..., S // 32) words -> bool (..., S)."""
    w = np.ascontiguousarray(words).view(np.uint8)
    return np.unpackbits(w, axis=-1, bitorder='little').astype(bool)


def _fill(ops, rings, origins, S):
    """-> (bool (n, S, S), status (n,)) of nuhtc_op_ring_fill."""
    verts, off = ringfeat.pack_rings(rings)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)
    masks, status = ops.fill(dev(verts), dev(off), dev(np.asarray(origins, np.int32).reshape(-1, 2)), S)
    torch.cuda.synchronize()
    return _bits(masks.cpu().numpy(), S), status.cpu().numpy()


def _host_fill(ring, origin, S):
    """contours.fill_rings's crop of one ring pasted into the S x S frame at `origin`."""
    boxes, areas, bits, woff = contours.fill_rings([np.asarray(ring)])
    x0, y0, x1, y1 = (int(v) for v in boxes[0])
    w, h = x1 - x0, y1 - y0
    wpr = (w + 31) // 32
    crop = _bits(bits[woff[0]:woff[0] + h * wpr].reshape(h, wpr), wpr * 32)[:, :w]
    assert int(crop.sum()) == int(areas[0])
    out = np.zeros((S, S), bool)
    out[y0 - origin[1]:y1 - origin[1], x0 - origin[0]:x1 - origin[0]] = crop
    return out


def _connected(mask):
    from scipy import ndimage
    return ndimage.label(mask, structure=np.ones((3, 3), int))[1] == 1


def traced_cases():
    """name -> ring (k, 2): the traced outer contours of the connected designed masks, each moved so that its rectangle starts at (0, 0)."""
    out = {}
    for name, m in tex_cases.small_masks().items():
        if m.any() and _connected(m):
            r = contours.trace_outer_contour(m)
            out[name] = r - r.min(0)
    return out


def designed_rings():
    """name -> (ring, pixels that must be set, pixels that must be clear), frame coordinates with the rectangle at (0, 0)."""
    yy, xx = np.mgrid[0:40, 0:40]
    blob = np.zeros((12, 40), bool); blob[2:10, 27:37] = True                                  # crosses x = 31 | 32
    cee = np.ones((7, 9), bool); cee[3, 2:] = False                                            # a pocket one pixel wide, open to the right
    vee = np.ones((9, 7), bool); vee[:7, 3] = False                                            # ... and one open to the top
    hole = ((yy - 20) ** 2 + (xx - 20) ** 2 <= 15 ** 2) & ((yy - 20) ** 2 + (xx - 20) ** 2 > 8 ** 2)
    bridge = np.zeros((9, 30), bool); bridge[0:9, 0:8] = True; bridge[4, 8:22] = True; bridge[1:8, 22:30] = True
    tr = lambda m: (lambda r: r - r.min(0))(contours.trace_outer_contour(m))
    d = {'single vertex': (np.array([[0, 0]]), [(0, 0)], [(1, 0), (0, 1)]),
         'two vertices': (np.array([[0, 0], [1, 0]]), [(0, 0), (1, 0)], [(2, 0), (0, 1)]),
         'blob across x=31|32': (tr(blob), [(4, 3), (5, 3)], []),
         'C pocket open right': (tr(cee), [(0, 3), (1, 3)], [(2, 3), (5, 3), (8, 3)]),
         'C pocket open top': (tr(vee), [(3, 7), (3, 8)], [(3, 0), (3, 6)]),
         'ring with a hole': (tr(hole), [(15, 15), (10, 14)], []),
         'bridge walked forth and back': (tr(bridge), [(15, 4), (3, 3)], [(15, 3), (15, 5)]),
         'bow-tie': (np.array([[0, 0], [8, 8], [8, 0], [0, 8]]), [(4, 4), (1, 4), (7, 4), (0, 0)], [(4, 1), (4, 7)]),
         # an outer and an inner square walked in the same sense, joined by a diagonal: the inner square is wound round twice, which a
         # crossing-parity fill would call outside; the flood calls it inside
         'winds twice': (np.array([[0, 0], [10, 0], [10, 10], [0, 10], [0, 2], [8, 2], [8, 8], [2, 8], [2, 2]]), [(5, 5), (1, 5), (9, 9)], [(11, 5)])}
    return d


def test_ring_fill_traced_and_designed_rings_at_64(ops):
    cases = {k: (v, [], []) for k, v in traced_cases().items()}
    assert len(cases) >= 14 and 'annulus' in cases and 'checkerboard' in cases and 'full frame' in cases
    cases.update(designed_rings())
    names = list(cases)
    origins = [(1000 + 37 * i, 50000 - 11 * i) for i in range(len(names))]                    # slide positions: the frame moves with its ring
    rings = [cases[n][0] + np.array(o) for n, o in zip(names, origins)]
    got, status = _fill(ops, rings, origins, 64)
    assert status.tolist() == [0] * len(names)
    for i, n in enumerate(names):
        want = _host_fill(rings[i], origins[i], 64)
        assert np.array_equal(got[i], want), (n, np.argwhere(got[i] != want)[:8])
        for x, y in cases[n][1]:
            assert got[i][y, x], (n, x, y)
        for x, y in cases[n][2]:
            assert not got[i][y, x], (n, x, y)
    # holes are filled: the annulus is a disc, the frame mask a full rectangle
    k = names.index('annulus')
    assert got[k].sum() > tex_cases.small_masks()['annulus'].sum()
    assert got[names.index('full frame')].sum() == 64 * 40 and got[names.index('single vertex')].sum() == 1


@pytest.mark.parametrize('S', [32, 256])
def test_ring_fill_whole_frame_and_every_side(ops, S):
    """A rectangle of exactly S x S: the border is the frame's rim, no outside is left inside it.  With it, in the same call, a ring in
    the last corner and one that reaches into every word of a row."""
    full = np.array([[0, 0], [0, S - 1], [S - 1, S - 1], [S - 1, 0]])
    corner = np.array([[S - 3, S - 2], [S - 2, S - 3], [S - 1, S - 2], [S - 2, S - 1]])       # a diamond whose last pixel is the frame's last
    comb = np.zeros((S, S), bool); comb[S // 2, :] = True; comb[S // 4:S // 2, ::5] = True      # teeth: pockets open to the top, across all words
    rings = [full, corner, contours.trace_outer_contour(comb)]
    got, status = _fill(ops, rings, [(0, 0)] * 3, S)
    assert status.tolist() == [0, 0, 0]
    assert got[0].all()
    for i in range(3):
        assert np.array_equal(got[i], _host_fill(rings[i], (0, 0), S)), i
    assert got[1].sum() == 5 and np.array_equal(got[2], comb)


def test_ring_fill_status_and_neighbours(ops):
    S = 64
    good = designed_rings()['winds twice'][0]
    rings = [good, np.array([[3, 3], [S, 3], [S, 5], [3, 5]]), good + 20, np.array([[5, 5], [7, 6], [5, 7]]), good + 40,
             np.array([[-1, 0], [4, 0], [4, 4]]), np.array([[0, S], [2, S]])]
    got, status = _fill(ops, rings, [(0, 0)] * len(rings), S)
    assert status.tolist() == [0, 1, 0, 2, 0, 1, 1]
    for i in (1, 3, 5, 6):
        assert not got[i].any(), i
    for i in (0, 2, 4):
        assert np.array_equal(got[i], _host_fill(rings[i], (0, 0), S)) and got[i].sum() == 120, i      # 11 x 11 less the pixel (0, 1), which no edge covers
    # the entry point refuses bad sizes before it launches anything
    lib, vp = ops.lib, lambda t: t.data_ptr()
    v, off, org = (torch.zeros(s, dtype=d, device=ops.device) for s, d in (((4, 2), torch.int32), ((2,), torch.int64), ((1, 2), torch.int32)))
    m, st = torch.zeros(8192, dtype=torch.int32, device=ops.device), torch.zeros(1, dtype=torch.int32, device=ops.device)
    from nuhtc_amd import hip
    assert lib.nuhtc_op_ring_fill(0, vp(v), 4, vp(off), vp(org), 1, 48, vp(m), vp(st), None) == hip.E_INVALID
    assert lib.nuhtc_op_ring_fill(0, vp(v), 4, vp(off), vp(org), 0, 32, vp(m), vp(st), None) == hip.E_INVALID
    assert lib.nuhtc_op_ring_fill(0, vp(v), 4, vp(off), vp(org), 4097, 32, vp(m), vp(st), None) == hip.E_INVALID
    assert lib.nuhtc_op_ring_fill(0, None, 4, vp(off), vp(org), 1, 32, vp(m), vp(st), None) == hip.E_INVALID
    assert lib.nuhtc_op_frame_gather(0, vp(m), 4, 4, 0, 0, vp(org), 1, 512, vp(m), None) == hip.E_INVALID
    assert lib.nuhtc_op_frame_gather(0, vp(m), 0, 4, 0, 0, vp(org), 1, 32, vp(m), None) == hip.E_INVALID
    assert lib.nuhtc_op_frame_gather(0, vp(m), 4, 4, 0, 0, None, 1, 32, vp(m), None) == hip.E_INVALID


def test_ring_fill_batch_of_1_and_of_300_twice(ops):
    pool = [r for r, _, _ in designed_rings().values()] + list(traced_cases().values())
    rng = np.random.default_rng(11)
    rings, origins = [], []
    for i in range(300):
        r = pool[i % len(pool)]
        shift = rng.integers(0, 64 - r.max(0))                                                 # anywhere the ring still fits the frame
        o = rng.integers(-5000, 5000, 2)
        rings.append(r + shift + o); origins.append(o)
    rings[7] = np.array([[1, 1], [4, 2], [1, 3]]) + origins[7]                                 # one that is refused, among the others
    a, sa = _fill(ops, rings, origins, 64)
    b, sb = _fill(ops, rings, origins, 64)
    assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()
    assert sa.tolist() == [2 if i == 7 else 0 for i in range(300)]
    for i in range(0, 300, 13):
        assert np.array_equal(a[i], _host_fill(rings[i], origins[i], 64)), i
    one, so = _fill(ops, rings[5:6], origins[5:6], 64)
    one2, _ = _fill(ops, rings[5:6], origins[5:6], 64)
    assert one.tobytes() == one2.tobytes() == a[5:6].tobytes() and so.tolist() == [0]


@pytest.mark.parametrize('S', [32, 64])
def test_frame_gather_against_slicing(ops, S):
    bh, bw, bx, by = 96, 80, 1000, 2000
    block = np.random.default_rng(3).integers(0, 256, (bh, bw, 3), dtype=np.uint8)
    org = [(bx + 7, by + 9), (bx, by), (bx + bw - S, by), (bx, by + bh - S), (bx + bw - S, by + bh - S),      # inside; at the four corners
           (bx - 5, by + 10), (bx + bw - 11, by + 10), (bx + 13, by - 6), (bx + 13, by + bh - 3),              # partly outside on each side
           (bx - 9, by - 9), (bx + bw - 1, by + bh - 1),                                                       # ... on two sides at once
           (bx - S, by), (bx + bw, by + 5), (bx + 3, by + bh), (0, 0)]                                         # wholly outside
    origin = torch.tensor(org, dtype=torch.int32, device=ops.device)
    got = ops.gather(torch.from_numpy(block).to(ops.device), bx, by, origin, S)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == (len(org), S, S, 3)
    for i, (ox, oy) in enumerate(org):
        want = np.zeros((S, S, 3), np.uint8)
        x0, y0 = max(ox, bx), max(oy, by)
        x1, y1 = min(ox + S, bx + bw), min(oy + S, by + bh)
        if x1 > x0 and y1 > y0:
            want[y0 - oy:y1 - oy, x0 - ox:x1 - ox] = block[y0 - by:y1 - by, x0 - bx:x1 - bx]
        assert np.array_equal(got[i], want), (i, ox - bx, oy - by)
    assert not got[11:].any() and got[0].any()


# ---------------------------------------------------------------------------------------------------------------- measure, end to end
SLIDE_H, SLIDE_W = 300, 260


def _slide():
    s = np.zeros((SLIDE_H, SLIDE_W, 3), np.uint8)
    s[:, :SLIDE_W // 2] = np.random.default_rng(21).integers(0, 256, (SLIDE_H, SLIDE_W // 2, 3), dtype=np.uint8)
    s[:, SLIDE_W // 2:] = tex_cases.ramp(SLIDE_H, SLIDE_W - SLIDE_W // 2)
    return s


def _placed_masks():
    """[(name, bool mask cropped to its rectangle, slide (x, y) of the rectangle)]: about twenty nuclei on the 300 x 260 slide."""
    small = {k: v for k, v in tex_cases.small_masks().items() if v.any() and _connected(v)}
    def crop(m):
        rows, cols = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
        return m[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
    c = {k: crop(v) for k, v in small.items()}
    yy, xx = np.mgrid[0:130, 0:130]
    big70 = ((yy[:70, :70] - 34.5) / 35.0) ** 2 + ((xx[:70, :70] - 34.5) / 30.0) ** 2 <= 1.0
    big70[34, :] = True; big70[:, 34] = True                                                   # side 70 both ways: bucket 128
    big130 = ((yy - 64.5) / 65.0) ** 2 + ((xx - 64.5) / 40.0) ** 2 <= 1.0
    big130[64, :] = True                                                                       # side 130: bucket 256
    at = [('disc r=7', 20, 30), ('annulus', 60, 20), ('checkerboard', 150, 40), ('L across x=31|32', 200, 10),
          ('horizontal line', 100, 5), ('vertical line', 5, 100), ('diagonal line', 170, 120), ('pixel', 77, 77),
          ('1x2 pair', 140, 3), ('2x1 pair', 250, 150),
          ('disc r=7', 0, 60), ('disc r=7', SLIDE_W - 15, 90), ('annulus', 100, 0), ('annulus', 40, SLIDE_H - 31),      # the slide's four edges
          ('pixel', SLIDE_W - 1, SLIDE_H - 1), ('pixel', 0, 0),                                                        # ... and its corners
          ('disc r=7', 120, 120), ('annulus', 115, 240), ('2x2 in the last corner', 127, 127), ('horizontal line', 110, 200),   # across x = 128 / y = 128 / y = 256
          ('L across x=31|32', 126, 250)]
    out = [(n, c[n], (x, y)) for n, x, y in at]
    out.append(('side 70', big70, (10, 180)))
    out.append(('side 130', big130, (128, 140)))
    out.append(('254 px', np.ones((6, 254), bool), (3, 290)))                                  # its rectangle plus a margin of 2 exceeds 256
    for n, m, (x, y) in out:
        assert x + m.shape[1] <= SLIDE_W and y + m.shape[0] <= SLIDE_H, n
    return out


def _features(placed):
    feats = []
    for k, (n, m, (x, y)) in enumerate(placed):
        feats.append(contours.feature(contours.mask_to_ring(m, (x, y)), k % 5, 0.5 + k / 100.0, CLASSES))
    return feats


@pytest.fixture(scope='module')
def scene(hip_device):
    """The slide, the features (the placed nuclei, then three that must be left out), and per kept nucleus the restatement of its
    integers on (frame crop of the slide, filled ring), computed once."""
    slide = _slide()
    placed = _placed_masks()
    feats = _features(placed)
    n_kept = len(feats)
    feats.insert(3, contours.feature(np.array([[30.5, 30.0], [30.0, 34.0], [35.0, 34.0], [30.5, 30.0]]), 1, 0.4, CLASSES))            # float
    feats.insert(9, contours.feature(np.array([[0, 0], [0, 9], [256, 9], [256, 0], [0, 0]]), 1, 0.4, CLASSES))                        # side 257
    feats.append(contours.feature(np.array([[50, 150], [53, 151], [50, 152], [50, 150]]), 1, 0.4, CLASSES))                           # off the chain directions
    want = []
    for n, m, (x, y) in placed:
        ring = contours.trace_outer_contour(m) + np.array([x, y])
        S = ringfeat.bucket(max(m.shape))
        frame = np.zeros((S, S, 3), np.uint8)
        part = slide[y:y + S, x:x + S]
        frame[:part.shape[0], :part.shape[1]] = part
        filled = _host_fill(ring, (x, y), S)
        raw, hist = nucmorph.morph_reference(frame, filled)
        whole = np.zeros(slide.shape[:2], bool)
        h, w = min(S, SLIDE_H - y), min(S, SLIDE_W - x)
        whole[y:y + h, x:x + w] = filled[:h, :w]
        assert whole.sum() == filled.sum()
        want.append((raw, hist, nuctex.glcm_reference(frame, filled), nucmorph.morph_reference(slide, whole)))
    return slide, feats, n_kept, placed, want


def test_measure_equals_the_restatement(scene):
    slide, feats, n_kept, placed, want = scene
    m = ringfeat.measure(slide, feats, device=0, block=128)
    assert m['left_out'] == dict(non_integer=1, no_ring=0, too_large=1, off_slide=0, not_traced=1)
    assert len(m['raw']) == n_kept == len(placed) and m['raw'].dtype == np.int64 and m['hist'].dtype == np.int32 and m['glcm'].dtype == np.int32
    assert m['raw'].shape == (n_kept, 16) and m['hist'].shape == (n_kept, 256) and m['glcm'].shape == (n_kept, 2, 136) and m['origin'].dtype == np.int64
    kept_pos = [k for k in range(len(feats)) if k not in (3, 9, len(feats) - 1)]
    assert m['nuclei_id'].tolist() == kept_pos                                                  # no nuclei_id property: the position in the file
    sides = set()
    for i, (n, mask, (x, y)) in enumerate(placed):
        raw, hist, glcm, _ = want[i]
        assert m['origin'][i].tolist() == [x, y], n
        assert np.array_equal(m['raw'][i], raw), (n, m['raw'][i], raw)
        assert np.array_equal(m['hist'][i], hist), n
        assert np.array_equal(m['glcm'][i], glcm), n
        sides.add(ringfeat.bucket(max(mask.shape)))
    assert sides == {32, 64, 128, 256}
    # the Identifier.* columns: the same derivation on the whole slide array with origin 0.  The four extremes are integers below 2^53
    # in both routes: equal.  A centroid is og + Sx / A here and Sx' / A there (Sx' = Sx + og A): each is the exact value rounded at
    # most twice, the values are below 512 (ulp 2^-44 = 5.7e-14), so they agree to within 2 ulp = 1.2e-13.
    cols, val = ringfeat.table(m)
    assert len(cols) == 55 and val.shape == (n_kept, 55) and np.isfinite(val).all()
    c = {name: k for k, name in enumerate(cols)}
    for i in range(n_kept):
        _, ref = nucmorph.derive(*want[i][3])
        for name in ('Identifier.Xmin', 'Identifier.Ymin', 'Identifier.Xmax', 'Identifier.Ymax'):
            assert val[i, c[name]] == ref[0, c[name]], (placed[i][0], name)
        for name in ('Identifier.CentroidX', 'Identifier.CentroidY'):
            assert abs(val[i, c[name]] - ref[0, c[name]]) <= 1.2e-13, (placed[i][0], name)
    # the block size changes which block reads a nucleus, not what is measured
    one = ringfeat.measure(slide, feats, device=0, block=2048)
    for k in ('raw', 'hist', 'glcm', 'origin', 'nuclei_id', 'rect', 'score', 'label'):
        assert one[k].dtype == m[k].dtype and one[k].tobytes() == m[k].tobytes(), k
    assert one['left_out'] == m['left_out'] and one['type'] == m['type']


def test_all_families_at_once_equal_each_alone_and_the_plain_call(scene):
    """One walk with every family selected against the walks with one or none: every field byte for byte, at both block sizes -- the
    frame plans share the block, the rings and the chunking, and must not reach into each other."""
    slide, feats, n_kept, placed, _ = scene
    every = ringfeat.measure(slide, feats, device=0, block=128, gradient=True, shape=True, fsd=True)
    parts = [ringfeat.measure(slide, feats, device=0, block=128, **kw) for kw in ({}, dict(gradient=True), dict(shape=True), dict(fsd=True))]
    parts.append(ringfeat.measure(slide, feats, device=0, block=2048, gradient=True, shape=True, fsd=True))
    assert set(every) == set(parts[0]) | {'grad', 'grad_ok', 'grad_origin', 'shape', 'fsd'} == set(parts[4])
    assert [sorted(set(m) - set(parts[0])) for m in parts[:4]] == [[], ['grad', 'grad_ok', 'grad_origin'], ['shape'], ['fsd']]
    for m in parts:
        for k, v in m.items():
            if isinstance(v, np.ndarray):
                assert every[k].dtype == v.dtype and every[k].shape == v.shape and every[k].tobytes() == v.tobytes(), k
            else:
                assert every[k] == v, k
    assert len(every['raw']) == n_kept and every['shape'].any() and every['fsd'].any()
    lack = [n for (n, _, _), ok in zip(placed, every['grad_ok']) if not ok]
    assert lack == ['254 px'] and not every['grad'][~every['grad_ok']].any() and every['grad'][every['grad_ok']].any(1).all()
    cols, val = ringfeat.table(every, gradient=True, shape=True, fsd=True)
    assert val.shape == (n_kept, 77) and np.array_equal(np.isnan(val), ~every['grad_ok'][:, None] & (np.arange(77) >= 55)[None] & (np.arange(77) < 63)[None])


def _run_tool(cmd, limit=120):
    p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, TOOL] + cmd, cwd=ROOT, capture_output=True, text=True)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, p.returncode
    return p.stdout, p.stderr


def test_tool_writes_resumes_and_reads_plain_files(scene, tmp_path):
    slide, _, _, placed, _ = scene
    data, seg = tmp_path / 'wsi', tmp_path / 'seg'
    data.mkdir(); (seg / 's1').mkdir(parents=True)
    np.save(data / 's1.npy', slide)
    feats = _features(placed)
    ids = [100 + 3 * k for k in range(len(feats))]
    for f, i in zip(feats, ids):
        f['properties']['nuclei_id'] = i
    with open(seg / 's1' / 's1_merged.geojson', 'w') as f:
        json.dump(feats, f)
    db = str(seg / 's1' / 'nuclei_feat.db')
    base = [str(data), '--segdir', str(seg), '--slide_ext', '.npy']
    _, err = _run_tool(base)
    assert f's1: {len(feats)} rows written, left out none' in err
    got = ringfeat.read_db(db)
    assert got['columns'] == ringfeat.db_columns() and len(got['rows']) == len(feats)
    m = ringfeat.measure(slide, feats, device=0)
    _, val = ringfeat.table(m)
    for i, r in enumerate(got['rows']):
        assert r[0] == 1 and list(r[1:56]) == val[i].tolist(), i
        assert r[56] == feats[i]['properties']['score'] and r[57] == CLASSES[i % 5] and r[58] == i % 5 and r[59] == ids[i]
        ring = np.asarray(feats[i]['geometry']['coordinates'][0])
        assert list(r[60:]) == [ring[:, 0].min(), ring[:, 1].min(), ring[:, 0].max(), ring[:, 1].max()]
    # a second run: the slide is skipped and the file stays as it is (a table of 24 rows is far below 1 MB)
    before = open(db, 'rb').read()
    assert len(before) < 1 << 20
    out, _ = _run_tool(base)
    assert 'skipped:s1' in out and open(db, 'rb').read() == before
    # two rows deleted: exactly those two return
    con = sqlite3.connect(db)
    con.execute(f'DELETE FROM {ringfeat.TABLE} WHERE nuclei_id IN (?, ?)', (ids[4], ids[17]))
    con.commit(); con.close()
    _, err = _run_tool(base)
    assert 's1: 2 rows written' in err
    again = ringfeat.read_db(db)['rows']
    assert [r[59] for r in again] == [i for i in ids if i not in (ids[4], ids[17])] + [ids[4], ids[17]]
    assert sorted(again) == sorted(got['rows'])
    # --geojson plain on a file without nuclei_id: the ids are the positions; --mag other than 40 is said once
    (seg / 's2').mkdir()
    np.save(data / 's2.npy', slide)
    with open(seg / 's2' / 's2.geojson', 'w') as f:
        json.dump(_features(placed), f)
    _, err = _run_tool(base + ['--geojson', 'plain', '--start', '1', '--mag', '20'])
    assert err.count('--mag 20') == 1 and 's2:' in err and 's1:' not in err
    rows = ringfeat.read_db(str(seg / 's2' / 'nuclei_feat.db'))['rows']
    assert [r[59] for r in rows] == list(range(len(placed))) and [r[1:59] for r in rows] == [r[1:59] for r in got['rows']]


# ---------------------------------------------------------------------------------------------------------------- the engine's own route
ENGINE_SEED, ENGINE_OBJ_BIAS, ENGINE_TILES = 0, 3.0, (10, 11)      # pinned on an MI355X: this synthetic model keeps 86 records on these two tiles, 19 of them simple


def test_rings_of_a_detection_run_measure_like_its_masks(hip_device, tmp_path):
    """infer_tiles(nucmorph=True, nuctex=True) measures every record under the tile's mask; the record's ring, measured here from the
    slide, must give the same integers whenever the ring stands for the same pixels: the mask is one component without a hole.  The
    engine's raw row is in tile pixels, ours in frame pixels; moving one to the other is host arithmetic on integers (below)."""
    from scipy import ndimage
    from nuhtc_amd import synth, weights, wsi
    from nuhtc_amd.apis import init_detector
    ck = str(tmp_path / 'w.pth')
    torch.save(dict(meta={}, state_dict=weights.bench_state_dict(ENGINE_SEED, obj_bias=ENGINE_OBJ_BIAS)), ck)
    model = init_detector(CFG, ck, device='cuda:0', max_batch=4)
    img = np.concatenate([synth.nuclei_tile(t, 64) for t in ENGINE_TILES], 1)                  # 64 x 128: two tiles side by side
    tiles, coords = wsi.tile_grid(img, 64, 64)
    assert len(tiles) == 2
    rec = wsi.infer_tiles(model, tiles, coords, batch_size=4, nucmorph=True, nuctex=True)
    n = len(rec['score'])
    raw_e, hist_e, org_e = nucmorph.unpack_rows(rec['morph'])
    glcm_e = nuctex.unpack_rows(rec['tex'])
    take, skipped = [], []
    for k in range(n):
        crop = rec['mask'][k][0]
        (take if _connected(crop) and np.array_equal(ndimage.binary_fill_holes(crop), crop) else skipped).append(k)
    print(f'{n} records on two 64-px tiles; {len(take)} are one component without a hole, skipped {skipped}')
    assert len(take) >= 3
    feats = [contours.feature(np.asarray(rec['ring'][k]), int(rec['label'][k]), float(rec['score'][k]), CLASSES) for k in take]
    # infer_tiles reads its RGB tiles with red in byte 2 (CH_SWAP); measure() reads a slide with red in byte 0
    m = ringfeat.measure(np.ascontiguousarray(img[..., ::-1]), feats, device=0)
    assert sum(m['left_out'].values()) == 0 and len(m['raw']) == len(take)
    I = nucmorph
    for i, k in enumerate(take):
        r = raw_e[k].copy()
        dx, dy = (int(v) for v in org_e[k] - m['origin'][i])                                  # tile origin - frame origin: x_frame = x_tile + dx
        A, Sx, Sy = int(r[I.I_A]), int(r[I.I_SX]), int(r[I.I_SY])
        r[I.I_X0] += dx; r[I.I_X1] += dx; r[I.I_Y0] += dy; r[I.I_Y1] += dy
        r[I.I_SX] = Sx + A * dx; r[I.I_SY] = Sy + A * dy
        r[I.I_SXX] += 2 * dx * Sx + A * dx * dx; r[I.I_SYY] += 2 * dy * Sy + A * dy * dy
        r[I.I_SXY] += dx * Sy + dy * Sx + A * dx * dy
        assert np.array_equal(m['raw'][i], r), (k, m['raw'][i], r)
        assert np.array_equal(m['hist'][i], hist_e[k]) and np.array_equal(m['glcm'][i], glcm_e[k]), k
