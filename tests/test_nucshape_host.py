"""Host tests of the per-nucleus shape features (nuhtc_amd/nucshape.py): the numpy restatement of the integers (np.add.reduceat) against
plain loops over pixels and boxes on the designed cases (tests/nucshape_cases.py), hand-counted rows, the Hu moments against scikit-image
0.18.3 (tests/golden/nucshape_skimage.npz, written by tools/dev/make_shape_golden.py), the closed-form slope against np.polyfit, the
degenerate rows, and the document route's host side (the four column sets of the table, the tool's flag)."""
import os
import sys

import numpy as np
import pytest

from nuhtc_amd import nucshape as ns

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucshape_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'nucshape_skimage.npz')
# |derive - skimage| <= HU_BOUND x h1^d, d the degree of an invariant in the second-order scale: the invariants are sums of products of d
# second-order-sized factors, so h1^d is their natural size.  Both sides are float64; ours starts from exact integers, skimage sums float64
# central moments in another order: a few thousand ulps of margin.
HU_BOUND = 1e-12
HU_DEGREE = (1, 2, 3, 3, 6, 4, 6)
COL = {c: i for i, c in enumerate(ns.COLUMNS)}


@pytest.fixture(scope='module')
def golden():
    z = np.load(GOLDEN)
    shapes, bits = z['shapes'], z['bits']
    masks, at = [], 0
    for h, w in shapes.tolist():
        nb = (h * w + 7) // 8
        masks.append(np.unpackbits(bits[at:at + nb], bitorder='little')[:h * w].reshape(h, w).astype(bool))
        at += nb
    assert at == len(bits)
    return masks, z['hu'], str(z['skimage_version'])


def test_restatement_against_plain_loops():
    every = dict(cases.small_masks())
    every.update(cases.hand_masks())
    for k, m in enumerate(cases.golden_blobs(6, seed=5)):
        every[f'golden-style blob {k}'] = m
    every['holed ellipse 96'] = cases.holed_ellipse(96)
    for name, m in every.items():
        assert ns.shape_reference(m).tolist() == cases.loops(m.tolist()), name
    assert cases.W_SMALL % 32 != 0 and len(cases.small_masks()) == 16


def test_hand_counted_rows():
    m = cases.hand_masks()
    # one pixel at (4, 3): every box of every size holds it and an unset position
    assert ns.shape_reference(m['pixel']).tolist() == [1, 4, 3, 5, 4, 4, 3, 16, 12, 9, 64, 48, 36, 27] + [1] * 10
    # a solid 8 x 8 at (5, 2): sixteen, four, one full box, then one box larger than the rectangle
    row = ns.shape_reference(m['solid 8x8'])
    sx, sy = 8 * sum(range(5, 13)), 8 * sum(range(2, 10))
    assert row[:7].tolist() == [64, 5, 2, 13, 10, sx, sy] and row[ns.I_BOX:].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1]
    assert row[ns.I_SXY] == sum(range(5, 13)) * sum(range(2, 10)) and row[ns.I_SYYY] == 8 * sum(y ** 3 for y in range(2, 10))
    assert ns.derive(row)[1][0, COL['Shape.FractalDimension']] == 0.0                          # N_2 = N_3 = 0
    # a 16 x 16 checkerboard: every box up to the whole board is half set
    assert ns.shape_reference(m['checkerboard 16x16'])[ns.I_BOX:].tolist() == [64, 16, 4, 1, 1, 1, 1, 1, 1, 1]
    # a solid 5 wide, 3 tall: 3 x 2 boxes of side 2, the two whole ones do not count, the four truncated ones do; 2 boxes of side 4, both truncated
    row = ns.shape_reference(m['solid 5x3'])
    assert row[:5].tolist() == [15, 2, 4, 7, 7] and row[ns.I_BOX:].tolist() == [4, 2, 1, 1, 1, 1, 1, 1, 1, 1]
    # the sums of a full 1024-px frame fit an int64 with room
    assert 1024 * sum(x ** 3 for x in range(1024)) < 2 ** 49


def test_hu_moments_against_skimage(golden):
    masks, hu, version = golden
    assert version == '0.18.3' and len(masks) == 40 and hu.shape == (40, 7)
    assert all(3 <= np.ptp(np.nonzero(m)[a]) + 1 <= 60 for m in masks for a in (0, 1))
    worst = 0.0
    for i, m in enumerate(masks):
        got = ns.derive(ns.shape_reference(m))[1][0, :7]
        h1 = hu[i, 0]
        for k in range(7):
            gap, bound = abs(got[k] - hu[i, k]), HU_BOUND * h1 ** HU_DEGREE[k]
            worst = max(worst, gap / h1 ** HU_DEGREE[k])
            assert gap <= bound, (i, k, got[k], hu[i, k], gap, bound)
    print(f'largest |derive - skimage| / h1^d: {worst:.3e}')
    # the sign of the seventh: scikit-image's (row, column) convention; the mirror image has the opposite sign, and so would (x, y)
    i = int(np.argmax(np.abs(hu[:, 6]) / hu[:, 0] ** 6))
    got = ns.derive(ns.shape_reference(masks[i]))[1][0]
    assert hu[i, 6] != 0 and np.sign(got[6]) == np.sign(hu[i, 6])
    flipped = ns.derive(ns.shape_reference(masks[i][:, ::-1]))[1][0]
    assert np.sign(flipped[6]) == -np.sign(got[6]) and np.allclose(flipped[:6], got[:6], rtol=1e-9, atol=0)


def test_hu7_sign_on_an_asymmetric_case():
    """A scalene shape whose Hu7 is far from zero: the stated convention (first index the power of y) against the other, computed here
    from the same sums."""
    m = np.zeros((30, 30), bool)
    m[2:5, 3:25] = True
    m[5:20, 3:6] = True
    m[12:14, 6:12] = True
    r = ns.shape_reference(m).tolist()
    got = ns.derive(r)[1][0]
    ys, xs = np.nonzero(m)
    A = len(xs)
    mu = lambda c, p, q: float((((c[0] - c[0].mean()) ** p) * ((c[1] - c[1].mean()) ** q)).sum()) / A ** ((p + q) / 2.0 + 1)
    yx = ns.hu_invariants(*[mu((ys, xs), p, q) for p, q in ((2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3))])
    xy = ns.hu_invariants(*[mu((xs, ys), p, q) for p, q in ((2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3))])
    assert abs(yx[6]) > 1e-6 and np.sign(got[6]) == np.sign(yx[6]) == -np.sign(xy[6])
    assert np.allclose(got[:7], yx, rtol=1e-9, atol=0) and np.allclose(xy[:6], yx[:6], rtol=1e-9, atol=0)


def test_fractal_slope_against_polyfit(golden):
    every = list(golden[0]) + [m for k, m in cases.small_masks().items() if k.startswith('blob') or k in ('annulus', 'disc r=12 at x=20', 'full frame')]
    every.append(cases.holed_ellipse(200))
    used = 0
    for m in every:
        row = ns.shape_reference(m)
        w, h = int(row[ns.I_X1] - row[ns.I_X0]), int(row[ns.I_Y1] - row[ns.I_Y0])
        js = ns.fractal_sizes(w, h)
        assert js == [j for j in range(2, 11) if 2 ** j <= min(w, h)]
        fd = ns.derive(row)[1][0, COL['Shape.FractalDimension']]
        counts = row[ns.I_BOX + np.array(js, int) - 1] if js else np.zeros(0)
        if len(js) < 2 or (counts == 0).any():
            assert fd == 0.0
            continue
        used += 1
        want = -np.polyfit(np.log(2.0 ** np.array(js)), np.log(counts.astype(np.float64)), 1)[0]
        assert abs(fd - want) <= 1e-9, (w, h, fd, want)
        assert np.isfinite(fd) and fd <= 2.0 + 1e-9                                          # a mixed box has at most four mixed children
    assert used >= 25


def test_degenerate_rows():
    assert ns.COLUMNS == ('Shape.HuMoments1', 'Shape.HuMoments2', 'Shape.HuMoments3', 'Shape.HuMoments4', 'Shape.HuMoments5', 'Shape.HuMoments6',
                          'Shape.HuMoments7', 'Shape.FractalDimension') and ns.ROW == 24
    empty = ns.shape_reference(np.zeros((9, 40), bool))
    assert not empty.any() and not ns.derive(empty)[1].any()                                    # A == 0: a zero row, zero values
    one = ns.derive(ns.shape_reference(cases.hand_masks()['pixel']))[1][0]                       # A == 1: no spread at all
    assert one.tolist() == [0.0] * 8
    for h, w in ((7, 50), (50, 7), (1, 9), (3, 3)):                                             # min side < 8: fewer than two sizes
        m = np.zeros((60, 60), bool)
        m[4:4 + h, 5:5 + w] = True
        val = ns.derive(ns.shape_reference(m))[1][0]
        assert np.isfinite(val).all() and val[7] == 0.0 and val[0] > 0
    m = np.zeros((20, 20), bool)
    m[3:11, 2:10] = True                                                                        # min side 8, a used N_j is 0
    assert ns.derive(ns.shape_reference(m))[1][0, 7] == 0.0
    row = ns.shape_reference(cases.disc(40, 40, 20, 20, 15, 6))                                 # an annulus of 31 px: the sizes 4, 8, 16
    assert row[ns.I_BOX + 1:ns.I_BOX + 4].min() > 0 and 1.0 < ns.derive(row)[1][0, 7] <= 2.0
    many = np.stack([ns.shape_reference(v) for v in cases.small_masks().values()])
    cols, val = ns.derive(many)
    assert cols == ns.COLUMNS and val.shape == (len(many), 8) and np.isfinite(val).all()
    assert np.array_equal(val[5], ns.derive(many[5])[1][0])
    # a solid square: Hu1 = (n^2 - 1) / (6 n^2), the others vanish exactly on the integers
    sq = ns.derive(ns.shape_reference(np.ones((8, 8), bool)))[1][0]
    assert abs(sq[0] - 63.0 / 384.0) <= 1e-16 and sq[1:7].tolist() == [0.0] * 6


def test_table_and_db_columns_of_the_four_sets(tmp_path):
    from nuhtc_amd import nucgrad, nucmorph, nuctex
    from nuhtc_amd import ringfeat as rf
    base = nucmorph.COLUMNS + nuctex.COLUMNS
    assert rf.table_columns() == base and rf.table_columns(gradient=True) == base + nucgrad.COLUMNS
    assert rf.table_columns(shape=True) == base + ns.COLUMNS and rf.table_columns(gradient=True, shape=True) == base + nucgrad.COLUMNS + ns.COLUMNS
    plain = rf.db_columns()
    for g in (False, True):
        with_s, without = rf.db_columns(gradient=g, shape=True), rf.db_columns(gradient=g)
        at = 56 + 8 * g
        assert len(with_s) == len(without) + 8 and with_s[:at] == without[:at] and with_s[at + 8:] == without[at:] and without[at][0] == 'score'
        assert with_s[at] == ('Shape_HuMoments1', 'REAL') and with_s[at + 7] == ('Shape_FractalDimension', 'REAL')
    assert rf.db_columns(gradient=False, shape=False) == plain
    n = 3
    args = (np.linspace(0.5, 0.9, n), ['a', 'b', 'c'], [1, 2, 3], [7, 8, 9], np.arange(n * 4).reshape(n, 4))
    sets = [(False, False), (True, False), (False, True), (True, True)]
    values = {s: np.arange(n * len(rf.table_columns(gradient=s[0], shape=s[1])), dtype=np.float64).reshape(n, -1) + 0.25 for s in sets}
    path = {s: str(tmp_path / f'g{int(s[0])}s{int(s[1])}.db') for s in sets}
    for s in sets:
        assert rf.write_db(path[s], values[s], *args, gradient=s[0], shape=s[1]) == n
        got = rf.read_db(path[s])
        assert got['columns'] == rf.db_columns(gradient=s[0], shape=s[1])
        assert [list(r[1:1 + values[s].shape[1]]) for r in got['rows']] == values[s].tolist()
    for s in sets:                                                                              # the four sets are told apart, each from each
        before = open(path[s], 'rb').read()
        for t in sets:
            why = rf.column_mismatch(path[s], gradient=t[0], shape=t[1])
            assert (why is None) == (s == t), (s, t, why)
            if s[1] != t[1]:
                assert 'Shape_HuMoments1' in why
            if s != t:
                with pytest.raises(ValueError):
                    rf.write_db(path[s], values[t], *args, gradient=t[0], shape=t[1])
        assert open(path[s], 'rb').read() == before
    assert rf.column_mismatch(str(tmp_path / 'none.db'), shape=True) is None


def test_tool_flag():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import wsi_feat_extract as tool
    p = tool.build_parser()
    assert p.parse_args(['data', '--segdir', 'seg']).shape is False
    a = p.parse_args(['data', '--segdir', 'seg', '--shape'])
    assert a.shape is True and a.gradient is False
    a = p.parse_args(['data', '--segdir', 'seg', '--gradient', '--shape'])
    assert a.shape is True and a.gradient is True
    assert 'FractalDimension' in p.format_help() and 'only histomicstk family that is not produced' in tool.__doc__
