"""Host tests of the per-nucleus gradient features (nuhtc_amd/nucgrad.py): the numpy restatement of the integers (np.gradient, math.isqrt,
np.histogram) against a plain double loop over the designed cases (tests/nucgrad_cases.py), derive() against numpy and scipy.stats on the
magnitudes themselves, the degenerate rows, hand-counted rows, and the document route's host side (frames with a margin, the table's
columns, the tool's flags)."""
import os
import sys

import numpy as np
import pytest

from nuhtc_amd import nucgrad as ng
from nuhtc_amd import nucmorph

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucgrad_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Largest relative difference measured on the CPU when the tests were written, derive() against np.mean / np.std / scipy.stats.skew /
# kurtosis / entropy and the histogram energy on m / 4 of every designed mask on every designed tile (columns that are exactly 0 on both
# sides excepted); the test asserts 16 times the figure.  It is the Skewness -0.00516 of 'block bottom right' on the ramp tile: a value
# near zero comes out of a cancellation ON SCIPY'S SIDE (float64 central moments; ours are exact integers).  Without Skewness and Kurtosis
# the largest is 2.7e-16.
MEASURED_REL = 4.171e-13


@pytest.fixture(scope='module')
def designed():
    """(tile name, mask name) -> (row int64 (18,), m of the mask pixels) of every designed mask on every designed tile."""
    tiles, masks = cases.tiles(cases.H_SMALL, cases.W_SMALL), cases.small_masks()
    out = {}
    for t, tile in tiles.items():
        mag = ng.magnitude(tile)[0]
        for k, m in masks.items():
            out[t, k] = (ng.grad_reference(tile, m), mag[m])
    return out


def test_cases_hold_what_they_were_designed_for():
    tiles = cases.tiles(cases.H_SMALL, cases.W_SMALL)
    h = {t: nucmorph.haematoxylin(v) for t, v in tiles.items()}
    assert all(len(np.unique(h[t])) == 1 for t in ('zeros', 'full', 'planes'))
    assert np.unique(h['vertical step']).tolist() == [0, 255] and np.unique(h['checker']).tolist() == [0, 255]
    greys, k = cases.ridge_greys()
    assert k >= 20 and np.unique(h['ridge']).tolist() == [0, k, 2 * k, 3 * k]
    gx2, gy2 = ng.gradient2(h['ridge'])
    R = cases.RIDGE_X
    assert gx2[5, R - 1:R + 5].tolist() == [0, k, 2 * k, 2 * k, k, 0] and not gy2.any()          # the plateau, two pixels wide
    m = ng.magnitude(tiles['checker'])[0]
    assert m.max() == ng.T_MAX == 1442 and m[0, 0] == 1442 and m[-1, -1] == 1442 and m[1:-1, 1:-1].max() == 0
    masks = cases.small_masks()
    assert len(masks) == len(set(masks)) and {'empty', 'full frame', 'pair across x=31|32', 'top edge', 'block bottom right', 'pixel at x=32'} <= set(masks)
    assert cases.W_SMALL % 32 != 0


@pytest.mark.parametrize('T', [1, 37, 1442])
def test_restatement_against_plain_loops(T):
    tiles, masks = cases.tiles(cases.H_SMALL, cases.W_SMALL), cases.small_masks()
    for t, tile in tiles.items():
        if T != 1 and t not in ('random', 'ramp', 'checker'):
            continue
        h = nucmorph.haematoxylin(tile).tolist()
        for k, m in masks.items():
            assert ng.grad_reference(tile, m, T).tolist() == cases.loops(h, m.tolist(), T), (t, k, T)


def test_restatement_small_frames_against_plain_loops():
    """Frames of one pixel, one column, one row and two by two (np.gradient itself refuses an axis of one pixel), and widths round 32."""
    rng = np.random.default_rng(3)
    for H, W in ((1, 1), (1, 7), (9, 1), (2, 2), (2, 33), (3, 32), (5, 31)):
        tile = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for mask in (np.ones((H, W), bool), rng.random((H, W)) < 0.5):
            want = cases.loops(nucmorph.haematoxylin(tile).tolist(), mask.tolist())
            assert ng.grad_reference(tile, mask).tolist() == want, (H, W)
    one = ng.grad_reference(rng.integers(0, 256, (9, 1, 3), dtype=np.uint8), np.ones((9, 1), bool))
    assert one[ng.I_A] == 9 and one[ng.I_MX] > 0                                                # a 1-px-wide frame: gx2 = 0, gy2 counts


def test_derive_against_numpy_and_scipy(designed):
    from scipy import stats
    rel, where, used = 0.0, None, 0
    for key, (row, m) in designed.items():
        if len(m) == 0:
            continue
        used += 1
        v = m / 4.0
        cols, val = ng.derive(row)
        hist = np.histogram(v, bins=10)[0]
        p = hist / hist.sum()
        const = len(np.unique(m)) == 1
        edge = float(row[ng.I_EDGE])
        want = [np.mean(v), np.std(v), 0.0 if const else stats.skew(v), 0.0 if const else stats.kurtosis(v), stats.entropy(hist), float((p * p).sum()),
                edge, edge / len(m)]
        assert np.isfinite(val).all(), key
        for c, (got, w) in enumerate(zip(val[0].tolist(), want)):
            w = float(w)
            if got != w:
                assert w != 0, (key, cols[c], got)
                if abs(got - w) / abs(w) > rel:
                    rel, where = abs(got - w) / abs(w), (key, cols[c], got, w)
    print(f'{used} rows; largest relative difference {rel:.3e} at {where}')
    assert used > 200
    assert rel <= 16 * MEASURED_REL, (rel, where)


def test_degenerate_rows(designed):
    col = {c: i for i, c in enumerate(ng.COLUMNS)}
    assert len(ng.COLUMNS) == 8 and ng.COLUMNS[0] == 'Nucleus.Gradient.Mag.Mean' and ng.COLUMNS[-1] == 'Nucleus.Gradient.Canny.Mean'
    for t in ('random', 'planes'):                                                              # the empty mask: a zero row, zero values
        assert not designed[t, 'empty'][0].any() and not ng.derive(designed[t, 'empty'][0])[1].any()
    row = designed['random', 'pixel'][0]                                                        # one pixel: mn == mx, bin 5, no variance
    assert row[ng.I_A] == 1 and row[ng.I_MN] == row[ng.I_MX] == row[ng.I_S1] > 0 and row[ng.I_HIST:].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0]
    val = ng.derive(row)[1][0]
    assert val[col['Nucleus.Gradient.Mag.Mean']] == row[ng.I_S1] / 4.0 and val[col['Nucleus.Gradient.Mag.Std']] == 0
    assert val[col['Nucleus.Gradient.Mag.Skewness']] == 0 and val[col['Nucleus.Gradient.Mag.Kurtosis']] == 0
    assert val[col['Nucleus.Gradient.Mag.HistEntropy']] == 0 and val[col['Nucleus.Gradient.Mag.HistEnergy']] == 1
    for t in ('zeros', 'full', 'planes'):                                                       # a constant tile: all m = 0, bin 5, no edge
        row = designed[t, 'full frame'][0]
        assert row.tolist() == [64 * 40, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 64 * 40, 0, 0, 0, 0], t
        assert ng.derive(row)[1][0].tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    many = ng.derive(np.stack([designed['random', k][0] for k in cases.small_masks()]))[1]
    assert np.isfinite(many).all() and np.array_equal(many[list(cases.small_masks()).index('disc r=7')], ng.derive(designed['random', 'disc r=7'][0])[1][0])
    with pytest.raises(ValueError):
        ng.grad_reference(np.zeros((4, 4, 3), np.uint8), np.ones((4, 4), bool), 0)
    with pytest.raises(ValueError):
        ng.grad_reference(np.zeros((4, 4, 3), np.uint8), np.ones((4, 4), bool), 1443)
    assert ng.threshold(0.25) == 1 and ng.threshold(2) == 8 and ng.threshold(360.5) == 1442
    for bad in (0, 0.1, 361):
        with pytest.raises(ValueError):
            ng.threshold(bad)


def test_hand_counted_rows(designed):
    """The vertical step between x = 19 (h = 0) and x = 20 (h = 255) of the 64 x 40 frame: the central difference is 255 at both columns
    and 0 elsewhere, so m = isqrt(4 x 255^2) = 510 on 2 x 64 pixels; of the two equal columns the tie rule counts x = 19 (q > q(18) = 0 and
    q >= q(20)) and not x = 20 (q > q(19) fails): 64 edge pixels; over [0, 510] the 2432 flat pixels fall into bin 0, the 128 into bin 9."""
    row = designed['vertical step', 'full frame'][0]
    assert row.tolist() == [2560, 128 * 510, 128 * 510 ** 2, 128 * 510 ** 3, 128 * 510 ** 4, 0, 510, 64, 2432, 0, 0, 0, 0, 0, 0, 0, 0, 128]
    # the mask's own columns decide, the neighbours are read through it: the left edge mask (x 0..2) sees nothing, a mask on x = 20 alone no edge
    assert designed['vertical step', 'left edge'][0][ng.I_MX] == 0
    only20 = np.zeros((64, 40), bool); only20[:, 20] = True
    assert ng.grad_reference(cases.step(64, 40), only20).tolist() == [64, 64 * 510, 64 * 510 ** 2, 64 * 510 ** 3, 64 * 510 ** 4, 510, 510, 0, 0, 0, 0, 0, 0, 64, 0, 0, 0, 0]
    # the horizontal step between y = 31 and y = 32: the same with rows for columns, 40 edge pixels
    row = designed['horizontal step', 'full frame'][0]
    assert row.tolist() == [2560, 80 * 510, 80 * 510 ** 2, 80 * 510 ** 3, 80 * 510 ** 4, 0, 510, 40, 2480, 0, 0, 0, 0, 0, 0, 0, 0, 80]
    # the ridge: doubled gradients k, 2k, 2k, k -- one edge pixel a row, on the first plateau column
    _, k = cases.ridge_greys()
    row = designed['ridge', 'full frame'][0]
    assert row[ng.I_EDGE] == 64 and row[ng.I_MX] == 4 * k and row[ng.I_S1] == 64 * (2 * k + 4 * k + 4 * k + 2 * k)
    assert row[ng.I_HIST:].tolist() == [64 * 36, 0, 0, 0, 0, 128, 0, 0, 0, 128]
    # the checkerboard's corners hold the largest magnitude, and a threshold above a pixel's m drops it
    row = designed['checker', 'corner top left'][0]
    assert row[:8].tolist() == [1, 1442, 1442 ** 2, 1442 ** 3, 1442 ** 4, 1442, 1442, 1]
    tile = cases.tiles(64, 40)['random']
    full = np.ones((64, 40), bool)
    edges = [int(ng.grad_reference(tile, full, T)[ng.I_EDGE]) for T in (1, 200, 600, 1442)]
    assert edges == sorted(edges, reverse=True) and edges[0] > edges[2] > 0 and edges[3] == 0
    # the S4 bound of a full 1024-px frame, in Python integers
    assert 1024 * 1024 * 1442 ** 4 < 2 ** 63


def test_margin_frames_and_table_columns():
    from nuhtc_amd import ringfeat as rf
    rect = np.array([[0, 0, 9, 9], [1, 5, 30, 20], [100, 200, 127, 227], [100, 200, 128, 227], [10, 10, 261, 40], [10, 10, 262, 40], [3, 1, 255, 256]], np.int64)
    origin, side = rf.gradient_frames(rect)
    assert origin.tolist() == [[0, 0], [0, 3], [98, 198], [98, 198], [8, 8], [8, 8], [1, 0]]
    # the side holds the rectangle and the margin on both sides, less what the slide's edge cut off the margin at the minimum corner
    assert side.tolist() == [32, 64, 32, 64, 256, 0, 0]
    assert rf.table_columns() == nucmorph.COLUMNS + rf.nuctex.COLUMNS and len(rf.table_columns(gradient=True)) == 63
    assert rf.table_columns(gradient=True)[55:] == ng.COLUMNS
    plain, with_g = rf.db_columns(), rf.db_columns(gradient=True)
    assert len(with_g) == len(plain) + 8 and with_g[:56] == plain[:56] and with_g[64:] == plain[56:] and plain[56][0] == 'score'
    assert with_g[56] == ('Nucleus_Gradient_Mag_Mean', 'REAL') and with_g[63] == ('Nucleus_Gradient_Canny_Mean', 'REAL')


def test_db_with_gradient_columns_and_resume_rule(tmp_path):
    from nuhtc_amd import ringfeat as rf
    n = 3
    values = np.arange(n * 55, dtype=np.float64).reshape(n, 55)
    grad = np.arange(n * 8, dtype=np.float64).reshape(n, 8) + 0.5
    args = (np.linspace(0.5, 0.9, n), ['a', 'b', 'c'], [1, 2, 3], [7, 8, 9], np.arange(n * 4).reshape(n, 4))
    plain, with_g = str(tmp_path / 'plain.db'), str(tmp_path / 'grad.db')
    rf.write_db(plain, values, *args)
    ok = np.array([True, False, True])
    wide = np.concatenate([values, np.where(ok[:, None], grad, np.nan)], 1)
    assert rf.write_db(with_g, wide, *args, gradient=True) == n
    a, b = rf.read_db(plain), rf.read_db(with_g)
    assert a['columns'] == rf.db_columns() and b['columns'] == rf.db_columns(gradient=True)
    for ra, rb, k in zip(a['rows'], b['rows'], range(n)):
        assert rb[:56] == ra[:56] and rb[64:] == ra[56:]
        assert list(rb[56:64]) == (grad[k].tolist() if ok[k] else [None] * 8)                    # no gradient frame: NULL
    assert rf.column_mismatch(plain, gradient=False) is None and rf.column_mismatch(with_g, gradient=True) is None
    assert rf.column_mismatch(str(tmp_path / 'none.db'), gradient=True) is None
    assert 'Nucleus_Gradient_Mag_Mean' in rf.column_mismatch(plain, gradient=True) and 'Nucleus_Gradient_Mag_Mean' in rf.column_mismatch(with_g, gradient=False)
    with pytest.raises(ValueError):
        rf.write_db(plain, wide, *args, gradient=True)                                           # never appended to under another column set
    with pytest.raises(ValueError):
        rf.write_db(with_g, values, *args)
    assert len(rf.read_db(plain)['rows']) == n and len(rf.read_db(with_g)['rows']) == n


def test_tool_flags():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import wsi_feat_extract as tool
    p = tool.build_parser()
    a = p.parse_args(['data', '--segdir', 'seg'])
    assert a.gradient is False and a.edge_thr == 0.25
    a = p.parse_args(['data', '--segdir', 'seg', '--gradient', '--edge-thr', '2.5'])
    assert a.gradient is True and ng.threshold(a.edge_thr) == 10
    assert 'Canny' in p.format_help()
