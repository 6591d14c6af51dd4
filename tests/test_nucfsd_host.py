"""Host tests of the Fourier-descriptor integers and features (nuhtc_amd/nucfsd.py): the numpy restatement against a plain loop in Python
integers, hand-counted rows, the properties of derive(), an independent float resampling, and the flag and column plumbing of
nuhtc_amd/ringfeat.py and tools/wsi_feat_extract.py.  No GPU."""
import itertools
import os
import sys
from argparse import ArgumentParser

import numpy as np
import pytest

from nuhtc_amd import nucfsd as nf
from nuhtc_amd import nucgrad, nucmorph, nucshape, nuctex, ringfeat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucfsd_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = nf.K


def exact_sign(p, q):
    """The sign of p + q sqrt 2 for Python integers of any size: by squaring."""
    if p >= 0 and q >= 0:
        return int(p > 0 or q > 0)
    if p <= 0 and q <= 0:
        return -1
    return (1 if p * p > 2 * q * q else -1) * (1 if p > 0 else -1)


def plain_row(ring):
    """The row of the module docstring by a loop over the edges, in Python integers."""
    v = [(int(x), int(y)) for x, y in np.asarray(ring).reshape(-1, 2)]
    n, row = len(v), [0] * nf.ROW
    if n < 1:
        row[0] = 1
        return row
    a, b, code, A, B = [], [], [], 0, 0
    for e in range(n):
        dx, dy = v[(e + 1) % n][0] - v[e][0], v[(e + 1) % n][1] - v[e][1]
        if dx and dy and abs(dx) != abs(dy):
            row[0] = 2
            return row
        a.append(A)
        b.append(B)
        sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
        code.append(next((d for d in range(8) if (nf.DX[d], nf.DY[d]) == (sx, sy)), 0))
        if dx and dy:
            B += abs(dx)
        else:
            A += abs(dx) + abs(dy)
    if A + B == 0 or A + B > nf.MAX_STEPS:
        row[0] = 1 if A + B == 0 else 3
        return row
    row[:4] = 0, A, B, n
    for k in range(K):
        e = max(e for e in range(n) if exact_sign(K * a[e] - k * A, K * b[e] - k * B) <= 0)
        row[4 + 5 * k:9 + 5 * k] = v[e][0], v[e][1], code[e], a[e], b[e]
    return row


@pytest.fixture(scope='module')
def rows():
    """name -> (ring, row of fsd_reference), computed once."""
    out = {name: (ring, nf.fsd_reference(ring)) for name, ring in cases.designed().items()}
    for _, r in out.values():
        r.setflags(write=False)
    return out


def test_reference_equals_the_plain_loop(rows):
    assert len(rows) >= 23
    for name, (ring, row) in rows.items():
        assert row.dtype == np.int32 and row.shape == (nf.ROW,)
        assert row.tolist() == plain_row(ring), name
        assert row[0] == cases.STATUS.get(name, 0), name
        if row[0]:
            assert not row[1:].any(), name
        else:
            assert row[nf.I_N] == len(ring) and row[nf.I_A] + row[nf.I_B] <= nf.MAX_STEPS, name
    assert len(rows['comb of 2082 vertices'][0]) > 2000 and rows['exactly 2^24 steps'][1][1] == 1 << 24
    assert rows['diamond, A = 0'][1][1] == 0 and rows['rectangle, B = 0'][1][2] == 0


def test_hand_counted_squares(rows):
    ring, row = rows['square of perimeter 128']                  # east, south, west, north: sample k lies k steps along, on edge k // 32
    want = [0, 128, 0, 4]
    for k in range(K):
        e = k // 32
        want += [int(ring[e, 0]), int(ring[e, 1]), (0, 6, 4, 2)[e], 32 * e, 0]
    assert row.tolist() == want
    ring, row = rows['square of perimeter 256']                  # south, east, north, west: sample k lies 2 k steps along
    want = [0, 256, 0, 4]
    for k in range(K):
        e = k // 32
        want += [int(ring[e, 0]), int(ring[e, 1]), (6, 0, 2, 4)[e], 64 * e, 0]
    assert row.tolist() == want
    row = rows['two vertices, diagonal'][1]                      # out (south-west, code 5) and back (code 1): the turn is sample 64
    assert row[:4].tolist() == [0, 0, 18, 2] and row[4 + 5 * 63:4 + 5 * 65].tolist() == [3, 3, 5, 0, 0, -6, 12, 1, 0, 9]
    row = rows['zero-length edges'][1]                           # a sample on a repeated vertex belongs to the LAST edge that starts there
    assert row[4:9].tolist() == [0, 0, 0, 0, 0] and row[3] == 9
    ring = rows['closing vertex repeated'][0]
    assert (rows['closing vertex repeated'][1][4::5] != 0).sum() == 64 and len(ring) == 5       # x_e is 6 on two of the four sides


def test_float64_picks_the_wrong_edge_on_the_pell_ring(rows):
    """The case cannot rot: at (k, vertex) of tests/nucfsd_cases.PELL p and q have opposite signs, p + q sqrt 2 is positive (the vertex
    lies beyond the sample) and float64 evaluates it to zero or less, which would hand the sample to the edge that starts there."""
    c = cases.PELL
    ring, row = rows['pell']
    on, steps, diag, _ = nf.edges(ring)
    assert on.all()
    a, b = int(np.where(diag, 0, steps)[:c['vertex']].sum()), int(np.where(diag, steps, 0)[:c['vertex']].sum())
    assert (a, b, int(row[nf.I_A]), int(row[nf.I_B])) == (c['a'], c['b'], c['A'], c['B'])
    p, q = K * a - c['k'] * c['A'], K * b - c['k'] * c['B']
    assert (p, q) == (c['p'], c['q']) and p > 0 > q and p * p - 2 * q * q == 2
    assert exact_sign(p, q) == 1 and int(nf.sign(p, q)) == 1
    assert cases.float_sign(p, q) <= 0                                                  # float64 disagrees
    got = row[4 + 5 * c['k']:9 + 5 * c['k']].tolist()
    assert got[3:] != [a, b] and got == plain_row(ring)[4 + 5 * c['k']:9 + 5 * c['k']]  # the exact decision: an earlier edge
    assert np.abs(ring).max() > 2 ** 29


def test_sign_against_python_integers():
    rng = np.random.default_rng(3)
    lim = K * (nf.MAX_STEPS - 1)
    p, q = [1], [1]
    while p[-1] + 2 * q[-1] <= lim:
        p, q = p + [p[-1] + 2 * q[-1]], q + [p[-1] + q[-1]]
    pairs = [(sp * (u + du), sq * (v + dv)) for u, v in zip(p, q) for sp in (1, -1) for sq in (1, -1) for du in (-1, 0, 1) for dv in (-1, 0, 1)]
    pairs += [(0, 0), (lim, -lim), (-lim, lim), (lim, lim), (0, -lim), (lim, 0)]
    pairs += [tuple(int(v) for v in rng.integers(-lim, lim + 1, 2) >> int(s)) for s in rng.integers(0, 31, 4000)]
    pairs = [(u, v) for u, v in pairs if abs(u) <= lim and abs(v) <= lim]
    got = nf.sign([u for u, _ in pairs], [v for _, v in pairs])
    assert got.tolist() == [exact_sign(u, v) for u, v in pairs]


def _ring_geometry(ring):
    v = np.asarray(ring, np.float64)
    d = np.roll(v, -1, 0) - v
    return v, d, np.hypot(d[:, 0], d[:, 1])


def test_derive_properties(rows):
    names = list(rows)
    cols, val = nf.derive(np.stack([rows[n][1] for n in names]))
    assert cols == nf.COLUMNS == tuple(f'Shape.FSD{i}' for i in range(1, 7)) and val.shape == (len(names), 6) and val.dtype == np.float64
    assert np.isfinite(val).all() and (val >= 0).all()
    for name, f in zip(names, val):
        if rows[name][1][0]:
            assert not f.any(), name
        else:
            assert abs(f.sum() - 1.0) <= 4 * 2.0 ** -52, (name, f.sum() - 1.0)
    assert np.array_equal(nf.derive(rows['pell'][1])[1][0], val[names.index('pell')])                # one row or many: the same values
    # the sample points: on their edge, and k L / K along the ring
    for name in names:
        ring, row = rows[name]
        if row[0]:
            continue
        P, s = nf.sample_points(row)
        v, d, length = _ring_geometry(ring)
        L = row[nf.I_A] + row[nf.I_B] * np.sqrt(2.0)
        start = row[4 + 3::5] + row[4 + 4::5] * np.sqrt(2.0)
        tol = 8 * 2.0 ** -52 * L
        assert np.abs(start + s[0] - np.arange(K) * L / K).max() <= tol, name
        # the edge of each sample, found again by its start vertex and start length
        a_e, b_e = np.cumsum(np.where(d[:, 0] * d[:, 1] == 0, length, 0)), np.cumsum(np.where(d[:, 0] * d[:, 1] != 0, np.abs(d[:, 0]), 0))
        a_e, b_e = np.concatenate([[0], a_e[:-1]]), np.concatenate([[0], b_e[:-1]])
        for k in range(K):
            e = max(np.nonzero((a_e == row[4 + 5 * k + 3]) & (b_e == row[4 + 5 * k + 4]))[0])
            assert (v[e] == row[4 + 5 * k:6 + 5 * k]).all(), (name, k)
            assert -tol <= s[0, k] <= length[e] + tol, (name, k)
            t = s[0, k] / length[e]
            assert np.abs(P[0, k] - (v[e] + t * d[e])).max() <= 8 * 2.0 ** -52 * (np.abs(v).max() + L), (name, k)


def _float_points(ring):
    """An independent resampling in floats: cumulative float lengths, np.searchsorted for the edge, np.interp for the point."""
    v, d, length = _ring_geometry(ring)
    cum = np.concatenate([[0.0], np.cumsum(length)])
    t = np.arange(K) * cum[-1] / K
    closed = np.concatenate([v, v[:1]])
    e = np.searchsorted(cum, t, 'right') - 1
    return np.stack([np.interp(t, cum, closed[:, 0]), np.interp(t, cum, closed[:, 1])], 1), e, np.abs(cum[None, :] - t[:, None]).min(1)


def test_derive_against_a_float_resampling():
    """Rings where no sample falls near a vertex (asserted: every sample is at least 1e-6 px from every vertex, or lies ON one in exact
    integers -- sample 0 always does -- where both routes return the vertex itself whichever edge they pick).  The bound on
    the distance of the two sample points, per coordinate, with u = 2^-52, n edges, perimeter L and coordinates up to X: the float
    route sums n lengths (each partial sum within n u L of the true one), forms t = k L / K (2 u L) and interpolates (one subtraction,
    one division, one multiplication and one addition on numbers up to X + L: 4 u (X + L)); the integer route forms q sqrt 2 / K, adds
    p / K and scales the direction (4 u L) and adds the vertex (u (X + L)).  A distance along the edge moves a coordinate by at most
    itself, so the gap is at most (n + 6) u L + 5 u (X + L) <= (n + 11) u (X + L)."""
    rings = {'disc 10': cases.traced(cases.disc(10), (100, 50)), 'disc 23': cases.traced(cases.disc(23)), 'ellipse 20x6': cases.traced(cases.ellipse(20, 6), (7, 9)),
             'clover': cases.traced(cases.clover(), (1000, 2000)), 'saw 257': cases.saw(257, seed=257), 'saw 1025': cases.saw(1025, seed=1025)}
    worst = 0.0
    for name, ring in rings.items():
        row = nf.fsd_reference(ring)
        assert row[0] == 0, name
        want, e, nearest = _float_points(ring)
        P, along = nf.sample_points(row)
        assert ((nearest >= 1e-6) | (along[0] == 0.0)).all() and (nearest >= 1e-6).sum() > K // 2, (name, nearest.min())
        _, _, length = _ring_geometry(ring)
        L, X = float(length.sum()), float(np.abs(ring).max())
        bound = (len(ring) + 11) * 2.0 ** -52 * (X + L)
        gap = float(np.abs(P[0] - want).max())
        print(f'{name}: n {len(ring)} L {L:.3f} gap {gap:.3e} bound {bound:.3e}')
        assert gap <= bound, (name, gap, bound)
        worst = max(worst, gap / bound)
    print(f'largest gap / bound {worst:.3f}')


def test_orderings_on_discs_an_ellipse_and_a_clover():
    f = lambda mask: nf.derive(nf.fsd_reference(cases.traced(mask)))[1][0]
    disc, ell, clo = f(cases.disc(10)), f(cases.ellipse(20, 6)), f(cases.clover())
    print(np.round(disc, 4), np.round(ell, 4), np.round(clo, 4))
    assert ell[1] > disc[1] and clo[2] > disc[2]
    assert 0.85 < disc[0] < 0.95 and disc[0] > ell[0]                          # a round nucleus keeps its energy in the lowest band
    big = f(cases.disc(23))
    assert big[0] > 0.85 and ell[1] > big[1]


def test_flags():
    p = ArgumentParser()
    ringfeat.add_fsd_flags(p)
    assert p.parse_args([]).fsd is False and p.parse_args(['--fsd']).fsd is True
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import wsi_feat_extract as tool
    a = tool.parse_args(['data', '--segdir', 'seg', '--fsd'])
    assert a.fsd and not a.shape and not a.gradient
    a = tool.parse_args(['data', '--segdir', 'seg', '--gradient', '--shape', '--fsd'])
    assert a.fsd and a.shape and a.gradient
    assert tool.parse_args(['data', '--segdir', 'seg']).fsd is False


def test_db_columns_order_for_every_selection(tmp_path):
    dot = lambda cols: [c.replace('.', '_') for c in cols]
    tail = ['score', 'type', 'class_id', 'nuclei_id', 'x_min', 'y_min', 'x_max', 'y_max']
    for g, s, f in itertools.product((False, True), repeat=3):
        want = ['Label'] + dot(nucmorph.COLUMNS + nuctex.COLUMNS) + (dot(nucgrad.COLUMNS) if g else []) + (dot(nucshape.COLUMNS) if s else []) + \
               (dot(nf.COLUMNS) if f else []) + tail
        got = ringfeat.db_columns(gradient=g, shape=s, fsd=f)
        assert [c for c, _ in got] == want, (g, s, f)
        assert all(t == 'REAL' for c, t in got if c.startswith('Shape_FSD'))
        assert list(ringfeat.table_columns(gradient=g, shape=s, fsd=f)) == [c for c in nucmorph.COLUMNS + nuctex.COLUMNS] + (list(nucgrad.COLUMNS) if g else []) + \
               (list(nucshape.COLUMNS) if s else []) + (list(nf.COLUMNS) if f else [])
    assert ringfeat.db_columns() == ringfeat.db_columns(fsd=False) and ringfeat.table_columns(gradient=False, shape=True) == ringfeat.table_columns(gradient=False, shape=True, fsd=False)
    # a table written with one selection is refused by every other, in both directions, and left alone
    n = 2
    rect = np.array([[0, 0, 3, 3], [4, 4, 9, 9]])
    path = str(tmp_path / 'a.db')
    vals = np.arange(n * len(ringfeat.table_columns(fsd=True)), dtype=np.float64).reshape(n, -1)
    assert ringfeat.write_db(path, vals, [0.5, 0.6], ['a', 'b'], [1, 2], [7, 8], rect, fsd=True) == n
    assert ringfeat.column_mismatch(path, fsd=True) is None
    assert 'Shape_FSD1' in ringfeat.column_mismatch(path) and 'Shape_HuMoments1' in ringfeat.column_mismatch(path, shape=True, fsd=True)
    before = open(path, 'rb').read()
    with pytest.raises(ValueError):
        ringfeat.write_db(path, vals[:, :55], [0.5, 0.6], ['a', 'b'], [1, 2], [7, 8], rect)
    assert open(path, 'rb').read() == before
    got = ringfeat.read_db(path)
    assert got['columns'] == ringfeat.db_columns(fsd=True) and list(got['rows'][1][56:62]) == vals[1, 55:].tolist()
