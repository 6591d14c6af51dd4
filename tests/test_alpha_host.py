"""Host-only checks of the alpha complex (nuhtc_amd/alphacomplex.py): `alpha_reference` against a loop in plain Python integers and
fractions.Fraction that passes NO witness over (tests/alpha_cases.py: fraction_loop), against hand-written edge lists and closed forms, the
identity with scipy's Delaunay triangulation on sets in general position, the Gabriel-flagged edges against proximity.proximity_reference
and the forest of mst.mst_reference inside the edges, int64 against Python integers at D = 1024, `derive` against rationals, the .npz
round trip, and the row of the table in nuhtc_amd/slidepoints.py with its flags and refusals.  The device is compared with
`alpha_reference` in tests/test_hip_alpha.py.

The issue's lattice case names the diameters 14 and 15 at spacing 10; D = 2 r is even in half pixels, so 15 is taken at twice the scale
(spacing 20, D = 28 and 30) and, at spacing 10, as the next diameter there is (16): the same two sides of the threshold s * sqrt(2)."""
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import alpha_cases as AL
from nuhtc_amd import alphacomplex as ax
from nuhtc_amd import mst, slidepoints
from nuhtc_amd import proximity as px

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def references():
    return {name: ax.alpha_reference(*case) for name, case in AL.small_cases().items()}


# ---- the restatement
@pytest.mark.parametrize('name', sorted(AL.small_cases()))
def test_reference_equals_the_loop_in_fractions(references, name):
    e, d2, apex, gab, deg, m, m_gab = references[name]
    n = len(AL.small_cases()[name][0])
    assert e.dtype == np.int32 and e.shape == (m, 2) and d2.dtype == np.int32 and d2.shape == (m,) and apex.dtype == np.int32 and apex.shape == (m, 2)
    assert gab.dtype == np.uint8 and gab.shape == (m,) and deg.dtype == np.int32 and deg.shape == (n, 2)
    want = AL.fraction_loop(*AL.small_cases()[name])
    assert e.tolist() == want[0] and d2.tolist() == want[1] and apex.tolist() == want[2] and gab.tolist() == want[3] and deg.tolist() == want[4]
    assert (m, m_gab) == want[5:]
    assert (deg[:, 1] <= deg[:, 0]).all() and int(deg[:, 0].sum()) == 2 * m and int(deg[:, 1].sum()) == 2 * m_gab


def test_reference_equals_the_hand_written_lists(references):
    AL.equal(references['two_at_D'], AL.expected(2, AL.TWO_AT_D), 'd2 = D * D')
    AL.equal(references['two_beyond'], AL.expected(2, []), 'beyond D')
    AL.equal(references['two_one_over'], AL.expected(2, []), 'd2 = D * D + 1')
    AL.equal(references['right_5'], AL.expected(3, AL.RIGHT_5), '6-8-10 at r = 5')
    AL.equal(references['right_4'], AL.expected(3, AL.RIGHT_4), '6-8-10 at r = 4')
    AL.equal(references['collinear'], AL.expected(6, AL.COLLINEAR), 'collinear')
    AL.equal(references['diametral'], AL.expected(6, AL.DIAMETRAL), 'on and inside the diametral circle')
    AL.equal(references['other_label_any'], AL.expected(6, AL.OTHER_LABEL[0]), 'any')
    AL.equal(references['other_label_class'], AL.expected(6, AL.OTHER_LABEL[1]), 'class')
    assert references['one_point'][4].tolist() == [[0, 0]] and references['one_point'][5:] == (0, 0)
    AL.equal(references['two_coincident'], AL.expected(2, [(0, 1, 0, -1, -1, 1)]), 'coincident')
    e, d2, apex, gab, deg, m, m_gab = references['far_witness']
    assert e[0].tolist() == [0, 1] and apex[0].tolist() == [2, -1] and 10 * 10 + 6 * 6 > d2[0] == 16       # the apex is farther from i than j is
    e = {tuple(x) for x in references['borders'][0].tolist()}
    assert (2, 3) not in e and (5, 6) not in e and (8, 9) in e and (11, 12) not in e and {(2, 4), (3, 4), (5, 7), (6, 7)} <= e
    row = references['borders'][0].tolist().index([8, 9])
    assert references['borders'][2][row].tolist() == [-1, 10]                            # the apex in the cell below
    empty = ax.alpha_reference(np.zeros((0, 2)), [], 3, 8, 0)
    assert empty[0].shape == (0, 2) and empty[1].shape == (0,) and empty[2].shape == (0, 2) and empty[3].shape == (0,) and empty[4].shape == (0, 2)
    assert empty[5:] == (0, 0) and empty[0].dtype == np.int32 and empty[3].dtype == np.uint8


@pytest.mark.parametrize('k', [3, 5, 7])
def test_points_on_a_circle_of_radius_r_keep_every_chord(references, k):
    """k points on the circle of radius 25 about a lattice point, r = 25: all chords are edges, every bound is the circle itself (lo = hi
    where both sides have a witness), and every circumradius is exactly r.  At r = 24 the circle is out of reach: no triangle."""
    case = AL.cocircular(k)
    e, d2, apex, gab, deg, m, m_gab = references[f'circle_{k}']
    assert m == k * (k - 1) // 2 and (deg[:, 0] == k - 1).all()
    p = case[0].astype(np.int64)
    d = ax.derive(e, d2, apex, gab, deg, p, case[1], 2, 25)
    two = (apex >= 0).all(1)
    assert int(d['n_degenerate']) == int(two.sum()) == (0 if k == 3 else k * (k - 3) // 2)         # the diagonals of the k-gon: lo = hi
    assert int(d['n_triangles']) == len(d['triangles']) and len(d['triangles']) >= k - 2
    for a, b, c in d['triangles'].tolist():                                                        # exact: |ab|^2 |bc|^2 |ca|^2 = 4 r^2 cross^2 (half pixels, r = 25)
        la, lb, lc = (int(((p[u] - p[v]) ** 2).sum()) for u, v in ((a, b), (b, c), (a, c)))
        cross = int((p[b][0] - p[a][0]) * (p[c][1] - p[a][1]) - (p[b][1] - p[a][1]) * (p[c][0] - p[a][0]))
        assert la * lb * lc == 4 * 625 * cross * cross
    assert np.allclose(d['triangle_circumradius_px'], 12.5, rtol=1e-14) and (d['voronoi_px'][two] == 0).all()
    if k < 7:
        out = references[f'circle_{k}_r24']
        assert (out[2] == -1).all() and out[5] >= 1


def test_the_lattice_in_closed_form(references):
    """4 x 4 at spacing 10: its 24 sides below the diagonal's length, and both diagonals of all 9 cells from there on: 42."""
    for name, want in (('lattice_14', 24), ('lattice_16', 42), ('lattice_28', 24), ('lattice_30', 42)):
        e, d2, apex, gab, deg, m, m_gab = references[name]
        s2 = 100 if name in ('lattice_14', 'lattice_16') else 400
        assert m == want == AL.lattice_edges(4, 4, want == 42) and m_gab == m, name
        assert int((d2 == s2).sum()) == 24 and int((d2 == 2 * s2).sum()) == want - 24
        if want == 24:
            assert (apex == -1).all()
        else:
            assert (apex[d2 == 2 * s2] >= 0).all() and int(ax.derive(e, d2, apex, gab, deg, AL.small_cases()[name][0], AL.small_cases()[name][1], 2,
                                                                       AL.small_cases()[name][3])['n_degenerate']) == 18
    e, d2, apex, gab, deg, m, m_gab = references['lattice_3x2']
    assert m == AL.lattice_edges(3, 2, True) == 11


def test_coincident_points_are_a_clique():
    case = AL.coincident(40)
    e, d2, apex, gab, deg, m, m_gab = ax.alpha_reference(*case)
    assert e[:39].tolist() == [[0, k] for k in range(1, 40)] and int((d2 == 0).sum()) == 40 * 39 // 2
    assert (gab[d2 == 0] == 1).all() and (apex[d2 == 0] == -1).all()
    assert m >= 780 > 4 * 45 and 300 * 299 // 2 > ax.first_edge_cap(305)              # the device-sized case needs the second call


def test_chain_closed_form_is_the_reference():
    for order in ('ascending', 'descending', 'shuffled'):
        case = AL.chain(order, 300)
        AL.equal(ax.alpha_reference(*case), AL.chain_expected(case), order)
    for n in (70, 300):                                                          # the crowded closed form: nine sites, every end repeated
        case = AL.crowded(n)
        AL.equal(ax.alpha_reference(*case), AL.crowded_expected(case), f'crowded {n}')


# ---- the neighbours of the family
def _exact_circumradius_le(p, tri, r):
    """Is circumradius^2 <= r^2 (half pixels), exactly: |ab|^2 |bc|^2 |ca|^2 <= 4 r^2 cross^2 in Python integers."""
    a, b, c = (tuple(int(v) for v in p[t]) for t in tri)
    l2 = lambda u, v: (u[0] - v[0]) ** 2 + (u[1] - v[1]) ** 2
    cross = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    return l2(a, b) * l2(b, c) * l2(a, c) <= 4 * r * r * cross * cross


@pytest.mark.parametrize('seed, r', [(5, 512), (6, 60), (7, 25), (8, 150)])
def test_the_identity_with_scipys_delaunay_in_general_position(seed, r):
    """`triangles` equals the simplices with exact circumradius^2 <= r^2, and the edges equal those triangles' sides plus the Gabriel edges
    at most D long."""
    from scipy.spatial import Delaunay
    p = AL.general_position(120, seed)
    lab = np.zeros(len(p), np.int64)
    e, d2, apex, gab, deg, m, m_gab = ax.alpha_reference(p, lab, 1, r, 0)
    d = ax.derive(e, d2, apex, gab, deg, p, lab, 1, r)
    assert int(d['n_degenerate']) == 0                                               # no four points on a circle: scipy's answer is unique
    simplices = Delaunay(p.astype(np.float64)).simplices
    kept = sorted(tuple(sorted(int(v) for v in t)) for t in simplices if _exact_circumradius_le(p, t, r))
    assert [tuple(t) for t in d['triangles'].tolist()] == kept and (r != 512 or len(kept) > len(simplices) - 30) and (r != 25 or 0 < len(kept) < len(simplices) // 2)
    gabriel = px.proximity_reference(p, lab, 1, 2 * r, 0)[0]
    want = {tuple(sorted((t[a], t[b]))) for t in kept for a, b in ((0, 1), (1, 2), (0, 2))} | {tuple(x) for x in gabriel.tolist()}
    assert {tuple(x) for x in e.tolist()} == want and len(want) == m
    assert np.isclose(float(d['alpha_area_px2']), sum(d['triangle_area_px2']), rtol=1e-14) and (d['triangle_circumradius_px'] <= r / 2 * (1 + 1e-14)).all()


@pytest.mark.parametrize('name', ['random_any', 'random_class', 'coarse_any', 'coarse_class', 'out_of_range_class', 'largest'])
def test_gabriel_flagged_edges_are_the_gabriel_graph_and_the_forest_lies_inside(references, name):
    p, lab, C, r, by = AL.small_cases()[name]
    e, d2, apex, gab, deg, m, m_gab = references[name]
    g = px.proximity_reference(p, lab, C, 2 * r, by)
    keep = gab == 1
    assert np.array_equal(e[keep], g[0]) and np.array_equal(d2[keep], g[1]) and np.array_equal(deg[:, 1], g[3][:, 0]) and m_gab == g[4]      # row for row
    forest = {tuple(x) for x in mst.mst_reference(p, lab, C, 2 * r, by)[0].tolist()}
    assert forest <= {tuple(x) for x in e.tolist()} and len(forest) >= 1


def test_int64_and_python_integers_agree_at_the_largest_diameter(references):
    """D = 1024 with witnesses at the largest offsets: m = 2**20 over s = 1024, the products of the compares at their bounds."""
    p, lab, C, r, by = AL.largest()
    e, d2, apex, gab, deg, m, m_gab = references['largest']
    rows = {tuple(x): k for k, x in enumerate(e.tolist())}
    assert apex[rows[(0, 1)]].tolist() == [2, 3] and d2[rows[(0, 1)]] == 1             # t = 1023 and -1023, each attained by two rows: the smaller one
    assert apex[rows[(7, 8)]].tolist() == [9, -1] and gab[rows[(7, 8)]] == 1 and d2[rows[(7, 8)]] == 1 << 20      # (512, 512) ON the circle, (512, -513) outside it
    assert (1023 ** 2) ** 2 * 1 <= 1023 ** 2 * ((1 << 20) - 1) < 1 << 60               # alpha_within_T at row 2: t = 1023 <= T, both sides within int64


# ---- derive
def _rational_derive(p, e, apex, r):
    """voronoi_px, the triangle areas and circumradii from rationals: (Fraction or float) per edge / triangle."""
    D2 = 4 * r * r
    p = [(int(x), int(y)) for x, y in p]
    vor = []
    for (i, j), (a0, a1) in zip(e.tolist(), apex.tolist()):
        q = (p[j][0] - p[i][0], p[j][1] - p[i][1])
        d2 = q[0] ** 2 + q[1] ** 2
        if d2 == 0:
            vor.append(0.0)
            continue
        bound = []
        for k in (a0, a1):
            if k < 0:
                bound.append(None)
                continue
            rho = (p[k][0] - p[i][0], p[k][1] - p[i][1])
            bound.append(Fraction(rho[0] * (rho[0] - q[0]) + rho[1] * (rho[1] - q[1]), q[0] * rho[1] - q[1] * rho[0]))
        T = float(np.sqrt(np.float64(D2 - d2) / np.float64(d2)))
        if bound[0] is not None and bound[1] is not None:
            span = float(bound[0] - bound[1])
        else:
            span = (float(bound[0]) if bound[0] is not None else T) - (float(bound[1]) if bound[1] is not None else -T)
        vor.append(float(np.sqrt(np.float64(d2))) * span / 4)
    return np.asarray(vor)


def test_derive_against_rationals_and_its_refusals():
    p, lab, C, r, by = AL.random_small(0, 6)
    e, d2, apex, gab, deg, m, m_gab = ax.alpha_reference(p, lab, C, r, by)
    d = ax.derive(e, d2, apex, gab, deg, p, lab, C, r)
    assert tuple(d) == ax.DERIVED_KEYS and all(np.isfinite(v).all() for v in d.values())
    assert np.array_equal(d['edge_len_px'], np.sqrt(d2.astype(np.float64)) / 2) and d['edge_len_px'].dtype == np.float64
    # two bounds.  An edge with BOTH apexes has a rational span, hi - lo = one quotient of integers: the rtol = 1e-14 ON THE VALUE of the
    # other derive tests, against the fraction itself.  An edge with an open side ends at the irrational +-T: its span is a rounded
    # difference of a rounded quotient and a rounded root, each of size <= T, so the error is a few ulp of T whatever is left after the
    # subtraction -- held to 1e-14 of the longest Voronoi edge the pair can have, |q| 2 T / 4
    scale = np.sqrt(d2.astype(np.float64)) * np.sqrt(np.maximum(4 * r * r - d2, 0) / np.maximum(d2, 1)) / 4
    want, both = _rational_derive(p, e, apex, r), (apex >= 0).all(1)
    assert both.sum() > 100 and (~both).sum() > 100
    assert np.allclose(d['voronoi_px'][both], want[both], rtol=1e-14, atol=0)
    assert (np.abs(d['voronoi_px'][~both] - want[~both]) <= 1e-14 * 2 * scale[~both]).all()
    assert (d['voronoi_px'] >= 0).all() and (d['voronoi_px'] <= 2 * scale * (1 + 1e-14)).all() and d['voronoi_px'].max() > 1
    assert np.array_equal(d['edge_kind'], (apex >= 0).sum(1)) and d['edge_kind'].dtype == np.uint8 and set(d['edge_kind'].tolist()) == {0, 1, 2}
    tri = {tuple(sorted((i, j, k))) for (i, j), ap in zip(e.tolist(), apex.tolist()) for k in ap if k >= 0}
    assert [tuple(t) for t in d['triangles'].tolist()] == sorted(tri) and d['triangles'].dtype == np.int32 and int(d['n_triangles']) == len(tri) > 20
    P = [(int(x), int(y)) for x, y in p]
    for t, area, radius in zip(d['triangles'].tolist(), d['triangle_area_px2'], d['triangle_circumradius_px']):
        a, b, c = (P[v] for v in t)
        cross = abs((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))
        l2 = lambda u, v: (u[0] - v[0]) ** 2 + (u[1] - v[1]) ** 2
        assert area == cross / 8 and np.isclose(radius, float(Fraction(l2(a, b) * l2(b, c) * l2(a, c), 16 * cross * cross)) ** 0.5, rtol=1e-14)
        assert Fraction(l2(a, b) * l2(b, c) * l2(a, c), 4 * cross * cross) <= r * r
    la, lb = lab[e[:, 0]].astype(np.int64), lab[e[:, 1]].astype(np.int64)
    known = (la >= 0) & (la < C) & (lb >= 0) & (lb < C)
    assert d['class_edge_count'].sum() == known.sum() and not np.tril(d['class_edge_count'], -1).any() and d['class_edge_count'].dtype == np.int64
    assert d['outline_class_count'].sum() == (known & (d['edge_kind'] == 1)).sum() and (d['outline_class_count'] <= d['class_edge_count']).all()
    on = np.zeros(len(p), np.uint8)
    on[e[d['edge_kind'] == 1].reshape(-1)] = 1
    assert np.array_equal(d['on_outline'], on) and d['on_outline'].dtype == np.uint8 and 0 < on.sum() < len(p)
    assert int(d['n_edges']) == m and int(d['n_gabriel']) == m_gab and d['n_edges'].dtype == np.int64 and float(d['alpha_area_px2']) == d['triangle_area_px2'].sum()
    none = ax.derive(np.zeros((0, 2)), [], np.zeros((0, 2)), [], np.zeros((3, 2)), [[0, 0], [50, 0], [0, 50]], [0, 1, 7], 2, 5)
    assert none['triangles'].shape == (0, 3) and none['voronoi_px'].shape == (0,) and float(none['alpha_area_px2']) == 0.0 and not none['on_outline'].any()
    good = dict(edges=e, edge_d2=d2, apex=apex, edge_gabriel=gab, degree=deg, points=p, labels=lab, num_classes=C, r=r)
    for bad in (dict(edge_d2=d2 + 1), dict(degree=deg[::-1].copy()), dict(apex=apex[:, ::-1].copy()), dict(apex=np.full_like(apex, len(p))), dict(edges=e[:-1]),
                dict(r=1)):
        with pytest.raises(ValueError):
            ax.derive(**dict(good, **bad))


def test_npz_round_trip(tmp_path):
    p, lab, C, r, by = AL.random_small(1)
    out = ax.alpha_reference(p, lab, C, r, by)
    ids = np.arange(len(p)) * 3 + 1
    path = ax.write_npz(str(tmp_path / 'a_nuclei_alpha.npz'), ids, p / 2.0, lab, *out[:5], C, r / 2, by)
    z = ax.read_npz(path)
    assert tuple(z) == ax.NPZ_KEYS
    assert np.array_equal(z['nuclei_id'], ids) and np.array_equal(z['xy'], p / 2.0) and np.array_equal(z['label'], lab) and z['label'].dtype == np.int64
    for name, want in zip(ax.INT_NAMES, out[:5]):
        assert np.array_equal(z[name], want) and z[name].dtype == want.dtype
    d = ax.derive(*out[:5], p, lab, C, r)
    for key in ax.DERIVED_KEYS:
        assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype and z[key].shape == d[key].shape, key
    assert float(z['radius_px']) == r / 2 and int(z['by_class']) == 1 and int(z['n_edges']) == out[5] and int(z['n_gabriel']) == out[6]
    bad = str(tmp_path / 'b.npz')
    with pytest.raises(ValueError):
        ax.write_npz(bad, ids, p / 2.0, lab, out[0][:, ::-1], *out[1:5], C, r / 2, by)       # (j, i)
    with pytest.raises(ValueError):
        ax.write_npz(bad, ids, p / 2.0, lab, *out[:4], out[4][:-1], C, r / 2, by)
    with pytest.raises(ValueError):
        ax.write_npz(bad, ids, p / 2.0, lab, *out[:5], C, 0.25, by)
    with pytest.raises(ValueError):
        ax.write_npz(bad, ids, p / 2.0 + 1, lab, out[0], out[1] + 1, *out[2:5], C, r / 2, by)     # d2 is not the distance of the file's own xy
    assert not os.path.exists(bad)


@pytest.mark.parametrize('C, r, by', [(0, 5, 0), (15, 5, 0), (3, 0, 0), (3, 513, 0), (3, 5, 2), (3, 5, -1), (3, 2.5, 0)])
def test_check_args_refuses(C, r, by):
    with pytest.raises(ValueError):
        ax.check_args(C, r, by)
    with pytest.raises(ValueError):
        ax.alpha_reference([[0, 0], [3, 4]], [0, 0], C, r, by)


def test_check_args_accepts_the_limits_and_the_reference_checks_its_points():
    ax.check_args(1, 1, 0); ax.check_args(14, 512, 1)
    with pytest.raises(ValueError):
        ax.alpha_reference([[0, 0], [1 << 27, 0]], [0, 0], 1, 5, 0)
    with pytest.raises(ValueError):
        ax.alpha_reference([[0, 0], [3, 4]], [0], 1, 5, 0)
    assert ax.BY == {'any': 0, 'class': 1} and ax.NPZ_KEYS == ('nuclei_id', 'xy', 'label') + ax.INT_NAMES + ax.DERIVED_KEYS + ('radius_px', 'by_class')
    assert ax.first_edge_cap(10) == 104 and ax.MAX_R == 512


# ---- the row of the table
@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('infer_wsi_for_alpha', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(tool, *flags):
    return tool.parse_args(['slide.npy', 'config.py', 'weights.pth', *flags])


def test_the_table_has_a_sixth_tuple_directly_behind_the_borders(tool, monkeypatch):
    (row,) = slidepoints.OF_THE_CIRCLES
    assert (row.cli, row.flag, row.suffix, row.module, row.second) == ('nuclei_alpha', '--nuclei-alpha', '_nuclei_alpha.npz', 'alphacomplex', None)
    assert row._fields == slidepoints.ANALYSES[0]._fields
    assert (len(slidepoints.ANALYSES), len(slidepoints.OF_THE_PLANE), len(slidepoints.OF_THE_BORDERS), len(slidepoints.AGAINST_CHANCE), len(slidepoints.WITH_INPUT)) == (6, 1, 1, 1, 2)
    plain = _args(tool)
    assert plain.nuclei_alpha is False and (plain.alpha_radius, plain.alpha_by) == (32.0, 'any')
    with pytest.raises(SystemExit):
        _args(tool, '--alpha-by', 'label')
    flags = ['--nuclei-enrichment', '--nuclei-alpha', '--alpha-radius', '12.5', '--alpha-by', 'class', '--nuclei-adjacency', '--nuclei-territory', '--nuclei-density',
             '--nuclei-graph']
    chosen = slidepoints.select(_args(tool, *flags), need_gpu=False)
    assert [an.module for an, _ in chosen] == ['cellgraph', 'density', 'territory', 'adjacency', 'alphacomplex', 'enrichment']
    assert dict((an.module, p) for an, p in chosen)['alphacomplex'] == (12.5, 1)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for bad in (['--alpha-radius', '0'], ['--alpha-radius', '0.25'], ['--alpha-radius', '257']):
        with pytest.raises(SystemExit) as refused:
            slidepoints.select(_args(tool, '--nuclei-alpha', *bad))
        assert str(refused.value).startswith('--nuclei-alpha: ') and 'no GPU' not in str(refused.value), str(refused.value)
    with pytest.raises(SystemExit) as good:
        slidepoints.select(_args(tool, '--nuclei-alpha'))
    assert str(good.value) == '--nuclei-alpha: no GPU is visible (there is no fallback)'
    with pytest.raises(SystemExit) as good:
        slidepoints.select(_args(tool, '--nuclei-alpha', '--alpha-radius', '256'))           # the largest radius passes the check
    assert str(good.value) == '--nuclei-alpha: no GPU is visible (there is no fallback)'


def test_the_closing_clause():
    (row,) = slidepoints.OF_THE_CIRCLES
    found = ax.alpha_reference(*AL.right_triangle(5))
    said = row.said(ax, found, (2.5, 0))
    assert said == '3 alpha-complex edges, 3 of them Gabriel edges, 3 on the outline (2.5 px radius, by any)', said
