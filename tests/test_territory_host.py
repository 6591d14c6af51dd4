"""Host-only checks of the nucleus territories (nuhtc_amd/territory.py): `territory_reference` against an independent double loop in plain
Python integers and against hand-written rasters, the tie rule, the inclusive reach, the closed forms of points placed on sites, scipy's
cKDTree wherever the nearest point is unique, `derive`, `window` / `check_args`, the .npz round trip, and the row of the table in
nuhtc_amd/slidepoints.py.  The device is compared with `territory_reference` in tests/test_hip_territory.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import territory_cases as TC
from nuhtc_amd import cellpoints, slidepoints
from nuhtc_amd import territory as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def double_loop(p, lab, C, r, s, win):
    """The definition word for word: Python integers, every site against every row, then every site against its four neighbours."""
    gx0, gy0, W, H = win
    n = len(p)
    owner, nearest = [[-1] * W for _ in range(H)], [[-1] * W for _ in range(H)]
    for v in range(H):
        for u in range(W):
            qx, qy, best = (gx0 + u) * s, (gy0 + v) * s, None
            for i, ((x, y), c) in enumerate(zip(p.tolist(), lab.tolist())):
                d2 = (qx - x) ** 2 + (qy - y) ** 2
                if 0 <= c < C and d2 <= r * r and (best is None or (d2, i) < best):
                    best = (d2, i)
            if best is not None:
                nearest[v][u], owner[v][u] = best
    area, border, is_open = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    contact, class_sites, free = np.zeros((C, C), np.int64), np.zeros(C, np.int64), 0
    for v in range(H):
        for u in range(W):
            i = owner[v][u]
            if i < 0:
                free += 1
                continue
            around = [owner[b][a] for a, b in ((u - 1, v), (u + 1, v), (u, v - 1), (u, v + 1)) if 0 <= a < W and 0 <= b < H]
            area[i] += 1
            class_sites[lab[i]] += 1
            border[i] += any(j != i for j in around)
            if u in (0, W - 1) or v in (0, H - 1) or any(j < 0 for j in around):
                is_open[i] = 1
            for j in around:
                if j >= 0 and j != i:
                    contact[lab[i], lab[j]] += 1
    return (np.array(owner, np.int32).reshape(H, W), np.array(nearest, np.int32).reshape(H, W), area, border, is_open, contact, class_sites,
            np.asarray(free, np.int64))


@pytest.mark.parametrize('name', ['patch', 'mirrored', 'labels', 'sparse', 'ties', 'bisector'])
def test_reference_equals_the_double_loop(name):
    case = dict(patch=TC.patch(), mirrored=TC.mirror(TC.patch()), labels=TC.labels_out_of_range(), sparse=TC.pitch_cases()['sparse'],
                ties=TC.ties(0, 60, extent=8), bisector=TC.bisector())[name]
    win = TC.default_window(case)
    assert win[2] * win[3] < 3000 and len(case[0]) <= 200
    got = tr.territory_reference(*case, win, block=97)
    TC.equal(got, double_loop(*case, win), name)
    assert int(got[6].sum()) + int(got[7]) == win[2] * win[3] and np.array_equal(got[5], got[5].T)
    if name != 'bisector':
        sub = (win[0] + 2, win[1] + 1, win[2] - 5, win[3] - 3)                # the owner is a slice, the tallies are the sub-window's own
        part = tr.territory_reference(*case, sub)
        assert np.array_equal(part[0], got[0][1:win[3] - 2, 2:win[2] - 3]) and np.array_equal(part[1], got[1][1:win[3] - 2, 2:win[2] - 3])
        TC.equal(part, double_loop(*case, sub), name + ', sub-window')


def test_hand_written_rasters():
    for h, s, at in ((9, 4, (5, -3)), (10, 5, (-2, 0)), (3, 1, (0, 0))):
        win, count, weight = TC.single_point_expected(h, s, at)               # density's raster of one point: who is in reach, and h * h - d2
        got = tr.territory_reference(*TC.single_point(h, s, at), win)
        assert np.array_equal(got[0], count[0] - 1) and np.array_equal(got[1], np.where(count[0] == 1, h * h - weight[0], -1))
        k = h // s
        assert got[0][k, k] == 0 and got[1][k, k] == 0 and got[1][k, k + 1] == s * s and got[0].dtype == got[1].dtype == np.int32
        assert got[2].tolist() == [int(count.sum())] and got[4].tolist() == [1] and got[5].tolist() == [[0]] and got[6].tolist() == [int(count.sum())]
        assert int(got[7]) == count.size - int(count.sum()) and got[3].tolist() == [int(got[2][0]) - _inner(count[0])]
    # three points on a row of nine sites, by hand: R = 3 leaves the site between 0 and 1 to the left one (a tie) and a gap before the third
    got = tr.territory_reference([[2, 0], [6, 0], [14, 0]], [0, 1, 5], 2, 3, 2, (0, 0, 9, 1))
    assert got[0].tolist() == [[0, 0, 0, 1, 1, -1, -1, -1, -1]] and got[1].tolist() == [[4, 0, 4, 0, 4, -1, -1, -1, -1]]       # label 5 owns nothing
    assert got[2].tolist() == [3, 2, 0] and got[3].tolist() == [1, 2, 0] and got[4].tolist() == [1, 1, 0]
    assert got[5].tolist() == [[0, 1], [1, 0]] and got[6].tolist() == [3, 2] and int(got[7]) == 4


def _inner(mask):
    """The sites of a 0 / 1 raster that are 1 with every neighbour they have inside the raster."""
    m = np.pad(mask.astype(bool), 1, constant_values=True)
    return int((m[1:-1, 1:-1] & m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]).sum())


def test_a_tie_goes_to_the_smaller_row():
    for swapped in (False, True):
        case = TC.bisector(swapped)
        win = TC.default_window(case)
        owner, nearest = tr.territory_reference(*case, win)[:2]
        col = 1 - win[0]                                                      # the sites with x = 4
        left = int(np.flatnonzero((case[0] == [0, 0]).all(1))[0])
        assert (owner[:, col][nearest[:, col] >= 0] == 0).all() and (nearest[:, col] >= 0).sum() >= 3
        assert owner[-win[1], col - 1] == left and owner[-win[1], col + 1] == 1 - left          # beside the bisector: the nearer point
        assert nearest[-win[1], col] == 16


def test_the_reach_is_inclusive():
    case = TC.three_four_five()
    owner, nearest = tr.territory_reference(*case, (-5, -5, 11, 11))[:2]
    assert owner[4 + 5, 3 + 5] == 0 and nearest[4 + 5, 3 + 5] == 25           # offset (3, 4): exactly R away
    assert owner[5 + 5, 3 + 5] == -1 and nearest[5 + 5, 3 + 5] == -1          # one half-pixel step farther: 34 > 25
    assert owner[5, 10] == 0 and owner[5, 0] == 0 and (owner >= 0).sum() == 81


@pytest.mark.parametrize('k, s, m, classes', [(3, 2, 5, 2), (5, 1, 4, 2), (3, 7, 4, 1), (1, 4, 6, 2)])
def test_points_on_sites_have_k_by_k_territories(k, s, m, classes):
    case = TC.on_sites(k, s, m, classes)
    win = TC.on_sites_window(k, m)
    owner, nearest, area, border, is_open, contact, class_sites, free = tr.territory_reference(*case, win)
    y, x = np.divmod(np.arange(m * m), m)
    rim = (x == 0) | (x == m - 1) | (y == 0) | (y == m - 1)
    assert int(free) == 0 and (area[~rim] == k * k).all() and not is_open[~rim].any() and is_open[rim].all()
    assert (border[~rim] == (k * k - (k - 2) ** 2 if k > 1 else 1)).all()
    # every one of the (m - 1) bisectors each way crosses all (m - 1) k + 1 rows (or columns) of the window: two ordered pairs per crossing
    crossings = 2 * (m - 1) * ((m - 1) * k + 1)
    want = [[0, crossings], [crossings, 0]] if classes == 2 else [[2 * crossings]]
    assert contact.tolist() == want and int(class_sites.sum()) == win[2] * win[3]
    full = tr.territory_reference(*case, TC.default_window(case))              # with the reach around it: the same interior, the rim still open
    assert (full[2][~rim] == k * k).all() and not full[4][~rim].any() and full[4][rim].all() and int(full[7]) > 0


@pytest.mark.parametrize('kind', ['uniform', 'clumps'])
def test_agrees_with_ckdtree_where_the_nearest_is_unique(kind):
    from scipy.spatial import cKDTree
    p, lab = TC.random_large(kind, 500)
    lab = np.abs(lab) % 5                                                      # every row competes: the tree knows no labels
    r, s = 30, 7
    win = tr.window(cellpoints.bounds_of(p), r, s)
    owner, nearest = tr.territory_reference(p, lab, 5, r, s, win)[:2]
    v, u = np.divmod(np.arange(win[2] * win[3]), win[2])
    q = np.stack([(win[0] + u) * s, (win[1] + v) * s], 1)
    _, idx = cKDTree(p.astype(np.float64)).query(q.astype(np.float64), k=2, distance_upper_bound=r + 0.5)
    d2 = np.full((len(q), 2), -1, np.int64)
    for j in range(2):
        found = idx[:, j] < len(p)
        d2[found, j] = ((q[found] - p[idx[found, j]].astype(np.int64)) ** 2).sum(1)
    d2[d2 > r * r] = -1
    unique = (d2[:, 0] != d2[:, 1]) | (d2[:, 0] < 0)                           # integers: the two nearest differ, or at most one is in reach
    want = np.where(d2[:, 0] >= 0, idx[:, 0], -1)
    assert unique.sum() > 0.9 * len(q) and (want[unique] >= 0).sum() > 1000
    assert np.array_equal(owner.reshape(-1)[unique], want[unique]) and np.array_equal(nearest.reshape(-1)[unique], d2[unique, 0])


def test_derive_properties():
    p, lab = TC.random_large('clumps', 400)
    r, s = 30, 5
    win = tr.window(cellpoints.bounds_of(p), r, s)
    out = tr.territory_reference(p, lab, 5, r, s, win)
    d = tr.derive(out[2], out[4], out[5], out[6], out[7], lab, s)
    assert tuple(d) == tr.DERIVED_KEYS and all(np.isfinite(v).all() for v in d.values())
    assert np.array_equal(d['area_px2'], out[2] * 6.25) and d['area_px2'].dtype == np.float64
    assert np.array_equal(d['closed'], ((out[4] == 0) & (out[2] > 0)).astype(np.uint8)) and d['closed'].sum() > 20
    assert abs(d['class_area_share'].sum() - 1) < 1e-12 and abs(d['contact_share'].sum() - 1) < 1e-12
    assert np.array_equal(d['contact_share'], d['contact_share'].T) and 0 < float(d['free_share']) < 1
    assert abs(float(d['free_share']) - int(out[7]) / (win[2] * win[3])) < 1e-15
    for c in range(5):
        a = d['area_px2'][(d['closed'] == 1) & (lab == c)]
        assert d['n_closed'][c] == len(a) and np.isclose(d['closed_area_mean_px2'][c], a.mean(), rtol=1e-14) and np.isclose(d['closed_area_std_px2'][c], a.std(), rtol=1e-12)
        assert np.isclose(d['area_disorder'][c], 1 - 1 / (1 + a.std() / a.mean()), rtol=1e-12) and 0 <= d['area_disorder'][c] < 1
    assert d['n_closed'].dtype == np.int64 and d['closed'].dtype == np.uint8
    empty = tr.derive(np.zeros(0), np.zeros(0), np.zeros((3, 3)), np.zeros(3), 12, np.zeros(0), 4)
    assert all(np.isfinite(v).all() for v in empty.values()) and float(empty['free_share']) == 1.0 and not empty['contact_share'].any()
    assert not empty['class_area_share'].any() and not empty['n_closed'].any() and not empty['area_disorder'].any()
    nothing = tr.derive(np.zeros(4), np.zeros(4), np.zeros((2, 2)), np.zeros(2), 9, [0, 1, 0, 7], 4)          # points, and no site in reach
    assert all(np.isfinite(v).all() for v in nothing.values()) and not nothing['closed'].any()
    with pytest.raises(ValueError):
        tr.derive(np.zeros(3), np.zeros(2), np.zeros((2, 2)), np.zeros(2), 0, np.zeros(3), 4)


def test_no_points_window_and_refused_arguments():
    out = tr.territory_reference(np.zeros((0, 2)), [], 2, 5, 3, (4, -4, 3, 2))
    assert out[0].shape == (2, 3) and (out[0] == -1).all() and (out[1] == -1).all() and out[2].shape == (0,) and not out[5].any() and int(out[7]) == 6
    assert tr.window((-10, -10, -10, -10), 3, 4) == (-3, -3, 2, 2) and tr.window((0, 0, 0, 0), 3, 4) == (0, 0, 1, 1)
    for C, r, s in ((0, 5, 3), (15, 5, 3), (3, 0, 3), (3, 16385, 3), (3, 5, 0), (3, 5, (1 << 20) + 1), (3, 5.5, 3)):
        with pytest.raises(ValueError):
            tr.check_args(C, r, s)
    tr.check_args(14, 16384, 1 << 20)
    for win in ((0, 0, 0, 1), (0, 0, 1, 0), (0, 0, (1 << 28) + 1, 1), (0, 0, 1 << 14, (1 << 14) + 1), (1 << 26, 0, 1, 1), (0, -(1 << 26), 1, 1),
                ((1 << 26) - 4, 0, 5, 1), (0, 0, 1)):
        with pytest.raises(ValueError):
            tr.check_args(3, 5, 4, win)
    with pytest.raises(ValueError, match='coarsen the pitch'):
        tr.check_args(3, 5, 4, (0, 0, 1 << 14, (1 << 14) + 1))
    tr.check_args(3, 5, 4, (0, 0, 1 << 14, 1 << 14))                          # 2**28 sites: this module's cap, not density's 2**24
    tr.check_args(3, 5, 4, (0, 0, (1 << 24) + 1, 1))
    tr.check_args(3, 5, 4, ((1 << 26) - 4, -(1 << 26) + 1, 4, 1 << 12))
    with pytest.raises(ValueError):
        tr.territory_reference([[1 << 27, 0]], [0], 1, 5, 3, (0, 0, 1, 1))
    with pytest.raises(ValueError):
        tr.territory_reference([[0, 0], [1, 1]], [0], 1, 5, 3, (0, 0, 1, 1))


def test_npz_round_trip_with_and_without_maps(tmp_path):
    p, lab = TC.random_large('uniform', 200)
    r, s = 30, 8
    win = tr.window(cellpoints.bounds_of(p), r, s)
    out = tr.territory_reference(p, lab, 5, r, s, win)
    head = (np.arange(200) * 3, p / 2.0, lab)
    plain = tr.read_npz(tr.write_npz(str(tmp_path / 'a_nuclei_territory.npz'), *head, out[2:], win, r / 2, s / 2))
    kept = tr.read_npz(tr.write_npz(str(tmp_path / 'b_nuclei_territory.npz'), *head, out[2:], win, r / 2, s / 2, maps=out[:2]))
    assert tuple(plain) == tr.NPZ_KEYS and tuple(kept) == tr.NPZ_KEYS + tr.MAP_NAMES
    for name, want in zip(TC.NAMES, out):
        if name in kept and (name in plain or name in tr.MAP_NAMES):
            assert np.array_equal(kept[name], want) and kept[name].dtype == want.dtype and kept[name].shape == want.shape, name
    for key in tr.NPZ_KEYS:
        assert np.array_equal(plain[key], kept[key]) and plain[key].dtype == kept[key].dtype, key
    assert plain['open'].dtype == np.uint8 and plain['free_sites'].shape == () and plain['contact'].dtype == np.int64
    assert float(plain['reach_px']) == 15.0 and float(plain['pitch_px']) == 4.0 and plain['window'].tolist() == list(win)
    assert plain['origin_px'].tolist() == [win[0] * 4.0, win[1] * 4.0] and np.array_equal(plain['nuclei_id'], np.arange(200) * 3)
    d = tr.derive(out[2], out[4], out[5], out[6], out[7], lab, s)
    for key in tr.DERIVED_KEYS:
        assert np.array_equal(plain[key], d[key]) and plain[key].dtype == d[key].dtype, key
    with pytest.raises(ValueError):
        tr.write_npz(str(tmp_path / 'c.npz'), *head, out[2:], (win[0], win[1], win[2] + 1, win[3]), r / 2, s / 2)
    with pytest.raises(ValueError):
        tr.write_npz(str(tmp_path / 'c.npz'), *head, out[2:], win, r / 2, s / 2, maps=(out[0][:-1], out[1][:-1]))
    with pytest.raises(ValueError):
        tr.write_npz(str(tmp_path / 'c.npz'), *head, (out[2][:-1],) + tuple(out[3:]), win, r / 2, s / 2)


# ---- the row of the table
@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('infer_wsi_for_territory', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(tool, *flags):
    return tool.parse_args(['slide.npy', 'config.py', 'weights.pth', *flags])


def test_the_table_has_a_fourth_tuple_directly_after_the_six(tool, monkeypatch):
    assert len(slidepoints.ANALYSES) == 6 and len(slidepoints.AGAINST_CHANCE) == 1 and len(slidepoints.WITH_INPUT) == 2
    assert [a.module for a in slidepoints.AGAINST_CHANCE + slidepoints.WITH_INPUT] == ['enrichment', 'regions', 'margin']
    (row,) = slidepoints.OF_THE_PLANE
    assert (row.cli, row.flag, row.suffix, row.module, row.second) == ('nuclei_territory', '--nuclei-territory', '_nuclei_territory.npz', 'territory', None)
    assert row._fields == slidepoints.ANALYSES[0]._fields
    plain = _args(tool)
    assert plain.nuclei_territory is False and (plain.territory_reach, plain.territory_pitch, plain.territory_maps) == (64.0, 4.0, False)
    flags = ['--nuclei-enrichment', '--nuclei-territory', '--territory-maps', '--territory-pitch', '2.5', '--nuclei-density', '--nuclei-graph']
    chosen = slidepoints.select(_args(tool, *flags), need_gpu=False)
    assert [an.module for an, _ in chosen] == ['cellgraph', 'density', 'territory', 'enrichment']
    assert dict((an.module, p) for an, p in chosen)['territory'] == (64.0, 2.5, None, True)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for bad in (['--territory-pitch', '0.25'], ['--territory-reach', '9000'], ['--territory-reach', '0']):
        with pytest.raises(SystemExit) as refused:
            slidepoints.select(_args(tool, '--nuclei-territory', *bad))
        assert str(refused.value).startswith('--nuclei-territory: ') and 'no GPU' not in str(refused.value), str(refused.value)
    with pytest.raises(SystemExit) as good:
        slidepoints.select(_args(tool, '--nuclei-territory'))
    assert str(good.value) == '--nuclei-territory: no GPU is visible (there is no fallback)'


def test_the_closing_clause_and_a_late_refusal(monkeypatch, tmp_path):
    (row,) = slidepoints.OF_THE_PLANE
    p, lab = TC.on_sites(3, 2, 5, 2)[:2]
    win = TC.on_sites_window(3, 5)
    out = tr.territory_reference(p, lab, 2, 6, 2, win)
    said = row.said(tr, (out[2:], win, None), (3.0, 1.0, None, False))
    assert said == ('territories of 25 nuclei on 13 x 13 sites (3 px reach, 1 px pitch; 9 closed, median area 9 px^2; largest area share: class 0 '
                    f'with {out[6][0] / 169:.1%} of the owned sites)'), said
    none = tr.territory_reference(np.zeros((0, 2)), [], 2, 6, 2, (0, 0, 1, 1))
    assert 'none' in row.said(tr, (none[2:], (0, 0, 1, 1), None), (3.0, 1.0, None, False))
    # a default window above the cap is refused by build, as late as the slide's own points are known: `run` says so in the flag's name
    def build(*a, **k):
        tr.check_args(2, 128, 1, (0, 0, 1 << 15, 1 << 15))
    monkeypatch.setattr(tr, 'build', build)
    boxes = np.array([[0, 0, 2, 2], [10, 10, 14, 14]], np.float64)
    with pytest.raises(SystemExit) as refused:
        slidepoints.run(((row, (64.0, 0.5, None, False)),), np.arange(2), boxes, np.array([0, 1]), 2, str(tmp_path), 's1', 0, {})
    assert str(refused.value).startswith('--nuclei-territory: ') and 'coarsen the pitch' in str(refused.value)
