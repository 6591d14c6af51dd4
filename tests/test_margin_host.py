"""The margin bands (nuhtc_amd/margin.py) without a GPU: `margin_reference` against a double loop in Python integers, the hand-written
rows, the pair that float64 decides wrongly, `regions_reference` for the census, derive, slots_needed against a direct loop, the argument
refusals, the file round trip and the tool's row in slidepoints."""
import importlib.util
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import margin_cases as MC
from nuhtc_amd import cellpoints, slidepoints
from nuhtc_amd import margin as mg
from nuhtc_amd import regions as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = MC.all_cases()


def near_int(ax, ay, bx, by, px, py, e):
    """near(p, a -> b, e) of the definition, written here again in Python integers."""
    dx, dy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    L2, s = dx * dx + dy * dy, wx * dx + wy * dy
    if L2 == 0 or s <= 0:
        return wx * wx + wy * wy <= e * e
    if s >= L2:
        return (px - bx) ** 2 + (py - by) ** 2 <= e * e
    return (dx * wy - dy * wx) ** 2 <= e * e * L2


def double_loop(p, lab, C, edges, edge_region, G, thresholds):
    """The definition, one point, one edge and one threshold at a time, in Python integers."""
    n, thr, B = len(p), [int(t) for t in thresholds], len(thresholds)
    E, er, lab = [tuple(int(v) for v in e) for e in edges.tolist()], edge_region.tolist(), lab.tolist()
    band_census = np.zeros((G, 2, B, C), np.int64)
    census = np.zeros((G, C), np.int64)
    band, band_region, band_inside = [B] * n, [-1] * n, [0] * n
    for i, (px, py) in enumerate(p.tolist()):
        parity, of = [0] * G, [B] * G
        for (ax, ay, bx, by), g in zip(E, er):
            if (ay <= py) != (by <= py):
                lx, ly, hx, hy = (ax, ay, bx, by) if ay < by else (bx, by, ax, ay)
                parity[g] ^= (hx - lx) * (py - ly) - (hy - ly) * (px - lx) > 0
            of[g] = min(of[g], next((t for t in range(B) if near_int(ax, ay, bx, by, px, py, thr[t])), B))
        for g in range(G):
            known = 0 <= lab[i] < C
            if of[g] < B and known:
                band_census[g, int(parity[g]), of[g], lab[i]] += 1
            if parity[g] and known:
                census[g, lab[i]] += 1
            if of[g] < band[i]:
                band[i], band_region[i], band_inside[i] = of[g], g, int(parity[g])
    return band_census, census, np.asarray(band, np.int32), np.asarray(band_region, np.int32), np.asarray(band_inside, np.uint8)


def _equal(got, want, what):
    for name, g, w in zip(mg.INT_NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:3].tolist())


SMALL = ('regimes', 'float64_pair', 'shared_edge', 'around_the_box', 'empty_slab', 'pythagorean_5', 'pythagorean_169', 'no_points', 'no_regions', 'neither',
         'regions_without_edges')


@pytest.mark.parametrize('name', SMALL)
def test_reference_equals_the_double_loop(name):
    _equal(mg.margin_reference(*CASES[name]), double_loop(*CASES[name]), name)


def test_reference_equals_the_double_loop_on_sampled_rows_of_the_large_sets():
    for name in ('holes_and_nested', 'staging', 'random_lattice_1', 'random_lattice_2'):
        case = CASES[name]
        pick = np.random.default_rng(1).choice(len(case[0]), 60, replace=False)
        full = mg.margin_reference(*case)
        loop = double_loop(case[0][pick], case[1][pick], *case[2:])
        for k in (2, 3, 4):
            assert np.array_equal(full[k][pick], loop[k]), (name, mg.INT_NAMES[k])
        _equal(mg.margin_reference(case[0][pick], case[1][pick], *case[2:], block=7), loop, name)


def test_rows_by_hand():
    case = MC.regimes()
    bc, census, band, band_region, band_inside = mg.margin_reference(*case)
    at = {tuple(p): i for i, p in enumerate(case[0].tolist())}
    for p, want in MC.REGIME_ROWS:
        assert band[at[p]] == want and band_region[at[p]] == (0 if want < 4 else -1) and band_inside[at[p]] == 0, (p, int(band[at[p]]), want)
    assert band[at[(40, 40)]] == 0 and band_region[at[(40, 40)]] == 1 and band[at[(43, 44)]] == 3 and band[at[(43, 45)]] == 4
    for p, (want, side) in MC.REGIME_SQUARE.items():
        assert band[at[p]] == want and band_inside[at[p]] == (side if want < 4 else 0) and band_region[at[p]] == (2 if want < 4 else -1), p
    lab = case[1]
    for g, rows in ((0, [p for p, w in MC.REGIME_ROWS]), (2, list(MC.REGIME_SQUARE))):
        hand = np.zeros((2, 4, 2), np.int64)
        for p in rows:
            want, side = (dict(MC.REGIME_ROWS)[p], 0) if g == 0 else MC.REGIME_SQUARE[p]
            if want < 4:
                hand[side, want, lab[at[p]]] += 1
        assert np.array_equal(bc[g], hand), g
    assert census[2].sum() == 4 and not census[:2].any()                                            # three min-side points and the centre
    for triple in MC.TRIPLES:
        case, want = MC.pythagorean(triple)
        got = mg.margin_reference(*case)
        assert np.array_equal(got[2], want) and got[2].dtype == want.dtype, triple
        assert (got[3] == np.where(want < 32, 0, -1)).all() and not got[4].any() and not got[1].any()


def test_the_pair_float64_decides_wrongly():
    (a, b), p, e = MC.F64_EDGE, MC.F64_POINT, MC.F64_E
    assert mg.near(*a, *b, *p, e) and near_int(*a, *b, *p, e)
    assert not mg.near(*a, *b, p[0] - 1, p[1], e) and not mg.near(*a, *b, *p, e - 1)                # one step farther out; one threshold lower
    d = np.asarray(b, np.float64) - a
    t = np.clip(np.dot(np.asarray(p, np.float64) - a, d) / np.dot(d, d), 0, 1)
    q = np.asarray(a, np.float64) + t * d
    assert not math.hypot(p[0] - q[0], p[1] - q[1]) <= e                                            # the usual float64 restatement says "not within"
    assert mg.margin_reference(*MC.float64_pair())[2].tolist() == [1, 2, 1]


def test_census_is_the_region_census():
    for name, case in CASES.items():
        got = mg.margin_reference(*case)
        want = rg.regions_reference(*case[:6])
        assert np.array_equal(got[1], want[3]) and got[1].dtype == want[3].dtype, name
        assert (got[0][:, 1].sum(1) <= got[1]).all(), name                                         # the inside bands hold no more than the region
    case = CASES['shared_edge']
    bc, census, band, band_region, band_inside = mg.margin_reference(*case)
    on = np.flatnonzero((case[0][:, 0] == 12) & (case[0][:, 1] >= 0) & (case[0][:, 1] < 8))            # (12, 8) is on the max-y side: in neither
    assert len(on) == 8 and (band[on] == 0).all() and (band_region[on] == 0).all()
    per = [mg.margin_reference(case[0][on], case[1][on], 1, case[3][case[4] == g], np.zeros(4, np.int32), 1, case[6]) for g in (0, 1)]
    assert all((q[2] == 0).all() for q in per) and (per[0][4].astype(int) + per[1][4] == 1).all()   # band 0 of both, inside exactly one


def test_derive():
    for name in ('holes_and_nested', 'staging', 'random_lattice_1', 'around_the_box', 'no_regions'):
        case = CASES[name]
        bc, census = mg.margin_reference(*case)[:2]
        d = mg.derive(bc, census, case[6])
        G, B, C = len(bc), len(case[6]), case[2]
        assert tuple(d) == mg.DERIVED_KEYS and d['profile'].shape == (G, 2 * B, C) and d['class_fraction'].shape == (G, 2, B, C)
        assert np.array_equal(d['profile'][:, :B].sum(1) + d['inside_beyond'], census), name        # the inside half and what lies beyond it
        assert np.array_equal(d['profile'][:, B - 1], bc[:, 1, 0]) and np.array_equal(d['profile'][:, B], bc[:, 0, 0]) and np.array_equal(d['profile'][:, 0], bc[:, 1, B - 1])
        assert np.array_equal(d['profile'][:, 2 * B - 1], bc[:, 0, B - 1]) and np.array_equal(d['n_near'], bc.sum((1, 2, 3)))
        assert not np.isnan(d['class_fraction']).any() and d['class_fraction'].dtype == np.float64
        total = bc.sum(3)
        assert np.allclose(d['class_fraction'].sum(3), total > 0) and (d['class_fraction'][total == 0] == 0).all()
        assert d['band_edges_px'].tolist() == [0.0] + [t / 2 for t in case[6].tolist()]
    assert not mg.margin_reference(*CASES['around_the_box'])[0][4:8].any()                          # whole regions of empty bands were met
    with pytest.raises(ValueError):
        mg.derive(np.ones((1, 2, 2, 1), np.int64), np.zeros((1, 1), np.int64), (1, 2))              # more in the inside bands than inside
    with pytest.raises(ValueError):
        mg.derive(np.zeros((1, 2, 3, 1), np.int64), np.zeros((1, 1), np.int64), (1, 2))


def _slots_loop(edges, bounds, slab, R):
    x_min, y_min, x_max, y_max = bounds
    side = cellpoints.cell_side(x_min, y_min, x_max, y_max, slab, mg.MAX_CELLS)
    total = 0
    for ax, ay, bx, by in edges.tolist():
        if ax < x_min - R and bx < x_min - R:
            continue
        for s in range((y_max - y_min) // side + 1):
            r0, r1 = y_min + s * side, min(y_min + (s + 1) * side - 1, y_max)
            total += max(ay, by) + R >= r0 and min(ay, by) - R <= r1
    return total


def test_the_slab_walk_case_is_laid_out_as_it_says():
    case = MC.slab_walk()
    p, lab, C, edges, er, G, thr = case
    points, records = MC.RC.slab_layout(case, MC.SLAB_WALK_SLAB, int(thr[-1]))
    assert points == [100, 60, 140] and [len(r) for r in records] == [4, 0, 256 + 256 + 8]       # as in the census: no grown range reaches slab 1
    assert records[2] == [0] * 256 + [1] * 260 + [2] * 4 and mg.slots_needed(edges, (0, 0, 1000, 599), MC.SLAB_WALK_SLAB, thr) == 524
    bc, census, band, band_region, band_inside = mg.margin_reference(*case)
    assert set(band.tolist()) == {0, 1, 2, 3} and set(band_inside.tolist()) == {0, 1} and set(band_region.tolist()) == {-1, 0, 1}
    assert bc[:2].sum(axis=(0, 3)).all() and not bc[2].any() and not census[2].any()              # every band on both sides; region 2 is never near
    assert np.array_equal(census, rg.regions_reference(*case[:6])[3])


def test_slots_needed_and_choose_slab():
    for name in ('around_the_box', 'empty_slab', 'staging', 'regimes'):
        case = CASES[name]
        bounds = cellpoints.bounds_of(case[0])
        for slab in (1, 7, 16384):
            assert mg.slots_needed(case[3], bounds, slab, case[6]) == _slots_loop(case[3], bounds, slab, int(case[6][-1])), (name, slab)
    e = np.array([[0, -5, 0, 25], [3, 3, 9, 3], [-4, 0, -1, 20], [-9, 0, -8, 20], [50, 9, 40, 10], [0, 23, 5, 30], [0, 24, 5, 30]], np.int64)
    # box (0, 0) .. (10, 20), slab 5, R 3: rows 0-4, .., 15-19, 20.  The first edge meets all five; the second (y 3 grown to 0 .. 6) two; the
    # third lies left of the box but within R of it: five; the fourth lies left of x_min - R; the fifth (y 6 .. 13) rows 1 and 2; the
    # sixth (y 20 .. 33) row 4; the last (21 ..) misses the box
    assert mg.slots_needed(e, (0, 0, 10, 20), 5, (1, 3)) == 5 + 2 + 5 + 0 + 2 + 1 + 0
    assert mg.slots_needed(e[:0], (0, 0, 10, 20), 5, (3,)) == 0
    assert mg.choose_slab((0, 0, 10, 20), (5, 9)) == 9 and mg.choose_slab((0, 0, 0, 2047 * 40), (5, 9)) == 40 and mg.choose_slab((0, 0, 9, 9), (16384,)) == 16384


def test_argument_refusals():
    mg.check_args(1), mg.check_args(14, 1 << 16, 1 << 22, 16384, np.arange(1, 33) * 512)
    for bad in ((), (0,), (1, 1), (2, 1), (1, 16385), np.arange(1, 34), (1.5, 2), (-3, 2)):
        with pytest.raises(ValueError):
            mg.as_thresholds(bad)
        with pytest.raises(ValueError):
            mg.check_args(1, 0, 0, 1, bad)
    for bad in ((0,), (15,), (1, (1 << 16) + 1), (1, 1, (1 << 22) + 1), (1, 1, 1, 0)):
        with pytest.raises(ValueError):
            mg.check_args(*bad)
    assert mg.as_thresholds([2, 5.0, 9]).dtype == np.int32 and mg.thresholds_from_step(50, 10).tolist() == list(range(100, 1001, 100))
    assert mg.thresholds_from_step(256, 32)[-1] == 16384 and mg.thresholds_from_step(0.5, 1).tolist() == [1]
    for step, bands in ((50, 0), (50, 33), (0.25, 4), (0, 4), (256.5, 32), (1000, 10)):
        with pytest.raises(ValueError):
            mg.thresholds_from_step(step, bands)
    p, lab, C, edges, er, G, thr = CASES['regimes']
    for bad in ((p, lab, C, edges, er[::-1], G, thr), (p, lab, C, edges + (1 << 27), er, G, thr), (p + (1 << 27), lab, C, edges, er, G, thr), (p, lab[:-1], C, edges, er, G, thr),
                (p, lab, C, edges, er, G, thr[::-1]), (p, lab, 15, edges, er, G, thr)):
        with pytest.raises(ValueError):
            mg.margin_reference(*bad)


def _write(tmp_path, doc, name='r.geojson'):
    path = tmp_path / name
    path.write_text(json.dumps(doc))
    return str(path)


def test_file_round_trip(tmp_path):
    import regions_cases as RC
    case = RC.overlap()
    t = rg.read_geojson(_write(tmp_path, RC.overlap_features()))
    thr = (2, 4, 7)
    found = mg.margin_reference(case[0], case[1], 3, t.edges, t.edge_region, 4, thr)
    n = len(case[0])
    path = mg.write_npz(str(tmp_path / 's_nuclei_margin.npz'), np.arange(n), case[0] / 2, case[1], *found, thr, t)
    z = mg.read_npz(path)
    assert tuple(z) == mg.NPZ_KEYS and z['names'].tolist() == ['small', 'other', 'mid', 'big'] and z['thresholds'].tolist() == [2, 4, 7]
    for name, want in zip(mg.INT_NAMES, found):
        assert np.array_equal(z[name], want) and z[name].dtype == want.dtype
    d = mg.derive(found[0], found[1], thr)
    for key in mg.DERIVED_KEYS:
        assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype, key
    assert np.array_equal(z['edges'], t.edges) and np.array_equal(z['edge_region'], t.edge_region) and np.array_equal(z['area2'], t.area2)
    with np.load(path, allow_pickle=False) as plain:                                                # nothing pickled
        assert set(plain.files) == set(mg.NPZ_KEYS)
    with pytest.raises(ValueError):
        mg.write_npz(str(tmp_path / 'bad.npz'), np.arange(n), case[0] / 2, case[1], *found[:2], found[2][:-1], *found[3:], thr, t)


# ---- the tool's argument checks
@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('infer_wsi_for_margin', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(tool, *flags):
    return tool.parse_args(['slide.npy', 'config.py', 'weights.pth', *flags])


def test_a_bad_path_or_step_is_named_before_the_missing_gpu(tool, monkeypatch, tmp_path):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SystemExit) as bad:
        slidepoints.select(_args(tool, '--nuclei-margin', str(tmp_path / 'nowhere.geojson')))
    assert str(bad.value).startswith('--nuclei-margin: ') and 'no GPU' not in str(bad.value) and 'nowhere.geojson' in str(bad.value)
    path = _write(tmp_path, [])
    for flags in (('--margin-step', '0.25'), ('--margin-bands', '33'), ('--margin-step', '1000', '--margin-bands', '10')):
        with pytest.raises(SystemExit) as bad:
            slidepoints.select(_args(tool, '--nuclei-margin', path, *flags))
        assert str(bad.value).startswith('--nuclei-margin: ') and 'no GPU' not in str(bad.value), flags
    with pytest.raises(SystemExit) as good:
        slidepoints.select(_args(tool, '--nuclei-margin', path))
    assert str(good.value) == '--nuclei-margin: no GPU is visible (there is no fallback)'


def test_the_row_is_selected_after_regions(tool, tmp_path):
    assert len(slidepoints.ANALYSES) == 6 and len(slidepoints.AGAINST_CHANCE) == 1 and [a.module for a in slidepoints.WITH_INPUT] == ['regions', 'margin']
    path = _write(tmp_path, [])
    chosen = slidepoints.select(_args(tool, '--nuclei-margin', path, '--margin-step', '25.5', '--margin-bands', '4', '--nuclei-regions', path, '--nuclei-graph'), need_gpu=False)
    assert [an.cli for an, _ in chosen] == ['nuclei_graph', 'nuclei_regions', 'nuclei_margin']
    an, params = chosen[-1]
    assert params[0] == path and params[1].tolist() == [51, 102, 153, 204] and an.suffix == '_nuclei_margin.npz' and an.flag == '--nuclei-margin'
    assert an.order(params) == 'file' and len(an.more(params)) == 1 and an.more(params)[0] is params[1]
    regions_row, regions_params = chosen[1]
    assert regions_row.order(regions_params) == 'file' and regions_row.more(regions_params) == ()
    assert an.missing(params, 's1') == f'no s1.geojson in {path}: no s1_nuclei_margin.npz'
    default = slidepoints.select(_args(tool, '--nuclei-margin', str(tmp_path)), need_gpu=False)[0][1]
    assert default[0] == str(tmp_path) and default[1].tolist() == list(range(100, 1001, 100))


def test_no_flag_selects_nothing_and_imports_nothing(tool, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.delitem(sys.modules, 'nuhtc_amd.margin', raising=False)
    plain = _args(tool)
    assert plain.nuclei_margin is None and plain.margin_step == 50.0 and plain.margin_bands == 10 and slidepoints.select(plain) == ()
    assert 'nuhtc_amd.margin' not in sys.modules
