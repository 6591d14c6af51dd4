"""The region census (nuhtc_amd/regions.py) without a GPU: `regions_reference` against a double loop in Python integers, the hand-written
rows, the tiling property, matplotlib on every point off the boundary, the GeoJSON reader, from_contours, derive, check_args, the file
round trip and the tool's argument checks through slidepoints.select."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

import regions_cases as RC
from nuhtc_amd import regions as rg
from nuhtc_amd import slidepoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def double_loop(p, lab, C, edges, edge_region, G):
    """The definition, one point and one edge at a time, in Python integers."""
    n = len(p)
    region, depth, on, census = [-1] * n, [0] * n, [0] * n, [[0] * C for _ in range(G)]
    E = [tuple(int(v) for v in e) for e in edges.tolist()]
    er = edge_region.tolist()
    for i, (px, py) in enumerate(p.tolist()):
        parity = [0] * G
        for (ax, ay, bx, by), g in zip(E, er):
            if (ay <= py) != (by <= py):
                lx, ly, hx, hy = (ax, ay, bx, by) if ay < by else (bx, by, ax, ay)
                parity[g] ^= (hx - lx) * (py - ly) - (hy - ly) * (px - lx) > 0
            if (bx - ax) * (py - ay) - (by - ay) * (px - ax) == 0 and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by):
                on[i] = 1
        for g in range(G):
            if parity[g]:
                region[i], depth[i] = g, depth[i] + 1
                if 0 <= lab[i] < C:
                    census[g][int(lab[i])] += 1
    return np.asarray(region, np.int32), np.asarray(depth, np.int32), np.asarray(on, np.uint8), np.asarray(census, np.int64).reshape(G, C)


def _equal(got, want, what):
    for name, g, w in zip(rg.INT_NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:3].tolist())


SMALL = ('unit_rectangle', 'tiling', 'notch', 'holes', 'holes_some_reversed', 'labels_out_of_range', 'degenerate', 'bit_budget', 'no_points', 'no_regions', 'neither',
         'region_without_edges')


@pytest.mark.parametrize('name', SMALL)
def test_reference_equals_the_double_loop(name):
    case = RC.all_cases()[name]
    _equal(rg.regions_reference(*case), double_loop(*case), name)


def test_reference_equals_the_double_loop_on_sampled_rows_of_the_large_sets():
    cases = RC.all_cases()
    for name in ('staging', 'random_lattice_1', 'random_lattice_2', 'chain_shuffled', 'overlap'):
        case = cases[name]
        pick = np.random.default_rng(1).choice(len(case[0]), 150, replace=False)
        full = rg.regions_reference(*case)
        loop = double_loop(case[0][pick], case[1][pick], *case[2:])
        for k in range(3):
            assert np.array_equal(full[k][pick], loop[k]), (name, rg.INT_NAMES[k])
        _equal(rg.regions_reference(case[0][pick], case[1][pick], *case[2:], block=7), loop, name)


def test_unit_rectangle_rows_by_hand():
    _equal(rg.regions_reference(*RC.unit_rectangle()), RC.unit_rectangle_expected(), 'unit rectangle')


def test_notch_rows_by_hand():
    case = RC.notch()
    region, depth, on, _ = rg.regions_reference(*case)
    at = {tuple(p): i for i, p in enumerate(case[0].tolist())}
    for p, want in RC.NOTCH_HAND.items():
        assert region[at[p]] == want, (p, int(region[at[p]]), want)
    assert on[at[(6, 4)]] and on[at[(13, 5)]] and on[at[(0, 0)]] and on[at[(2, 10)]] and on[at[(3, 0)]] and not on[at[(5, 10)]] and not on[at[(2, 4)]]


def test_tiling_every_point_of_the_union_is_in_exactly_one_piece():
    case = RC.tiling()
    region, depth, on, census = rg.regions_reference(*case)
    union = RC.tiling_union(case[0])
    assert np.array_equal(depth, union.astype(np.int32)) and np.array_equal(region >= 0, union)
    assert census.sum() == union.sum() and union.sum() == 12 * 4 + 8 * 8 and (census[:, 0] > 0).all()
    apex = np.flatnonzero((case[0] == (24, 4)).all(1))[0]
    assert depth[apex] == 1 and on[apex] == 1


def test_orientation_does_not_matter():
    want = rg.regions_reference(*RC.holes())
    for flip in ((True, True, True), (False, True, False), (True, False, True)):
        _equal(rg.regions_reference(*RC.holes(flip)), want, flip)
    p, depth = RC.holes()[0], want[1]
    at = lambda x, y: depth[np.flatnonzero((p == (x, y)).all(1))[0]]
    assert at(2, 2) == 1 and at(6, 6) == 0 and at(10, 10) == 1 and at(32, 3) == 1 and at(38, 3) == 0 and at(42, 4) == 1
    assert at(4, 4) == 0 and at(16, 16) == 1 and at(8, 8) == 1 and at(12, 12) == 0                  # the hole's min corner is out, its max corner in


def test_overlap_largest_index_and_every_containing_region():
    case = RC.overlap()
    p, lab = case[0], case[1]
    region, depth, on, census = rg.regions_reference(*case)
    inside = np.stack([(p[:, 0] >= x0) & (p[:, 0] < x1) & (p[:, 1] >= y0) & (p[:, 1] < y1) for x0, y0, x1, y1 in RC.OVERLAP_RECTS], 1)
    assert np.array_equal(depth, inside.sum(1)) and np.array_equal(region, np.where(inside.any(1), 3 - np.argmax(inside[:, ::-1], 1), -1))
    assert np.array_equal(census, np.stack([np.bincount(lab[inside[:, g]], minlength=3) for g in range(4)])) and depth.max() == 3
    out = RC.overlap('out')
    assert np.array_equal(rg.regions_reference(*out)[3], np.stack([np.bincount(out[1][inside[:, g] & (out[1] >= 0) & (out[1] < 3)], minlength=3) for g in range(4)]))


def test_degenerate_rings():
    case = RC.degenerate()
    region, depth, on, census = rg.regions_reference(*case)
    at = lambda x, y: np.flatnonzero((case[0] == (x, y)).all(1))[0]
    assert on[at(3, 3)] and region[at(3, 3)] == 1 and not on[at(3, 4)]                             # the zero-length edge touches its own point only
    assert census[0, 0] == 0 and census[2, 0] == 0 and census[1, 0] == 36                          # one point and two points contain nothing
    assert all(on[at(10 + k, k)] and region[at(10 + k, k)] == -1 for k in range(5)) and not on[at(11, 2)]


def test_bit_budget_float64_decides_the_side_wrongly():
    case, (i1, i2), (A, B) = RC.bit_budget()
    p = case[0].astype(np.int64)
    exact = [(B[0] - A[0]) * (int(p[i, 1]) - A[1]) - (B[1] - A[1]) * (int(p[i, 0]) - A[0]) for i in (i1, i2)]
    assert exact == [1, -1]
    as_float = [float(B[0] - A[0]) * float(p[i, 1] - A[1]) - float(B[1] - A[1]) * float(p[i, 0] - A[0]) for i in (i1, i2)]
    assert [f > 0 for f in as_float] != [True, False], as_float                                    # float64 cannot tell the two sides apart
    region, depth, on, census = rg.regions_reference(*case)
    _equal((region, depth, on, census), double_loop(*case), 'bit budget')
    assert region[i1] != region[i2] and not on[i1] and not on[i2] and on[2] and on[3]


def test_matplotlib_agrees_off_the_boundary():
    """matplotlib.path.Path.contains_points ring by ring, in float64: a region holds a point when an odd number of its rings do (the rings
    of the designed sets are simple).  Compared on every point with on_boundary 0; the bit-budget set is left to the test above, float64
    is wrong there."""
    from matplotlib.path import Path
    checked = 0
    for name, case in RC.all_cases().items():
        p, lab, C, edges, er, G = case
        if name == 'bit_budget' or len(p) == 0 or G == 0:
            continue
        region, depth, on, census = rg.regions_reference(*case)
        got = np.zeros(len(p), np.int64)
        for g in range(G):
            e = edges[er == g].astype(np.float64)
            start = np.flatnonzero(np.r_[True, (e[1:, :2] != e[:-1, 2:]).any(1)]) if len(e) else []
            rings = np.zeros(len(p), np.int64)
            for r0, r1 in zip(start, np.r_[start[1:], len(e)]):
                if r1 - r0 >= 3:                                                                   # (a ring of one or two points holds nothing)
                    rings += Path(np.concatenate([e[r0:r1, :2], e[r0:r0 + 1, :2]], 0), closed=True).contains_points(p.astype(np.float64))
            got += rings & 1
        off = on == 0
        assert np.array_equal(got[off], depth[off]), (name, np.flatnonzero(got[off] != depth[off])[:5].tolist())
        checked += int(off.sum())
    assert checked > 40000


# ---- the reader
def _write(tmp_path, doc, name='r.geojson'):
    path = tmp_path / name
    path.write_text(json.dumps(doc))
    return str(path)


def _feature(kind, coords, **props):
    return dict(type='Feature', geometry=dict(type=kind, coordinates=coords), properties=props)


def test_read_geojson(tmp_path):
    sq = lambda x0, y0, x1, y1: [[x0, y0], [x1, y0], [x1, y1], [x0, y1], [x0, y0]]
    feats = [_feature('Polygon', [sq(0, 0, 10, 10), sq(2, 2, 5, 5)], classification=dict(name='Tumor')),
             _feature('LineString', [[0, 0], [5, 5]], name='line'),
             _feature('MultiPolygon', [[sq(20, 0, 24, 3)], [sq(30.25, 0, 32.25, 1), sq(30.75, 0.25, 31.25, 0.75)]], name='Stroma'),
             _feature('Polygon', [[[0, 0], [3, 0], [0, 4]]])]                                          # an open ring: closed by the reader
    for doc in (feats, dict(type='FeatureCollection', features=feats)):
        t = rg.read_geojson(_write(tmp_path, doc))
        assert t.skipped == 1 and t.names.tolist() == ['Tumor', 'Stroma', ''] and t.ring_start.tolist() == [0, 4, 8, 12, 16, 20, 23]
        assert t.edge_region.tolist() == [0] * 8 + [1] * 12 + [2] * 3 and t.edges.dtype == np.int32 and t.edge_region.dtype == np.int32
        assert t.edges[:4].tolist() == [[0, 0, 20, 0], [20, 0, 20, 20], [20, 20, 0, 20], [0, 20, 0, 0]]
        assert t.edges[12:16].tolist() == [[60, 0, 64, 0], [64, 0, 64, 2], [64, 2, 60, 2], [60, 2, 60, 0]]       # rint(60.5) = 60, rint(64.5) = 64: half to even
        assert t.edges[20:].tolist() == [[0, 0, 6, 0], [6, 0, 0, 8], [0, 8, 0, 0]]
        # twice the area in half pixels squared: 2 * (400 - 36), 2 * (8 * 6) + 2 * (4 * 2) - 2 * (2 * 0) [the inner ring is 62 .. 62 wide after rounding], 6 * 8
        assert t.area2.tolist() == [2 * (400 - 36), 2 * 48 + 2 * 8 - 2 * 0, 48] and t.area2.dtype == np.int64
    by_area = rg.read_geojson(_write(tmp_path, feats), order='area')
    assert by_area.names.tolist() == ['Tumor', 'Stroma', ''] and by_area.area2.tolist() == sorted(by_area.area2.tolist(), reverse=True)
    with pytest.raises(ValueError):
        rg.read_geojson(_write(tmp_path, feats), order='size')
    with pytest.raises(ValueError):
        rg.read_geojson(_write(tmp_path, [_feature('Polygon', [sq(0, 0, 1 << 26, 5)])]))           # 2 * 2**26 = 2**27: outside the range
    empty = rg.read_geojson(_write(tmp_path, []))
    assert empty.edges.shape == (0, 4) and len(empty.names) == 0 and empty.ring_start.tolist() == [0]


def test_order_area_puts_the_innermost_on_top(tmp_path):
    feats = RC.overlap_features()
    as_file, by_area = rg.read_geojson(_write(tmp_path, feats)), rg.read_geojson(_write(tmp_path, feats), order='area')
    assert as_file.names.tolist() == ['small', 'other', 'mid', 'big'] and by_area.names.tolist() == ['big', 'other', 'mid', 'small']
    assert by_area.area2.tolist() == [2 * 900, 2 * 400, 2 * 400, 2 * 25]                           # the tie keeps the file order
    case = RC.overlap()
    want = rg.regions_reference(*case)                                                               # the designed order: big, mid, small, other
    got = rg.regions_reference(case[0], case[1], 3, by_area.edges, by_area.edge_region, 4)
    back = np.array([0, 3, 1, 2])                                                                    # by_area index -> designed index
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3][back])
    p = case[0]
    small = (p[:, 0] >= 10) & (p[:, 0] < 15) & (p[:, 1] >= 10) & (p[:, 1] < 15)
    assert (got[0][small] == 3).all() and small.sum() == 25                                         # the innermost is on top


def test_from_contours():
    contours = [np.array([[[0, 0]], [[10, 0]], [[10, 10]], [[0, 10]]], np.int32), np.array([[20, 0], [25, 0], [25, 5]], np.int32)]
    holes_ = [[np.array([[2, 2], [4, 2], [4, 4], [2, 4]], np.int32)], []]
    t = rg.from_contours(contours, holes_)
    assert t.names.tolist() == ['', ''] and t.ring_start.tolist() == [0, 4, 8, 11] and t.edge_region.tolist() == [0] * 8 + [1] * 3
    assert t.edges[4].tolist() == [4, 4, 8, 4] and t.area2.tolist() == [2 * (400 - 16), 100]
    got = rg.regions_reference(np.array([[2, 2], [6, 6], [10, 10], [48, 2], [60, 60]]), np.zeros(5), 1, t.edges, t.edge_region, 2)
    assert got[0].tolist() == [0, -1, 0, 1, -1]
    with pytest.raises(ValueError):
        rg.from_contours(contours, holes_[:1])


def test_derive_on_hand_counted_rows():
    census = np.array([[3, 1], [0, 0], [2, 2]], np.int64)
    d = rg.derive(census, [16, 0, 64], depth=[1, 2, 0, 0, 1, 1, 0, 3], labels=[0, 0, 0, 1, 1, 1, 5, -1])
    assert tuple(d) == rg.DERIVED_KEYS
    assert d['area_px2'].tolist() == [2.0, 0.0, 8.0] and d['density_per_px2'][0].tolist() == [1.5, 0.5] and np.isnan(d['density_per_px2'][1]).all()
    assert d['density_per_px2'][2].tolist() == [0.25, 0.25] and d['class_fraction'].tolist() == [[0.75, 0.25], [0.0, 0.0], [0.5, 0.5]]
    assert int(d['n_inside']) == 5 and int(d['n_outside']) == 3 and d['class_share_inside'].tolist() == [2 / 3, 2 / 3]
    with pytest.raises(ValueError):
        rg.derive(census, [16, 0], [1], [0])


def test_check_args_and_as_edges():
    rg.check_args(1), rg.check_args(14, 1 << 16, 1 << 22, 16384)
    for bad in ((0,), (15,), (1, -1), (1, (1 << 16) + 1), (1, 1, (1 << 22) + 1), (1, 1, 1, 0), (1, 1, 1, 16385), (1.5,)):
        with pytest.raises(ValueError):
            rg.check_args(*bad)
    e, er, G = RC.table([[RC.rect(0, 0, 4, 4)], [RC.rect(5, 5, 9, 9)]])
    rg.as_edges(e, er, G)
    for edges, region, g in ((e, er[::-1], G), (e, er, 1), (e, er - 1, G), (e, er[:-1], G), (e + (1 << 27), er, G), (e + 0.5, er, G)):
        with pytest.raises(ValueError):
            rg.as_edges(edges, region, g)
    with pytest.raises(ValueError):
        rg.regions_reference(np.array([[1 << 27, 0]]), [0], 1, e, er, G)


def test_the_slab_walk_case_is_laid_out_as_it_says():
    case = RC.slab_walk()
    p, lab, C, edges, er, G = case
    points, records = RC.slab_layout(case, RC.SLAB_WALK_SLAB)
    assert points == [100, 60, 140] and len(p) == 300                                # records 0 .. 255 lie in three slabs; the second workgroup has 44
    assert [len(r) for r in records] == [4, 0, 256 + 256 + 8]                       # the middle slab has no edge record at all
    assert records[2] == [0] * 256 + [1] * 260 + [2] * 4                              # the changes: at record 256, and at 516 inside the last pass
    assert rg.slots_needed(edges, (0, 0, 1000, 599), RC.SLAB_WALK_SLAB) == 524 and (edges[er == 2][:, [0, 2]] > 1000 + 20).all()
    region, depth, on, census = rg.regions_reference(*case)
    assert set(region.tolist()) == {-1, 0, 1} and depth.max() == 2 and on.sum() >= 4 and not census[2].any() and census[0].sum() > census[1].sum() > 0


def test_the_record_protocol_on_a_stub_call():
    """cellpoints.grow_to_fit as regions.build and margin.build run it: their refusal of more than 2**28 records in place of the edge
    lists' limit, the outputs made once, and the wording of the records."""
    from nuhtc_amd import cellpoints
    refuse = lambda m: f'regions: {m} (edge, slab) records, more than 2**28: a larger slab makes them fewer' if m > rg.MAX_SLOTS else None
    out, log = ['out'], []

    def run(answers, first_cap):
        answers = list(answers)
        return cellpoints.grow_to_fit(lambda cap, o: log.append((cap, o)) or answers.pop(0), lambda cap: out, first_cap, 'nuhtc_stub', 'regions',
                                      refuse=refuse, unit='records')
    assert run([(0, 7)], 1 << 28) == (out, 7, (), 1) and run([(0, 9), (0, 9)], 3)[3] == 2 and all(o is out for _, o in log)
    assert run([(0, 1 << 28), (0, 1 << 28)], 5)[1:] == (1 << 28, (), 2)                                  # 2**28 records are not too many
    del log[:]
    with pytest.raises(ValueError, match=r'regions: 268435457 \(edge, slab\) records, more than 2\*\*28: a larger slab makes them fewer'):
        run([(0, (1 << 28) + 1)], 5)
    assert len(log) == 1                                                                                 # no second call
    with pytest.raises(RuntimeError, match='nuhtc_stub: 8 records on the second call, 9 on the first'):
        run([(0, 9), (0, 8)], 3)


def test_slots_needed_and_choose_slab():
    e = np.array([[0, -5, 0, 25], [3, 3, 9, 3], [-4, 0, -1, 20], [50, 9, 40, 10], [0, 21, 5, 30], [0, -9, 5, -1]], np.int64)
    # box (0, 0) .. (10, 20), slab 5: rows 0-4, 5-9, 10-14, 15-19, 20.  The first edge meets all five, the second one, the third lies left
    # of the box, the fourth (right of it) meets rows 1 and 2, the last two lie below and above
    assert rg.slots_needed(e, (0, 0, 10, 20), 5) == 5 + 1 + 0 + 2 + 0 + 0
    assert rg.slots_needed(e, (0, 0, 10, 20), 16384) == 3 and rg.slots_needed(e[:0], (0, 0, 10, 20), 5) == 0
    assert rg.choose_slab((0, 0, 10, 20)) == 1 and rg.choose_slab((0, 0, 0, 2047)) == 1 and rg.choose_slab((0, 0, 0, 2048)) == 2
    assert rg.choose_slab((0, -(1 << 27) + 1, 0, (1 << 27) - 1)) == 16384


def test_file_round_trip(tmp_path):
    case = RC.overlap()
    t = rg.read_geojson(_write(tmp_path, RC.overlap_features()), order='area')
    found = rg.regions_reference(case[0], case[1], 3, t.edges, t.edge_region, 4)
    n = len(case[0])
    path = rg.write_npz(str(tmp_path / 's_nuclei_regions.npz'), np.arange(n), case[0] / 2, case[1], *found, t, 'area')
    z = rg.read_npz(path)
    assert tuple(z) == rg.NPZ_KEYS and str(z['order']) == 'area' and z['names'].tolist() == ['big', 'other', 'mid', 'small']
    for name, want in zip(rg.INT_NAMES, found):
        assert np.array_equal(z[name], want) and z[name].dtype == want.dtype
    d = rg.derive(found[3], t.area2, found[1], case[1])
    for key in rg.DERIVED_KEYS:
        assert np.array_equal(z[key], d[key], equal_nan=True) and z[key].dtype == d[key].dtype, key
    assert np.array_equal(z['edges'], t.edges) and np.array_equal(z['edge_region'], t.edge_region) and np.array_equal(z['area2'], t.area2)
    assert np.array_equal(z['ring_start'], t.ring_start) and z['area_px2'].tolist() == [225.0, 100.0, 100.0, 6.25]
    with np.load(path, allow_pickle=False) as plain:                                                # nothing pickled
        assert set(plain.files) == set(rg.NPZ_KEYS)
    with pytest.raises(ValueError):
        rg.write_npz(str(tmp_path / 'bad.npz'), np.arange(n), case[0] / 2, case[1], found[0][:-1], *found[1:], t)


# ---- the tool's argument checks
@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('infer_wsi_for_regions', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(tool, *flags):
    return tool.parse_args(['slide.npy', 'config.py', 'weights.pth', *flags])


def test_a_bad_path_is_named_before_the_missing_gpu(tool, monkeypatch, tmp_path):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SystemExit) as bad:
        slidepoints.select(_args(tool, '--nuclei-regions', str(tmp_path / 'nowhere.geojson')))
    assert str(bad.value).startswith('--nuclei-regions: ') and 'no GPU' not in str(bad.value) and 'nowhere.geojson' in str(bad.value)
    path = _write(tmp_path, [])
    with pytest.raises(SystemExit) as good:
        slidepoints.select(_args(tool, '--nuclei-regions', path))
    assert str(good.value) == '--nuclei-regions: no GPU is visible (there is no fallback)'
    with pytest.raises(SystemExit):
        _args(tool, '--nuclei-regions', path, '--regions-order', 'size')


def test_the_row_stands_outside_the_table_and_is_selected_last(tool, tmp_path):
    assert len(slidepoints.ANALYSES) == 6 and 'regions' not in [a.module for a in slidepoints.ANALYSES]
    path = _write(tmp_path, [])
    chosen = slidepoints.select(_args(tool, '--nuclei-regions', path, '--regions-order', 'area', '--nuclei-density', '--nuclei-graph'), need_gpu=False)
    assert [an.cli for an, _ in chosen] == ['nuclei_graph', 'nuclei_density', 'nuclei_regions'] and chosen[-1][1] == (path, 'area')
    assert chosen[-1][0].suffix == '_nuclei_regions.npz' and chosen[-1][0].flag == '--nuclei-regions'
    m = slidepoints.module_of(chosen[-1][0])
    assert m.source_for(path, 's1') == path and m.source_for(str(tmp_path), 'r') == path and m.source_for(str(tmp_path), 's1') is None
    assert slidepoints.select(_args(tool, '--nuclei-regions', str(tmp_path)), need_gpu=False)[0][1] == (str(tmp_path), 'file')


def test_no_flag_selects_nothing_and_imports_nothing(tool, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.delitem(sys.modules, 'nuhtc_amd.regions', raising=False)
    plain = _args(tool)
    assert plain.nuclei_regions is None and plain.regions_order == 'file' and slidepoints.select(plain) == ()
    assert 'nuhtc_amd.regions' not in sys.modules
