"""Host tests of the alpha-shape outline (nuhtc_amd/outline.py): `outline_reference` against hand-written rings, against an independent
walk that orders the half-edges at a vertex by exact rational slopes, and against the identities of the definition -- the successor map
is a bijection, every component has exactly one ring of positive area, the ring areas add up to the triangles' where nothing is
cocircular, the kept edges are the alpha complex of the distinct positions; `derive`, the .npz round trip, the GeoJSON through
regions.read_geojson and regions_reference, the row of the slidepoints table and the argparse lines.  No GPU."""
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import outline_cases as OC
from nuhtc_amd import alphacomplex as ax
from nuhtc_amd import outline as ol
from nuhtc_amd import regions, slidepoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = OC.small_cases()


@pytest.fixture(scope='module')
def complexes():
    return {name: ax.alpha_reference(*case) for name, case in SMALL.items()}


@pytest.fixture(scope='module')
def references(complexes):
    return {name: OC.reference(case, complexes[name]) for name, case in SMALL.items()}


# ---- the hand-written rings and what the designed sets are for
@pytest.mark.parametrize('name', sorted(OC.HAND_WRITTEN))
def test_hand_written_rings(references, name):
    OC.equal(references[name], OC.HAND_WRITTEN[name], name)


@pytest.mark.parametrize('name', sorted(OC.SHAPES))
def test_rings_holes_and_components_of_the_designed_sets(references, name):
    got = references[name]
    assert (got[7], int((got[2] < 0).sum()), got[8]) == OC.SHAPES[name], name


def test_what_the_designed_sets_are_for(references, complexes):
    assert complexes['triangle_over_r'][5] == 3 and (complexes['triangle_over_r'][2] == -1).all()          # three singular edges, one step over r
    tails = ol.half_edges(*complexes['bow_tie'][:3], 5)[1]
    assert (tails == 0).sum() == 2                                              # two out-half-edges at the shared row
    ring = references['pinched'][0].tolist()
    assert len(ring) == 18 and [v for v in set(ring) if ring.count(v) == 2] == [2]   # ONE ring through the pinch twice
    assert references['annulus'][2].tolist() == [2 * 1600, -2 * 200] and references['annulus'][3].tolist() == [0, 0]
    island = references['island']
    assert island[3].tolist() == [0, 0, 1] and (island[2] > 0).tolist() == [True, False, True] and island[4][-3:].tolist() == [1, 1, 1]
    assert references['square'][2].tolist() == [200] and references['circle_of_twelve'][6:] == (12, 1, 1) and references['lattice_6'][6] == 20
    assert references['coincident_corner'][4].tolist() == [0] * 5
    for name in ('path', 'none', 'one', 'two'):
        assert references[name][6:] == (0, 0, 0) and (references[name][4] == -1).all() and references[name][1].tolist() == [0]
    assert references['two_classes_class'][5].tolist() == [0, 1] and references['two_classes_any'][5].tolist() == [-1]
    assert references['strip_41'][6:] == (41, 1, 1) and int(references['strip_41'][2][0]) == 39 * 80


# ---- an independent walk: the out-half-edges at a vertex sorted by (quadrant, rational slope) of the clockwise turn
def _turn_key(a, b):
    x, y = a[0] * b[0] + a[1] * b[1], -(a[0] * b[1] - a[1] * b[0])                # the frame of a; y > 0: clockwise of a
    if x > 0 and y >= 0:
        return 0, Fraction(y, x)
    if x <= 0 and y > 0:
        return 1, Fraction(-x, y)
    if x < 0 and y <= 0:
        return 2, Fraction(-y, -x)
    return 3, Fraction(x, -y)


def _independent_rings(case, alpha):
    p = [tuple(int(c) for c in v) for v in case[0]]
    ids, tail, head, kept, rep = ol.half_edges(*alpha[:3], len(p))
    ids, tail, head = ids.tolist(), tail.tolist(), head.tolist()
    succ, pred = {}, {}
    for x, u, v in zip(ids, tail, head):
        a = (p[u][0] - p[v][0], p[u][1] - p[v][1])
        keys = sorted((_turn_key(a, (p[w][0] - p[v][0], p[w][1] - p[v][1])), y) for y, t, w in zip(ids, tail, head) if t == v)
        assert keys and keys[0][0] > (0, 0) and (len(keys) == 1 or keys[0][0] < keys[1][0])       # a strict first, never the direction of a
        succ[x] = keys[0][1]
        assert succ[x] not in pred, 'two half-edges share a successor'
        pred[succ[x]] = x
    assert sorted(pred) == ids                                                  # the bijection
    rings, seen = [], set()
    for x, u in zip(ids, tail):
        if x in seen:
            continue
        ring, y = [], x
        while y not in seen:
            seen.add(y)
            ring.append(tail[ids.index(y)])
            y = succ[y]
        rings.append(ring)
    return rings


@pytest.mark.parametrize('name', sorted(n for n, c in SMALL.items() if len(c[0]) <= 400))
def test_against_an_independent_walk_by_rational_slopes(references, complexes, name):
    got = references[name]
    rings = _independent_rings(SMALL[name], complexes[name])
    assert [got[0][a:b].tolist() for a, b in zip(got[1][:-1], got[1][1:])] == rings
    area2 = []
    for ring in rings:                                                          # the shoelace sum relative to the ORIGIN: the same total
        v = [tuple(int(c) for c in SMALL[name][0][k]) for k in ring]
        area2.append(sum(v[k - 1][0] * v[k][1] - v[k - 1][1] * v[k][0] for k in range(len(v))))
    assert got[2].tolist() == area2
    pos = np.bincount(got[3][got[2] > 0], minlength=got[8])
    assert (pos == 1).all()                                                     # one ring of positive area per component


# ---- the identities
@pytest.mark.parametrize('name', sorted(SMALL))
def test_ring_areas_add_up_to_the_triangles(references, complexes, name):
    p, lab, C, r, by = SMALL[name]
    got, alpha = references[name], complexes[name]
    ids, tail, head, kept, rep = ol.half_edges(*alpha[:3], len(p))
    keep = np.flatnonzero(rep == np.arange(len(p)))
    d = ax.derive(*alpha[:5], p, lab, C, r)
    if int(d['n_degenerate']) == 0 and len(keep) == len(p):
        cross = np.rint(d['triangle_area_px2'] * 8).astype(np.int64)
        assert int(got[2].sum()) == int(cross.sum()), name                      # EQUAL: both are sums of twice-areas in half pixels squared
    assert got[6] == int(((alpha[2] >= 0).sum(1) == 1)[kept].sum())
    comp = got[4]
    assert np.array_equal(comp, comp[rep]) and ((comp >= 0) == np.isin(np.arange(len(p)), np.concatenate([alpha[0][kept & (alpha[2] >= 0).any(1)].reshape(-1), np.flatnonzero(comp[rep] >= 0)]))).all()


def test_some_set_without_cocircular_points_was_checked(complexes):
    p, lab, C, r, by = SMALL['scattered']
    assert int(ax.derive(*complexes['scattered'][:5], p, lab, C, r)['n_degenerate']) == 0 and complexes['scattered'][5] > 500


@pytest.mark.parametrize('name', ['coincident_corner', 'coarse_any', 'coarse_class', 'coarse_any_r5'])
def test_the_kept_edges_are_the_alpha_complex_of_the_distinct_positions(complexes, name):
    p, lab, C, r, by = SMALL[name]
    alpha = complexes[name]
    ids, tail, head, kept, rep = ol.half_edges(*alpha[:3], len(p))
    keep = np.flatnonzero(rep == np.arange(len(p)))
    assert len(keep) < len(p)
    new = np.full(len(p), -1, np.int64)
    new[keep] = np.arange(len(keep))
    alone = ax.alpha_reference(p[keep], lab[keep], C, r, by)
    assert np.array_equal(new[alpha[0][kept]], alone[0]) and np.array_equal(alpha[1][kept], alone[1])
    assert np.array_equal(np.where(alpha[2][kept] >= 0, new[np.maximum(alpha[2][kept], 0)], -1), alone[2])


def test_permuted_rows_give_the_same_shapes(references):
    for name in ('annulus', 'island', 'coarse_any', 'scattered'):
        case = SMALL[name]
        moved = OC.permuted(case)
        a, b = references[name], OC.reference(moved)
        assert a[6:] == b[6:] and sorted(a[2].tolist()) == sorted(b[2].tolist())
        order = np.random.default_rng(4).permutation(len(case[0]))
        assert np.array_equal(a[4][order] >= 0, b[4] >= 0)                       # (a pinch row takes the SMALLEST of its components: the numbers move with the rows)


def test_the_reference_refuses_what_is_no_alpha_complex():
    p, lab, C, r, by = OC.triangle()
    e, d2, ap = ax.alpha_reference(p, lab, C, r, by)[:3]
    with pytest.raises(ValueError):
        ol.outline_reference(p, lab, e[::-1], d2[::-1], ap[::-1])
    with pytest.raises(ValueError):
        ol.outline_reference(p, lab, e, d2, ap[:, ::-1])                         # the apexes on the wrong sides
    with pytest.raises(ValueError):
        ol.outline_reference(p, lab, e, d2, ap, 2)
    with pytest.raises(AssertionError):
        ol.outline_reference(p, lab, e[:2], d2[:2], ap[:2])                      # an open chain of half-edges


# ---- derive, the files
def test_derive_on_the_island(references):
    p, lab, C, r, by = SMALL['island']
    got = references['island']
    d = ol.derive(*got[:6], p, lab, C)
    assert tuple(d) == ol.DERIVED_KEYS
    middle = 60 * 60 - 4 * 50                                                   # the empty middle: its four corner cells keep the triangle of their three sites
    assert d['area_px2'].tolist() == [(80 * 80 - middle) / 4, 8 * 7 / 2 / 4] and d['hole_area_px2'].tolist() == [middle / 4, 0.0]
    assert d['n_holes'].tolist() == [1, 0] and d['n_nuclei'].tolist() == [len(p) - 3, 3] and d['class_count'].tolist() == [[len(p) - 3], [3]]
    side = np.sqrt(16 + 49.0)
    assert abs(d['perimeter_px'][1] - (8 + 2 * side) / 2) < 1e-12 and abs(d['perimeter_px'][0] - (4 * 80 + 4 * 40 + 4 * np.sqrt(200)) / 2) < 1e-9
    assert int(d['n_components']) == 2 and int(d['n_rings']) == 3 and int(d['largest_component']) == 0 and d['area_share_by_label'].tolist() == [0.0]
    for key, t in (('area_px2', np.float64), ('n_holes', np.int64), ('n_nuclei', np.int64), ('class_count', np.int64), ('largest_component', np.int64)):
        assert d[key].dtype == t
    two = ol.derive(*OC.reference(OC.two_classes(1))[:6], *OC.two_classes(1)[:3])
    assert two['area_share_by_label'].tolist() == [0.5, 0.5] and two['class_count'].tolist() == [[16, 0], [0, 16]]
    none = ol.derive(*OC.reference(SMALL['path'])[:6], *SMALL['path'][:3])
    assert int(none['largest_component']) == -1 and none['area_px2'].shape == (0,) and none['class_count'].shape == (0, 1)
    with pytest.raises(ValueError):
        ol.derive(got[0], got[1][:-1], *got[2:6], p, lab, C)


def test_npz_round_trip_and_the_geojson_beside_it(references, tmp_path):
    p, lab, C, r, by = SMALL['island']
    got = references['island']
    path = str(tmp_path / 's_nuclei_outline.npz')
    assert ol.write_npz(path, np.arange(len(p)) + 100, p / 2.0, lab, *got[:6], C, r / 2, by, min_nuclei=4) == path
    z = ol.read_npz(path)
    assert tuple(z) == ol.NPZ_KEYS and float(z['radius_px']) == 4.0 and int(z['by_class']) == 0
    for name, a, t in zip(ol.INT_NAMES, got, ol.INT_TYPES):
        assert np.array_equal(z[name], a) and z[name].dtype == t, name
    d = ol.derive(*got[:6], p, lab, C)
    for key in ol.DERIVED_KEYS:
        assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype, key
    table = regions.read_geojson(ol.geojson_path(path))                         # the triangle has three nuclei: left out of the GeoJSON only
    assert ol.geojson_path(path).endswith('s_nuclei_outline.geojson') and table.names.tolist() == ['alpha-0'] and len(table.ring_start) == 3
    assert table.area2.tolist() == [int(got[2][:2].sum())]
    with pytest.raises(ValueError):
        ol.write_npz(path, np.arange(len(p)), p / 2.0, lab, *got[:6], C, r / 2, by, min_nuclei=-1)
    with pytest.raises(ValueError):
        ol.write_npz(path, np.arange(len(p) - 1), p[:-1] / 2.0, lab[:-1], *got[:6], C, r / 2, by)


@pytest.mark.parametrize('name', ['triangle_at_r', 'bow_tie', 'annulus', 'pinched', 'island', 'coincident_corner', 'two_classes_any', 'coarse_any', 'scattered'])
def test_geojson_round_trip_through_the_region_census(references, tmp_path, name):
    """Every row has depth > 0 or on_boundary exactly when component >= 0 (by_class 0: nothing of another label lies inside a triangle)."""
    p, lab, C, r, by = SMALL[name]
    got = references[name]
    path = str(tmp_path / 's_nuclei_outline.npz')
    ol.write_npz(path, np.arange(len(p)), p / 2.0, lab, *got[:6], C, r / 2, by, min_nuclei=0)
    table = regions.read_geojson(ol.geojson_path(path))
    assert len(table.names) == got[8] and table.skipped == 0
    region, depth, on, census = regions.regions_reference(p, lab, C, table.edges, table.edge_region, len(table.names))
    assert np.array_equal((depth > 0) | (on > 0), got[4] >= 0), name
    feats = ol.features(*got[:6], p)
    assert [f['properties']['name'] for f in feats] == [f'alpha-{k}' for k in range(got[8])]
    assert all(ring[0] == ring[-1] for f in feats for ring in f['geometry']['coordinates'])               # rings closed
    assert all(set(f['properties']) == {'name', 'label', 'n_nuclei', 'area_px2'} for f in feats)


# ---- the row of the table, the argparse lines
@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('infer_wsi_for_outline', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(tool, *flags):
    return tool.parse_args(['slide.npy', 'config.py', 'weights.pth', *flags])


def test_the_table_has_a_seventh_tuple_directly_behind_the_circles(tool, monkeypatch):
    (row,) = slidepoints.OF_THE_OUTLINES
    assert (row.cli, row.flag, row.suffix, row.module, row.second) == ('nuclei_outline', '--nuclei-outline', '_nuclei_outline.npz', 'outline', None)
    assert row._fields == slidepoints.ANALYSES[0]._fields
    assert (len(slidepoints.ANALYSES), len(slidepoints.OF_THE_PLANE), len(slidepoints.OF_THE_BORDERS), len(slidepoints.OF_THE_CIRCLES), len(slidepoints.AGAINST_CHANCE),
            len(slidepoints.WITH_INPUT)) == (6, 1, 1, 1, 1, 2)
    plain = _args(tool)
    assert plain.nuclei_outline is False and (plain.outline_radius, plain.outline_by, plain.outline_min_nuclei) == (32.0, 'any', 3)
    with pytest.raises(SystemExit):
        _args(tool, '--outline-by', 'label')
    flags = ['--nuclei-enrichment', '--nuclei-outline', '--outline-radius', '12.5', '--outline-by', 'class', '--outline-min-nuclei', '7', '--nuclei-alpha', '--nuclei-adjacency',
             '--nuclei-graph']
    chosen = slidepoints.select(_args(tool, *flags), need_gpu=False)
    assert [an.module for an, _ in chosen] == ['cellgraph', 'adjacency', 'alphacomplex', 'outline', 'enrichment']
    assert dict((an.module, p) for an, p in chosen)['outline'] == (12.5, 1, 7)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for bad in (['--outline-radius', '0'], ['--outline-radius', '0.25'], ['--outline-radius', '257'], ['--outline-min-nuclei', '-1']):
        with pytest.raises(SystemExit) as refused:
            slidepoints.select(_args(tool, '--nuclei-outline', *bad))
        assert str(refused.value).startswith('--nuclei-outline: ') and 'no GPU' not in str(refused.value), str(refused.value)
    for good_flags in ([], ['--outline-radius', '256']):                        # the limits of --alpha-radius
        with pytest.raises(SystemExit) as good:
            slidepoints.select(_args(tool, '--nuclei-outline', *good_flags))
        assert str(good.value) == '--nuclei-outline: no GPU is visible (there is no fallback)'


def test_the_closing_clause(references):
    (row,) = slidepoints.OF_THE_OUTLINES
    said = row.said(ol, references['island'], (4.0, 0, 3))
    assert said == ('2 alpha-shape components in 3 rings, 1 of them holes (4 px radius, by any; the largest of 750 px^2 with 56 nuclei; components of fewer than 3 nuclei '
                    'left out of the GeoJSON)'), said
    assert row.said(ol, references['path'], (2.5, 1, 0)).startswith('0 alpha-shape components in 0 rings, 0 of them holes (2.5 px radius, by class; none;')
