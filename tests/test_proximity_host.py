"""Host-only checks of the proximity graphs (nuhtc_amd/proximity.py): `proximity_reference` against an independent triple loop in plain
Python integers, against the hand-written and closed-form cases of tests/proximity_cases.py, the chain MSF in RNG in Gabriel against
mst.mst_reference, Gabriel in Delaunay against scipy, `derive` on hand-counted rows and on a two-class checkerboard, `check_args` and the
.npz round trip.  The device is compared with `proximity_reference` in tests/test_hip_proximity.py."""
import importlib.util
import os

import numpy as np
import pytest

import proximity_cases as PC
from nuhtc_amd import mst
from nuhtc_amd import proximity as px

NAMES = px.INT_NAMES + ('m', 'm_rng')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def triple_loop(p, lab, C, r, by_class):
    """The definition word for word: Python integers, every pair, every other row as a witness."""
    p, lab, n = [(int(x), int(y)) for x, y in p], [int(v) for v in lab], len(p)
    d2 = lambda a, b: (p[a][0] - p[b][0]) ** 2 + (p[a][1] - p[b][1]) ** 2
    edges, dist, flags, degree = [], [], [], [[0, 0] for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            dij = d2(i, j)
            if dij > r * r or (by_class and lab[i] != lab[j]):
                continue
            gabriel = rng = True
            for k in range(n):
                if k == i or k == j or (by_class and lab[k] != lab[i]):
                    continue
                dik, djk = d2(i, k), d2(j, k)
                if dik + djk < dij:
                    gabriel = False
                if max(dik, djk) < dij:
                    rng = False
            if gabriel:
                edges.append([i, j]); dist.append(dij); flags.append(int(rng))
                for end in (i, j):
                    degree[end][0] += 1
                    degree[end][1] += int(rng)
    return edges, dist, flags, degree, len(edges), sum(flags)


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        if name in ('m', 'm_rng'):
            assert int(g) == int(w), (what, name, int(g), int(w))
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name)


@pytest.fixture(scope='module')
def references():
    return {name: px.proximity_reference(*case) for name, case in PC.small_cases().items()}


@pytest.mark.parametrize('name', sorted(PC.small_cases()))
def test_reference_equals_the_triple_loop(references, name):
    e, d2, rng, deg, m, m_rng = references[name]
    n = len(PC.small_cases()[name][0])
    assert e.dtype == np.int32 and e.shape == (m, 2) and d2.dtype == np.int32 and d2.shape == (m,) and rng.dtype == np.uint8 and rng.shape == (m,)
    assert deg.dtype == np.int32 and deg.shape == (n, 2)
    want = triple_loop(*PC.small_cases()[name])
    assert e.tolist() == want[0] and d2.tolist() == want[1] and rng.tolist() == want[2] and deg.tolist() == want[3] and (m, m_rng) == want[4:]
    assert (deg[:, 1] <= deg[:, 0]).all() and int(deg[:, 0].sum()) == 2 * m and int(deg[:, 1].sum()) == 2 * m_rng


def test_reference_equals_the_hand_written_and_closed_form_cases(references):
    _same(references['circles'], PC._expected(12, PC.CIRCLES), 'circles')
    _same(references['radius'], PC._expected(6, PC.RADIUS), 'radius')
    _same(references['other_label_any'], PC._expected(6, PC.OTHER_LABEL[0]), 'any')
    _same(references['other_label_class'], PC._expected(6, PC.OTHER_LABEL[1]), 'class')
    _same(references['lattice'], PC.lattice_expected(), 'lattice')
    _same(references['lattice_3x2'], PC.lattice_expected(3, 2, 5), 'lattice 3 x 2')
    e, d2, rng, deg, m, m_rng = references['lattice']
    assert m == 7 * 4 + 5 * 6 + 2 * 6 * 4 and m_rng == 7 * 4 + 5 * 6 and int(d2.max()) == 200        # nothing longer than a diagonal
    _same(references['crowded_small'], PC.crowded_expected(PC.crowded(70)), 'crowded')
    e, d2, rng, deg, m, m_rng = references['borders']
    pairs = {tuple(x) for x in e.tolist()}
    assert (2, 3) not in pairs and (5, 6) not in pairs and (8, 9) in pairs and (11, 12) not in pairs and {(2, 4), (3, 4), (5, 7), (6, 7)} <= pairs
    assert references['one_point'][3].tolist() == [[0, 0]] and references['one_point'][4:] == (0, 0)
    assert references['two_points'][0].tolist() == [[0, 1]] and references['two_points_apart'][4:] == (0, 0)
    assert references['two_coincident'][1].tolist() == [0] and references['two_coincident'][2].tolist() == [1]
    empty = px.proximity_reference(np.zeros((0, 2)), [], 3, 8, 0)
    assert empty[0].shape == (0, 2) and empty[1].shape == (0,) and empty[2].shape == (0,) and empty[3].shape == (0, 2) and empty[4:] == (0, 0)
    assert empty[0].dtype == np.int32 and empty[2].dtype == np.uint8


def test_coincident_points_are_a_clique_of_rng_edges():
    case = PC.coincident(40)
    e, d2, rng, deg, m, m_rng = px.proximity_reference(*case)
    assert e[:39].tolist() == [[0, k] for k in range(1, 40)] and int((d2 == 0).sum()) == 40 * 39 // 2 and (rng[d2 == 0] == 1).all()
    assert m >= 780 > 4 * 45                                                          # a clique: not bounded by a multiple of n
    assert 300 * 299 // 2 == 44850 and 44850 > px.first_edge_cap(305)                 # the device-sized case needs the second call


def test_chain_and_crowded_closed_forms_are_the_reference():
    for order in ('ascending', 'descending', 'shuffled'):
        case = PC.chain(order, 300)
        _same(px.proximity_reference(*case), PC.chain_expected(case), order)
    case = PC.crowded(200)
    _same(px.proximity_reference(*case), PC.crowded_expected(case), 'crowded 200')


@pytest.mark.parametrize('by', [0, 1])
@pytest.mark.parametrize('seed', [1, 2])
def test_forest_in_rng_in_gabriel_on_sets_with_ties(seed, by):
    rng = np.random.default_rng(seed)
    p, lab = rng.integers(0, 14, (260, 2)), rng.integers(-1, 3, 260)
    e, d2, flag, deg, m, m_rng = px.proximity_reference(p, lab, 3, 5, by)
    gabriel = {tuple(x) for x in e.tolist()}
    rng_edges = {tuple(x) for x in e[flag == 1].tolist()}
    forest = {tuple(x) for x in mst.mst_reference(p, lab, 3, 5, by)[0].tolist()}
    assert forest <= rng_edges <= gabriel and len(gabriel) == m and len(rng_edges) == m_rng and len(forest) >= 1


def test_ties_on_a_12_x_12_lattice():
    case = PC.random_ties()
    e, d2, rng, deg, m, m_rng = px.proximity_reference(*case)
    assert len(case[0]) == 300 and m > px.first_edge_cap(300) // 2 and 0 < m_rng < m and int((d2 == 0).sum()) > 100


def test_every_gabriel_edge_is_a_delaunay_edge():
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(5)
    p = rng.integers(0, 5000, (250, 2))                                           # jittered: no four points on a circle to speak of
    e, d2, flag, deg, m, m_rng = px.proximity_reference(p, np.zeros(250, int), 1, 8000, 0)      # r beyond the diameter of the set
    tri = Delaunay(p.astype(np.float64)).simplices
    delaunay = {tuple(sorted((int(t[a]), int(t[b])))) for t in tri for a, b in ((0, 1), (1, 2), (0, 2))}
    assert {tuple(x) for x in e.tolist()} <= delaunay and 250 - 1 <= m_rng <= m <= len(delaunay)


def test_derive_on_hand_counted_rows():
    # rows 0-1-2: edges (0, 1) 3 px rng, (1, 2) 4 px rng, (0, 2) 5 px Gabriel only; rows 3-4 coincident; row 5 alone; labels 0, 1, 1, 2, 7, 0; C = 3
    e, d2, flag = [[0, 1], [0, 2], [1, 2], [3, 4]], [36, 100, 64, 0], [1, 0, 1, 1]
    deg = [[2, 1], [2, 2], [2, 1], [1, 1], [1, 1], [0, 0]]
    d = px.derive(e, d2, flag, deg, [0, 1, 1, 2, 7, 0], 3)
    assert set(d) == set(px.DERIVED_KEYS)
    assert d['edge_len_px'].tolist() == [3.0, 5.0, 4.0, 0.0] and d['edge_len_px'].dtype == np.float64
    assert d['gabriel_class_count'].tolist() == [[0, 2, 0], [0, 1, 0], [0, 0, 0]] and d['gabriel_class_count'].dtype == np.int64     # (2, 7) nowhere
    assert d['rng_class_count'].tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 0]]
    assert d['mean_len_px'].tolist() == [[4.0, 3.0], [3.5, 3.5], [4.5, 4.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]] and d['mean_len_px'].dtype == np.float64
    assert d['other_class_share'].tolist() == [1.0, 0.5, 0.5, 1.0, 1.0, 0.0]
    assert int(d['n_edges']) == 4 and int(d['n_rng']) == 3 and d['n_edges'].dtype == np.int64
    # n = 6, sizes 2, 2, 1: E[0][1] = 4 * 2 * 2 * 2 / 30, E[1][1] = 4 * 2 * 1 / 30, E[2][2] = 0
    enr = d['gabriel_class_enrichment']
    assert enr.dtype == np.float64 and enr.shape == (3, 3) and np.isfinite(enr).all()
    assert np.isclose(enr[0, 1], 2 / (4 * 8 / 30), rtol=1e-14) and np.isclose(enr[1, 1], 1 / (4 * 2 / 30), rtol=1e-14) and enr[0, 0] == 0.0 and enr[2, 2] == 0.0 and enr[1, 0] == 0.0
    for none in (px.derive(np.zeros((0, 2)), [], [], [[0, 0], [0, 0]], [0, 0], 2), px.derive([], [], [], np.zeros((0, 2)), [], 2),
                 px.derive([], [], [], [[0, 0]], [1], 2)):
        assert np.isfinite(none['gabriel_class_enrichment']).all() and (none['gabriel_class_enrichment'] == 0).all() and int(none['n_edges']) == 0
        assert none['edge_len_px'].shape == (0,) and (none['mean_len_px'] == 0).all() and (none['other_class_share'] == 0).all()
    with pytest.raises(ValueError):
        px.derive([[0, 3]], [4], [1], [[1, 1], [0, 0], [0, 0]], [0, 0, 0], 1)
    with pytest.raises(ValueError):
        px.derive([[0, 1]], [4], [1], [[1, 1], [1, 0]], [0, 0], 1)                  # the degree of row 1 is wrong


def test_enrichment_on_a_two_class_checkerboard():
    """4 x 4 points, label (x + y) % 2: 24 sides, all between the classes; 18 diagonals, 9 inside each class.  n = 16, 8 of each."""
    case = PC.lattice(4, 4)
    e, d2, flag, deg, m, m_rng = px.proximity_reference(*case)
    d = px.derive(e, d2, flag, deg, case[1], 2)
    assert m == 42 and m_rng == 24 and d['gabriel_class_count'].tolist() == [[9, 24], [0, 9]] and d['rng_class_count'].tolist() == [[0, 24], [0, 0]]
    enr = d['gabriel_class_enrichment']
    assert np.isclose(enr[0, 1], 24 / 22.4, rtol=1e-14) and enr[0, 0] == enr[1, 1] and np.isclose(enr[0, 0], 9 / 9.8, rtol=1e-14) and enr[1, 0] == 0.0
    corner, inner = 0, 5
    assert d['other_class_share'][corner] == 2 / 3 and d['other_class_share'][inner] == 0.5
    assert np.allclose(d['mean_len_px'][corner], [(5 + 5 + np.sqrt(200) / 2) / 3, 5.0], rtol=1e-14)


@pytest.mark.parametrize('C, r, by', [(0, 5, 0), (15, 5, 0), (3, 0, 0), (3, 16385, 0), (3, 5, 2), (3, 5, -1), (3, 2.5, 0)])
def test_check_args_refuses(C, r, by):
    with pytest.raises(ValueError):
        px.check_args(C, r, by)
    with pytest.raises(ValueError):
        px.proximity_reference([[0, 0], [3, 4]], [0, 0], C, r, by)


def test_check_args_accepts_the_limits_and_the_reference_checks_its_points():
    px.check_args(1, 1, 0); px.check_args(14, 16384, 1)
    with pytest.raises(ValueError):
        px.proximity_reference([[0, 0], [1 << 27, 0]], [0, 0], 1, 5, 0)
    with pytest.raises(ValueError):
        px.proximity_reference([[0, 0], [3, 4]], [0], 1, 5, 0)
    assert px.BY == {'any': 0, 'class': 1} and px.NPZ_KEYS == ('nuclei_id', 'xy', 'label') + px.INT_NAMES + px.DERIVED_KEYS + ('radius_px', 'by_class')
    assert px.first_edge_cap(10) == 104


def test_the_capacity_protocol_on_a_stub_call():
    """cellpoints.grow_to_fit, which proximity.build, alphacomplex.build and adjacency.build run, against a call that is not the device."""
    from nuhtc_amd import cellpoints, hip
    log = []

    def stub(answers):
        answers = list(answers)

        def call(cap, out):
            log.append((cap, out))
            return answers.pop(0)
        return call

    make = lambda cap: ['out', cap]
    run = lambda answers, first_cap: cellpoints.grow_to_fit(stub(answers), make, first_cap, 'nuhtc_stub', 'stub')
    assert run([(0, 7, 3)], 10) == (['out', 10], 7, (3,), 1) and log == [(10, ['out', 10])]                  # room enough: one call
    assert run([(0, 10)], 10) == (['out', 10], 10, (), 1)                                                   # exactly enough, and nothing behind m
    del log[:]
    assert run([(0, 25, 4), (0, 25, 4)], 10) == (['out', 25], 25, (4,), 2)                                    # too small: ONE more, with room for exactly m
    assert log == [(10, ['out', 10]), (25, ['out', 25])]
    with pytest.raises(RuntimeError, match='nuhtc_stub: 26 edges on the second call, 25 on the first'):
        run([(0, 25, 4), (0, 26, 4)], 10)
    del log[:]
    with pytest.raises(ValueError, match=r'stub: 2147483648 edges, more than 2\*\*31 - 1'):
        run([(0, 1 << 31, 0)], 10)
    assert len(log) == 1                                                                                     # no second call
    assert run([(0, (1 << 31) - 1, 0), (0, (1 << 31) - 1, 0)], 10)[1] == (1 << 31) - 1
    assert cellpoints.grow_to_fit(stub([(0, 1 << 31), (0, 1 << 31)]), make, 10, 'nuhtc_stub', 'stub', limit=None)[1:] == (1 << 31, (), 2)
    with pytest.raises(ValueError, match='nuhtc_stub: invalid arguments'):
        run([(hip.E_INVALID, None, None)], 10)
    with pytest.raises(ValueError, match='nuhtc_stub: invalid arguments'):
        run([(0, 25, 4), (hip.E_INVALID, None, None)], 10)
    with pytest.raises(RuntimeError, match='nuhtc_stub failed'):
        run([(hip.E_HIP, None)], 10)
    assert cellpoints.first_edge_cap(10) == 104 and cellpoints.first_edge_cap(10, 3) == 94 and cellpoints.first_edge_cap(0) == 64


def test_npz_round_trip(tmp_path):
    p, lab, C, r, by = PC.random_small(1)
    e, d2, flag, deg, m, m_rng = px.proximity_reference(p, lab, C, r, by)
    ids = np.arange(len(p)) * 3 + 1
    path = px.write_npz(str(tmp_path / 'a_nuclei_proximity.npz'), ids, p / 2.0, lab, e, d2, flag, deg, C, r / 2, by)
    z = px.read_npz(path)
    assert tuple(z) == px.NPZ_KEYS
    assert np.array_equal(z['nuclei_id'], ids) and np.array_equal(z['xy'], p / 2.0) and np.array_equal(z['label'], lab) and z['label'].dtype == np.int64
    for name, want in zip(px.INT_NAMES, (e, d2, flag, deg)):
        assert np.array_equal(z[name], want) and z[name].dtype == want.dtype
    d = px.derive(e, d2, flag, deg, lab, C)
    for key in px.DERIVED_KEYS:
        assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype and z[key].shape == d[key].shape, key
    assert float(z['radius_px']) == r / 2 and int(z['by_class']) == 1 and int(z['n_edges']) == m and int(z['n_rng']) == m_rng
    with pytest.raises(ValueError):
        px.write_npz(str(tmp_path / 'b.npz'), ids, p / 2.0, lab, e[:, ::-1], d2, flag, deg, C, r / 2, by)      # (j, i)
    with pytest.raises(ValueError):
        px.write_npz(str(tmp_path / 'b.npz'), ids, p / 2.0, lab, e, d2, flag, deg[:-1], C, r / 2, by)
    with pytest.raises(ValueError):
        px.write_npz(str(tmp_path / 'b.npz'), ids, p / 2.0, lab, e, d2, flag, deg, C, 0.25, by)


def test_tool_flags_parse_with_their_defaults_and_bad_values_are_refused_by_main():
    spec = importlib.util.spec_from_file_location('infer_wsi_tool', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(['slide.npy', 'cfg.py', 'w.pth'])
    assert a.nuclei_proximity is False and a.proximity_radius == 64 and a.proximity_by == 'any'
    a = tool.parse_args(['slide.npy', 'cfg.py', 'w.pth', '--nuclei-proximity', '--proximity-radius', '12.5', '--proximity-by', 'class'])
    assert a.nuclei_proximity is True and a.proximity_radius == 12.5 and a.proximity_by == 'class'
    with pytest.raises(SystemExit):
        tool.parse_args(['slide.npy', 'cfg.py', 'w.pth', '--proximity-by', 'label'])
    base = ['slide.npy', 'cfg.py', 'w.pth', '--save_dir', 'out', '--nuclei-proximity']
    for bad, said in ((['--proximity-radius', '4.25'], 'half pixels'), (['--proximity-radius', '0'], 'r 1..16384'), (['--proximity-radius', '8192.5'], 'r 1..16384')):
        with pytest.raises(SystemExit, match=said):                            # refused before anything else runs, as --nuclei-mst is
            tool.main(base + bad)
