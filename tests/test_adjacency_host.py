"""Host-only checks of the territory adjacency (nuhtc_amd/adjacency.py): `adjacency_reference` against edges written out by hand on the
designed maps of tests/adjacency_cases.py and against a double loop in plain Python, the identity of its shared borders with the `contact`
table of `territory_reference`, `derive` (the empty graph included), the .npz round trip and its refusals, and the row of the table in
nuhtc_amd/slidepoints.py.  The device is compared with `adjacency_reference` in tests/test_hip_adjacency.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import adjacency_cases as AC
import territory_cases as TC
from nuhtc_amd import adjacency as adj
from nuhtc_amd import cellpoints, slidepoints
from nuhtc_amd import territory as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def double_loop(owner, n):
    """The definition word for word: every site with its right and its lower neighbour, a dictionary of the pairs."""
    own = np.asarray(owner).tolist()
    H, W = len(own), len(own[0])
    found = {}
    for v in range(H):
        for u in range(W):
            for vv, uu in ((v, u + 1), (v + 1, u)):
                if vv < H and uu < W:
                    a, b = own[v][u], own[vv][uu]
                    if a != b and a >= 0 and b >= 0:
                        found[(min(a, b), max(a, b))] = found.get((min(a, b), max(a, b)), 0) + 1
    edges = sorted(found)
    degree = [0] * n
    for i, j in edges:
        degree[i] += 1
        degree[j] += 1
    return (np.asarray(edges, np.int32).reshape(-1, 2), np.asarray([found[e] for e in edges], np.int32), np.asarray(degree, np.int32), len(edges))


# ---- the restatement
def test_the_designed_maps_against_edges_written_out_by_hand():
    cases = dict(AC.smallest(), checkerboard=AC.checkerboard(), stripes=AC.stripes(), far_apart=AC.far_apart(), long_row=AC.long_row(),
                 long_row_descending=AC.long_row(True), long_row_upright=AC.long_row(False, True))
    for name, case in cases.items():
        got = adj.adjacency_reference(case[0], case[1])
        AC.equal(got, AC.as_arrays(case), name)
        AC.equal(got, double_loop(case[0], case[1]), name + ' (double loop)')
    assert AC.checkerboard()[3] == [544] and len(AC.stripes()[2]) == 32 and AC.stripes()[3][0] == 18
    got = adj.adjacency_reference(*AC.long_row()[:2])
    assert got[2][0] == 300 and (got[2][1:] == 1).all() and got[1].tolist() == [2] * 300
    got = adj.adjacency_reference(*AC.long_row(True)[:2])
    assert got[2][300] == 300 and got[0][0].tolist() == [0, 300] and got[0][-1].tolist() == [299, 300]


def test_random_maps_against_the_double_loop_and_the_edge_cases():
    for W, H, n, free in ((9, 7, 4, 0.0), (23, 5, 60, 0.3), (1, 30, 3, 0.1), (30, 1, 3, 0.1)):
        own, n = AC.random_map(W, H, n, seed=W, free=free)[:2]
        AC.equal(adj.adjacency_reference(own, n), double_loop(own, n), f'{W} x {H}')
    edges, shared, degree, m = adj.adjacency_reference(np.full((2, 3), -1), 0)             # n = 0: nobody's
    assert edges.shape == (0, 2) and shared.shape == (0,) and degree.shape == (0,) and m == 0 and edges.dtype == shared.dtype == degree.dtype == np.int32
    for own, n in (([[0, 2]], 2), ([[0, -2]], 2), ([0, 1], 2), (np.zeros((0, 3)), 1), ([[0]], 0)):
        with pytest.raises(ValueError):
            adj.adjacency_reference(own, n)
    assert adj.first_edge_cap(0) >= 1 and adj.first_edge_cap(1000) == 3064


@pytest.mark.parametrize('name', ['patch', 'ties', 'labels', 'on_sites', 'sub-window'])
def test_shared_summed_by_class_is_the_contact_table_of_the_territories(name):
    case = dict(patch=TC.patch(4), ties=TC.ties(0), labels=TC.labels_out_of_range(), on_sites=TC.on_sites(3, 2, 5, 2))[name if name != 'sub-window' else 'patch']
    win = TC.on_sites_window(3, 5) if name == 'on_sites' else TC.default_window(case)
    if name == 'sub-window':
        win = (win[0] + 5, win[1] + 3, win[2] - 9, win[3] - 7)
    out = tr.territory_reference(*case, win)
    p, lab, C = case[:3]
    edges, shared, degree, m = adj.adjacency_reference(out[0], len(p))
    assert m > 3 and np.array_equal(adj.contact_of(edges, shared, lab, C), out[5]) and out[5].sum() == 2 * int(shared.sum())
    assert not degree[out[2] == 0].any() and (edges[:, 0] < edges[:, 1]).all()             # a row that owns nothing has no edge
    key = edges[:, 0].astype(np.int64) * len(p) + edges[:, 1]
    assert (np.diff(key) > 0).all()
    if name == 'on_sites':                                                                 # points on sites, the window their box: 4 neighbours, 3 sites of border, 2 along the rim
        inner = np.flatnonzero(out[4] == 0)
        assert len(inner) == 9 and (degree[inner] == 4).all() and set(shared.tolist()) == {2, 3} and m == 40


# ---- derive
def test_derive_properties_and_the_empty_graph():
    p, lab = TC.random_large('clumps', 400)
    r, s, C = 30, 5, 5
    win = tr.window(cellpoints.bounds_of(p), r, s)
    out = tr.territory_reference(p, lab, C, r, s, win)
    edges, shared, degree, m = adj.adjacency_reference(out[0], len(p))
    d = adj.derive(edges, shared, degree, p, lab, C, s, out[2], out[4])
    assert tuple(d) == adj.DERIVED_KEYS and all(np.isfinite(v).all() for v in d.values())
    e = edges.astype(np.int64)
    assert d['edge_d2'].dtype == np.int64 and np.array_equal(d['edge_d2'], ((p[e[:, 0]].astype(np.int64) - p[e[:, 1]]) ** 2).sum(1))
    assert np.array_equal(d['edge_px'], np.sqrt(d['edge_d2'].astype(np.float64)) / 2) and np.array_equal(d['border_px'], shared * 2.5)
    assert d['edge_px'].dtype == d['border_px'].dtype == np.float64 and d['edge_px'].max() <= 2 * 15 + 2.5 * 2
    assert d['class_edge_count'].sum() == m and not np.tril(d['class_edge_count'], -1).any() and d['class_border'].sum() == shared.sum()
    assert np.array_equal(d['class_border'] + d['class_border'].T, out[5])                 # the upper-triangle fold of contact: the diagonal counts once
    assert d['neighbour_class'].dtype == np.int32 and d['neighbour_class'].shape == (400, C) and np.array_equal(d['neighbour_class'].sum(1), degree)
    closed = (out[4] == 0) & (out[2] > 0)
    for c in range(C):
        assert d['n_closed'][c] == (closed & (lab == c)).sum()
        assert d['closed_degree_mean'][c] == (degree[closed & (lab == c)].mean() if d['n_closed'][c] else 0.0)
    assert d['n_closed'].sum() > 20 and 3 < d['closed_degree_mean'].max() < 9 and int(d['n_edges']) == m
    big = adj.derive([[0, 1]], [1], [1, 1], [[-(1 << 27) + 1, 0], [(1 << 27) - 1, 0]], [0, 0], 1, 1 << 20)   # two centres 2**28 - 2 apart
    assert int(big['edge_d2'][0]) == ((1 << 28) - 2) ** 2 > 1 << 31 and float(big['border_px'][0]) == float(1 << 19)
    empty = adj.derive(np.zeros((0, 2)), [], np.zeros(4), np.zeros((4, 2)), [0, 1, 0, 7], 2, 4, np.zeros(4), np.zeros(4))
    assert all(np.isfinite(v).all() for v in empty.values()) and empty['edge_d2'].shape == (0,) and not empty['class_edge_count'].any()
    assert not empty['neighbour_class'].any() and not empty['closed_degree_mean'].any() and int(empty['n_edges']) == 0
    nothing = adj.derive(np.zeros((0, 2)), [], [], np.zeros((0, 2)), [], 3, 4)
    assert nothing['neighbour_class'].shape == (0, 3) and all(np.isfinite(v).all() for v in nothing.values())
    for bad in (dict(degree=[1, 0]), dict(shared=[0]), dict(edges=[[0, 2]]), dict(s=0), dict(labels=[0, 5])):
        args = dict(edges=[[0, 1]], shared=[2], degree=[1, 1], points=[[0, 0], [4, 0]], labels=[0, 1], num_classes=2, s=4)
        args.update(bad)
        with pytest.raises(ValueError):
            adj.derive(**args)


def test_npz_round_trip_and_refusals(tmp_path):
    p, lab = TC.random_large('uniform', 200)
    r, s, C = 30, 8, 5
    win = tr.window(cellpoints.bounds_of(p), r, s)
    out = tr.territory_reference(p, lab, C, r, s, win)
    graph = adj.adjacency_reference(out[0], len(p))[:3]
    head = (np.arange(200) * 3, p / 2.0, lab)
    z = adj.read_npz(adj.write_npz(str(tmp_path / 'a_nuclei_adjacency.npz'), *head, graph, out[2:], win, r / 2, s / 2))
    assert tuple(z) == adj.NPZ_KEYS
    for name, want in zip(adj.INT_NAMES + tr.INT_NAMES, graph + tuple(out[2:])):
        assert np.array_equal(z[name], want) and z[name].dtype == want.dtype and z[name].shape == np.asarray(want).shape, name
    d = adj.derive(*graph, p, lab, C, s, out[2], out[4])
    for key in adj.DERIVED_KEYS:
        assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype, key
    assert float(z['reach_px']) == 15.0 and float(z['pitch_px']) == 4.0 and z['window'].tolist() == list(win) and z['window'].dtype == np.int64
    assert np.array_equal(z['nuclei_id'], np.arange(200) * 3) and z['open'].dtype == np.uint8
    path = str(tmp_path / 'c.npz')
    with pytest.raises(ValueError):
        adj.write_npz(path, *head, graph, out[2:], (win[0], win[1], win[2] + 1, win[3]), r / 2, s / 2)         # class_sites + free_sites != W * H
    with pytest.raises(ValueError):
        adj.write_npz(path, *head, (graph[0][:, ::-1], graph[1], graph[2]), out[2:], win, r / 2, s / 2)          # i > j
    with pytest.raises(ValueError):
        adj.write_npz(path, *head, (graph[0], graph[1][:-1], graph[2]), out[2:], win, r / 2, s / 2)
    with pytest.raises(ValueError, match='contact'):
        adj.write_npz(path, *head, (graph[0], graph[1] + 1, graph[2]), out[2:], win, r / 2, s / 2)              # shared no longer sums to contact
    with pytest.raises(ValueError):
        adj.write_npz(path, *head, (graph[0][:-1], graph[1][:-1], graph[2]), out[2:], win, r / 2, s / 2)        # degree is not the edges' count
    with pytest.raises(ValueError):
        adj.write_npz(path, *head, graph, out[2:], win, r / 2, 0.25)
    assert not os.path.exists(path)


# ---- the row of the table
@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('infer_wsi_for_adjacency', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(tool, *flags):
    return tool.parse_args(['slide.npy', 'config.py', 'weights.pth', *flags])


def test_the_table_has_a_fifth_tuple_directly_behind_the_plane(tool, monkeypatch):
    (row,) = slidepoints.OF_THE_BORDERS
    assert (row.cli, row.flag, row.suffix, row.module, row.second) == ('nuclei_adjacency', '--nuclei-adjacency', '_nuclei_adjacency.npz', 'adjacency', None)
    assert row._fields == slidepoints.ANALYSES[0]._fields
    plain = _args(tool)
    assert plain.nuclei_adjacency is False and (plain.adjacency_reach, plain.adjacency_pitch) == (64.0, 4.0)
    flags = ['--nuclei-enrichment', '--nuclei-adjacency', '--adjacency-pitch', '2.5', '--nuclei-territory', '--nuclei-density', '--nuclei-graph']
    chosen = slidepoints.select(_args(tool, *flags), need_gpu=False)
    assert [an.module for an, _ in chosen] == ['cellgraph', 'density', 'territory', 'adjacency', 'enrichment']
    assert dict((an.module, p) for an, p in chosen)['adjacency'] == (64.0, 2.5)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for bad in (['--adjacency-pitch', '0.25'], ['--adjacency-reach', '9000'], ['--adjacency-reach', '0'], ['--adjacency-pitch', '0']):
        with pytest.raises(SystemExit) as refused:
            slidepoints.select(_args(tool, '--nuclei-adjacency', *bad))
        assert str(refused.value).startswith('--nuclei-adjacency: ') and 'no GPU' not in str(refused.value), str(refused.value)
    with pytest.raises(SystemExit) as good:
        slidepoints.select(_args(tool, '--nuclei-adjacency'))
    assert str(good.value) == '--nuclei-adjacency: no GPU is visible (there is no fallback)'


def test_the_closing_clause_and_a_late_refusal(monkeypatch, tmp_path):
    (row,) = slidepoints.OF_THE_BORDERS
    case = TC.on_sites(3, 2, 5, 2)
    win = TC.on_sites_window(3, 5)
    out = tr.territory_reference(*case, win)
    graph = adj.adjacency_reference(out[0], 25)[:3]
    said = row.said(adj, (graph, out[2:], win), (3.0, 1.0))
    assert said == '40 territory borders between 25 nuclei on 13 x 13 sites (3 px reach, 1 px pitch; 9 closed territories, mean neighbours 4.00)', said
    none = tr.territory_reference(np.zeros((0, 2)), [], 2, 6, 2, (0, 0, 1, 1))
    assert row.said(adj, (adj.adjacency_reference(none[0], 0)[:3], none[2:], (0, 0, 1, 1)), (3.0, 1.0)).endswith('0 closed territories, mean neighbours none)')
    # a default window above the cap is refused by build, as late as the slide's own points are known: `run` says so in the flag's name
    def build(*a, **k):
        adj.check_args(2, 128, 1, (0, 0, 1 << 15, 1 << 15))
    monkeypatch.setattr(adj, 'build', build)
    boxes = np.array([[0, 0, 2, 2], [10, 10, 14, 14]], np.float64)
    with pytest.raises(SystemExit) as refused:
        slidepoints.run(((row, (64.0, 0.5)),), np.arange(2), boxes, np.array([0, 1]), 2, str(tmp_path), 's1', 0, {})
    assert str(refused.value).startswith('--nuclei-adjacency: ') and 'coarse' in str(refused.value)
