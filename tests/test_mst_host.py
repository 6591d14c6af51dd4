"""Host-only checks of the minimum spanning forest (nuhtc_amd/mst.py): `mst_reference` against an independent Prim in plain Python integers
and against hand-written forests, its total weight and edge count against scipy's minimum_spanning_tree, its `tree` partition against
scipy's connected components and clusters.cluster_reference(min_pts = 1), the cut property (the forest IS the single-linkage dendrogram up
to r), `derive` on hand-counted rows, `check_args` and the .npz round trip.  The device is compared with `mst_reference` in
tests/test_hip_mst.py."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components, minimum_spanning_tree

import mst_cases as MC
from nuhtc_amd import clusters as cl
from nuhtc_amd import mst


def prim(p, lab, C, r, by_class):
    """The unique minimum forest under the key (d2, i, j), grown tree by tree from the smallest unvisited row: Python integers, every
    pair, no union-find and no sorting of the edge list -- nothing in common with Kruskal but the definition."""
    p, lab, n = [(int(x), int(y)) for x, y in p], [int(v) for v in lab], len(p)

    def key(i, j):
        d2 = (p[i][0] - p[j][0]) ** 2 + (p[i][1] - p[j][1]) ** 2
        if d2 > r * r or (by_class and lab[i] != lab[j]):
            return None
        return (d2, min(i, j), max(i, j))
    tree, edges, t = [-1] * n, [], 0
    for start in range(n):
        if tree[start] >= 0:
            continue
        tree[start] = t
        best = {}                                              # outside row -> its smallest key into the tree
        fresh = start
        while True:
            for j in range(n):
                if tree[j] < 0:
                    k = key(fresh, j)
                    if k is not None and (j not in best or k < best[j]):
                        best[j] = k
            if not best:
                break
            fresh = min(best, key=best.get)
            edges.append(best.pop(fresh))
            tree[fresh] = t
        t += 1
    edges.sort(key=lambda e: (e[1], e[2]))
    return [[e[1], e[2]] for e in edges], [e[0] for e in edges], tree, len(edges), t


def _edge_list(p, lab, r, by_class):
    """Every edge i < j of the definition -> (i, j, d2), numpy int64."""
    p = np.asarray(p, np.int64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(2)
    ok = (d2 <= r * r) & np.triu(np.ones_like(d2, bool), 1)
    if by_class:
        ok &= np.asarray(lab)[:, None] == np.asarray(lab)[None, :]
    i, j = np.nonzero(ok)
    return i, j, d2[i, j]


def _components(n, i, j):
    g = coo_matrix((np.ones(len(i)), (i, j)), shape=(n, n))
    return connected_components(g, directed=False)[1]


def _same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.fixture(scope='module')
def references():
    return {name: mst.mst_reference(*case) for name, case in MC.small_cases().items()}


@pytest.mark.parametrize('name', sorted(MC.small_cases()))
def test_reference_equals_prim(references, name):
    e, d2, tree, m, t = references[name]
    n = len(MC.small_cases()[name][0])
    assert e.dtype == np.int32 and e.shape == (m, 2) and d2.dtype == np.int32 and d2.shape == (m,) and tree.dtype == np.int32 and tree.shape == (n,)
    want = prim(*MC.small_cases()[name])
    assert e.tolist() == want[0] and d2.tolist() == want[1] and tree.tolist() == want[2] and (m, t) == want[3:] and m == n - t


def test_reference_equals_the_hand_written_forests(references):
    for name, want in (('equidistant', MC.EQUIDISTANT_FOREST), ('collinear', MC.COLLINEAR_FOREST), ('groups', MC.GROUPS_FOREST)):
        e, d2, tree, m, t = references[name]
        assert e.tolist() == want[0] and d2.tolist() == want[1] and tree.tolist() == want[2] and m == len(want[0]) and t == max(want[2]) + 1, name
    e, d2, tree, m, t = references['edge_pairs']
    assert e.tolist() == [[0, 1]] and d2.tolist() == [100] and tree.tolist() == [0, 0, 1, 2, 3, 4]
    e, d2, tree, m, t = references['coincident']
    assert e[:299].tolist() == [[0, k] for k in range(1, 300)] and (d2[:299] == 0).all() and t == 1 and m == 304      # the star on row 0
    e, d2, tree, m, t = references['lattice']
    assert m == 63 and t == 1 and (d2 == 9).all() and e[:7].tolist() == [[0, 1], [0, 8], [1, 2], [1, 9], [2, 3], [2, 10], [3, 4]]
    assert references['interleaved_any'][4] == 1 and references['interleaved_class'][4] == 2 and (references['interleaved_class'][1] == 16).all()
    assert references['interleaved_class'][2].tolist() == [0, 1] * 10
    assert references['one_point'][2].tolist() == [0] and references['one_point'][3:] == (0, 1)
    assert references['two_points'][0].tolist() == [[0, 1]] and references['two_points_apart'][3:] == (0, 2)
    empty = mst.mst_reference(np.zeros((0, 2)), [], 3, 8, 0)
    assert empty[0].shape == (0, 2) and empty[1].shape == (0,) and empty[2].shape == (0,) and empty[3:] == (0, 0) and empty[0].dtype == np.int32


def test_chain_closed_form_is_the_reference():
    for order in ('ascending', 'descending', 'shuffled'):
        case = MC.chain(order, 300)
        got, want = mst.mst_reference(*case), MC.chain_forest(case)
        assert all(np.array_equal(g, w) and np.asarray(g).dtype == np.asarray(w).dtype for g, w in zip(got[:3], want[:3])) and got[3:] == want[3:], order


@pytest.mark.parametrize('name', sorted(MC.small_cases()))
def test_weight_partition_and_cuts_against_scipy(references, name):
    p, lab, C, r, by = MC.small_cases()[name]
    e, d2, tree, m, t = references[name]
    n = len(p)
    i, j, w = _edge_list(p, lab, r, by)
    sp = minimum_spanning_tree(coo_matrix((w + 1, (i, j)), shape=(n, n)).tocsr())      # + 1: scipy reads a weight of 0 as no edge
    assert sp.nnz == m and int(round(sp.sum())) - sp.nnz == int(d2.astype(np.int64).sum())
    assert _same_partition(tree, _components(n, i, j)) and t == len(set(tree.tolist()))
    first = {}
    for row, tr in enumerate(tree.tolist()):
        first.setdefault(tr, row)
    assert list(first) == list(range(t)) and list(first.values()) == sorted(first.values())    # numbered by ascending smallest row
    assert np.array_equal(tree, cl.cluster_reference(p, lab, C, r, 1, by)[0])
    for cut in sorted(set(np.sqrt(w).astype(int).tolist() + [0, 1, r - 1, r])):      # every t <= r at which the graph can change
        if 0 <= cut <= r:
            keep, gkeep = d2 <= cut * cut, w <= cut * cut
            assert _same_partition(_components(n, e[keep, 0], e[keep, 1]), _components(n, i[gkeep], j[gkeep])), (name, cut)


def test_derive_on_hand_counted_rows():
    # rows 0-1-2 a path with lengths 3 px and 4 px, rows 3-4 an edge of 0 px (coincident), row 5 alone; labels 0, 1, 1, 2, 7, 0 with C = 3
    d = mst.derive([[0, 1], [1, 2], [3, 4]], [36, 64, 0], [0, 0, 0, 1, 1, 2], [0, 1, 1, 2, 7, 0], 3)
    assert set(d) == set(mst.DERIVED_KEYS)
    assert d['edge_len_px'].tolist() == [3.0, 4.0, 0.0] and d['edge_len_px'].dtype == np.float64
    assert d['mst_degree'].tolist() == [1, 2, 1, 1, 1, 0] and d['mst_degree'].dtype == np.int32
    assert d['tree_size'].tolist() == [3, 2, 1] and d['tree_size'].dtype == np.int32 and d['tree_length_px'].tolist() == [7.0, 0.0, 0.0]
    assert d['edge_class_count'].tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 0]] and d['edge_class_count'].dtype == np.int64     # (2, 7) is counted nowhere
    assert int(d['n_trees']) == 3 and int(d['n_edges']) == 3 and d['n_trees'].dtype == np.int64
    lengths = np.array([3.0, 4.0, 0.0])
    assert float(d['length_mean_px']) == lengths.mean() and float(d['length_std_px']) == lengths.std() and float(d['length_min_max_ratio']) == 0.0
    assert float(d['length_disorder']) == 1 - 1 / (1 + lengths.std() / lengths.mean())
    d = mst.derive([[0, 2], [1, 2]], [4, 16], [0, 0, 0], [1, 0, 0], 2)
    assert float(d['length_min_max_ratio']) == 0.5 and d['edge_class_count'].tolist() == [[1, 1], [0, 0]] and float(d['length_mean_px']) == 1.5
    for none in (mst.derive(np.zeros((0, 2)), [], [0, 1], [0, 0], 2), mst.derive([], [], [], [], 2)):       # m = 0: zeros, never NaN
        assert all(float(none[k]) == 0.0 for k in ('length_mean_px', 'length_std_px', 'length_min_max_ratio', 'length_disorder'))
        assert none['edge_len_px'].shape == (0,) and int(none['n_edges']) == 0 and none['edge_class_count'].tolist() == [[0, 0], [0, 0]]
    assert mst.derive(np.zeros((0, 2)), [], [0, 1], [0, 0], 2)['tree_size'].tolist() == [1, 1]
    zero = mst.derive([[0, 1]], [0], [0, 0], [0, 0], 1)                                                      # every edge of length 0
    assert float(zero['length_disorder']) == 0.0 and float(zero['length_min_max_ratio']) == 0.0
    with pytest.raises(ValueError):
        mst.derive([[0, 3]], [4], [0, 0, 0], [0, 0, 0], 1)


@pytest.mark.parametrize('C, r, by', [(0, 5, 0), (15, 5, 0), (3, 0, 0), (3, 16385, 0), (3, 5, 2), (3, 5, -1), (3, 2.5, 0)])
def test_check_args_refuses(C, r, by):
    with pytest.raises(ValueError):
        mst.check_args(C, r, by)
    with pytest.raises(ValueError):
        mst.mst_reference([[0, 0], [3, 4]], [0, 0], C, r, by)


def test_check_args_accepts_the_limits_and_the_reference_checks_its_points():
    mst.check_args(1, 1, 0); mst.check_args(14, 16384, 1)
    with pytest.raises(ValueError):
        mst.mst_reference([[0, 0], [1 << 27, 0]], [0, 0], 1, 5, 0)
    with pytest.raises(ValueError):
        mst.mst_reference([[0, 0], [3, 4]], [0], 1, 5, 0)
    assert mst.BY == {'any': 0, 'class': 1} and mst.NPZ_KEYS == ('nuclei_id', 'xy', 'label') + mst.INT_NAMES + mst.DERIVED_KEYS + ('radius_px', 'by_class')


def test_npz_round_trip(tmp_path):
    p, lab, C, r, by = MC.random_small(1)
    e, d2, tree, m, t = mst.mst_reference(p, lab, C, r, by)
    ids = np.arange(len(p)) * 3 + 1
    path = mst.write_npz(str(tmp_path / 'a_nuclei_mst.npz'), ids, p / 2.0, lab, e, d2, tree, C, r / 2, by)
    z = mst.read_npz(path)
    assert tuple(z) == mst.NPZ_KEYS
    assert np.array_equal(z['nuclei_id'], ids) and np.array_equal(z['xy'], p / 2.0) and np.array_equal(z['label'], lab) and z['label'].dtype == np.int64
    for name, want in zip(mst.INT_NAMES, (e, d2, tree)):
        assert np.array_equal(z[name], want) and z[name].dtype == np.int32
    d = mst.derive(e, d2, tree, lab, C)
    for key in mst.DERIVED_KEYS:
        assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype and z[key].shape == d[key].shape, key
    assert float(z['radius_px']) == r / 2 and int(z['by_class']) == 1 and int(z['n_trees']) == t and int(z['n_edges']) == m
    with pytest.raises(ValueError):
        mst.write_npz(str(tmp_path / 'b.npz'), ids, p / 2.0, lab, e[:, ::-1], d2, tree, C, r / 2, by)      # (j, i)
    with pytest.raises(ValueError):
        mst.write_npz(str(tmp_path / 'b.npz'), ids, p / 2.0, lab, e, d2, tree[:-1], C, r / 2, by)
    with pytest.raises(ValueError):
        mst.write_npz(str(tmp_path / 'b.npz'), ids, p / 2.0, lab, e, d2, tree, C, 0.25, by)
