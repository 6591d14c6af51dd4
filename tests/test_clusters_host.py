"""Host-only checks of the nucleus clusters (nuhtc_amd/clusters.py): `cluster_reference` against a plain double loop in Python integers
with a textbook union-find, hand-counted rows, scikit-learn's DBSCAN (core set, noise set and the partition of the core points: border
points are DBSCAN's to choose), scipy's connected components, `derive`, the .npz round trip and the tool's flags.  The device is compared
with `cluster_reference` in tests/test_hip_clusters.py."""
import importlib.util
import os

import numpy as np
import pytest

import clusters_cases as CC
from nuhtc_amd import cellgraph
from nuhtc_amd import clusters as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def double_loop(p, lab, C, r, min_pts, by_class):
    """The definition read out loud: Python integers, every pair, a union-find with path compression."""
    p, lab, n = [(int(x), int(y)) for x, y in p], [int(v) for v in lab], len(p)
    d2 = lambda i, j: (p[i][0] - p[j][0]) ** 2 + (p[i][1] - p[j][1]) ** 2
    adj = lambda i, j: d2(i, j) <= r * r and (not by_class or lab[i] == lab[j])
    degree = [sum(adj(i, j) for j in range(n)) for i in range(n)]
    core = [d >= min_pts for d in degree]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i in range(n):
        for j in range(i):
            if core[i] and core[j] and adj(i, j):
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    root = [-1] * n
    for i in range(n):
        if core[i]:
            root[i] = find(i)
        else:
            near = [(d2(i, j), j) for j in range(n) if core[j] and adj(i, j)]
            if near:
                root[i] = find(min(near)[1])
    roots = sorted(set(x for x in root if x >= 0))
    cluster = [roots.index(x) if x >= 0 else -1 for x in root]
    m = len(roots)
    size, n_core, cc = [0] * m, [0] * m, [[0] * C for _ in range(m)]
    sxy, bb = [[0, 0] for _ in range(m)], [[2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, -2 ** 31] for _ in range(m)]
    for i, c in enumerate(cluster):
        if c < 0:
            continue
        size[c] += 1
        n_core[c] += core[i]
        if 0 <= lab[i] < C:
            cc[c][lab[i]] += 1
        sxy[c][0] += p[i][0]
        sxy[c][1] += p[i][1]
        bb[c] = [min(bb[c][0], p[i][0]), min(bb[c][1], p[i][1]), max(bb[c][2], p[i][0]), max(bb[c][3], p[i][1])]
    return (np.array(cluster, np.int32), np.array(core, np.uint8), np.array(degree, np.int32), np.array(size, np.int32), np.array(n_core, np.int32),
            np.array(cc, np.int32).reshape(m, C), np.array(sxy, np.int64).reshape(m, 2), np.array(bb, np.int32).reshape(m, 4))


def _equal(got, want, what):
    for name, g, w in zip(cl.INT_NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (what, name, g.tolist()[:40], w.tolist()[:40])


@pytest.mark.parametrize('name', sorted(CC.small_cases()))
def test_reference_against_a_double_loop_in_python_integers(name):
    case = CC.small_cases()[name]
    _equal(cl.cluster_reference(*case), double_loop(*case), name)
    far = CC.translate(case, (1 << 26) + 12345, -(1 << 26) - 321)
    moved = cl.cluster_reference(*far)
    _equal(moved[:6], cl.cluster_reference(*case)[:6], name + ' translated')
    _equal(moved, double_loop(*far), name + ' translated, against the loop')


@pytest.mark.parametrize('order', ['descending', 'shuffled'])
def test_a_chain_in_another_row_order_is_the_ascending_result_permuted(order):
    asc, case = cl.cluster_reference(*CC.chain('ascending', n=300)), CC.chain(order, n=300)
    got = cl.cluster_reference(*case)
    _equal(got, double_loop(*case), order)
    k = (case[0][:, 0] + 7) // case[3]
    _equal(got, tuple(a[k] for a in asc[:3]) + asc[3:], order + ' against ascending')
    assert (got[0] == 0).all() and got[3].tolist() == [300]


def test_hand_counted_rows():
    c, core, deg, size, n_core, cc, sxy, bb = cl.cluster_reference(*CC.edge_pairs())
    assert deg.tolist() == [2, 2, 1, 1] and core.tolist() == [1, 1, 0, 0] and c.tolist() == [0, 0, -1, -1]           # 100 <= 100, 117 > 100
    assert size.tolist() == [2] and n_core.tolist() == [2] and cc.tolist() == [[1, 1]] and sxy.tolist() == [[6, 8]] and bb.tolist() == [[0, 0, 6, 8]]
    c, core, deg, size, n_core, cc, sxy, bb = cl.cluster_reference(*CC.min_pts_threshold())
    assert deg.tolist() == [3, 2, 2] + [4, 2, 2, 2] + [5, 2, 2, 2, 2]          # min_pts - 2 others, min_pts - 1 others, min_pts others
    assert core.tolist() == [0, 0, 0] + [1, 0, 0, 0] + [1, 0, 0, 0, 0]
    assert c.tolist() == [-1] * 3 + [0] * 4 + [1] * 5 and size.tolist() == [4, 5] and n_core.tolist() == [1, 1]
    assert sxy.tolist() == [[4000, 10], [10000, 0]] and bb.tolist() == [[990, 0, 1010, 10], [1990, -10, 2010, 10]]
    # the bridge: a border point of both clusters joins one and connects neither
    p, lab, C, r, k, by = CC.bridge_equidistant()
    c, core, deg = cl.cluster_reference(p, lab, C, r, k, by)[:3]
    b = int(np.nonzero((p == [10, 0]).all(1))[0][0])
    assert deg[b] == 3 and core[b] == 0 and core.sum() == 10 and c.max() == 1
    assert (p[1] == [20, 0]).all() and (p[2] == [0, 0]).all() and c[0] == 0 and c[2] == 0 and c[1] == 1 and c[b] == 1      # row 1 < row 2
    p, lab, C, r, k, by = CC.bridge_nearer_later()
    c, core, deg = cl.cluster_reference(p, lab, C, r, k, by)[:3]
    assert deg[10] == 3 and core[10] == 0 and c[0] == 0 and c[5] == 1 and c[10] == 1 and c.max() == 1                         # 81 < 121
    # two classes on the same positions
    assert cl.cluster_reference(*CC.interleaved_classes(0))[0].tolist() == [0] * 20
    assert cl.cluster_reference(*CC.interleaved_classes(1))[0].tolist() == [0, 1] * 10
    assert cl.cluster_reference(*CC.interleaved_classes(1))[1].tolist() == [0, 0] + [1] * 16 + [0, 0]
    got = cl.cluster_reference(*CC.labels_out_of_range(1))
    assert got[5][:, [0, 2]].sum() == 0 and (got[5].sum(1) < got[3]).any() and got[3].sum() > got[5].sum()


@pytest.mark.parametrize('seed, n, extent, r, min_pts', [(0, 600, 400, 14, 5), (1, 900, 500, 16, 4), (2, 500, 200, 9, 8), (3, 700, 900, 40, 3)])
def test_core_set_noise_set_and_core_partition_against_scikit_learn(seed, n, extent, r, min_pts):
    DBSCAN = pytest.importorskip('sklearn.cluster').DBSCAN
    rng = np.random.default_rng(seed)
    p = rng.integers(0, extent, (n, 2))
    c, core, deg = cl.cluster_reference(p, np.zeros(n), 1, r, min_pts, 0)[:3]
    sk = DBSCAN(eps=float(r), min_samples=min_pts, algorithm='brute').fit(p.astype(np.float64))      # integer d2 <= 2^21: exact in float64
    sk_core = np.zeros(n, bool)
    sk_core[sk.core_sample_indices_] = True
    assert np.array_equal(core.astype(bool), sk_core) and 0 < core.sum() < n
    assert np.array_equal(c == -1, sk.labels_ == -1) and (c == -1).any()
    ours, theirs = c[sk_core], sk.labels_[sk_core]                             # the same partition up to relabelling: a bijection
    pairs = set(zip(ours.tolist(), theirs.tolist()))
    assert len(pairs) == len(set(ours.tolist())) == len(set(theirs.tolist())) and len(pairs) > 1
    print(f'seed {seed}: {len(pairs)} clusters, {int(core.sum())} core, {int((c == -1).sum())} noise, {int((~sk_core & (c >= 0)).sum())} border points')


@pytest.mark.parametrize('seed', [0, 1])
def test_min_pts_one_is_connected_components_against_scipy(seed):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(100 + seed)
    n, r = 800, 13                                                             # 169 = 5^2 + 12^2: pairs exactly at r exist, and are removed
    p = rng.integers(0, 400, (n, 2))
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    p = p[~(d2 == r * r).any(1)]
    n = len(p)
    assert n > 400
    pairs = cKDTree(p.astype(np.float64)).query_pairs(float(r), output_type='ndarray')
    m, lab = connected_components(coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n)), directed=False)
    c, core, deg, size = cl.cluster_reference(p, np.zeros(n), 1, r, 1, 0)[:4]
    assert core.all() and (c >= 0).all() and len(size) == m and 1 < m < n
    first = np.full(m, n)
    np.minimum.at(first, lab, np.arange(n))                                    # scipy's components, renumbered by their smallest row
    assert np.array_equal(c, np.argsort(np.argsort(first))[lab])
    assert np.array_equal(size, np.bincount(c))


def test_a_lattice_wider_than_the_radius_with_min_pts_one_is_one_cluster_per_row():
    """The construction of tests/test_hip_cellpoints.py (the root numbering across scan chunks) at n = 40: spacing 3 r, rows shuffled."""
    n, r = 40, 8
    at = np.arange(n)
    p = (np.stack([at % 7, at // 7], 1) * 3 * r - 1000)[np.random.default_rng(5).permutation(n)]
    lab = np.arange(n) % 3
    cluster, core, degree, size, n_core, class_count, sum_xy, bbox = cl.cluster_reference(p, lab, 3, r, 1, 0)
    assert len(size) == n and np.array_equal(cluster, np.arange(n)) and core.all() and (degree == 1).all()
    assert (size == 1).all() and (n_core == 1).all() and np.array_equal(class_count, np.eye(3, dtype=np.int32)[lab])
    assert np.array_equal(sum_xy, p) and np.array_equal(bbox, np.concatenate([p, p], 1))


def test_derive_against_numpy_on_a_small_table():
    p, lab, C = np.array([[0, 0], [6, 8], [3, 3], [100, 0], [300, 1], [301, 4], [299, 0]]), np.array([0, 1, 1, 2, 5, 1, 1]), 4
    out = cl.cluster_reference(p, lab, C, 10, 2, 0)
    c, core, deg, size, n_core, cc, sxy, bb = out
    assert c.tolist() == [0, 0, 0, -1, 1, 1, 1] and size.tolist() == [3, 3]
    d = cl.derive(c, lab, C, size, cc, sxy, bb)
    assert set(d) == set(cl.DERIVED_KEYS) and all(d[k].dtype == np.float64 for k in ('centroid_px', 'bbox_px', 'class_fraction', 'class_clustered_share'))
    assert d['centroid_px'].tolist() == [[9 / 6, 11 / 6], [900 / 6, 5 / 6]]
    assert d['bbox_px'].tolist() == [[0.0, 0.0, 3.0, 4.0], [149.5, 0.0, 150.5, 2.0]]
    assert d['class_fraction'].tolist() == [[1 / 3, 2 / 3, 0.0, 0.0], [0.0, 2 / 3, 0.0, 0.0]]          # label 5 is in no class
    assert int(d['n_clusters']) == 2 and int(d['n_noise']) == 1
    assert d['class_n'].tolist() == [1, 4, 1, 0] and d['class_clustered'].tolist() == [1, 4, 0, 0]
    assert d['class_clustered_share'].tolist() == [1.0, 1.0, 0.0, 0.0] and np.isfinite(d['class_clustered_share']).all()
    e = cl.derive(np.full(3, -1), [0, 1, 1], 2, np.zeros(0), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 4)))
    assert e['centroid_px'].shape == (0, 2) and int(e['n_noise']) == 3 and e['class_clustered_share'].tolist() == [0.0, 0.0]


def test_npz_round_trip(tmp_path):
    p, lab, C = np.array([[0, 0], [6, 8], [3, 3], [100, 0], [300, 1], [301, 4], [299, 0]]), np.array([0, 1, 1, 2, 5, 1, 1]), 4
    out = cl.cluster_reference(p, lab, C, 10, 2, 1)
    ids, xy = [3, 4, 8, 9, 11, 12, 20], p / 2 + 0.25
    path = cl.write_npz(str(tmp_path / 's_nuclei_clusters.npz'), ids, xy, lab, *out, radius_px=5.0, min_pts=2, by_class=1)
    z = cl.read_npz(path)
    assert set(z) == set(cl.NPZ_KEYS) and {'cluster', 'core', 'degree', 'size', 'n_core', 'class_count', 'sum_xy', 'bbox', 'centroid_px'} <= set(z)
    assert z['nuclei_id'].dtype == np.int64 and z['nuclei_id'].tolist() == ids and z['xy'].dtype == np.float64 and np.array_equal(z['xy'], xy)
    assert z['label'].dtype == np.int64 and z['label'].tolist() == lab.tolist()
    for name, want in zip(cl.INT_NAMES, out):
        assert z[name].dtype == want.dtype and np.array_equal(z[name], want), name
    assert z['sum_xy'].dtype == np.int64 and z['core'].dtype == np.uint8 and z['cluster'].dtype == np.int32
    d = cl.derive(out[0], lab, C, out[3], out[5], out[6], out[7])
    for key in cl.DERIVED_KEYS:
        assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype, key
    assert float(z['radius_px']) == 5.0 and int(z['min_pts']) == 2 and int(z['by_class']) == 1 and z['radius_px'].shape == ()
    with pytest.raises(ValueError):
        cl.write_npz(str(tmp_path / 'bad.npz'), ids[:-1], xy, lab, *out, radius_px=5.0, min_pts=2, by_class=1)
    with pytest.raises(ValueError):
        cl.write_npz(str(tmp_path / 'bad.npz'), ids, xy, lab, *out[:3], out[3][:-1], *out[4:], radius_px=5.0, min_pts=2, by_class=1)
    none = cl.cluster_reference(np.zeros((0, 2)), [], 5, 64, 5, 0)
    e = cl.read_npz(cl.write_npz(str(tmp_path / 'e.npz'), [], np.zeros((0, 2)), [], *none, radius_px=32, min_pts=5, by_class=0))
    assert e['cluster'].shape == (0,) and e['class_count'].shape == (0, 5) and int(e['n_clusters']) == 0 and e['class_clustered_share'].tolist() == [0.0] * 5


def test_arguments_out_of_range_are_refused():
    p, lab = np.array([[0, 0], [3, 4]]), np.array([0, 1])
    for C, r, k, by in ((0, 5, 2, 0), (15, 5, 2, 0), (2, 0, 2, 0), (2, 16385, 2, 0), (2, 5, 0, 0), (2, 5, -3, 0), (2, 5, 2, 2), (2, 5, 2, -1), (2, 5.5, 2, 0)):
        with pytest.raises(ValueError):
            cl.cluster_reference(p, lab, C, r, k, by)
        with pytest.raises(ValueError):
            cl.check_args(C, r, k, by)
    cl.check_args(14, 16384, 1, 1)
    with pytest.raises(ValueError):
        cl.cluster_reference(p, lab[:1], 2, 5, 2, 0)
    with pytest.raises(ValueError):
        cl.cluster_reference([[1 << 27, 0]], [0], 1, 4, 1, 0)
    assert cl.quantize_centres is cellgraph.quantize_centres and cl.cell_side is cellgraph.cell_side and cl.half_pixel_radius is cellgraph.half_pixel_radius


def test_tool_flags_parse_with_their_defaults_and_bad_values_are_refused_by_main():
    spec = importlib.util.spec_from_file_location('infer_wsi_tool', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(['slide.npy', 'cfg.py', 'w.pth'])
    assert a.nuclei_clusters is False and a.cluster_radius == 32 and a.cluster_min == 5 and a.cluster_by == 'any'
    a = tool.parse_args(['slide.npy', 'cfg.py', 'w.pth', '--nuclei-clusters', '--cluster-radius', '12.5', '--cluster-min', '3', '--cluster-by', 'class'])
    assert a.nuclei_clusters is True and a.cluster_radius == 12.5 and a.cluster_min == 3 and a.cluster_by == 'class'
    helps = {act.dest: act.help for act in tool.build_parser()._actions}
    assert '8 um at 40x' in helps['cluster_radius']
    with pytest.raises(SystemExit):
        tool.parse_args(['slide.npy', 'cfg.py', 'w.pth', '--cluster-by', 'label'])
    base = ['slide.npy', 'cfg.py', 'w.pth', '--save_dir', 'out', '--nuclei-clusters']
    for bad, said in ((['--cluster-radius', '4.25'], 'half pixels'), (['--cluster-radius', '0'], 'r 1..16384'), (['--cluster-radius', '8192.5'], 'r 1..16384'),
                      (['--cluster-min', '0'], 'min_pts >= 1')):
        with pytest.raises(SystemExit, match=said):                            # refused before anything else runs
            tool.main(base + bad)
