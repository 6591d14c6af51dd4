"""CPU tests of the cell graph's host side (nuhtc_amd/cellgraph.py): the half-pixel quantisation, `graph_reference` (the int64 restatement
the GPU tests demand equality with) on cases worked out by hand and against scipy's KD-tree, the <id>_nuclei_graph.npz round trip, and the
tool's three flags."""
import importlib.util
import os

import numpy as np
import pytest

from nuhtc_amd import cellgraph as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quantize_centres_rounds_half_to_even():
    boxes = np.array([[0.25, 0.0, 0.25, 1.0],          # x0 + x1 = 0.5 -> 0;   y0 + y1 = 1   -> 1
                      [1.0, 1.25, 0.5, 1.25],          #           1.5 -> 2;             2.5 -> 2
                      [2.0, 3.0, 1.5, 0.5],            #           3.5 -> 4;             3.5 -> 4
                      [-0.25, -1.0, -0.25, -1.5],      #          -0.5 -> -0;           -2.5 -> -2
                      [10.0, 20.0, 13.0, 27.0],        #           23;                   47    (an integer box: centre 11.5, 23.5 exactly)
                      [100.2, 7.0, 103.9, 7.3]], np.float64)
    got = cg.quantize_centres(boxes)
    assert got.dtype == np.int32 and got.shape == (6, 2)
    assert got.tolist() == [[0, 1], [2, 2], [4, 4], [0, -2], [23, 47], [204, 14]]
    assert cg.centres(boxes)[4].tolist() == [11.5, 23.5] and cg.centres(boxes).dtype == np.float64
    assert cg.quantize_centres(np.zeros((0, 4))).shape == (0, 2)
    with pytest.raises(ValueError):
        cg.quantize_centres(np.array([[2.0 ** 26, 0, 2.0 ** 26, 0]]))


def test_reference_three_collinear_points():
    # x = 0, 10, 30 half pixels; r = 20: 0 <-> 10 (d2 100), 10 <-> 30 (d2 400, exactly r^2), 0 <-> 30 (d2 900) too far
    p = np.array([[0, 5], [10, 5], [30, 5]])
    nb, d2, cc = cg.graph_reference(p, [0, 1, 1], 2, 20, 2)
    assert nb.dtype == d2.dtype == cc.dtype == np.int32
    assert nb.tolist() == [[1, -1], [0, 2], [1, -1]]
    assert d2.tolist() == [[100, -1], [100, 400], [400, -1]]
    assert cc.tolist() == [[0, 1], [1, 1], [0, 1]]
    nb1, d21, cc1 = cg.graph_reference(p, [0, 1, 1], 2, 20, 1)         # the cut at k = 1 keeps the nearer one; the census still counts both
    assert nb1.tolist() == [[1], [0], [1]] and d21.tolist() == [[100], [100], [400]] and np.array_equal(cc1, cc)


def test_reference_radius_is_inclusive_to_the_half_pixel():
    # R = 5 px = 10 half pixels; (6, 8) is at exactly 10 (a 3-4-5 triangle), (0, 11) and (7, 8) (d2 113) are just outside
    p = np.array([[0, 0], [6, 8], [0, 11], [7, 8], [0, -10]])
    nb, d2, cc = cg.graph_reference(p, [0, 0, 0, 0, 0], 1, 10, 4)
    assert nb[0].tolist() == [1, 4, -1, -1] and d2[0].tolist() == [100, 100, -1, -1] and cc[0].tolist() == [2]     # the tie at d2 = 100 by index
    assert 0 not in nb[2] and 0 not in nb[3]
    assert nb[4].tolist() == [0, -1, -1, -1]


def test_reference_coincident_points_are_neighbours():
    p = np.array([[4, 4], [4, 4], [4, 4], [5, 4]])
    nb, d2, cc = cg.graph_reference(p, [2, 0, 0, 1], 3, 1, 2)
    assert nb.tolist() == [[1, 2], [0, 2], [0, 1], [0, 1]]
    assert d2.tolist() == [[0, 0], [0, 0], [0, 0], [1, 1]]
    assert cc.tolist() == [[2, 1, 0], [1, 1, 1], [1, 1, 1], [2, 0, 1]]           # every point in the disc but the node itself; not cut at k
    # a label outside 0..C-1 is still a neighbour and is counted nowhere
    nb2, _, cc2 = cg.graph_reference(p, [2, 7, -1, 1], 3, 1, 2)
    assert np.array_equal(nb2, nb) and cc2.tolist() == [[0, 1, 0], [0, 1, 1], [0, 1, 1], [0, 0, 1]]


def test_reference_edge_sizes_and_arguments():
    for n in (0, 1):
        nb, d2, cc = cg.graph_reference(np.zeros((n, 2), np.int64), np.zeros(n, np.int64), 3, 8, 5)
        assert nb.shape == d2.shape == (n, 5) and cc.shape == (n, 3) and (nb == -1).all() and (d2 == -1).all() and not cc.any()
    p = np.array([[0, 0], [1, 0]])
    for C, r, k in ((0, 1, 1), (15, 1, 1), (1, 0, 1), (1, 16385, 1), (1, 1, 0), (1, 1, 33)):
        with pytest.raises(ValueError):
            cg.graph_reference(p, [0, 0], C, r, k)
    with pytest.raises(ValueError):
        cg.graph_reference(np.array([[1 << 27, 0], [0, 0]]), [0, 0], 1, 1, 1)
    assert cg.half_pixel_radius(64) == 128 and cg.half_pixel_radius(7.5) == 15
    with pytest.raises(ValueError):
        cg.half_pixel_radius(7.3)
    assert cg.cell_side(0, 0, 8191, 8191, 128) == 128
    side = cg.cell_side(0, 0, 1 << 22, 1 << 22, 8)                                   # the 2^22-cell cap lifts the side above the radius
    assert side % 8 == 0 and side > 8 and ((1 << 22) // side + 1) ** 2 <= 1 << 22 < ((1 << 22) // (side - 8) + 1) ** 2


def _distinct_points(n, extent):
    """n seeded random integer points whose pairwise squared distances are ALL different (so a float KD-tree has no tie to break its own
    way); reseeded until that holds."""
    for seed in range(1000):
        p = np.random.default_rng(seed).integers(0, extent, (n, 2)).astype(np.int64)
        d = p[:, None, :] - p[None, :, :]
        d2 = (d * d).sum(-1)[np.triu_indices(n, 1)]
        if len(np.unique(d2)) == len(d2) and d2.min() > 0:
            return p, seed
    raise AssertionError('no seed gave distinct distances')


def test_reference_equals_the_kdtree_on_points_with_distinct_distances():
    from scipy.spatial import cKDTree
    n, k, r, C = 500, 6, 16000, 4
    p, seed = _distinct_points(n, 1 << 18)
    d = p[:, None, :] - p[None, :, :]
    d2_all = (d * d).sum(-1)
    iu = np.triu_indices(n, 1)
    assert len(np.unique(d2_all[iu])) == n * (n - 1) // 2, seed                       # the premise, checked here
    lab = np.random.default_rng(1).integers(0, C, n)
    nb, d2, cc = cg.graph_reference(p, lab, C, r, k)
    # distances up to 2^18.5 are exact in float64 once squared (< 2^53); the radius handed to the tree is nudged up so sqrt's rounding cannot drop r itself
    dist, idx = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=k + 1, distance_upper_bound=r * (1 + 1e-12))
    assert (idx[:, 0] == np.arange(n)).all() and (dist[:, 0] == 0).all()              # distinct points: each finds itself first
    want = np.where(np.isfinite(dist[:, 1:]), idx[:, 1:], -1)
    assert 0 < (want >= 0).sum() and (want == -1).any() and (want[:, -1] >= 0).any()  # short lists and full lists both occur
    assert np.array_equal(nb, want)
    want_d2 = np.full(want.shape, -1, np.int64)
    want_d2[want >= 0] = np.rint(dist[:, 1:][want >= 0] ** 2)
    assert np.array_equal(d2, want_d2)
    within = (d2_all <= r * r) & ~np.eye(n, dtype=bool)
    assert np.array_equal(cc, np.stack([(within & (lab[None, :] == c)).sum(1) for c in range(C)], 1))


def test_npz_round_trip(tmp_path):
    nb = np.array([[1, 2], [0, -1], [-1, -1]], np.int32)
    d2 = np.array([[9, 200], [9, -1], [-1, -1]], np.int32)
    cc = np.array([[1, 1, 0], [1, 0, 0], [0, 0, 0]], np.int32)
    xy = np.array([[10.5, 3.25], [12.0, 3.25], [400.0, 9.5]])
    path = cg.write_npz(str(tmp_path / 's_nuclei_graph.npz'), [4, 7, 9], xy, nb, d2, cc, [0, 1, 2], 7.5, 2)
    z = cg.read_npz(path)
    assert set(z) == set(cg.NPZ_KEYS)
    assert z['nuclei_id'].dtype == np.int64 and z['nuclei_id'].tolist() == [4, 7, 9]
    assert z['xy'].dtype == np.float64 and np.array_equal(z['xy'], xy)
    assert z['neighbors'].dtype == np.int32 and np.array_equal(z['neighbors'], nb)
    assert z['dist'].dtype == np.float32 and z['dist'].shape == (3, 2)
    assert np.array_equal(np.isinf(z['dist']), nb == -1) and (z['dist'][nb == -1] > 0).all()
    assert z['dist'][0].tolist() == [1.5, float(np.float32(np.sqrt(200.0) / 2))] and z['dist'][1, 0] == 1.5
    assert z['class_count'].dtype == np.int32 and np.array_equal(z['class_count'], cc)
    assert z['label'].dtype == np.int64 and z['label'].tolist() == [0, 1, 2]
    assert z['radius_px'].shape == () and float(z['radius_px']) == 7.5 and z['k'].shape == () and int(z['k']) == 2
    with pytest.raises(ValueError):
        cg.write_npz(str(tmp_path / 'bad.npz'), [4, 7, 9], xy, nb, np.where(d2 < 0, 0, d2), cc, [0, 1, 2], 7.5, 2)
    empty = cg.read_npz(cg.write_npz(str(tmp_path / 'e.npz'), [], np.zeros((0, 2)), np.zeros((0, 8)), np.zeros((0, 8)), np.zeros((0, 5)), [], 64, 8))
    assert empty['neighbors'].shape == (0, 8) and empty['dist'].shape == (0, 8) and empty['class_count'].shape == (0, 5)


def test_tool_flags_parse_with_their_defaults():
    spec = importlib.util.spec_from_file_location('infer_wsi_tool', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(['slide.npy', 'cfg.py', 'w.pth'])
    assert a.nuclei_graph is False and a.graph_radius == 64 and a.graph_k == 8 and a.nuclei_feat is False
    a = tool.parse_args(['slide.npy', 'cfg.py', 'w.pth', '--nuclei-graph', '--graph-radius', '24.5', '--graph-k', '12'])
    assert a.nuclei_graph is True and a.graph_radius == 24.5 and a.graph_k == 12
    helps = {act.dest: act.help for act in tool.build_parser()._actions}
    assert '16 um at 40x' in helps['graph_radius']
