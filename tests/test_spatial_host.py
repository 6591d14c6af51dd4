"""CPU tests of the spatial statistics' host side (nuhtc_amd/spatial.py): `spatial_reference` (the int64 restatement the GPU tests demand
equality with) against a plain double loop in Python integers, hand counts on a lattice whose distances sit on and beside the bin edges,
and scipy's KD-tree; `derive`; the <id>_nuclei_spatial.npz round trip; and the tool's three flags."""
import importlib.util
import os

import numpy as np
import pytest

from nuhtc_amd import spatial as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _double_loop(p, lab, C, edges):
    """The definition in Python integers, pair by pair."""
    p, lab, e = [[int(v) for v in q] for q in p], [int(v) for v in lab], [int(v) for v in edges]
    n, B = len(p), len(e)
    hist = [[[0] * B for _ in range(C)] for _ in range(C)]
    nn = [[-1] * C for _ in range(n)]
    cn = [sum(1 for v in lab if v == c) for c in range(C)]
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            d2 = (p[i][0] - p[j][0]) ** 2 + (p[i][1] - p[j][1]) ** 2
            t = next((t for t in range(B) if d2 <= e[t] * e[t]), None)
            if t is None or not 0 <= lab[j] < C:
                continue
            if nn[i][lab[j]] < 0 or d2 < nn[i][lab[j]]:
                nn[i][lab[j]] = d2
            if 0 <= lab[i] < C:
                hist[lab[i]][lab[j]][t] += 1
    return np.array(hist, np.int64).reshape(C, C, B), np.array(nn, np.int32).reshape(n, C), np.array(cn, np.int64)


def _lattice():
    """The 12 x 12 lattice of tests/test_hip_cellgraph.py: pitch 12 half pixels, row-major; labels cycle through 0..3."""
    gy, gx = np.mgrid[0:12, 0:12]
    p = np.stack([gx.ravel() * 12 + 40, gy.ravel() * 12 + 24], 1).astype(np.int32)
    return p, (np.arange(144) % 4).astype(np.int32)


def test_reference_equals_a_double_loop_with_labels_out_of_range():
    rng = np.random.default_rng(7)
    p = rng.integers(-60, 60, (150, 2))
    p[10] = p[11] = p[12]                                          # coincident points: d2 = 0, bin 0
    lab = rng.integers(-1, 5, 150)                                 # -1 and 4 lie outside 0..3
    edges = [3, 7, 8, 20, 41]
    got = sp.spatial_reference(p, lab, 4, edges)
    want = _double_loop(p, lab, 4, edges)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int64
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)
    assert got[0][:, :, 0].sum() >= 6 and (got[1][(lab < 0) | (lab > 3)] >= 0).any()      # rows of unlabelled points are still written
    assert got[2].sum() == ((lab >= 0) & (lab < 4)).sum()


def test_reference_lattice_hand_counts_on_the_edges():
    # ordered pairs of the 12 x 12 lattice by offset (a, b): (12 - |a|) (12 - |b|) each.  d2 / 144 = 1 (528 pairs) lies exactly on the
    # edge 12; 2 (d2 = 288 = 17^2 - 1: 484) falls in bin 1; 4 (d2 = 576 = 24^2, on the edge: 480) in bin 2; 5 (880) and 8 (400) in bin 3;
    # 9 (d2 = 1296 > 34^2 = 1156) has no bin
    p, lab = _lattice()
    ph, nn, cn = sp.spatial_reference(p, lab, 4, [12, 17, 24, 34])
    assert ph.sum(axis=(0, 1)).tolist() == [528, 484, 480, 1280]
    assert cn.tolist() == [36, 36, 36, 36]
    i = 5 * 12 + 6                       # interior, label 2: the row's neighbours carry 1 and 3, the column's 2, the diagonals 1 and 3; 0 sits two along the row
    assert nn[i].tolist() == [576, 144, 144, 144]
    for g, w in zip((ph, nn, cn), _double_loop(p, lab, 4, [12, 17, 24, 34])):
        assert np.array_equal(g, w)
    one = sp.spatial_reference(p, lab, 4, [11])                    # nothing within 11 half pixels
    assert one[0].sum() == 0 and (one[1] == -1).all()


def test_reference_against_a_kd_tree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(3)
    p = 2 * rng.integers(0, 1000, (600, 2)) + 1                    # odd coordinates: every d2 is a multiple of 4 ...
    lab = rng.integers(0, 3, 600)
    edges = np.array([41, 91, 131, 201])                           # ... and every squared radius is odd
    ph, nn, cn = sp.spatial_reference(p, lab, 3, edges)
    d2_all = ((p[:, None, :] - p[None, :, :]).astype(np.int64) ** 2).sum(-1)
    assert not np.isin(d2_all, edges.astype(np.int64) ** 2).any()                      # no pair distance equals a radius: float compares are safe
    trees = [cKDTree(p[lab == c].astype(np.float64)) for c in range(3)]
    for a in range(3):
        for b in range(3):
            cum = trees[a].count_neighbors(trees[b], edges.astype(np.float64))
            if a == b:
                cum = cum - cn[a]                                                       # the tree counts every point with itself
            assert np.array_equal(np.cumsum(ph[a, b]), cum), (a, b)
    for c in range(3):
        dist, _ = trees[c].query(p.astype(np.float64), k=2)
        near = np.where(lab == c, dist[:, 1], dist[:, 0]) ** 2                          # a point of class c skips itself
        want = np.where(near <= 201.0 ** 2, np.rint(near), -1).astype(np.int32)
        assert np.array_equal(nn[:, c], want), c


def test_reference_and_check_args_refuse_bad_arguments():
    p, lab = _lattice()
    for edges in ([], list(range(1, 34)), [5, 5], [9, 4], [0, 4], [4, 16385], [2.5, 4]):
        with pytest.raises(ValueError):
            sp.spatial_reference(p, lab, 4, edges)
    for C in (0, 15):
        with pytest.raises(ValueError):
            sp.spatial_reference(p, lab, C, [4])
    with pytest.raises(ValueError):
        sp.spatial_reference(p, lab[:-1], 4, [4])
    with pytest.raises(ValueError):
        sp.spatial_reference([[1 << 27, 0]], [0], 1, [4])
    assert sp.check_args(14, list(range(1, 33))).dtype == np.int32 and sp.check_args(1, [16384]).tolist() == [16384]
    empty = sp.spatial_reference(np.zeros((0, 2)), [], 2, [4, 8])
    assert empty[0].shape == (2, 2, 2) and empty[1].shape == (0, 2) and empty[2].tolist() == [0, 0]


def test_derive_cumulative_mean_g_and_k_only_with_an_area():
    # class 0: three points on a line 6 apart; class 1: one point 8 above the first; class 2 is absent
    p = np.array([[0, 0], [6, 0], [12, 0], [0, 8]])
    lab = np.array([0, 0, 0, 1])
    edges = [6, 10, 13]
    ph, nn, cn = sp.spatial_reference(p, lab, 3, edges)
    assert ph[0, 0].tolist() == [4, 0, 2] and ph[0, 1].tolist() == [0, 2, 0] and ph[1, 0].tolist() == [0, 2, 0]      # (6, 8): d2 100 = 10^2; (12, 8): 208 > 169
    d = sp.derive(ph, nn, lab, cn, edges)
    assert set(d) == {'cumulative', 'mean_within', 'G'}
    assert d['cumulative'].dtype == np.int64 and d['cumulative'][0, 0].tolist() == [4, 4, 6] and d['cumulative'][0, 1].tolist() == [0, 2, 2]
    assert d['mean_within'].dtype == np.float64
    assert d['mean_within'][0, 0].tolist() == [4 / 3, 4 / 3, 2.0] and d['mean_within'][1, 0].tolist() == [0.0, 2.0, 2.0]
    # G[0][1]: the nearest class-1 point of the three class-0 points lies at d2 = 64, 100 and none
    assert nn[:3, 1].tolist() == [64, 100, -1]
    assert d['G'][0, 1].tolist() == [0.0, 2 / 3, 2 / 3] and d['G'][0, 0].tolist() == [1.0, 1.0, 1.0] and d['G'][1, 0].tolist() == [0.0, 1.0, 1.0]
    assert d['G'][1, 1].tolist() == [0.0, 0.0, 0.0]
    for key in ('mean_within', 'G'):                                                   # the absent class: zeros, nothing undefined
        assert np.isfinite(d[key]).all() and (d[key][2] == 0).all() and (d[key][:, 2] == 0).all()
    k = sp.derive(ph, nn, lab, cn, edges, area_px=600.0)
    assert set(k) == {'cumulative', 'mean_within', 'G', 'K', 'L'}
    assert np.isfinite(k['K']).all() and np.isfinite(k['L']).all() and (k['K'][2] == 0).all() and (k['K'][:, 2] == 0).all()
    assert k['K'][0, 1].tolist() == [0.0, 600.0 * 2 / 3, 600.0 * 2 / 3] and k['K'][0, 0, 2] == 600.0 * 6 / 9
    assert np.array_equal(k['L'], np.sqrt(k['K'] / np.pi))
    for key in ('cumulative', 'mean_within', 'G'):
        assert np.array_equal(k[key], d[key])


def test_npz_round_trip(tmp_path):
    p = np.array([[0, 0], [6, 0], [12, 0], [0, 8]])
    lab = np.array([0, 0, 0, 1])
    edges = [6, 10, 13]
    ph, nn, cn = sp.spatial_reference(p, lab, 3, edges)
    xy = p / 2 + 0.25
    path = sp.write_npz(str(tmp_path / 's_nuclei_spatial.npz'), [4, 7, 9, 11], xy, lab, edges, ph, nn, cn, tiles_area_px=600.0)
    z = sp.read_npz(path)
    assert set(z) == set(sp.NPZ_KEYS)
    for key in ('nuclei_id', 'xy', 'label', 'edges_px', 'pair_hist', 'nn_dist', 'class_n', 'nn_d2', 'mean_within', 'G', 'tiles_area_px'):
        assert key in z
    assert z['nuclei_id'].dtype == np.int64 and z['nuclei_id'].tolist() == [4, 7, 9, 11]
    assert z['xy'].dtype == np.float64 and np.array_equal(z['xy'], xy)
    assert z['label'].dtype == np.int64 and z['label'].tolist() == [0, 0, 0, 1]
    assert z['edges_px'].dtype == np.float64 and z['edges_px'].tolist() == [3.0, 5.0, 6.5]
    assert z['pair_hist'].dtype == np.int64 and np.array_equal(z['pair_hist'], ph)
    assert z['class_n'].dtype == np.int64 and z['class_n'].tolist() == [3, 1, 0]
    assert z['nn_d2'].dtype == np.int32 and np.array_equal(z['nn_d2'], nn)
    assert z['nn_dist'].dtype == np.float32 and z['nn_dist'].shape == (4, 3)
    assert np.array_equal(np.isinf(z['nn_dist']), nn == -1) and z['nn_dist'][0].tolist() == [3.0, 4.0, float('inf')]
    d = sp.derive(ph, nn, lab, cn, edges, area_px=600.0)
    assert np.array_equal(z['mean_within'], d['mean_within']) and np.array_equal(z['G'], d['G'])
    assert z['tiles_area_px'].shape == () and float(z['tiles_area_px']) == 600.0
    assert np.array_equal(z['K_tiles_area'], d['K']) and np.array_equal(z['L_tiles_area'], d['L'])
    with pytest.raises(ValueError):
        sp.write_npz(str(tmp_path / 'bad.npz'), [4, 7, 9], xy, lab, edges, ph, nn, cn, tiles_area_px=600.0)
    e = sp.read_npz(sp.write_npz(str(tmp_path / 'e.npz'), [], np.zeros((0, 2)), [], [4, 8], np.zeros((5, 5, 2)), np.zeros((0, 5)), np.zeros(5), 0.0))
    assert e['nn_dist'].shape == (0, 5) and e['G'].shape == (5, 5, 2) and np.isfinite(e['K_tiles_area']).all()


def test_tool_flags_parse_with_their_defaults_and_the_step_is_half_pixels():
    spec = importlib.util.spec_from_file_location('infer_wsi_tool', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(['slide.npy', 'cfg.py', 'w.pth'])
    assert a.nuclei_spatial is False and a.spatial_step == 8 and a.spatial_bins == 32 and a.nuclei_graph is False
    a = tool.parse_args(['slide.npy', 'cfg.py', 'w.pth', '--nuclei-spatial', '--spatial-step', '4.5', '--spatial-bins', '8'])
    assert a.nuclei_spatial is True and a.spatial_step == 4.5 and a.spatial_bins == 8
    helps = {act.dest: act.help for act in tool.build_parser()._actions}
    assert '64 um at 40x' in helps['spatial_bins']
    e = sp.edges_from_step(8, 32)                                                      # the default: 16 half pixels a bin, 256 px reach
    assert e.dtype == np.int32 and e.tolist() == [16 * b for b in range(1, 33)] and e[-1] == 512
    assert sp.edges_from_step(4.5, 8).tolist() == [9 * b for b in range(1, 9)]
    for step, bins in ((4.25, 8), (0, 8), (-2, 8), (8, 0), (8, 33), (300, 32)):
        with pytest.raises(ValueError):
            sp.edges_from_step(step, bins)
    with pytest.raises(SystemExit, match='half pixels'):                               # refused before anything else runs
        tool.main(['slide.npy', 'cfg.py', 'w.pth', '--save_dir', 'out', '--nuclei-spatial', '--spatial-step', '4.25'])
