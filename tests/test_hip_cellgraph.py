"""GPU tests of the cell graph (csrc/cellgraph.hip, nuhtc_cell_graph): every result must EQUAL nuhtc_amd.cellgraph.graph_reference, the
brute-force int64 restatement of the definition -- no tolerance, nothing left out.  Designed point sets (a lattice full of ties, coincident
points in one cell, slide-scale offsets, a grid whose 2^22-cell cap lifts the cell side above the radius), the edge sizes and the refused
arguments, bitwise repeatability, and tools/infer_wsi.py --nuclei-graph end to end."""
import json
import os

import numpy as np
import pytest
import torch

import points_util
from nuhtc_amd import cellgraph as cg
from nuhtc_amd import hip, nucfeat

pytestmark = pytest.mark.gpu


def _equal(got, want, what):
    for name, g, w in zip(('neighbors', 'd2', 'class_count'), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert len(bad) == 0, (what, name, f'{len(bad)} rows differ, first {int(bad[0])}', g[bad[0]].tolist(), w[bad[0]].tolist())


# ---- 1, 2: the lattice
def _lattice():
    """12 x 12 points 6 px = 12 half pixels apart, row-major; labels cycle through 0..3."""
    gy, gx = np.mgrid[0:12, 0:12]
    p = np.stack([gx.ravel() * 12 + 40, gy.ravel() * 12 + 24], 1).astype(np.int32)
    return p, (np.arange(144) % 4).astype(np.int32)


def test_lattice_ties_inclusive_radius_and_the_cut_at_k(hip_device):
    p, lab = _lattice()
    got = cg.build(p, lab, 4, 12, 8)
    _equal(got, cg.graph_reference(p, lab, 4, 24, 8), 'lattice R = 12 k = 8')
    nb, d2, cc = got
    i = 5 * 12 + 6                                                 # an interior point: 4 at 6 px, 4 at 6 sqrt(2) px, 4 at exactly 12 px
    assert d2[i].tolist() == [144] * 4 + [288] * 4                 # ... of which k = 8 keep the first two rings, ties by index
    assert nb[i].tolist() == [i - 12, i - 1, i + 1, i + 12, i - 13, i - 11, i + 11, i + 13]
    assert cc[i].sum() == 12                                       # the census still counts all twelve
    assert cc[0].sum() == 5 and cc[1].sum() == 7                   # a corner: 2 + 1 + 2; its neighbour on the edge: 3 + 2 + 2


def test_lattice_short_lists_at_k_32(hip_device):
    p, lab = _lattice()
    got = cg.build(p, lab, 4, 7, 32)
    _equal(got, cg.graph_reference(p, lab, 4, 14, 32), 'lattice R = 7 k = 32')
    nb, d2, cc = got
    per_row = (nb >= 0).sum(1).reshape(12, 12)
    assert per_row[5, 6] == 4 and per_row[0, 0] == 2 and per_row[0, 5] == 3          # interior, corner, edge
    assert (nb[:, 4:] == -1).all() and (d2[:, 4:] == -1).all() and np.array_equal(nb < 0, d2 < 0)
    assert np.array_equal(cc.sum(1), per_row.ravel())


# ---- 3: one cell with more points than a workgroup has threads
def test_coincident_points_in_one_cell(hip_device):
    p = np.concatenate([np.full((300, 2), 5000), np.array([[5003, 5000], [5000, 4996], [4990, 5001], [5007, 5007], [5000, 5016]])]).astype(np.int32)
    rng = np.random.default_rng(5)
    order = rng.permutation(305)                                   # the five others sit among the 300, not behind them
    p, lab = p[order], rng.integers(0, 3, 305).astype(np.int32)
    got = cg.build(p, lab, 3, 8, 16)                               # r = 16: all 305 within reach of the 300
    _equal(got, cg.graph_reference(p, lab, 3, 16, 16), 'coincident')
    nb, d2, cc = got
    first = int(np.nonzero((p == 5000).all(1))[0][0])
    assert (d2[first] == 0).all() and (np.diff(nb[first]) > 0).all() and cc[first].sum() == 304


# ---- 4, 7: random points, slide-scale coordinates, repeatability
@pytest.fixture(scope='module')
def random_case():
    rng = np.random.default_rng(2024)
    p = rng.integers(0, 2 * 4096, (2000, 2)).astype(np.int32)     # a 4096 x 4096 px square in half pixels
    lab = rng.integers(0, 6, 2000).astype(np.int32)
    return p, lab, cg.graph_reference(p, lab, 6, 128, 16)


def test_random_points_and_the_same_points_shifted_to_slide_scale(hip_device, random_case):
    p, lab, want = random_case
    got = cg.build(p, lab, 6, 64, 16)
    _equal(got, want, 'random')
    assert (got[0][:, 1] >= 0).any() and (got[0][:, 0] < 0).any() and np.array_equal(got[2].sum(1), (got[0] >= 0).sum(1))   # about 1.5 neighbours a point
    shifted = p + np.array([2 * 150000, 2 * 90000], np.int32)
    _equal(cg.build(shifted, lab, 6, 64, 16), got, 'shifted by (150000, 90000) px')


def test_two_runs_are_bitwise_equal(hip_device, random_case):
    p, lab, want = random_case
    a, b = cg.build(p, lab, 6, 64, 16), cg.build(p, lab, 6, 64, 16)
    for x, y, w in zip(a, b, want):
        assert x.tobytes() == y.tobytes() == w.tobytes()


# ---- 5: the cell cap
def test_far_clusters_force_a_cell_side_above_the_radius(hip_device):
    rng = np.random.default_rng(9)
    far = 2 * (1 << 21)                                            # 2^21 px apart, along both axes
    p = np.concatenate([rng.integers(0, 40, (50, 2)), rng.integers(0, 40, (50, 2)) + far]).astype(np.int32)
    lab = rng.integers(0, 2, 100).astype(np.int32)
    side = cg.cell_side(int(p[:, 0].min()), int(p[:, 1].min()), int(p[:, 0].max()), int(p[:, 1].max()), 8)
    assert side > 8 and side % 8 == 0
    got = cg.build(p, lab, 2, 4, 8)
    _equal(got, cg.graph_reference(p, lab, 2, 8, 8), 'two clusters')
    assert (got[0][:50] < 50).all() and ((got[0][50:] >= 50) | (got[0][50:] == -1)).all() and (got[0] >= 0).any()


# ---- 6: edge sizes and refused arguments
def _raw(p, lab, C, r, k, fill=77, bounds=None):
    dev = torch.device('cuda', 0)
    p = np.asarray(p, np.int32).reshape(-1, 2)
    n = len(p)
    out = [torch.full((max(n, 1), w), fill, dtype=torch.int32, device=dev) for w in (max(k, 1), max(k, 1), max(C, 1))]
    rc = cg.call(torch.from_numpy(p).to(dev), torch.from_numpy(np.asarray(lab, np.int32)).to(dev), C, r, k, *out, bounds=bounds)
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy() for t in out]


def test_empty_and_single_point(hip_device):
    rc, out = _raw(np.zeros((0, 2)), np.zeros(0), 3, 8, 4)
    assert rc == hip.OK and all((o == 77).all() for o in out)                           # n == 0: nothing touched
    nb, d2, cc = cg.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, 4, 4)
    assert nb.shape == d2.shape == (0, 4) and cc.shape == (0, 3)
    rc, out = _raw([[123456, -7890]], [2], 3, 8, 4)
    assert rc == hip.OK and (out[0] == -1).all() and (out[1] == -1).all() and (out[2] == 0).all()
    _equal(cg.build(np.array([[123456, -7890]], np.int32), [2], 3, 4, 4), cg.graph_reference([[123456, -7890]], [2], 3, 8, 4), 'n = 1')


@pytest.mark.parametrize('C, r, k', [(3, 8, 0), (3, 8, 33), (3, 0, 4), (3, 16385, 4), (0, 8, 4), (15, 8, 4)])
def test_arguments_out_of_range_are_refused_before_anything_runs(hip_device, C, r, k):
    rc, out = _raw([[0, 0], [3, 4], [6, 0]], [0, 1, 2], C, r, k)
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)


def test_a_coordinate_out_of_range_is_refused(hip_device):
    rc, out = _raw([[0, 0], [1 << 27, 4], [6, 0]], [0, 1, 2], 3, 8, 4)
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)
    rc, out = _raw([[0, 0], [3, -(1 << 27)], [6, 0]], [0, 1, 2], 3, 8, 4)
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)
    with pytest.raises(ValueError):
        cg.build(np.array([[0, 0], [1 << 27, 4]], np.int32), [0, 1], 3, 4, 4)
    # a bounding box that does not hold every point: refused by the binning, the outputs still untouched
    rc, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, 8, 4, bounds=(0, 0, 10, 10))
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)
    rc, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, 8, 4)                      # (the same points with their own box are fine)
    assert rc == hip.OK and out[0][:, 0].tolist() == [1, 0, -1]


# ---- 8: the tool
_run = points_util.run_tool


def test_cli_nuclei_graph(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-feat --nuclei-graph on the synthetic .npy slide of tests/test_hip_nucfeat.py, plain, with --merge and on two
    ranks: one row per row of <id>_nuclei_feat.npz, the centres of <id>_point.geojson, the graph graph_reference gives on them, and every
    other file byte for byte as without the flag."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-feat')
    graph = ['--nuclei-graph', '--graph-radius', '24', '--graph-k', '6']
    docs = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d))) if f.endswith('.geojson')}
    feat = lambda d: nucfeat.read_npz(str(folder(d) / 's1_nuclei_feat.npz'))
    _run(base + ['--save_dir', str(tmp_path / 'plain0')], env)
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    _run(base + graph + ['--save_dir', str(tmp_path / 'plain')], env)
    _run(base + graph + ['--save_dir', str(tmp_path / 'merge'), '--merge'], env)
    _run(base + graph + ['--save_dir', str(tmp_path / 'two'), '--merge', '--gpus', '2'], two)
    assert not os.path.exists(folder('plain0') / 's1_nuclei_graph.npz') and not os.path.exists(folder('merge0') / 's1_nuclei_graph.npz')
    for run, ref in (('plain', 'plain0'), ('merge', 'merge0'), ('two', 'merge0')):
        assert docs(run) == docs(ref) and len(docs(run)) == (2 if run == 'plain' else 3), run
        assert sorted(os.listdir(folder(run))) == sorted(os.listdir(folder(ref)) + ['s1_nuclei_graph.npz']), run
        assert open(folder(run) / 's1_nuclei_feat.npz', 'rb').read() == open(folder(ref) / 's1_nuclei_feat.npz', 'rb').read(), run
        f = feat(run)
        g = cg.read_npz(str(folder(run) / 's1_nuclei_graph.npz'))
        points = json.loads(docs(run)['s1_point.geojson'])
        n = len(f['nuclei_id'])
        assert n > 10 and np.array_equal(g['nuclei_id'], f['nuclei_id']) and g['nuclei_id'].dtype == np.int64
        assert (n == len(points)) == (run == 'plain')
        xy = np.array([points[i]['geometry']['coordinates'] for i in g['nuclei_id']], np.float64)
        assert g['xy'].dtype == np.float64 and np.array_equal(g['xy'], xy)
        assert g['label'].tolist() == [points[i]['properties']['label'] for i in g['nuclei_id']] and np.array_equal(g['label'], f['label'])
        half = np.rint(2 * xy).astype(np.int32)
        nb, d2, cc = cg.graph_reference(half, g['label'], 5, 48, 6)
        assert np.array_equal(g['neighbors'], nb) and g['neighbors'].dtype == np.int32 and g['neighbors'].shape == (n, 6)
        assert np.array_equal(g['dist'], cg.distances_px(d2)) and g['dist'].dtype == np.float32
        assert np.array_equal(np.isinf(g['dist']), nb == -1)
        assert np.array_equal(g['class_count'], cc) and g['class_count'].shape == (n, 5)
        assert float(g['radius_px']) == 24 and int(g['k']) == 6
        print(f"{run}: {n} nodes, {int((nb >= 0).sum())} edges")
        assert (nb >= 0).any()
    gm, gt = cg.read_npz(str(folder('merge') / 's1_nuclei_graph.npz')), cg.read_npz(str(folder('two') / 's1_nuclei_graph.npz'))
    for key in cg.NPZ_KEYS:
        assert np.array_equal(gm[key], gt[key]), key
