"""GPU tests of the spatial statistics (csrc/cellspatial.hip, nuhtc_cell_spatial): every result must EQUAL nuhtc_amd.spatial.spatial_reference,
the brute-force int64 restatement of the definition -- no tolerance, nothing left out.  Designed point sets (a lattice with distances on
and beside the bin edges, coincident points in one cell, slide-scale offsets, a grid whose cell cap lifts the side above the reach, a pair
count beyond 2^32), the edge sizes and the refused arguments, bitwise repeatability, and tools/infer_wsi.py --nuclei-spatial end to end."""
import json
import os

import numpy as np
import pytest
import torch

import points_util
from nuhtc_amd import hip, nucfeat
from nuhtc_amd import spatial as sp

pytestmark = pytest.mark.gpu
NAMES = ('pair_hist', 'nn_d2', 'class_n')


def _equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, f'{len(bad)} entries differ, first at {bad[0].tolist()}', int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


# ---- 1: the lattice
def test_lattice_distances_on_and_beside_the_edges(hip_device):
    gy, gx = np.mgrid[0:12, 0:12]
    p = np.stack([gx.ravel() * 12 + 40, gy.ravel() * 12 + 24], 1).astype(np.int32)      # 12 x 12 points 12 half pixels apart
    lab = (np.arange(144) % 4).astype(np.int32)
    edges = [12, 17, 24, 34]                                        # d2 = 144 and 576 lie on an edge, 288 one below 17^2
    got = sp.build(p, lab, 4, edges)
    _equal(got, sp.spatial_reference(p, lab, 4, edges), 'lattice')
    assert got[0].sum(axis=(0, 1)).tolist() == [528, 484, 480, 1280] and got[2].tolist() == [36] * 4


# ---- 2: one cell with more points than a workgroup has threads
def test_coincident_points_in_one_cell(hip_device):
    p = np.concatenate([np.full((300, 2), 5000), np.array([[5003, 5000], [5000, 4996], [4990, 5001], [5007, 5007], [5000, 5016]])]).astype(np.int32)
    rng = np.random.default_rng(5)
    order = rng.permutation(305)                                    # the five others sit among the 300, not behind them
    p, lab = p[order], rng.integers(0, 3, 305).astype(np.int32)
    got = sp.build(p, lab, 3, [2, 5, 16])
    _equal(got, sp.spatial_reference(p, lab, 3, [2, 5, 16]), 'coincident')
    first = int(np.nonzero((p == 5000).all(1))[0][0])
    assert (got[1][first] == 0).all() and got[0][:, :, 0].sum() == 300 * 299               # every pair of the 300 has d2 = 0: bin 0


# ---- 3: random points, labels out of range, an absent class, slide-scale coordinates, repeatability
@pytest.fixture(scope='module')
def random_case():
    rng = np.random.default_rng(2024)
    p = rng.integers(0, 2 * 4096, (2000, 2)).astype(np.int32)      # a 4096 x 4096 px square in half pixels
    lab = rng.integers(0, 5, 2000).astype(np.int32)
    lab[lab == 3] = 5                                               # class 3 is absent
    lab[::97] = -1
    lab[5::101] = 6
    edges = sp.edges_from_step(8, 32)                               # the tool's default: 32 bins up to 256 px
    return p, lab, edges, sp.spatial_reference(p, lab, 6, edges)


def test_random_points_and_the_same_points_shifted_to_slide_scale(hip_device, random_case):
    p, lab, edges, want = random_case
    got = sp.build(p, lab, 6, edges)
    _equal(got, want, 'random')
    ph, nn, cn = got
    assert (lab == -1).any() and (lab == 6).any() and cn[3] == 0 and cn.sum() == ((lab >= 0) & (lab < 6)).sum()
    assert (nn[:, 3] == -1).all() and (ph[3] == 0).all() and (ph[:, 3] == 0).all() and (ph.sum(axis=(0, 1)) > 0).all()
    assert (nn[lab == -1] >= 0).any()                               # written for every i, whatever its own label
    shifted = p + np.array([2 * 150000, 2 * 90000], np.int32)
    _equal(sp.build(shifted, lab, 6, edges), got, 'shifted by (150000, 90000) px')


def test_two_runs_are_bitwise_equal(hip_device, random_case):
    p, lab, edges, want = random_case
    a, b = sp.build(p, lab, 6, edges), sp.build(p, lab, 6, edges)
    for x, y, w in zip(a, b, want):
        assert x.tobytes() == y.tobytes() == w.tobytes()


# ---- 4: the cell cap
def test_far_clusters_force_a_cell_side_above_the_reach(hip_device):
    rng = np.random.default_rng(9)
    far = 2 * (1 << 21)                                             # 2^21 px apart, along both axes
    p = np.concatenate([rng.integers(0, 40, (50, 2)), rng.integers(0, 40, (50, 2)) + far]).astype(np.int32)
    lab = rng.integers(0, 2, 100).astype(np.int32)
    side = sp.cell_side(int(p[:, 0].min()), int(p[:, 1].min()), int(p[:, 0].max()), int(p[:, 1].max()), 8)
    assert side > 8 and side % 8 == 0
    got = sp.build(p, lab, 2, [3, 8])
    _equal(got, sp.spatial_reference(p, lab, 2, [3, 8]), 'two clusters')
    assert got[0].sum() > 0


# ---- 5: the extremes of B and C
@pytest.mark.parametrize('C, B', [(1, 1), (1, 32), (14, 1), (14, 32)])
def test_fewest_and_most_bins_and_classes(hip_device, C, B):
    rng = np.random.default_rng(100 * C + B)
    p = rng.integers(0, 300, (700, 2)).astype(np.int32)            # three blocks of queries, the last one partly idle
    lab = rng.integers(-1, C + 1, 700).astype(np.int32)
    edges = [40] if B == 1 else list(range(2, 2 + 2 * B, 2))
    _equal(sp.build(p, lab, C, edges), sp.spatial_reference(p, lab, C, edges), f'C = {C}, B = {B}')


# ---- 6: a count beyond 2^32
def test_seventy_thousand_coincident_points_count_past_32_bits(hip_device):
    n = 70000
    ph, nn, cn = sp.build(np.full((n, 2), 777, np.int32), np.zeros(n, np.int32), 1, [1, 2])
    assert ph.dtype == np.int64 and ph.tolist() == [[[n * (n - 1), 0]]] and n * (n - 1) == 4899930000 > 2 ** 32     # the closed form
    assert (nn == 0).all() and cn.tolist() == [n]


# ---- 7, 8: edge sizes and refused arguments
def _raw(p, lab, C, edges, fill=77, bounds=None):
    dev = torch.device('cuda', 0)
    p = np.asarray(p, np.int32).reshape(-1, 2)
    n, Cs, Bs = len(p), max(C, 1), max(len(edges), 1)
    out = [torch.full((Cs, Cs, Bs), fill, dtype=torch.int64, device=dev), torch.full((max(n, 1), Cs), fill, dtype=torch.int32, device=dev),
           torch.full((Cs,), fill, dtype=torch.int64, device=dev)]
    rc = sp.call(torch.from_numpy(p).to(dev), torch.from_numpy(np.asarray(lab, np.int32)).to(dev), C, edges, *out, bounds=bounds)
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy() for t in out]


def test_empty_and_single_point(hip_device):
    rc, out = _raw(np.zeros((0, 2)), np.zeros(0), 3, [4, 8])
    assert rc == hip.OK and (out[0] == 0).all() and (out[2] == 0).all() and (out[1] == 77).all()       # n == 0: the counts are zeroed
    ph, nn, cn = sp.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, [4, 8])
    assert ph.shape == (3, 3, 2) and nn.shape == (0, 3) and cn.tolist() == [0, 0, 0]
    rc, out = _raw([[123456, -7890]], [2], 3, [4, 8])
    assert rc == hip.OK and (out[0] == 0).all() and (out[1] == -1).all() and out[2].tolist() == [0, 0, 1]
    _equal(sp.build(np.array([[123456, -7890]], np.int32), [2], 3, [4, 8]), sp.spatial_reference([[123456, -7890]], [2], 3, [4, 8]), 'n = 1')


@pytest.mark.parametrize('C, edges', [(3, []), (3, list(range(1, 34))), (3, [4, 4]), (3, [8, 4]), (3, [0, 4]), (3, [4, 16385]), (0, [4, 8]), (15, [4, 8])])
def test_arguments_out_of_range_are_refused_before_anything_runs(hip_device, C, edges):
    rc, out = _raw([[0, 0], [3, 4], [6, 0]], [0, 1, 2], C, edges)
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)


def test_a_coordinate_out_of_range_is_refused(hip_device):
    rc, out = _raw([[0, 0], [1 << 27, 4], [6, 0]], [0, 1, 2], 3, [4, 8])
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)
    rc, out = _raw([[0, 0], [3, -(1 << 27)], [6, 0]], [0, 1, 2], 3, [4, 8])
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)
    with pytest.raises(ValueError):
        sp.build(np.array([[0, 0], [1 << 27, 4]], np.int32), [0, 1], 3, [4, 8])
    # a bounding box that does not hold every point: refused by the binning, the outputs still untouched
    rc, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, [4, 8], bounds=(0, 0, 10, 10))
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)
    rc, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, [4, 8])                    # (the same points with their own box are fine)
    assert rc == hip.OK and out[0][0, 1].tolist() == [0, 1] and out[1][:, 0].tolist() == [-1, 25, -1]


# ---- 9: the tool
_run = points_util.run_tool


def test_cli_nuclei_spatial(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-feat --nuclei-spatial on the synthetic .npy slide of tests/test_hip_cellgraph.py, plain, with --merge and
    on two ranks: the rows of <id>_nuclei_feat.npz, the centres of <id>_point.geojson, the integers spatial_reference gives on them, and
    every other file byte for byte as without the flag."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-feat')
    flags = ['--nuclei-spatial', '--spatial-step', '4', '--spatial-bins', '8']
    docs = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d))) if f.endswith('.geojson')}
    _run(base + ['--save_dir', str(tmp_path / 'plain0')], env)
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    _run(base + flags + ['--save_dir', str(tmp_path / 'plain')], env)
    _run(base + flags + ['--save_dir', str(tmp_path / 'merge'), '--merge'], env)
    _run(base + flags + ['--save_dir', str(tmp_path / 'two'), '--merge', '--gpus', '2'], two)
    assert not os.path.exists(folder('plain0') / 's1_nuclei_spatial.npz') and not os.path.exists(folder('merge0') / 's1_nuclei_spatial.npz')
    edges = sp.edges_from_step(4, 8)
    for run, ref in (('plain', 'plain0'), ('merge', 'merge0'), ('two', 'merge0')):
        assert docs(run) == docs(ref) and len(docs(run)) == (2 if run == 'plain' else 3), run
        assert sorted(os.listdir(folder(run))) == sorted(os.listdir(folder(ref)) + ['s1_nuclei_spatial.npz']), run
        assert open(folder(run) / 's1_nuclei_feat.npz', 'rb').read() == open(folder(ref) / 's1_nuclei_feat.npz', 'rb').read(), run
        f = nucfeat.read_npz(str(folder(run) / 's1_nuclei_feat.npz'))
        g = sp.read_npz(str(folder(run) / 's1_nuclei_spatial.npz'))
        points = json.loads(docs(run)['s1_point.geojson'])
        n = len(f['nuclei_id'])
        assert n > 10 and np.array_equal(g['nuclei_id'], f['nuclei_id']) and g['nuclei_id'].dtype == np.int64
        assert (n == len(points)) == (run == 'plain')
        xy = np.array([points[i]['geometry']['coordinates'] for i in g['nuclei_id']], np.float64)
        assert g['xy'].dtype == np.float64 and np.array_equal(g['xy'], xy)
        assert g['label'].tolist() == [points[i]['properties']['label'] for i in g['nuclei_id']] and np.array_equal(g['label'], f['label'])
        assert g['edges_px'].tolist() == [4.0 * b for b in range(1, 9)]
        ph, nn, cn = sp.spatial_reference(np.rint(2 * xy).astype(np.int32), g['label'], 5, edges)
        assert np.array_equal(g['pair_hist'], ph) and g['pair_hist'].dtype == np.int64 and g['pair_hist'].shape == (5, 5, 8)
        assert np.array_equal(g['nn_d2'], nn) and g['nn_d2'].dtype == np.int32 and g['nn_d2'].shape == (n, 5)
        assert np.array_equal(g['class_n'], cn) and g['class_n'].dtype == np.int64
        assert np.array_equal(g['nn_dist'], sp.distances_px(nn)) and g['nn_dist'].dtype == np.float32
        assert np.array_equal(np.isinf(g['nn_dist']), g['nn_d2'] == -1)
        area = float(g['tiles_area_px'])                           # the inferred tiles x step_size^2
        d = sp.derive(ph, nn, g['label'], cn, edges, area_px=area)
        assert area >= 6 * 48.0 ** 2 and area % 48.0 ** 2 == 0 and np.array_equal(g['mean_within'], d['mean_within']) and np.array_equal(g['G'], d['G'])
        assert np.array_equal(g['K_tiles_area'], d['K']) and np.array_equal(g['L_tiles_area'], d['L'])
        print(f"{run}: {n} nuclei, {int(ph.sum())} ordered pairs within 32 px, classes {cn.tolist()}")
        assert ph.sum() > 0
    gm, gt = sp.read_npz(str(folder('merge') / 's1_nuclei_spatial.npz')), sp.read_npz(str(folder('two') / 's1_nuclei_spatial.npz'))
    for key in sp.NPZ_KEYS:
        assert np.array_equal(gm[key], gt[key]), key
