"""GPU tests of the neighbourhood enrichment (csrc/cellenrich.hip, nuhtc_cell_enrichment): every result must EQUAL
nuhtc_amd.enrichment.enrichment_reference, the brute-force restatement of the definition -- no tolerance, nothing left out.  The generator
first (the library's host-only export against numpy), then designed point sets (a lattice with the radius on a lattice distance,
coincident points in one cell, slide-scale offsets, a grid whose cell cap lifts the side above the radius, counts beyond 2^32), the
extremes of C and P, the cross-check against nuhtc_cell_spatial, the edge sizes and the refused arguments, bitwise repeatability, and
tools/infer_wsi.py --nuclei-enrichment end to end."""
import json
import os

import numpy as np
import pytest
import torch

import points_util
from nuhtc_amd import enrichment as en
from nuhtc_amd import hip, nucfeat
from nuhtc_amd import spatial as sp

pytestmark = pytest.mark.gpu
NAMES = ('observed', 'perm_counts', 'class_n')


def _equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype == np.int64 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, f'{len(bad)} entries differ, first at {bad[0].tolist()}', int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


# ---- 0: the generator, before any kernel: a disagreement here names the generator
@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 1025, 4097, 70000])
def test_the_library_generator_equals_numpy(n):
    for p in (1, 2, 1024):
        for seed in (0, 2 ** 32 - 1):
            got = en.host_permutation(n, seed, p)
            assert got.dtype == np.int32 and np.array_equal(got, en.permutation(n, seed, p)), (n, p, seed)
    for bad in ((n, 0, 0), (n, 0, 1025), (2 ** 24 + 1, 0, 1)):
        with pytest.raises(ValueError):
            en.host_permutation(*bad)


# ---- 1: the lattice
def test_lattice_with_the_radius_on_a_lattice_distance(hip_device):
    gy, gx = np.mgrid[0:12, 0:12]
    p = np.stack([gx.ravel() * 12 + 40, gy.ravel() * 12 + 24], 1).astype(np.int32)      # 12 x 12 points 12 half pixels apart
    lab = (np.arange(144) % 4).astype(np.int32)
    for r, contacts in ((12, 528), (17, 528 + 484), (24, 528 + 484 + 480)):              # d2 = 144, 288 (just inside 17^2), 576: inclusive
        got = en.build(p, lab, 4, r / 2, 20, seed=3)                                     # P = 20: one full batch and one partial batch
        _equal(got, en.enrichment_reference(p, lab, 4, r, 20, 3), f'lattice, r = {r}')
        assert got[0].sum() == contacts and (got[1].sum(axis=(1, 2)) == contacts).all() and got[2].tolist() == [36] * 4
    assert len({got[1][k].tobytes() for k in range(20)}) > 1


# ---- 2: one cell with more points than a workgroup has threads
def test_coincident_points_in_one_cell(hip_device):
    p = np.concatenate([np.full((300, 2), 5000), np.array([[5003, 5000], [5000, 4996], [4990, 5001], [5007, 5007], [5000, 5016]])]).astype(np.int32)
    rng = np.random.default_rng(5)
    order = rng.permutation(305)                                    # the five others sit among the 300, not behind them
    p, lab = p[order], rng.integers(0, 3, 305).astype(np.int32)
    got = en.build(p, lab, 3, 2.5, 17, seed=1)
    _equal(got, en.enrichment_reference(p, lab, 3, 5, 17, 1), 'coincident')
    assert got[0].sum() >= 300 * 299 and (got[1].sum(axis=(1, 2)) == got[0].sum()).all()


# ---- 3: random points, labels out of range, an absent class, slide-scale coordinates, repeatability, the row order
@pytest.fixture(scope='module')
def random_case():
    rng = np.random.default_rng(2024)
    p = rng.integers(0, 2 * 1024, (2000, 2)).astype(np.int32)      # a 1024 x 1024 px square in half pixels
    lab = rng.integers(0, 5, 2000).astype(np.int32)
    lab[lab == 3] = 5                                               # class 3 is absent
    lab[::97] = -1
    lab[5::101] = 6                                                 # C itself
    return p, lab, en.enrichment_reference(p, lab, 6, 128, 40, 77)


def test_random_points_and_the_same_points_shifted_to_slide_scale(hip_device, random_case):
    p, lab, want = random_case
    got = en.build(p, lab, 6, 64, 40, seed=77)
    _equal(got, want, 'random')
    obs, perm, cn = got
    assert (lab == -1).any() and (lab == 6).any() and cn[3] == 0 and cn.sum() == ((lab >= 0) & (lab < 6)).sum()
    assert (obs[3] == 0).all() and (obs[:, 3] == 0).all() and (perm[:, 3] == 0).all() and (perm[:, :, 3] == 0).all() and obs.sum() > 10000
    assert np.array_equal(obs, obs.T) and len({int(t.sum()) for t in perm}) > 1           # rows without a class move in and out of contact
    shifted = p + np.array([2 * 150000, 2 * 90000], np.int32)
    _equal(en.build(shifted, lab, 6, 64, 40, seed=77), got, 'shifted by (150000, 90000) px')


def test_two_runs_are_bitwise_equal(hip_device, random_case):
    p, lab, want = random_case
    a, b = en.build(p, lab, 6, 64, 40, seed=77), en.build(p, lab, 6, 64, 40, seed=77)
    for x, y, w in zip(a, b, want):
        assert x.tobytes() == y.tobytes() == w.tobytes()


def test_observed_does_not_depend_on_the_row_order(hip_device, random_case):
    p, lab, want = random_case
    order = np.random.default_rng(8).permutation(len(p))
    got = en.build(p[order], lab[order], 6, 64, 40, seed=77)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    _equal(got, en.enrichment_reference(p[order], lab[order], 6, 128, 40, 77), 'reordered')
    assert not np.array_equal(got[1], want[1])                      # pi acts on row numbers: the shuffles are others


def test_another_seed_gives_other_shuffles_and_the_same_observed(hip_device, random_case):
    p, lab, want = random_case
    got = en.build(p, lab, 6, 64, 40, seed=78)
    assert np.array_equal(got[0], want[0]) and not np.array_equal(got[1], want[1])
    _equal(got, en.enrichment_reference(p, lab, 6, 128, 40, 78), 'seed 78')


# ---- 4: the cell cap
def test_far_clusters_force_a_cell_side_above_the_radius(hip_device):
    from nuhtc_amd import cellpoints
    rng = np.random.default_rng(9)
    far = 2 * (1 << 21)                                             # 2^21 px apart, along both axes
    p = np.concatenate([rng.integers(0, 40, (50, 2)), rng.integers(0, 40, (50, 2)) + far]).astype(np.int32)
    lab = rng.integers(0, 2, 100).astype(np.int32)
    side = cellpoints.cell_side(*cellpoints.bounds_of(p), 8, 1 << 22)
    assert side > 8 and side % 8 == 0
    got = en.build(p, lab, 2, 4, 18, seed=2)
    _equal(got, en.enrichment_reference(p, lab, 2, 8, 18, 2), 'two clusters')
    assert got[0].sum() > 0


# ---- 5: the extremes of C and P
@pytest.mark.parametrize('C, P', [(1, 1), (1, 1024), (14, 16), (14, 17)])
def test_fewest_and_most_classes_and_permutations(hip_device, C, P):
    rng = np.random.default_rng(100 * C + P)
    p = rng.integers(0, 300, (700, 2)).astype(np.int32)            # three blocks of queries, the last one partly idle
    lab = rng.integers(-1, C + 1, 700).astype(np.int32)
    _equal(en.build(p, lab, C, 10, P, seed=P), en.enrichment_reference(p, lab, C, 20, P, P), f'C = {C}, P = {P}')


# ---- 6: counts beyond 2^32
def test_seventy_thousand_coincident_points_count_past_32_bits(hip_device):
    n = 70000
    obs, perm, cn = en.build(np.full((n, 2), 777, np.int32), (np.arange(n) % 2).astype(np.int32), 2, 0.5, 2, seed=4)
    h = n // 2
    closed = [[h * (h - 1), h * h], [h * h, h * (h - 1)]]           # every pair is a contact, and a shuffle keeps the class sizes
    assert obs.dtype == np.int64 and obs.tolist() == closed and perm.tolist() == [closed, closed] and cn.tolist() == [h, h]
    assert h * h == 1225000000 and int(obs.sum()) == n * (n - 1) == 4899930000 > 2 ** 32


# ---- 7: against the kernel already here
def test_observed_equals_the_spatial_statistics_at_one_edge(hip_device, random_case):
    p, lab, want = random_case
    obs, _, cn = en.build(p, lab, 6, 64, 1, seed=0)
    ph, _, sn = sp.build(p, lab, 6, [128])
    assert np.array_equal(obs, ph[:, :, 0]) and np.array_equal(cn, sn) and np.array_equal(obs, want[0])


# ---- 8, 9: edge sizes and refused arguments
def _raw(p, lab, C, r, P, seed=0, fill=77, bounds=None):
    dev = torch.device('cuda', 0)
    p = np.asarray(p, np.int32).reshape(-1, 2)
    Cs, Ps = max(C, 1), min(max(P, 1), 1024)
    out = [torch.full(shape, fill, dtype=torch.int64, device=dev) for shape in ((Cs, Cs), (Ps, Cs, Cs), (Cs,))]
    rc = en.call(torch.from_numpy(p).to(dev), torch.from_numpy(np.asarray(lab, np.int32)).to(dev), C, r, P, seed, *out, bounds=bounds)
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy() for t in out]


def test_empty_and_single_point(hip_device):
    rc, out = _raw(np.zeros((0, 2)), np.zeros(0), 3, 8, 5)
    assert rc == hip.OK and all((o == 0).all() for o in out)       # n == 0: the outputs are zeroed
    obs, perm, cn = en.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, 4, 5)
    assert obs.shape == (3, 3) and perm.shape == (5, 3, 3) and cn.tolist() == [0, 0, 0]
    rc, out = _raw([[123456, -7890]], [2], 3, 8, 5)
    assert rc == hip.OK and (out[0] == 0).all() and (out[1] == 0).all() and out[2].tolist() == [0, 0, 1]
    _equal(en.build(np.array([[123456, -7890]], np.int32), [2], 3, 4, 5), en.enrichment_reference([[123456, -7890]], [2], 3, 8, 5, 0), 'n = 1')


@pytest.mark.parametrize('C, r, P', [(3, 8, 0), (3, 8, 1025), (3, 0, 4), (3, 16385, 4), (0, 8, 4), (15, 8, 4)])
def test_arguments_out_of_range_are_refused_before_anything_runs(hip_device, C, r, P):
    rc, out = _raw([[0, 0], [3, 4], [6, 0]], [0, 1, 2], C, r, P)
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)


def test_a_coordinate_out_of_range_is_refused(hip_device):
    rc, out = _raw([[0, 0], [1 << 27, 4], [6, 0]], [0, 1, 2], 3, 8, 4)
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)
    rc, out = _raw([[0, 0], [3, -(1 << 27)], [6, 0]], [0, 1, 2], 3, 8, 4)
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)
    with pytest.raises(ValueError):
        en.build(np.array([[0, 0], [1 << 27, 4]], np.int32), [0, 1], 3, 4, 4)
    # a bounding box that does not hold every point: refused by the binning, the outputs still untouched
    rc, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, 8, 4, bounds=(0, 0, 10, 10))
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)
    rc, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, 8, 4)                       # (the same points with their own box are fine)
    assert rc == hip.OK and out[0].tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 0]] and out[2].tolist() == [1, 1, 1]
    assert (out[1].sum(axis=(1, 2)) == 2).all()                     # the one pair in contact, under any labels of the three classes


# ---- 10: the tool
_run = points_util.run_tool


def test_cli_nuclei_enrichment(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-feat --nuclei-enrichment on the synthetic .npy slide of tests/points_util.py, plain, with --merge and on
    two ranks: the rows of <id>_nuclei_feat.npz, the centres of <id>_point.geojson, the integers enrichment_reference gives on the written
    centres, the derived arrays of `derive`, and every other file byte for byte as without the flag."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-feat')
    flags = ['--nuclei-enrichment', '--enrichment-radius', '24', '--enrichment-perms', '20', '--enrichment-seed', '5']
    docs = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d))) if f.endswith('.geojson')}
    _run(base + ['--save_dir', str(tmp_path / 'plain0')], env)
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    said = _run(base + flags + ['--save_dir', str(tmp_path / 'plain')], env)
    _run(base + flags + ['--save_dir', str(tmp_path / 'merge'), '--merge'], env)
    _run(base + flags + ['--save_dir', str(tmp_path / 'two'), '--merge', '--gpus', '2'], two)
    assert 'contacts within 24 px against 20 label permutations (seed 5; largest |z|: class ' in said and ' in s1_nuclei_enrichment.npz' in said
    assert not os.path.exists(folder('plain0') / 's1_nuclei_enrichment.npz') and not os.path.exists(folder('merge0') / 's1_nuclei_enrichment.npz')
    for run, ref in (('plain', 'plain0'), ('merge', 'merge0'), ('two', 'merge0')):
        assert docs(run) == docs(ref) and len(docs(run)) == (2 if run == 'plain' else 3), run
        assert sorted(os.listdir(folder(run))) == sorted(os.listdir(folder(ref)) + ['s1_nuclei_enrichment.npz']), run
        assert open(folder(run) / 's1_nuclei_feat.npz', 'rb').read() == open(folder(ref) / 's1_nuclei_feat.npz', 'rb').read(), run
        f = nucfeat.read_npz(str(folder(run) / 's1_nuclei_feat.npz'))
        g = en.read_npz(str(folder(run) / 's1_nuclei_enrichment.npz'))
        points = json.loads(docs(run)['s1_point.geojson'])
        n = len(f['nuclei_id'])
        assert n > 10 and np.array_equal(g['nuclei_id'], f['nuclei_id']) and g['nuclei_id'].dtype == np.int64
        assert (n == len(points)) == (run == 'plain')
        xy = np.array([points[i]['geometry']['coordinates'] for i in g['nuclei_id']], np.float64)
        assert g['xy'].dtype == np.float64 and np.array_equal(g['xy'], xy)
        assert g['label'].tolist() == [points[i]['properties']['label'] for i in g['nuclei_id']] and np.array_equal(g['label'], f['label'])
        assert float(g['radius_px']) == 24.0 and int(g['perms']) == 20 and int(g['seed']) == 5
        obs, perm, cn = en.enrichment_reference(np.rint(2 * xy).astype(np.int32), g['label'], 5, 48, 20, 5)
        assert np.array_equal(g['observed'], obs) and g['observed'].dtype == np.int64 and g['observed'].shape == (5, 5)
        assert np.array_equal(g['perm_counts'], perm) and g['perm_counts'].dtype == np.int64 and g['perm_counts'].shape == (20, 5, 5)
        assert np.array_equal(g['class_n'], cn) and g['class_n'].dtype == np.int64
        d = en.derive(obs, perm)
        for key in en.DERIVED_KEYS:
            assert np.array_equal(g[key], d[key]) and g[key].dtype == np.float64 and g[key].shape == (5, 5), key
        print(f"{run}: {n} nuclei, {int(obs.sum())} contacts within 24 px, classes {cn.tolist()}")
        assert obs.sum() > 0
    gm, gt = en.read_npz(str(folder('merge') / 's1_nuclei_enrichment.npz')), en.read_npz(str(folder('two') / 's1_nuclei_enrichment.npz'))
    for key in en.NPZ_KEYS:
        assert np.array_equal(gm[key], gt[key]), key
