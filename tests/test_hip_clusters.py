"""GPU tests of the nucleus clusters (csrc/cellcluster.hip, nuhtc_cell_clusters): every output must EQUAL nuhtc_amd.clusters.cluster_reference,
the brute-force int64 restatement of the definition -- no tolerance, nothing left out.  The designed sets of tests/clusters_cases.py
(distances on and beside the radius, degrees around min_pts, a border point between two clusters, cell boundaries, negative and slide-scale
coordinates, the two label modes), a chain of 20000 points in three row orders (deep parent trees), a cell fuller than a workgroup, random
sets over several blocks, bitwise repeatability, the refused arguments, and tools/infer_wsi.py --nuclei-clusters end to end."""
import json
import os

import numpy as np
import pytest
import torch

import clusters_cases as CC
import points_util
from nuhtc_amd import cellgraph, hip
from nuhtc_amd import clusters as cl

pytestmark = pytest.mark.gpu


def _equal(got, want, what):
    for name, g, w in zip(cl.INT_NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, f'{len(bad)} entries differ, first at {bad[0].tolist()}', int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


def _build(case):
    p, lab, C, r, min_pts, by = case
    return cl.build(p, lab, C, r / 2, min_pts, by)


# ---- 1: deep trees and a crowded cell (run these first, on their own: a hooking loop that does not end shows up here)
@pytest.fixture(scope='module')
def chain_reference():
    return cl.cluster_reference(*CC.chain('ascending'))


@pytest.mark.parametrize('order', ['ascending', 'descending', 'shuffled'])
def test_chain_of_20000_points_at_spacing_r(hip_device, chain_reference, order):
    """The reference is computed once, for the ascending order.  Another order is a permutation k of the rows of one single cluster: the
    per-row outputs are the reference's at k, the tables do not change (tests/test_clusters_host.py checks on a short chain that the
    restatement itself says so)."""
    case = CC.chain(order)
    got = _build(case)
    k = (case[0][:, 0] + 7) // case[3]                    # the place of every row along the line
    _equal(got, tuple(a[k] for a in chain_reference[:3]) + chain_reference[3:], f'chain, {order}')
    first = int(np.argmin(case[0][:, 0]))                  # where the first point of the line sits; its root is ROW 0 all the same
    assert first == dict(ascending=0, descending=19999).get(order, first)
    assert (got[0] == 0).all() and got[1].all() and got[3].tolist() == [20000] and got[4].tolist() == [20000] and got[5].tolist() == [[10000, 10000]]
    assert got[2][first] == 2 and sorted(np.bincount(got[2]).tolist()) == [0, 0, 2, 19998]


def test_3000_coincident_points_in_one_cell(hip_device):
    case = CC.crowded_cell()
    got = _build(case)
    _equal(got, cl.cluster_reference(*case), 'crowded cell')
    pile = (case[0] == 5000).all(1)
    assert pile.sum() == 3000 and (got[2][pile] == 3000).all() and got[1][pile].all() and not got[1][~pile].any()
    assert got[3].tolist() == [3000] and (got[0][~pile] == -1).all() and got[7].tolist() == [[5000] * 4]
    one_more = case[:4] + (3001, 0)
    alone = _build(one_more)
    _equal(alone, cl.cluster_reference(*one_more), 'crowded cell, min_pts 3001')
    assert (alone[0] == -1).all() and len(alone[3]) == 0


# ---- 2: the designed sets, as they are and moved to the far corners of the coordinate range
@pytest.fixture(scope='module')
def small_references():
    return {name: cl.cluster_reference(*case) for name, case in CC.small_cases().items()}


@pytest.mark.parametrize('name', sorted(CC.small_cases()))
def test_designed_sets_and_the_same_sets_translated(hip_device, small_references, name):
    case, want = CC.small_cases()[name], small_references[name]
    got = _build(case)
    _equal(got, want, name)
    for dx, dy in (((1 << 26) + 12345, -(1 << 26) - 321), (-(1 << 26) - 7, (1 << 26) + 50001)):
        moved = _build(CC.translate(case, dx, dy))
        _equal(moved[:6], want[:6], f'{name} moved by ({dx}, {dy})')
        assert np.array_equal(moved[6], want[6] + want[3][:, None].astype(np.int64) * np.array([dx, dy])) and moved[6].dtype == np.int64
        assert np.array_equal(moved[7], want[7] + np.array([dx, dy, dx, dy], np.int32))


def test_what_the_designed_sets_are_for(hip_device):
    got = _build(CC.edge_pairs())
    assert got[0].tolist() == [0, 0, -1, -1] and got[2].tolist() == [2, 2, 1, 1]                        # d2 = r * r and r * r + 17
    got = _build(CC.one_above_the_radius())
    assert got[0].tolist() == [-1, -1, 0, 0] and got[2].tolist() == [1, 1, 2, 2] and got[3].tolist() == [2]   # d2 = r * r + 1 and r * r
    got = _build(CC.min_pts_threshold())
    assert got[1].tolist() == [0, 0, 0] + [1, 0, 0, 0] + [1, 0, 0, 0, 0] and got[0].tolist() == [-1] * 3 + [0] * 4 + [1] * 5
    got = _build(CC.bridge_equidistant())
    assert got[0][10] == 1 and got[1][10] == 0 and got[0][2] == 0 and got[0][1] == 1 and len(got[3]) == 2    # the smaller index, not the smaller cluster
    got = _build(CC.bridge_nearer_later())
    assert got[0][10] == 1 and got[1][10] == 0 and got[0][0] == 0 and len(got[3]) == 2 and got[3].tolist() == [5, 6]
    assert _build(CC.interleaved_classes(0))[0].tolist() == [0] * 20 and _build(CC.interleaved_classes(1))[0].tolist() == [0, 1] * 10
    got = _build(CC.labels_out_of_range(1))
    assert len(got[3]) >= 3 and got[5][:, [0, 2]].sum() == 0 and (got[5].sum(1) == 0).any() and (got[5].sum(1) == got[3]).any()
    many = _build(CC.small_cases()['components'])
    assert many[1].all() and (many[0] >= 0).all() and np.array_equal(many[3], np.bincount(many[0])) and np.array_equal(many[3], many[4])
    none = _build(CC.small_cases()['min_pts_above_n'])
    assert (none[0] == -1).all() and not none[1].any() and len(none[3]) == 0 and none[5].shape == (0, 3)


# ---- 3: random sets over twenty blocks of threads, both label modes; repeatability; permuted rows
LARGE = [('uniform', 60, 4, 0), ('uniform', 25, 2, 0), ('uniform', 140, 12, 1), ('clumps', 60, 4, 1), ('clumps', 25, 2, 0), ('clumps', 140, 12, 0)]


@pytest.mark.parametrize('kind, r, min_pts, by', LARGE)
def test_5000_random_points(hip_device, kind, r, min_pts, by):
    case = CC.random_large(kind, r, min_pts, by)
    got = _build(case)
    _equal(got, cl.cluster_reference(*case), f'{kind}, r {r}, min_pts {min_pts}, by_class {by}')
    print(f'{kind} r {r} min_pts {min_pts} by {by}: {len(got[3])} clusters, largest {int(got[3].max())}, {int((got[0] < 0).sum())} noise, '
          f'{int(((got[0] >= 0) & (got[1] == 0)).sum())} border')
    assert len(got[3]) > 1 and got[3].sum() == (got[0] >= 0).sum()


def test_two_runs_are_bitwise_equal_and_permuted_rows_equal_their_own_reference(hip_device):
    case = CC.random_large('clumps', 60, 4, 0)
    a, b = _build(case), _build(case)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    order = np.random.default_rng(4).permutation(len(case[0]))
    perm = (case[0][order], case[1][order]) + case[2:]
    got = _build(perm)
    _equal(got, cl.cluster_reference(*perm), 'permuted rows')
    assert np.array_equal(got[2], a[2][order]) and np.array_equal(got[1], a[1][order]) and sorted(got[4].tolist()) == sorted(a[4].tolist())


# ---- 4: edge sizes and refused arguments
def _raw(p, lab, C, r, min_pts, by, fill=77, bounds=None):
    dev = torch.device('cuda', 0)
    p = np.asarray(p, np.int32).reshape(-1, 2)
    out = cl.outputs(max(len(p), 1), max(C, 1), dev, fill=fill)
    rc, m = cl.call(torch.from_numpy(p).to(dev), torch.from_numpy(np.asarray(lab, np.int32)).to(dev), C, r, min_pts, by, *out, bounds=bounds)
    torch.cuda.synchronize()
    return rc, m, [t.cpu().numpy() for t in out]


def test_empty_single_and_two_points(hip_device):
    rc, m, out = _raw(np.zeros((0, 2)), np.zeros(0), 3, 8, 1, 0)
    assert rc == hip.OK and m == 0 and all((o == 77).all() for o in out)                              # n == 0: nothing is launched
    got = cl.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, 4, 5)
    _equal(got, cl.cluster_reference(np.zeros((0, 2)), [], 3, 8, 5, 0), 'n = 0')
    rc, m, out = _raw([[123456, -7890]], [2], 3, 8, 1, 0)
    assert rc == hip.OK and m == 1 and out[0].tolist() == [0] and out[1].tolist() == [1] and out[2].tolist() == [1] and out[3].tolist() == [1]
    assert out[5].tolist() == [[0, 0, 1]] and out[6].tolist() == [[123456, -7890]] and out[7].tolist() == [[123456, -7890, 123456, -7890]]
    rc, m, out = _raw([[0, 0], [3, 4], [900, 900]], [0, 1, 1], 2, 5, 2, 0)
    assert rc == hip.OK and m == 1 and out[0].tolist() == [0, 0, -1] and out[3].tolist() == [2, 77, 77] and (out[7][1:] == 77).all()   # rows past m untouched


@pytest.mark.parametrize('C, r, min_pts, by', [(3, 0, 2, 0), (3, 16385, 2, 0), (3, 5, 0, 0), (3, 5, -1, 0), (15, 5, 2, 0), (0, 5, 2, 0), (3, 5, 2, 2)])
def test_arguments_out_of_range_are_refused_before_anything_runs(hip_device, C, r, min_pts, by):
    rc, m, out = _raw([[0, 0], [3, 4], [6, 0]], [0, 1, 2], C, r, min_pts, by)
    assert rc == hip.E_INVALID and m is None and all((o == 77).all() for o in out)


def test_more_than_2_to_the_24_points_are_refused(hip_device):
    dev = torch.device('cuda', 0)
    n = (1 << 24) + 1                                                          # real buffers of that size: about 1 GB, filled on the device
    out = cl.outputs(n, 1, dev, fill=77)
    rc, m = cl.call(torch.zeros((n, 2), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), 1, 5, 2, 0, *out, bounds=(0, 0, 0, 0))
    torch.cuda.synchronize()
    assert rc == hip.E_INVALID and m is None and all(bool((o == 77).all()) for o in out)
    with pytest.raises(ValueError):
        cl.build(np.zeros((n, 2), np.int32), np.zeros(n, np.int32), 1, 2.5, 2)


def test_a_point_outside_the_stated_box_is_refused(hip_device):
    rc, m, out = _raw([[0, 0], [1 << 27, 4], [6, 0]], [0, 1, 2], 3, 5, 2, 0)
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)
    rc, m, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, 5, 2, 0, bounds=(0, 0, 10, 10))         # refused by the binning, outputs untouched
    assert rc == hip.E_INVALID and m is None and all((o == 77).all() for o in out)
    rc, m, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, 5, 2, 0)                                # (the same points with their own box are fine)
    assert rc == hip.OK and m == 1 and out[0].tolist() == [0, 0, -1]
    with pytest.raises(ValueError):
        cl.build(np.array([[0, 0], [1 << 27, 4]], np.int32), [0, 1], 3, 2.5, 2)


# ---- 5: the tool
_run = points_util.run_tool


def test_cli_nuclei_clusters(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-graph --nuclei-clusters on the synthetic .npy slide of tests/test_hip_cellgraph.py, plain, with --merge
    and on two ranks: the folder gains exactly the one file, every other file is the same bytes as without the flag, the rows are those of
    <id>_nuclei_graph.npz, and the tables equal cluster_reference on the file's own xy and label."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-graph')
    flags = ['--nuclei-clusters', '--cluster-radius', '12', '--cluster-min', '3', '--cluster-by', 'class']
    files = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d)))}
    _run(base + ['--save_dir', str(tmp_path / 'plain0')], env)
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    _run(base + flags + ['--save_dir', str(tmp_path / 'plain')], env)
    _run(base + flags + ['--save_dir', str(tmp_path / 'merge'), '--merge'], env)
    said = _run(base + flags + ['--save_dir', str(tmp_path / 'two'), '--merge', '--gpus', '2'], two)
    assert 'clusters and' in said and 's1_nuclei_clusters.npz' in said
    for run, ref in (('plain', 'plain0'), ('merge', 'merge0'), ('two', 'merge0')):
        with_flag, without = files(run), files(ref)
        assert sorted(with_flag) == sorted(list(without) + ['s1_nuclei_clusters.npz']), run
        for f in without:
            assert with_flag[f] == without[f], (run, f)
        g = cellgraph.read_npz(str(folder(run) / 's1_nuclei_graph.npz'))
        z = cl.read_npz(str(folder(run) / 's1_nuclei_clusters.npz'))
        n = len(g['nuclei_id'])
        assert n > 10 and np.array_equal(z['nuclei_id'], g['nuclei_id']) and np.array_equal(z['xy'], g['xy']) and np.array_equal(z['label'], g['label'])
        points = json.loads(with_flag['s1_point.geojson'])
        assert (n == len(points)) == (run == 'plain')
        assert float(z['radius_px']) == 12.0 and int(z['min_pts']) == 3 and int(z['by_class']) == 1
        want = cl.cluster_reference(np.rint(2 * z['xy']).astype(np.int32), z['label'], 5, 24, 3, 1)
        _equal([z[name] for name in cl.INT_NAMES], want, run)
        d = cl.derive(want[0], z['label'], 5, want[3], want[5], want[6], want[7])
        for key in cl.DERIVED_KEYS:
            assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype, (run, key)
        print(f"{run}: {n} nuclei, {int(z['n_clusters'])} clusters, {int(z['n_noise'])} isolated, sizes {z['size'].tolist()}")
        assert int(z['n_clusters']) >= 1
    zm, zt = cl.read_npz(str(folder('merge') / 's1_nuclei_clusters.npz')), cl.read_npz(str(folder('two') / 's1_nuclei_clusters.npz'))
    for key in cl.NPZ_KEYS:
        assert np.array_equal(zm[key], zt[key]), key
