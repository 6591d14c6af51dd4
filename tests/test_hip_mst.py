"""GPU tests of the minimum spanning forest (csrc/cellmst.hip, nuhtc_cell_mst): edges, edge_d2, tree, m and T must EQUAL
nuhtc_amd.mst.mst_reference, the brute-force int64 restatement of the definition -- same dtype and shape, no tolerance, nothing left out.
A chain of 20000 points in three row orders (a union 20000 deep, rows over two scan chunks), the designed sets of tests/mst_cases.py
(distances on and beside the radius, ties that only the (i, j) order decides, mutual and one-sided picks, a cell fuller than a workgroup,
trees of size 1, the two label modes, cell boundaries, negative and slide-scale coordinates), the ruler that takes exactly log2 n rounds,
random sets with many ties, bitwise repeatability, permuted rows, the clusters kernel as a cross-check, the refused arguments, and
tools/infer_wsi.py --nuclei-mst end to end."""
import math
import os

import numpy as np
import pytest
import torch

import mst_cases as MC
import points_util
from nuhtc_amd import cellgraph, hip, mst
from nuhtc_amd import clusters as cl

pytestmark = pytest.mark.gpu
NAMES = mst.INT_NAMES + ('m', 'T')


def _equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        if name in ('m', 'T'):
            assert int(g) == int(w), (what, name, int(g), int(w))
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, f'{len(bad)} entries differ, first at {bad[0].tolist()}', int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


def _build(case):
    """-> (edges, edge_d2, tree, m, T), rounds"""
    p, lab, C, r, by = case
    got = mst.build(p, lab, C, r / 2, by, with_rounds=True)
    n = len(p)
    assert got[5] <= (math.ceil(math.log2(n)) if n > 1 else 0), (got[5], n)
    return got[:5], got[5]


# ---- 1: a deep union and a crowded cell (run these first, on their own: a union or a round loop that does not end shows up here)
@pytest.mark.parametrize('order', ['ascending', 'descending', 'shuffled'])
def test_chain_of_20000_points_at_spacing_r(hip_device, order):
    """The expected forest is the closed form of tests/mst_cases.py (the links between neighbouring places of the line), which
    tests/test_mst_host.py holds against the restatement on a short chain."""
    case = MC.chain(order)
    got, rounds = _build(case)
    _equal(got, MC.chain_forest(case), f'chain, {order}')
    assert got[3] == 19999 and got[4] == 1 and (got[1] == 256).all()
    if order == 'ascending':
        assert rounds == 1 and got[0].tolist() == [[k, k + 1] for k in range(19999)]


def test_300_coincident_points_in_one_cell(hip_device):
    case = MC.coincident()
    got, rounds = _build(case)
    _equal(got, mst.mst_reference(*case), 'coincident')
    assert got[0][:299].tolist() == [[0, k] for k in range(1, 300)] and (got[1][:299] == 0).all() and got[4] == 1
    big = MC.coincident(3000)
    got, rounds = _build(big)
    assert got[0][:2999].tolist() == [[0, k] for k in range(1, 3000)] and (got[1][:2999] == 0).all() and got[3] == 3004 and got[4] == 1 and (got[2] == 0).all()


def test_100_coincident_points_a_segment_of_99_at_row_0(hip_device):
    """The forest is the star of row 0 (the smallest keys are (0, 0, k)) and the five points around it: 104 edges, 100 of them in the one
    segment of row 0 (its 99 coincident rows and the nearest of the five), longer than 64, ranked by the place stage."""
    case = MC.coincident(100)
    want = mst.mst_reference(*case)
    assert want[3] == 104 and int((want[0][:, 0] == 0).sum()) == 100 and want[4] == 1
    got, rounds = _build(case)
    _equal(got, want, '100 coincident')


# ---- 2: the designed sets, as they are and moved to the far corners of the coordinate range
@pytest.fixture(scope='module')
def small_references():
    return {name: mst.mst_reference(*case) for name, case in MC.small_cases().items()}


@pytest.mark.parametrize('name', sorted(MC.small_cases()))
def test_designed_sets_and_the_same_sets_translated(hip_device, small_references, name):
    case, want = MC.small_cases()[name], small_references[name]
    _equal(_build(case)[0], want, name)
    for dx, dy in (((1 << 26) + 12345, -(1 << 26) - 321), (-(1 << 26) - 7, (1 << 26) + 50001)):
        _equal(_build(MC.translate(case, dx, dy))[0], want, f'{name} moved by ({dx}, {dy})')


def test_what_the_designed_sets_are_for(hip_device):
    got, rounds = _build(MC.edge_pairs())
    assert got[0].tolist() == [[0, 1]] and got[1].tolist() == [100] and got[2].tolist() == [0, 0, 1, 2, 3, 4] and rounds == 1
    for case, want in ((MC.equidistant(), MC.EQUIDISTANT_FOREST), (MC.collinear(), MC.COLLINEAR_FOREST), (MC.groups(), MC.GROUPS_FOREST)):
        got, rounds = _build(case)
        assert got[0].tolist() == want[0] and got[1].tolist() == want[1] and got[2].tolist() == want[2] and got[4] == max(want[2]) + 1
    assert _build(MC.collinear())[1] == 1                                       # the mutual and the one-sided pick in the same round
    got, rounds = _build(MC.lattice())
    assert got[3] == 63 and (got[1] == 9).all() and got[0][:4].tolist() == [[0, 1], [0, 8], [1, 2], [1, 9]]
    assert _build(MC.interleaved_classes(0))[0][4] == 1 and _build(MC.interleaved_classes(1))[0][2].tolist() == [0, 1] * 10


def test_the_ruler_takes_exactly_log2_n_rounds(hip_device):
    case = MC.ruler()
    got, rounds = _build(case)
    _equal(got, mst.mst_reference(*case), 'ruler')
    assert len(case[0]) == 1024 and rounds == 10 and got[0].tolist() == [[k, k + 1] for k in range(1023)]
    assert _build(MC.ruler(256))[1] == 8


# ---- 3: random sets with many ties over twelve blocks of threads, both label modes; repeatability; permuted rows; the clusters kernel
LARGE = [('uniform', 12, 0), ('uniform', 5, 1), ('uniform', 30, 1), ('clumps', 12, 1), ('clumps', 4, 0), ('clumps', 30, 0)]


@pytest.mark.parametrize('kind, r, by', LARGE)
def test_3000_random_points(hip_device, kind, r, by):
    case = MC.random_large(kind, r, by)
    got, rounds = _build(case)
    _equal(got, mst.mst_reference(*case), f'{kind}, r {r}, by_class {by}')
    print(f'{kind} r {r} by {by}: {got[3]} edges, {got[4]} trees, {rounds} rounds, {int((got[1] == 0).sum())} edges of length 0')
    assert got[3] + got[4] == 3000 and got[4] >= 1                             # one tree at the widest radius on the clumps
    same = cl.build(case[0], case[1], case[2], r / 2, 1, by)[0]                 # min_pts 1: every point is core, the clusters ARE the trees
    assert np.array_equal(got[2], same) and got[2].dtype == same.dtype


def test_two_runs_are_bitwise_equal_and_permuted_rows_equal_their_own_reference(hip_device):
    case = MC.random_large('clumps', 12, 0)
    (a, ra), (b, rb) = _build(case), _build(case)
    assert ra == rb
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    order = np.random.default_rng(4).permutation(len(case[0]))
    perm = (case[0][order], case[1][order]) + case[2:]
    got, _ = _build(perm)
    _equal(got, mst.mst_reference(*perm), 'permuted rows')
    assert got[3] == a[3] and got[4] == a[4] and int(got[1].astype(np.int64).sum()) == int(a[1].astype(np.int64).sum())


# ---- 4: edge sizes and refused arguments
def _raw(p, lab, C, r, by, fill=77, bounds=None):
    dev = torch.device('cuda', 0)
    p = np.asarray(p, np.int32).reshape(-1, 2)
    out = mst.outputs(max(len(p), 1), dev, fill=fill)
    rc, m, t, rounds = mst.call(torch.from_numpy(p).to(dev), torch.from_numpy(np.asarray(lab, np.int32)).to(dev), C, r, by, *out, bounds=bounds)
    torch.cuda.synchronize()
    return rc, (m, t, rounds), [o.cpu().numpy() for o in out]


def test_empty_single_and_three_points(hip_device):
    rc, counts, out = _raw(np.zeros((0, 2)), np.zeros(0), 3, 8, 0)
    assert rc == hip.OK and counts == (0, 0, 0) and all((o == 77).all() for o in out)                 # n == 0: nothing is launched
    _equal(mst.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, 4), mst.mst_reference(np.zeros((0, 2)), [], 3, 8, 0), 'n = 0')
    rc, counts, out = _raw([[123456, -7890]], [2], 3, 8, 0)
    assert rc == hip.OK and counts == (0, 1, 0) and out[2].tolist() == [0] and (out[0] == 77).all() and (out[1] == 77).all()
    rc, counts, out = _raw([[0, 0], [3, 4], [900, 900]], [0, 1, 1], 2, 5, 0)
    assert rc == hip.OK and counts == (1, 2, 1) and out[2].tolist() == [0, 0, 1]
    assert out[0].tolist() == [[0, 1], [77, 77], [77, 77]] and out[1].tolist() == [25, 77, 77]       # rows past m untouched


@pytest.mark.parametrize('C, r, by', [(3, 0, 0), (3, 16385, 0), (0, 5, 0), (15, 5, 0), (3, 5, 2)])
def test_arguments_out_of_range_are_refused_before_anything_runs(hip_device, C, r, by):
    rc, counts, out = _raw([[0, 0], [3, 4], [6, 0]], [0, 1, 2], C, r, by)
    assert rc == hip.E_INVALID and counts == (None, None, None) and all((o == 77).all() for o in out)


def test_a_point_outside_the_stated_box_is_refused(hip_device):
    rc, counts, out = _raw([[0, 0], [1 << 27, 4], [6, 0]], [0, 1, 2], 3, 5, 0)
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)
    rc, counts, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, 5, 0, bounds=(0, 0, 10, 10))      # refused by the binning, outputs untouched
    assert rc == hip.E_INVALID and counts == (None, None, None) and all((o == 77).all() for o in out)
    rc, counts, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, 5, 0)                             # (the same points with their own box are fine)
    assert rc == hip.OK and counts == (1, 2, 1) and out[2].tolist() == [0, 0, 1]
    with pytest.raises(ValueError):
        mst.build(np.array([[0, 0], [1 << 27, 4]], np.int32), [0, 1], 3, 2.5)


# ---- 5: the tool
_run = points_util.run_tool


def test_cli_nuclei_mst(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-graph --nuclei-mst on the synthetic .npy slide of tests/test_hip_clusters.py, plain, with --merge and on
    two ranks: the folder gains exactly the one file, every other file is the same bytes as without the flag, the rows are those of
    <id>_nuclei_graph.npz, and the integers equal mst_reference on the file's own xy and label."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-graph')
    flags = ['--nuclei-mst', '--mst-radius', '20', '--mst-by', 'class']
    files = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d)))}
    _run(base + ['--save_dir', str(tmp_path / 'plain0')], env)
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    _run(base + flags + ['--save_dir', str(tmp_path / 'plain')], env)
    _run(base + flags + ['--save_dir', str(tmp_path / 'merge'), '--merge'], env)
    said = _run(base + flags + ['--save_dir', str(tmp_path / 'two'), '--merge', '--gpus', '2'], two)
    assert 'forest edges' in said and 's1_nuclei_mst.npz' in said
    for run, ref in (('plain', 'plain0'), ('merge', 'merge0'), ('two', 'merge0')):
        with_flag, without = files(run), files(ref)
        assert sorted(with_flag) == sorted(list(without) + ['s1_nuclei_mst.npz']), run
        for f in without:
            assert with_flag[f] == without[f], (run, f)
        g = cellgraph.read_npz(str(folder(run) / 's1_nuclei_graph.npz'))
        z = mst.read_npz(str(folder(run) / 's1_nuclei_mst.npz'))
        n = len(g['nuclei_id'])
        assert n > 10 and np.array_equal(z['nuclei_id'], g['nuclei_id']) and np.array_equal(z['xy'], g['xy']) and np.array_equal(z['label'], g['label'])
        assert float(z['radius_px']) == 20.0 and int(z['by_class']) == 1
        want = mst.mst_reference(np.rint(2 * z['xy']).astype(np.int32), z['label'], 5, 40, 1)
        _equal([z[name] for name in mst.INT_NAMES] + [int(z['n_edges']), int(z['n_trees'])], want, run)
        d = mst.derive(want[0], want[1], want[2], z['label'], 5)
        for key in mst.DERIVED_KEYS:
            assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype, (run, key)
        print(f"{run}: {n} nuclei, {int(z['n_edges'])} edges, {int(z['n_trees'])} trees, mean {float(z['length_mean_px']):.2f} px")
        assert int(z['n_edges']) >= 1
    zm, zt = mst.read_npz(str(folder('merge') / 's1_nuclei_mst.npz')), mst.read_npz(str(folder('two') / 's1_nuclei_mst.npz'))
    for key in mst.NPZ_KEYS:
        assert np.array_equal(zm[key], zt[key]), key
