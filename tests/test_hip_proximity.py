"""GPU tests of the proximity graphs (csrc/cellprox.hip, nuhtc_cell_proximity): edges, edge_d2, edge_rng, degree, m and m_rng must EQUAL
nuhtc_amd.proximity.proximity_reference, the brute-force int64 restatement of the definition -- same dtype and shape, no tolerance,
nothing left out.  A chain of 20000 points in three row orders (rows over two scan chunks), 1500 points in two cells (fuller than a
workgroup, 680 000 edges) and 300 coincident points (a clique that needs the second call) first and on their own, against closed forms that
tests/test_proximity_host.py holds against the restatement; then the designed sets of tests/proximity_cases.py (on and beside the circle
and the radius, the lattice, witnesses across cell borders, the two label modes, negative and slide-scale coordinates), random sets with
many ties, the cap path, bitwise repeatability, permuted rows, the forest kernel as a cross-check, the refused arguments, and
tools/infer_wsi.py --nuclei-proximity end to end."""
import os

import numpy as np
import pytest
import torch

import proximity_cases as PC
import points_util
from nuhtc_amd import cellgraph, hip, mst
from nuhtc_amd import proximity as px

pytestmark = pytest.mark.gpu
NAMES = px.INT_NAMES + ('m', 'm_rng')


def _equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        if name in ('m', 'm_rng'):
            assert int(g) == int(w), (what, name, int(g), int(w))
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, f'{len(bad)} entries differ, first at {bad[0].tolist()}', int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


def _build(case, calls=None):
    p, lab, C, r, by = case
    got = px.build(p, lab, C, r / 2, by, with_calls=True)
    if calls is not None:
        assert got[6] == calls, (got[6], calls)
    return got[:6]


# ---- 1: rows over two scan chunks, a crowded cell, more edges than the first call has room for (run these first, on their own)
@pytest.mark.parametrize('order', ['ascending', 'descending', 'shuffled'])
def test_chain_of_20000_points_at_spacing_half_r(hip_device, order):
    """The edges are exactly the 19 999 links between neighbouring places; the pairs two places apart are candidates at d2 = r * r that the
    place between them blocks in both graphs."""
    case = PC.chain(order)
    got = _build(case, calls=1)
    _equal(got, PC.chain_expected(case), f'chain, {order}')
    assert got[4] == got[5] == 19999 and (got[1] == 64).all() and (got[2] == 1).all()
    if order == 'ascending':
        assert got[0].tolist() == [[k, k + 1] for k in range(19999)] and got[3][0].tolist() == [1, 1] and (got[3][1:-1] == 2).all()


def test_1500_points_on_nine_sites_in_two_cells(hip_device):
    case = PC.crowded()
    got = _build(case, calls=2)
    _equal(got, PC.crowded_expected(case), 'crowded')
    assert got[4] > 500000 and (got[2][got[1] == 8] == 0).all() and (got[2][got[1] < 8] == 1).all()


def test_300_coincident_points_in_one_cell(hip_device):
    case = PC.coincident()
    got = _build(case, calls=2)                                                # 44 850 edges and more: over 4 n + 64
    _equal(got, px.proximity_reference(*case), 'coincident')
    assert int((got[1] == 0).sum()) == 44850 and (got[2][got[1] == 0] == 1).all() and got[0][:299].tolist() == [[0, k] for k in range(1, 300)]


def test_130_coincident_points_a_segment_of_129_through_the_capacity_protocol(hip_device):
    """Row 0 owns a segment of 129 edges: longer than one wave's ballot and than the 64 kept flags, so the place stage ranks a segment
    whose tail the emit stage tested again.  First with room for 8 edges (nothing written but degree, m and m_rng), then for exactly m."""
    p, lab = np.full((130, 2), [40, -12], np.int32), np.zeros(130, np.int32)
    want = px.proximity_reference(p, lab, 3, 4, 0)
    m = want[4]
    assert m == 130 * 129 // 2 and int((want[0][:, 0] == 0).sum()) == 129
    rc, counts, out = _raw(p, lab, 3, 4, 0, cap=8)
    assert rc == hip.OK and counts == (m, want[5]) and all((o == 77).all() for o in out[:3]) and np.array_equal(out[3], want[3])
    rc, counts, out = _raw(p, lab, 3, 4, 0, cap=m)
    assert rc == hip.OK
    _equal((out[0], out[1], out[2], out[3]) + counts, want, '130 coincident')


# ---- 2: the designed sets, as they are and moved to the far corners of the coordinate range
@pytest.fixture(scope='module')
def small_references():
    return {name: px.proximity_reference(*case) for name, case in PC.small_cases().items()}


@pytest.mark.parametrize('name', sorted(PC.small_cases()))
def test_designed_sets_and_the_same_sets_translated(hip_device, small_references, name):
    case, want = PC.small_cases()[name], small_references[name]
    _equal(_build(case), want, name)
    for dx, dy in (((1 << 26) + 12345, -(1 << 26) - 321), (-(1 << 26) - 7, (1 << 26) + 50001)):
        _equal(_build(PC.translate(case, dx, dy)), want, f'{name} moved by ({dx}, {dy})')


def test_what_the_designed_sets_are_for(hip_device):
    for case, rows in ((PC.circles(), PC.CIRCLES), (PC.radius(), PC.RADIUS), (PC.other_label_witness(0), PC.OTHER_LABEL[0]),
                       (PC.other_label_witness(1), PC.OTHER_LABEL[1])):
        _equal(_build(case), PC._expected(len(case[0]), rows), 'hand-written')
    _equal(_build(PC.lattice()), PC.lattice_expected(), 'lattice')
    got = _build(PC.lattice(40, 30, 6, 9, (-777, 31)))                          # 1200 points over five blocks, cells of 9 against a pitch of 6
    _equal(got, PC.lattice_expected(40, 30, 6), 'lattice 40 x 30')
    assert got[4] == 40 * 29 + 30 * 39 + 2 * 39 * 29 and got[5] == 40 * 29 + 30 * 39


# ---- 3: random sets with many ties over twelve blocks of threads, both label modes; the cap path; repeatability; permuted rows; the forest
LARGE = [('uniform', 12, 0), ('uniform', 5, 1), ('uniform', 30, 1), ('clumps', 12, 1), ('clumps', 4, 0), ('clumps', 12, 0)]


@pytest.fixture(scope='module')
def large_references():
    return {key: px.proximity_reference(*PC.random_large(*key)) for key in LARGE}


@pytest.mark.parametrize('kind, r, by', LARGE)
def test_3000_random_points_and_the_forest_inside_the_rng(hip_device, large_references, kind, r, by):
    case = PC.random_large(kind, r, by)
    got = _build(case)
    _equal(got, large_references[(kind, r, by)], f'{kind}, r {r}, by_class {by}')
    print(f'{kind} r {r} by {by}: {got[4]} Gabriel edges, {got[5]} RNG edges, {int((got[1] == 0).sum())} of length 0')
    rng_edges = {tuple(e) for e in got[0][got[2] == 1].tolist()}
    forest = mst.build(case[0], case[1], case[2], r / 2, by)[0]                 # nuhtc_cell_mst at the same radius and mode
    assert len(forest) >= 1 and {tuple(e) for e in forest.tolist()} <= rng_edges


def test_ties_on_a_12_x_12_lattice_both_modes(hip_device):
    for by in (0, 1):
        case = PC.random_ties(by)
        _equal(_build(case), px.proximity_reference(*case), f'ties, by_class {by}')


def _raw(p, lab, C, r, by, cap, fill=77, bounds=None):
    dev = torch.device('cuda', 0)
    p = np.asarray(p, np.int32).reshape(-1, 2)
    out = px.outputs(len(p), cap, dev, fill=fill)
    rc, m, m_rng = px.call(torch.from_numpy(p).to(dev), torch.from_numpy(np.asarray(lab, np.int32)).to(dev), C, r, by, cap, *out, bounds=bounds)
    torch.cuda.synchronize()
    return rc, (m, m_rng), [o.cpu().numpy() for o in out]


def test_with_room_for_one_edge_less_the_edge_arrays_are_untouched(hip_device, large_references):
    key = ('clumps', 12, 0)
    case, want = PC.random_large(*key), large_references[key]
    m = want[4]
    rc, counts, out = _raw(*case, cap=m - 1)
    assert rc == hip.OK and counts == (m, want[5]) and all((o == 77).all() for o in out[:3])
    assert np.array_equal(out[3], want[3]) and out[3].dtype == want[3].dtype
    rc, counts, out = _raw(*case, cap=m)                                       # exactly enough
    assert rc == hip.OK and counts == (m, want[5])
    _equal((out[0], out[1], out[2], out[3]) + counts, want, 'cap == m')
    rc, counts, out = _raw(*case, cap=m + 5)                                    # rows past m untouched
    assert rc == hip.OK and (out[0][m:] == 77).all() and (out[1][m:] == 77).all() and (out[2][m:] == 77).all() and np.array_equal(out[0][:m], want[0])
    rc, counts, out = _raw(*case, cap=0)
    assert rc == hip.OK and counts == (m, want[5]) and np.array_equal(out[3], want[3])


def test_two_runs_are_bitwise_equal_and_permuted_rows_map_to_the_same_edge_set(hip_device):
    case = PC.random_large('clumps', 12, 0)
    a, b = _build(case), _build(case)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()
    assert a[4:] == b[4:]
    order = np.random.default_rng(4).permutation(len(case[0]))                 # new row k is old row order[k]
    got = _build((case[0][order], case[1][order]) + case[2:])
    back = np.sort(order[got[0]], 1)
    key = np.lexsort((back[:, 1], back[:, 0]))
    assert np.array_equal(back[key], a[0]) and np.array_equal(got[1][key], a[1]) and np.array_equal(got[2][key], a[2])
    assert np.array_equal(got[3], a[3][order]) and got[4:] == a[4:]


# ---- 4: edge sizes and refused arguments
def test_empty_single_and_three_points(hip_device):
    rc, counts, out = _raw(np.zeros((0, 2)), np.zeros(0), 3, 8, 0, cap=4)
    assert rc == hip.OK and counts == (0, 0) and all((o == 77).all() for o in out)                    # n == 0: nothing is launched
    _equal(px.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, 4), px.proximity_reference(np.zeros((0, 2)), [], 3, 8, 0), 'n = 0')
    rc, counts, out = _raw([[123456, -7890]], [2], 3, 8, 0, cap=4)
    assert rc == hip.OK and counts == (0, 0) and out[3].tolist() == [[0, 0]] and all((o == 77).all() for o in out[:3])
    rc, counts, out = _raw([[0, 0], [3, 4], [900, 900]], [0, 1, 1], 2, 5, 0, cap=3)
    assert rc == hip.OK and counts == (1, 1) and out[3].tolist() == [[1, 1], [1, 1], [0, 0]]
    assert out[0].tolist() == [[0, 1], [77, 77], [77, 77]] and out[1].tolist() == [25, 77, 77] and out[2].tolist() == [1, 77, 77]


@pytest.mark.parametrize('C, r, by, cap', [(3, 0, 0, 8), (3, 16385, 0, 8), (0, 5, 0, 8), (15, 5, 0, 8), (3, 5, 2, 8), (3, 5, 0, -1), (3, 5, 0, 1 << 31)])
def test_arguments_out_of_range_are_refused_before_anything_runs(hip_device, C, r, by, cap):
    dev = torch.device('cuda', 0)
    out = px.outputs(3, 8, dev, fill=77)
    p, lab = torch.tensor([[0, 0], [3, 4], [6, 0]], dtype=torch.int32, device=dev), torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    rc, m, m_rng = px.call(p, lab, C, r, by, cap, *out)
    torch.cuda.synchronize()
    assert rc == hip.E_INVALID and (m, m_rng) == (None, None) and all((o == 77).all() for o in out)


def test_a_point_outside_the_stated_box_is_refused(hip_device):
    rc, counts, out = _raw([[0, 0], [1 << 27, 4], [6, 0]], [0, 1, 2], 3, 5, 0, cap=8)
    assert rc == hip.E_INVALID and all((o == 77).all() for o in out)
    rc, counts, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, 5, 0, cap=8, bounds=(0, 0, 10, 10))   # refused by the binning, outputs untouched
    assert rc == hip.E_INVALID and counts == (None, None) and all((o == 77).all() for o in out)
    rc, counts, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, 5, 0, cap=8)                          # (the same points with their own box are fine)
    assert rc == hip.OK and counts == (1, 1) and out[3].tolist() == [[1, 1], [1, 1], [0, 0]]
    with pytest.raises(ValueError):
        px.build(np.array([[0, 0], [1 << 27, 4]], np.int32), [0, 1], 3, 2.5)


# ---- 5: the tool
_run = points_util.run_tool


def test_cli_nuclei_proximity(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-graph --nuclei-proximity on the synthetic .npy slide of tests/test_hip_clusters.py, with --merge on one
    rank and on two (three runs of the tool, to keep the test short): the folder gains exactly the one file, every other file is the same bytes as without the flag, the rows are those of
    <id>_nuclei_graph.npz, and the integers equal proximity_reference on the file's own xy and label."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-graph')
    flags = ['--nuclei-proximity', '--proximity-radius', '20', '--proximity-by', 'class']
    files = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d)))}
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    _run(base + flags + ['--save_dir', str(tmp_path / 'merge'), '--merge'], env)
    said = _run(base + flags + ['--save_dir', str(tmp_path / 'two'), '--merge', '--gpus', '2'], two)
    assert 'Gabriel edges' in said and 's1_nuclei_proximity.npz' in said
    for run, ref in (('merge', 'merge0'), ('two', 'merge0')):
        with_flag, without = files(run), files(ref)
        assert sorted(with_flag) == sorted(list(without) + ['s1_nuclei_proximity.npz']), run
        for f in without:
            assert with_flag[f] == without[f], (run, f)
        g = cellgraph.read_npz(str(folder(run) / 's1_nuclei_graph.npz'))
        z = px.read_npz(str(folder(run) / 's1_nuclei_proximity.npz'))
        assert tuple(z) == px.NPZ_KEYS
        n = len(g['nuclei_id'])
        assert n > 10 and np.array_equal(z['nuclei_id'], g['nuclei_id']) and np.array_equal(z['xy'], g['xy']) and np.array_equal(z['label'], g['label'])
        assert float(z['radius_px']) == 20.0 and int(z['by_class']) == 1
        want = px.proximity_reference(np.rint(2 * z['xy']).astype(np.int32), z['label'], 5, 40, 1)
        _equal([z[name] for name in px.INT_NAMES] + [int(z['n_edges']), int(z['n_rng'])], want, run)
        d = px.derive(want[0], want[1], want[2], want[3], z['label'], 5)
        for key in px.DERIVED_KEYS:
            assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype, (run, key)
        print(f"{run}: {n} nuclei, {int(z['n_edges'])} Gabriel edges, {int(z['n_rng'])} RNG edges")
        assert int(z['n_edges']) >= 1
    zm, zt = px.read_npz(str(folder('merge') / 's1_nuclei_proximity.npz')), px.read_npz(str(folder('two') / 's1_nuclei_proximity.npz'))
    for key in px.NPZ_KEYS:
        assert np.array_equal(zm[key], zt[key]), key
