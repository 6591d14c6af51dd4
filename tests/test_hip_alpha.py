"""GPU tests of the alpha complex (csrc/cellalpha.hip, nuhtc_cell_alpha): edges, edge_d2, apex, edge_gabriel, degree, m and m_gabriel must
EQUAL nuhtc_amd.alphacomplex.alpha_reference, the brute-force int64 restatement of the definition -- same dtype and shape, no tolerance,
nothing left out.  A chain of 20000 points in three row orders (rows over two scan chunks), 1500 points in two cells (fuller than a
workgroup), 300 coincident points (a clique that needs the second call) and 300 points around a corner of four cells first; then the
designed sets of tests/alpha_cases.py as they are and moved to the corners of the coordinate range, random sets on a coarse lattice
(collinear, cocircular and coincident points: twice for bitwise repeatability, once with permuted rows), both label modes, r = 512, the
capacity protocol, the refused arguments, nuhtc_cell_proximity and nuhtc_cell_mst on the same tensors as cross-checks, the profile tags,
and tools/infer_wsi.py --nuclei-alpha end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

import alpha_cases as AL
import points_util
from nuhtc_amd import alphacomplex as ax
from nuhtc_amd import cellgraph, hip, mst
from nuhtc_amd import proximity as px

pytestmark = pytest.mark.gpu
FILL = 77


def _build(case, calls=None):
    p, lab, C, r, by = case
    got = ax.build(p, lab, C, r / 2, by, with_calls=True)
    if calls is not None:
        assert got[7] == calls, (got[7], calls)
    return got[:7]


def _raw(p, lab, C, r, by, cap, bounds=None):
    dev = torch.device('cuda', 0)
    p = np.asarray(p, np.int32).reshape(-1, 2)
    out = ax.outputs(len(p), cap, dev, fill=FILL)
    rc, m, m_gab = ax.call(torch.from_numpy(p).to(dev), torch.from_numpy(np.asarray(lab, np.int32)).to(dev), C, r, by, cap, *out, bounds=bounds)
    torch.cuda.synchronize()
    return rc, (m, m_gab), [o.cpu().numpy() for o in out]


def _untouched(arrays):
    return all((a == FILL).all() for a in arrays)


# ---- 1: rows over two scan chunks, a crowded cell, more edges than the first call has room for, witnesses in the side and corner cells
@pytest.mark.parametrize('order', ['ascending', 'descending', 'shuffled'])
def test_chain_of_20000_points_at_spacing_r(hip_device, order):
    """Four candidates per point; the edges are exactly the 19 999 links between neighbouring places.  Against the closed form, which
    tests/test_alpha_host.py holds against the restatement, and in the shuffled order against the restatement itself (a few seconds: its
    tables hold only the rows near a block)."""
    case = AL.chain(order)
    got = _build(case, calls=1)
    if order == 'shuffled':
        AL.equal(got, ax.alpha_reference(*case), f'chain, {order}')
    AL.equal(got, AL.chain_expected(case), f'chain, {order} (closed form)')
    assert got[5] == got[6] == 19999 and (got[1] == 64).all() and (got[2] == -1).all()
    if order == 'ascending':
        assert got[0].tolist() == [[k, k + 1] for k in range(19999)] and got[4][0].tolist() == [1, 1] and (got[4][1:-1] == 2).all()


def test_1500_points_on_nine_sites_in_two_cells(hip_device):
    """All seven outputs against the closed form of tests/alpha_cases.py (the complex of the nine sites in fractions, every end repeated),
    which tests/test_alpha_host.py holds against the restatement; the restatement itself would take minutes on 590 000 edges.  The same
    sites with 300 points go against the restatement directly."""
    case = AL.crowded()
    got = _build(case, calls=2)
    AL.equal(got, AL.crowded_expected(case), 'crowded')
    assert got[5] > 500000 and got[6] == got[5] and (got[2][got[1] == 8] >= 0).all() and (got[2][got[1] == 0] == -1).all()
    small = AL.crowded(300)
    AL.equal(_build(small), ax.alpha_reference(*small), 'crowded 300')


def test_300_coincident_points_in_one_cell(hip_device):
    case = AL.coincident()
    got = _build(case, calls=2)                                                # 44 850 edges and more: over 4 n + 64
    AL.equal(got, ax.alpha_reference(*case), 'coincident')
    zero = got[1] == 0
    assert int(zero.sum()) == 44850 and (got[3][zero] == 1).all() and (got[2][zero] == -1).all() and got[0][:299].tolist() == [[0, k] for k in range(1, 300)]


def test_witnesses_in_the_side_and_corner_cells(hip_device):
    case = AL.side_and_corner_cells()
    got = _build(case)
    AL.equal(got, ax.alpha_reference(*case), 'around a corner of four cells')
    cell = case[0] // 16
    e, apex = got[0], got[2]
    across = [(apex[:, c] >= 0) & (cell[e[:, 0]] != cell[np.maximum(apex[:, c], 0)]).any(1) & (cell[e[:, 1]] != cell[np.maximum(apex[:, c], 0)]).any(1) for c in (0, 1)]
    assert across[0].sum() > 20 and across[1].sum() > 20                       # apexes in another cell than both ends


# ---- 2: the designed sets, as they are and moved to the far corners of the coordinate range
@pytest.fixture(scope='module')
def small_references():
    return {name: ax.alpha_reference(*case) for name, case in AL.small_cases().items()}


@pytest.mark.parametrize('name', sorted(AL.small_cases()))
def test_designed_sets_and_the_same_sets_translated(hip_device, small_references, name):
    case, want = AL.small_cases()[name], small_references[name]
    AL.equal(_build(case), want, name)
    for dx, dy in (((1 << 26) + 12345, -(1 << 26) - 321), (-(1 << 27) + 1 - int(case[0][:, 0].min()), (1 << 27) - 1 - int(case[0][:, 1].max()))):
        AL.equal(_build(AL.translate(case, dx, dy)), want, f'{name} moved by ({dx}, {dy})')


def test_what_the_designed_sets_are_for(hip_device):
    for case, rows in ((AL.two_points(0), AL.TWO_AT_D), (AL.two_points(1), []), (AL.two_points_one_over(), []), (AL.right_triangle(5), AL.RIGHT_5),
                       (AL.right_triangle(4), AL.RIGHT_4), (AL.collinear(), AL.COLLINEAR), (AL.diametral(), AL.DIAMETRAL),
                       (AL.other_label_witness(0), AL.OTHER_LABEL[0]), (AL.other_label_witness(1), AL.OTHER_LABEL[1])):
        AL.equal(_build(case), AL.expected(len(case[0]), rows), 'hand-written')
    for r, s, want in ((7, 10, 24), (8, 10, 42), (14, 20, 24), (15, 20, 42)):
        assert _build(AL.lattice(r, s=s))[5] == want
    got = _build(AL.lattice(8, 40, 30, 10, (-777, 31)))                          # 1200 points over five blocks, cells of 16 against a pitch of 10
    assert got[5] == AL.lattice_edges(40, 30, True) and got[6] == got[5]
    for k in (3, 5, 7):
        assert _build(AL.cocircular(k))[5] == k * (k - 1) // 2
    got = _build(AL.far_witness())
    assert got[0][0].tolist() == [0, 1] and got[2][0].tolist() == [2, -1]


# ---- 3: random sets full of ties, both label modes; repeatability; permuted rows; r = 512; the neighbouring kernels
COARSE = [(0, 4), (1, 4), (0, 5), (1, 2)]


@pytest.mark.parametrize('by, r', COARSE)
def test_coarse_lattice_twice_and_with_permuted_rows(hip_device, by, r):
    """600 points with the coordinates 0 .. 40 (three blocks of threads): collinear, cocircular and coincident points everywhere."""
    case = AL.coarse(by, 600, 41, r, seed=12 + r)
    want = ax.alpha_reference(*case)
    a, b = _build(case), _build(case)
    AL.equal(a, want, f'coarse, by_class {by}, r {r}')
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:5], b[:5])) and a[5:] == b[5:]
    order = np.random.default_rng(4).permutation(len(case[0]))                 # new row k is old row order[k]: the apexes and the order of the edges change
    moved = (case[0][order], case[1][order]) + case[2:]
    AL.equal(_build(moved), ax.alpha_reference(*moved), f'coarse, by_class {by}, r {r}, permuted rows')
    print(f'coarse by {by} r {r}: {a[5]} edges, {a[6]} Gabriel, {int((a[1] == 0).sum())} of length 0, {int(((a[2] >= 0).sum(1) == 2).sum())} interior')


LARGE = [('uniform', 6, 0), ('clumps', 6, 1), ('clumps', 2, 0)]


@pytest.mark.parametrize('kind, r, by', LARGE)
def test_3000_random_points_beside_the_proximity_and_the_forest_kernels(hip_device, kind, r, by):
    case = AL.random_large(kind, r, by)
    got = _build(case)
    AL.equal(got, ax.alpha_reference(*case), f'{kind}, r {r}, by_class {by}')
    p, lab, C = case[:3]
    gabriel = px.build(p, lab, C, r, by)                                        # nuhtc_cell_proximity at radius D = 2 r half pixels = r px
    keep = got[3] == 1
    assert np.array_equal(got[0][keep], gabriel[0]) and np.array_equal(got[1][keep], gabriel[1]) and np.array_equal(got[4][:, 1], gabriel[3][:, 0]) and got[6] == gabriel[4]
    forest = mst.build(p, lab, C, r, by)[0]                                     # nuhtc_cell_mst at radius D
    assert len(forest) >= 1 and {tuple(e) for e in forest.tolist()} <= {tuple(e) for e in got[0].tolist()}
    print(f'{kind} r {r} by {by}: {got[5]} edges, {got[6]} Gabriel, forest {len(forest)}')


def test_the_largest_radius(hip_device):
    rng = np.random.default_rng(9)
    p = np.concatenate([AL.largest()[0], rng.integers(0, 9000, (700, 2)) + [20000, -3000]]).astype(np.int32)
    case = (p, rng.integers(0, 3, len(p)).astype(np.int32), 3, 512, 0)
    got = _build(case)
    AL.equal(got, ax.alpha_reference(*case), 'r = 512')
    assert int(got[1].max()) > 900 ** 2 and ((got[2] >= 0).sum(1) == 2).sum() > 500
    AL.equal(_build(case[:4] + (1,)), ax.alpha_reference(*case[:4], 1), 'r = 512, by class')


# ---- 4: the protocol, edge sizes and refused arguments
def test_capacity_protocol_with_untouched_edge_buffers(hip_device):
    case = AL.random_large('clumps', 6, 0)
    want = ax.alpha_reference(*case)
    m = want[5]
    assert m > 3000
    for cap in (0, m - 1, m, m + 5):
        rc, counts, out = _raw(*case, cap=cap)
        assert rc == hip.OK and counts == (m, want[6]) and np.array_equal(out[4], want[4]) and out[4].dtype == want[4].dtype, cap   # degree and the counts always
        if cap < m:
            assert _untouched(out[:4]), cap
        else:
            AL.equal([o[:m] for o in out[:4]] + [out[4]] + list(counts), want, f'cap {cap}')
            assert _untouched([o[m:] for o in out[:4]])


def test_empty_single_and_three_points(hip_device):
    rc, counts, out = _raw(np.zeros((0, 2)), np.zeros(0), 3, 8, 0, cap=4)
    assert rc == hip.OK and counts == (0, 0) and _untouched(out)                                      # n == 0: nothing is launched
    AL.equal(ax.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, 4), ax.alpha_reference(np.zeros((0, 2)), [], 3, 8, 0), 'n = 0')
    rc, counts, out = _raw([[123456, -7890]], [2], 3, 8, 0, cap=4)
    assert rc == hip.OK and counts == (0, 0) and out[4].tolist() == [[0, 0]] and _untouched(out[:4])
    rc, counts, out = _raw([[0, 0], [6, 8], [900, 900]], [0, 1, 1], 2, 5, 0, cap=3)
    assert rc == hip.OK and counts == (1, 1) and out[4].tolist() == [[1, 1], [1, 1], [0, 0]]
    assert out[0].tolist() == [[0, 1], [77, 77], [77, 77]] and out[1].tolist() == [100, 77, 77] and out[2].tolist() == [[-1, -1], [77, 77], [77, 77]] and out[3].tolist() == [1, 77, 77]


@pytest.mark.parametrize('C, r, by, cap', [(3, 0, 0, 8), (3, 513, 0, 8), (3, 16384, 0, 8), (0, 5, 0, 8), (15, 5, 0, 8), (3, 5, 2, 8), (3, 5, 0, -1), (3, 5, 0, 1 << 31)])
def test_arguments_out_of_range_are_refused_before_anything_runs(hip_device, C, r, by, cap):
    dev = torch.device('cuda', 0)
    out = ax.outputs(3, 8, dev, fill=FILL)
    p, lab = torch.tensor([[0, 0], [3, 4], [6, 0]], dtype=torch.int32, device=dev), torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    rc, m, m_gab = ax.call(p, lab, C, r, by, cap, *out)
    torch.cuda.synchronize()
    assert rc == hip.E_INVALID and (m, m_gab) == (None, None) and all((o == FILL).all() for o in out)


def test_null_pointers_are_refused(hip_device):
    dev = torch.device('cuda', 0)
    out = ax.outputs(3, 8, dev, fill=FILL)
    p, lab = torch.tensor([[0, 0], [3, 4], [6, 0]], dtype=torch.int32, device=dev), torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    fn = hip.load().nuhtc_cell_alpha
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    m, g = ctypes.c_int64(-7), ctypes.c_int64(-7)
    ptrs = [vp(p), vp(lab)] + [vp(t) for t in out]
    call = lambda q, mp, gp: fn(0, q[0], q[1], 3, 3, 5, 0, 8, 0, 0, 6, 4, q[2], q[3], q[4], q[5], q[6], mp, gp, None)
    for k in range(7):
        assert call(ptrs[:k] + [None] + ptrs[k + 1:], ctypes.byref(m), ctypes.byref(g)) == hip.E_INVALID, k
    assert call(ptrs, None, ctypes.byref(g)) == hip.E_INVALID and call(ptrs, ctypes.byref(m), None) == hip.E_INVALID
    torch.cuda.synchronize()
    assert m.value == -7 and g.value == -7 and all((t == FILL).all().item() for t in out)
    assert call(ptrs, ctypes.byref(m), ctypes.byref(g)) == hip.OK and (m.value, g.value) == (3, 3)


def test_a_point_outside_the_stated_box_is_refused(hip_device):
    rc, counts, out = _raw([[0, 0], [1 << 27, 4], [6, 0]], [0, 1, 2], 3, 5, 0, cap=8)
    assert rc == hip.E_INVALID and _untouched(out)
    rc, counts, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, 5, 0, cap=8, bounds=(0, 0, 10, 10))   # refused by the binning, outputs untouched
    assert rc == hip.E_INVALID and counts == (None, None) and _untouched(out)
    rc, counts, out = _raw([[0, 0], [3, 4], [600, 0]], [0, 1, 2], 3, 5, 0, cap=8)                          # (the same points with their own box are fine)
    assert rc == hip.OK and counts == (1, 1) and out[4].tolist() == [[1, 1], [1, 1], [0, 0]]
    with pytest.raises(ValueError):
        ax.build(np.array([[0, 0], [1 << 27, 4]], np.int32), [0, 1], 3, 2.5)
    with pytest.raises(ValueError):
        ax.build(np.array([[0, 0], [3, 4]], np.int32), [0, 1], 3, 256.5)


# ---- 5: the profile
def test_profile_tags_of_one_call(hip_device):
    case = AL.lattice(8)
    hip.profile_enable(True)
    try:
        rc, counts, out = _raw(*case, cap=64)
        tags = {tag for tag in hip.profile_read() if tag.startswith('cell_alpha')}
    finally:
        hip.profile_enable(False)
    assert rc == hip.OK and counts == (42, 42) and tags == {'cell_alpha_bin', 'cell_alpha_count', 'cell_alpha_scan', 'cell_alpha_emit', 'cell_alpha_place'}, tags


# ---- 6: the tool
_run = points_util.run_tool


def test_cli_nuclei_alpha(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-graph --nuclei-alpha on the synthetic .npy slide of tests/points_util.py, with --merge: without the flag,
    with it, and with it on two ranks (three runs of the tool).  The folder gains exactly the one file, every other file is the same bytes
    as without the flag, the rows are those of <id>_nuclei_graph.npz, every integer equals `build` and the restatement on the file's own
    xy and label, every derived key equals `derive` of them, and the closing clause ends with the file's name."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-graph')
    flags = ['--nuclei-alpha', '--alpha-radius', '10', '--alpha-by', 'class']
    files = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d)))}
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    said = {'one': _run(base + flags + ['--save_dir', str(tmp_path / 'one'), '--merge'], env),
            'two': _run(base + flags + ['--save_dir', str(tmp_path / 'two'), '--merge', '--gpus', '2'], two)}
    z = {}
    for run in ('one', 'two'):
        assert 'alpha-complex edges' in said[run] and '(10 px radius, by class) in s1_nuclei_alpha.npz' in said[run], said[run][-400:]
        with_flag, without = files(run), files('merge0')
        assert sorted(with_flag) == sorted(list(without) + ['s1_nuclei_alpha.npz']), run
        for f in without:
            assert with_flag[f] == without[f], (run, f)
        g = cellgraph.read_npz(str(folder(run) / 's1_nuclei_graph.npz'))
        z[run] = ax.read_npz(str(folder(run) / 's1_nuclei_alpha.npz'))
        assert tuple(z[run]) == ax.NPZ_KEYS
        n = len(g['nuclei_id'])
        assert n > 10 and all(np.array_equal(z[run][k], g[k]) for k in ('nuclei_id', 'xy', 'label'))
        assert float(z[run]['radius_px']) == 10.0 and int(z[run]['by_class']) == 1
        pts = np.rint(2 * z[run]['xy']).astype(np.int32)
        built = ax.build(pts, z[run]['label'], 5, 10.0, 1)                     # the gathered rows through `build` again
        want = ax.alpha_reference(pts, z[run]['label'], 5, 20, 1)
        AL.equal(built, want, run + ': build')
        AL.equal([z[run][name] for name in ax.INT_NAMES] + [int(z[run]['n_edges']), int(z[run]['n_gabriel'])], want, run)
        d = ax.derive(*want[:5], pts, z[run]['label'], 5, 20)
        for key in ax.DERIVED_KEYS:
            assert np.array_equal(z[run][key], d[key]) and z[run][key].dtype == d[key].dtype, (run, key)
        print(f"{run}: {n} nuclei, {want[5]} edges, {want[6]} Gabriel, {int(d['n_triangles'])} triangles")
        assert want[5] >= 1
    for key in ax.NPZ_KEYS:
        assert np.array_equal(z['one'][key], z['two'][key]), key
