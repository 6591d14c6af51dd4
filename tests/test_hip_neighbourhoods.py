"""GPU tests of the cellular neighbourhoods (csrc/cellhood.hip, nuhtc_cell_neighbourhoods): every result must EQUAL
nuhtc_amd.neighbourhoods.neighbourhoods_reference, the numpy restatement of the definition -- no tolerance, nothing left out.  The rules
first (the library's host-only exports against numpy), then the designed sets of tests/neighbourhoods_cases.py: the window through the
graph, the seeding picks on both sides of a prefix and in the first and last workgroup, T == 0, ties, duplicate and emptied types, the
rounding on one half, the extremes of K and C, max_iter below and at the reference's n_iter, given centres, the refused arguments,
bitwise repeatability, the profile tags and tools/infer_wsi.py --nuclei-neighbourhoods end to end."""
import os

import numpy as np
import pytest
import torch

import neighbourhoods_cases as NC
import points_util
from nuhtc_amd import cellgraph, hip
from nuhtc_amd import neighbourhoods as nh

pytestmark = pytest.mark.gpu


def _list(case):
    nb, lab, C, K, seed, max_iter, centres = case
    return nh.from_neighbors(nb, lab, C, K, seed, max_iter, centres)


# ---- 0: the rules, before any kernel: a disagreement here names the rule
def test_the_library_rules_equal_numpy():
    for seed in (0, 1, 2024, 2 ** 32 - 1):
        assert nh.host_draws(seed, 32) == nh.draws(seed, 32), seed
    rng = np.random.default_rng(3)
    g = rng.integers(0, 4, 200)
    prefix = np.cumsum(g)
    for t in range(int(prefix[-1])):
        assert nh.host_rule('pick', prefix, t) == nh.pick(prefix, t), t
    for s, m in ((1025, 2048), (1023, 2048), (0, 5), (33 * 2 ** 24, 2 ** 24), (7, 3), (1, 2 ** 24)):
        assert nh.host_rule('round', s, m) == (2 * 1024 * s + m) // (2 * m), (s, m)
    assert nh.host_rule('round', 1025, 2048) == 513 and nh.host_rule('round', 0, 0, 777) == 777
    for C in (1, 5, 14):
        w, q = rng.integers(0, 3, C), rng.integers(0, 34001, C)
        assert nh.host_rule('distance', w, q) == int(((1024 * w - q) ** 2).sum()), C
    assert nh.host_rule('distance', [33] + [0] * 13, [0] + [34000] * 13) == 33792 ** 2 + 13 * 34000 ** 2 > 2 ** 33
    for bad in (lambda: nh.host_draws(0, 33), lambda: nh.host_rule('pick', prefix, int(prefix[-1])), lambda: nh.host_rule('distance', [34], [0]),
                lambda: nh.host_rule('distance', [1], [34001])):
        with pytest.raises(ValueError):
            bad()


# ---- 1: the window, through the graph
@pytest.mark.parametrize('name', ['sparse', 'one_class_one_neighbour', 'fourteen_classes_32_neighbours'])
def test_windows_of_the_graph(hip_device, name):
    p, lab, C, r, k, K, seed, max_iter = NC.point_cases()[name]
    want = NC.point_reference(name)
    NC.equal(nh.build(p, lab, C, r / 2, k, K, seed, max_iter), want, name)
    w = want[0]
    if name == 'sparse':
        nb = cellgraph.graph_reference(p, lab, C, r, k)[0]
        assert (nb[:, -1] < 0).any() and (nb[:, -1] >= 0).any() and (w.sum(1) == 0).sum() == 4 and w[69].tolist() == [int(lab[69] == c) for c in range(3)]
        assert (w[60:65].sum(1) >= 4).all()                       # the coincident rows list each other
        assert (w.sum(1) < (nb >= 0).sum(1) + 1).any()            # a row or a neighbour of unknown label is counted nowhere
    else:
        assert w.shape[1] == C and w.sum(1).max() <= k + 1


# ---- 2, 3: seeding and Lloyd on designed neighbour lists
@pytest.mark.parametrize('name', ['pick_t_is_prefix_minus_1', 'pick_t_is_prefix', 'pick_in_first_block', 'pick_in_last_block', 'one_past_a_scan_chunk',
                                  'one_past_a_block', 'all_rows_equal', 'more_types_than_windows', 'fewer_rows_than_types', 'one_row', 'half_rounds_up',
                                  'most_types_most_classes', 'tie_goes_to_the_smaller_type', 'duplicate_given_centres', 'a_type_loses_all_members',
                                  'zones_20000'])
def test_designed_lists(hip_device, name):
    case, want = NC.list_cases()[name], NC.list_reference(name)
    got = _list(case)
    NC.equal(got, want, name)
    window, hood, q, s, m, rows, inertia, n_iter, converged = got
    if name == 'half_rounds_up':
        assert q.tolist() == [[513, 512]] and s.tolist() == [[1025, 1023]] and m.tolist() == [2048] and (n_iter, converged) == (2, True)
    if name == 'tie_goes_to_the_smaller_type':
        assert hood.tolist() == [0, 0, 1] and n_iter == 0 and converged and rows.tolist() == [-1, -1, -1]
    if name == 'duplicate_given_centres':
        assert m[1] == 0 and q.tolist() == [[1024, 0], [1024, 0], [0, 1024]] and inertia == 0
    if name == 'a_type_loses_all_members':
        assert m.tolist() == [7, 2, 0] and len({tuple(window[r]) for r in rows}) == 3
    if name in ('all_rows_equal', 'one_row'):
        assert len(set(rows.tolist())) == 1 and m[0] == len(hood) and (m[1:] == 0).all()
    if name == 'fewer_rows_than_types':
        assert rows.tolist().count(rows[0]) >= 3 and m.sum() == 3
    if name == 'pick_in_first_block':
        assert rows[1] < 256 <= rows[0]
    if name == 'pick_in_last_block':
        assert rows[0] < 768 <= rows[1]
    if name == 'zones_20000':
        assert converged and 7 <= n_iter <= 22 and (m > 0).all()


@pytest.mark.parametrize('name', ['zones_20000', 'most_types_most_classes'])
def test_max_iter_below_and_at_the_iteration_that_converges(hip_device, name):
    case = NC.list_cases()[name]
    full = NC.list_reference(name)[7]
    assert NC.list_reference(name)[8] and full >= 8
    for max_iter in sorted({full - 1, full, 7, 8, 9}):           # 7, 8, 9: inside, at the end of and behind the first batch of launches
        want = NC.list_reference(name, max_iter)
        assert want[7:] == (min(max_iter, full), max_iter >= full)
        NC.equal(_list(case[:5] + (max_iter,) + case[6:]), want, f'{name}, max_iter = {max_iter}')


def test_two_runs_are_bitwise_equal(hip_device):
    case = NC.list_cases()['zones_20000']
    a, b, want = _list(case), _list(case), NC.list_reference('zones_20000')
    for x, y, w in zip(a[:6], b[:6], want[:6]):
        assert x.tobytes() == y.tobytes() == w.tobytes()
    assert a[6:] == b[6:] == want[6:]


# ---- 4: given centres
def test_given_centres_assign_without_fitting(hip_device):
    nb, lab, C, K, seed, max_iter, _ = NC.list_cases()['zones_20000']
    fitted = NC.list_reference('zones_20000')
    again = nh.from_neighbors(nb, lab, C, K, seed, max_iter, centres=fitted[2])
    assert again[6:] == (fitted[6], 0, True) and again[5].tolist() == [-1] * K
    for k in range(5):                                           # the centres a run wrote reproduce that run's hood, sums and members
        assert np.array_equal(again[k], fitted[k]), NC.NAMES[k]
    rng = np.random.default_rng(5)
    q0 = rng.integers(0, 34001, (K, C))
    got = nh.from_neighbors(nb, lab, C, K, seed, max_iter, centres=q0)
    D = ((1024 * fitted[0].astype(np.int64)[:, None, :] - q0[None]) ** 2).sum(2)
    assert np.array_equal(got[1], D.argmin(1)) and got[6] == int(D.min(1).sum()) and got[7] == 0 and np.array_equal(got[2], q0)
    NC.equal(got, (fitted[0],) + nh.cluster_reference(fitted[0], K, seed, max_iter, q0), 'random given centres')


# ---- 5: refused arguments and the edge sizes
FILL = 77


def _raw(nb, lab, n, k, C, K, seed=0, max_iter=10, given=False, q0=None):
    dev = torch.device('cuda', 0)
    out = nh.outputs(min(n, 8), min(max(C, 1), 14), min(max(K, 1), 32), dev, fill=FILL)
    if q0 is not None:
        out[2].copy_(torch.from_numpy(np.asarray(q0, np.int32)))
    rc = nh.call(torch.from_numpy(np.asarray(nb, np.int32)).to(dev), torch.from_numpy(np.asarray(lab, np.int32)).to(dev), n, k, C, K, seed, max_iter, given, *out)
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy() for t in out]


@pytest.mark.parametrize('k, C, K, max_iter', [(0, 2, 2, 10), (33, 2, 2, 10), (2, 0, 2, 10), (2, 15, 2, 10), (2, 2, 0, 10), (2, 2, 33, 10), (2, 2, 2, 0),
                                               (2, 2, 2, 1001)])
def test_arguments_out_of_range_are_refused_before_anything_runs(hip_device, k, C, K, max_iter):
    rc, out = _raw(np.full((3, 33), -1), [0, 1, 0], 3, k, C, K, max_iter=max_iter)
    assert rc == (hip.E_INVALID, None, None, None) and all((o == FILL).all() for o in out)


def test_more_rows_than_the_limit_and_bad_centres_are_refused(hip_device):
    rc, out = _raw(np.full((3, 2), -1), [0, 1, 0], 2 ** 24 + 1, 2, 2, 2)
    assert rc[0] == hip.E_INVALID and all((o == FILL).all() for o in out)
    for q0 in ([[0, 34001], [0, 0]], [[0, 0], [-1, 0]]):
        rc, out = _raw(np.full((3, 2), -1), [0, 1, 0], 3, 2, 2, 2, given=True, q0=q0)
        assert rc[0] == hip.E_INVALID and all((o == FILL).all() for k, o in enumerate(out) if k != 2)
    rc, out = _raw(np.full((3, 2), -1), [0, 1, 0], 3, 2, 2, 2, given=True, q0=[[0, 34000], [0, 0]])
    assert rc == (hip.OK, 0, True, 3 * 1024 ** 2) and out[1][:3].tolist() == [1, 1, 1] and out[4].tolist() == [0, 3]
    with pytest.raises(ValueError):
        nh.from_neighbors(np.full((3, 2), -1), [0, 1, 0], 2, 2, centres=[[0, 34001], [0, 0]])


@pytest.mark.parametrize('bad', [3, -2, 2 ** 31 - 1, -2 ** 31])
def test_a_neighbour_index_out_of_range_is_refused(hip_device, bad):
    nb = np.full((3, 2), -1)
    nb[1, 1] = bad
    for given in (False, True):
        rc, out = _raw(nb, [0, 1, 0], 3, 2, 2, 2, given=given, q0=[[FILL, FILL], [FILL, FILL]])
        assert rc[0] == hip.E_INVALID and all((o == FILL).all() for o in out), (bad, given)
    nb[1, 1] = 2
    rc, out = _raw(nb, [0, 1, 0], 3, 2, 2, 2)
    assert rc[0] == hip.OK and out[0][:3].tolist() == [[1, 0], [1, 1], [1, 0]]


def test_no_rows(hip_device):
    got = nh.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, 4, 5, 4)
    NC.equal(got, nh.neighbourhoods_reference(np.zeros((0, 2)), np.zeros(0), 3, 8, 5, 4), 'n = 0')
    assert got[0].shape == (0, 3) and got[2].tolist() == [[0] * 3] * 4 and got[5].tolist() == [-1] * 4 and got[6:] == (0, 0, True)
    q0 = np.arange(12).reshape(4, 3) * 100
    got = nh.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, 4, 5, 4, centres=q0)
    assert np.array_equal(got[2], q0) and not got[3].any() and not got[4].any()
    with pytest.raises(ValueError):
        nh.build(np.array([[0, 0], [3, 4]], np.int32), [0, 1], 3, 4, 5, 33)


# ---- 6: the profile
def test_profile_tags_of_one_call(hip_device):
    case = NC.list_cases()['one_past_a_block']
    hip.profile_enable(True)
    try:
        got = _list(case)
        fit = {tag for tag in hip.profile_read() if tag.startswith('cell_hood')}
        _list(case[:6] + (got[2],))
        given = {tag for tag in hip.profile_read() if tag.startswith('cell_hood')}
    finally:
        hip.profile_enable(False)
    assert fit == {'cell_hood_window', 'cell_hood_seed', 'cell_hood_iterate', 'cell_hood_final'} and given == {'cell_hood_window', 'cell_hood_final'}, (fit, given)


# ---- 7: the tool
_run = points_util.run_tool


def test_cli_nuclei_neighbourhoods(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-graph --nuclei-neighbourhoods on the synthetic .npy slide of tests/points_util.py, with --merge: without the
    flag, with it, with the centres of that run given back, and with it on two ranks (four runs of the tool).  The folder gains exactly the
    one file, every other file is the same bytes as without the flag, the rows are those of <id>_nuclei_graph.npz, every integer equals
    `neighbourhoods_reference` on the file's own xy and label, every derived key equals `derive`, and the closing clause names the file."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-graph')
    flags = ['--nuclei-neighbourhoods', '--neighbourhood-k', '4', '--neighbourhood-radius', '24', '--neighbourhood-types', '3', '--neighbourhood-seed', '5']
    files = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d)))}
    name = 's1_nuclei_neighbourhoods.npz'
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    said = {'one': _run(base + flags + ['--save_dir', str(tmp_path / 'one'), '--merge'], env)}
    said['given'] = _run(base + flags + ['--save_dir', str(tmp_path / 'given'), '--merge', '--neighbourhood-centres', str(folder('one') / name)], env)
    said['two'] = _run(base + flags + ['--save_dir', str(tmp_path / 'two'), '--merge', '--gpus', '2'], two)
    z = {}
    for run in ('one', 'given', 'two'):
        assert ' of 3 neighbourhood types in use (' in said[run] and f'k 4, 24 px); ' in said[run] and f' in {name}' in said[run], said[run][-400:]
        assert ('assigned to given centres' in said[run]) == (run == 'given') and ('iterations, converged; seed 5' in said[run]) == (run != 'given')
        with_flag, without = files(run), files('merge0')
        assert sorted(with_flag) == sorted(list(without) + [name]), run
        for f in without:
            assert with_flag[f] == without[f], (run, f)
        z[run] = g = nh.read_npz(str(folder(run) / name))
        graph = cellgraph.read_npz(str(folder(run) / 's1_nuclei_graph.npz'))
        n = len(g['nuclei_id'])
        assert n > 10 and np.array_equal(g['nuclei_id'], graph['nuclei_id']) and np.array_equal(g['xy'], graph['xy']) and np.array_equal(g['label'], graph['label'])
        centres = z['one']['centre_q'] if run == 'given' else None
        want = nh.neighbourhoods_reference(np.rint(2 * g['xy']).astype(np.int32), g['label'], 5, 48, 4, 3, 5, 100, centres)
        for key, w, t in zip(nh.INT_NAMES, want[:6], nh.INT_TYPES):
            assert np.array_equal(g[key], w) and g[key].dtype == t, (run, key)
        assert (int(g['inertia']), int(g['n_iter']), bool(g['converged'])) == want[6:] and int(g['centres_given']) == (run == 'given')
        assert (float(g['radius_px']), int(g['k']), int(g['types']), int(g['seed']), int(g['max_iter'])) == (24.0, 4, 3, 5, 100)
        d = nh.derive(want[1], want[3], want[4], want[6], g['label'])
        for key in nh.DERIVED_KEYS:
            assert np.array_equal(g[key], d[key]) and g[key].dtype == d[key].dtype, (run, key)
        print(f"{run}: {n} nuclei, types of {g['centre_n'].tolist()} nuclei after {int(g['n_iter'])} iterations")
    for key in nh.NPZ_KEYS:
        assert np.array_equal(z['one'][key], z['two'][key]), key
        if key not in ('seed_rows', 'n_iter', 'centres_given'):
            assert np.array_equal(z['one'][key], z['given'][key]), key
