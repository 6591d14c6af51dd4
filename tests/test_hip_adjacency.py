"""GPU tests of the territory adjacency (csrc/celladjacency.hip, nuhtc_territory_adjacency): edges, shared, degree and m must EQUAL
nuhtc_amd.adjacency.adjacency_reference, the numpy restatement of the definition -- same dtype, shape and order, no tolerance, nothing
left out; every buffer is pre-filled with 77 so that "untouched" can be tested.  The designed maps of tests/adjacency_cases.py (the
smallest ones, merges across tiles, a row with 300 neighbours, a full tile table, a window of many tiles in x), the capacity protocol, the
refused arguments, the cases of tests/territory_cases.py from points through `build` (against the reference on the reference's owner
map, the identity with the device's own `contact`, repeatable, independent of the row order), the profile tags, and tools/infer_wsi.py
--nuclei-adjacency end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

import adjacency_cases as AC
import points_util
import proximity_cases as PC
import territory_cases as TC
from nuhtc_amd import adjacency as adj
from nuhtc_amd import cellgraph, cellpoints, hip
from nuhtc_amd import territory as tr

pytestmark = pytest.mark.gpu
FILL = 77


def _raw(owner, n, cap):
    """One call on buffers filled with 77 -> (return code, m, [edges (cap', 2), shared (cap',), degree (n',)]), cap' and n' one at least."""
    dev = torch.device('cuda', 0)
    own = torch.from_numpy(np.ascontiguousarray(owner, np.int32)).to(dev)
    out = adj.outputs(n, cap, dev, fill=FILL)
    rc, m = adj.call(own, n, cap, *out)
    torch.cuda.synchronize()
    return rc, m, [t.cpu().numpy() for t in out]


def _untouched(got):
    return all((g == FILL).all() for g in got)


def _check(owner, n, what, want=None, spare=5):
    """The device on a map with room for m + spare edges against the reference (and the hand-written expectation): the first m rows, the
    rows behind them untouched."""
    ref = adj.adjacency_reference(owner, n)
    if want is not None:
        AC.equal(ref, want, what + ' (by hand)')
    rc, m, got = _raw(owner, n, ref[3] + spare)
    assert rc == hip.OK and m == ref[3], (what, rc, m, ref[3])
    AC.equal((got[0][:m], got[1][:m], got[2][:n], m), ref, what)
    assert (got[0][m:] == FILL).all() and (got[1][m:] == FILL).all() and (n > 0 or _untouched(got)), what
    return ref


# ---- 1: the smallest maps
def test_the_smallest_maps(hip_device):
    for name, case in AC.smallest().items():
        _check(case[0], case[1], name, AC.as_arrays(case))
        _check(case[0], case[1], name + ', no room to spare', spare=0)


# ---- 2: merges across tiles
def test_one_edge_from_many_tiles(hip_device):
    for name, case in (('checkerboard', AC.checkerboard()), ('stripes', AC.stripes()), ('far apart', AC.far_apart())):
        ref = _check(case[0], case[1], name, AC.as_arrays(case))
        assert ref[3] == len(case[2]) and ref[1].tolist() == case[3]
    assert AC.checkerboard()[3] == [544] and AC.stripes()[3] == [18] * 32 and AC.far_apart()[3] == [3]


# ---- 3: a long row
@pytest.mark.parametrize('descending', [False, True])
@pytest.mark.parametrize('upright', [False, True])
def test_a_row_with_300_neighbours(hip_device, descending, upright):
    case = AC.long_row(descending, upright)
    ref = _check(case[0], case[1], f'long row, descending {descending}, upright {upright}', AC.as_arrays(case))
    assert ref[2][300 if descending else 0] == 300 and ref[3] == 300 and (ref[1] == 2).all()


def test_two_rows_of_130_sites_owner_0_with_129_neighbours(hip_device):
    """Row 0 of the map is all owner 0, row 1 holds the owners 1 .. 129 and then 0: owner 0 is the smaller row of 129 edges, a segment
    longer than 64 that the gather fills in arrival order over nine tiles and the place stage ranks."""
    own = np.stack([np.zeros(130, np.int64), np.concatenate([np.arange(1, 130), [0]])])
    ref = _check(own, 130, '2 x 130')
    assert int((ref[0][:, 0] == 0).sum()) == 129 and ref[2][0] == 129 and ref[3] == 129 + 128


# ---- 4: a full tile table
@pytest.mark.parametrize('W, H, n, free', [(64, 64, 2000, 0.0), (53, 37, 40, 0.0), (53, 37, 40, 0.25)])
def test_random_owners_at_every_site(hip_device, W, H, n, free):
    own = AC.random_map(W, H, n, seed=W + n, free=free)[0]
    ref = _check(own, n, f'{W} x {H} of {n}')
    if n == 2000:
        assert ref[3] > 0.95 * (2 * W * H - W - H)                                          # almost every site pair is an edge of its own
    else:
        assert ref[3] <= n * (n - 1) // 2 and ref[1].max() > 1


# ---- 5: many tiles in x
def test_a_window_of_70000_by_2_sites(hip_device):
    own, n = AC.wide()[:2]
    assert own.shape == (2, 70000)
    ref = _check(own, n, '70000 x 2')
    assert ref[3] > 20000 and (own[:, -600:] >= 0).any() and ref[2].min() > 0


# ---- 6: the protocol
def test_capacity_protocol(hip_device):
    own, n = AC.random_map(53, 37, 40, seed=3, free=0.1)[:2]
    ref = adj.adjacency_reference(own, n)
    m = ref[3]
    assert m > 100
    for cap in (0, m - 1, m, m + 5):
        rc, got_m, got = _raw(own, n, cap)
        assert rc == hip.OK and got_m == m and np.array_equal(got[2], ref[2]), cap      # degree and m are always written
        if cap < m:
            assert _untouched(got[:2]), cap                                                # edges and shared stay untouched
        else:
            AC.equal((got[0][:m], got[1][:m], got[2], got_m), ref, f'cap {cap}')
            assert _untouched([got[0][m:], got[1][m:]])
    rc, got_m, got = _raw(np.full((3, 4), -1), 0, 0)                                       # n = 0
    assert rc == hip.OK and got_m == 0 and _untouched(got)
    rc, got_m, got = _raw(np.full((20, 33), -1), 5, 3)                                     # rows, and nobody owns anything
    assert rc == hip.OK and got_m == 0 and not got[2].any() and _untouched(got[:2])
    rc, got_m, got = _raw(np.full((20, 33), 2), 5, 3)                                      # one territory
    assert rc == hip.OK and got_m == 0 and not got[2].any() and _untouched(got[:2])


# ---- 7: refusals
@pytest.mark.parametrize('bad', [5, -2, 1 << 24, -(1 << 31)])
def test_an_owner_out_of_range_is_refused_with_every_output_untouched(hip_device, bad):
    for at in ((0, 0), (36, 52), (17, 16)):
        own = AC.random_map(53, 37, 5, seed=1)[0]
        own[at] = bad
        rc, m, got = _raw(own, 5, 4000)
        assert rc == hip.E_INVALID and m is None and _untouched(got), (bad, at)
    rc, m, got = _raw(np.zeros((2, 2)), 0, 4)                                              # n = 0 admits -1 alone
    assert rc == hip.E_INVALID and _untouched(got)


def test_arguments_out_of_range_and_null_pointers_are_refused(hip_device):
    dev = torch.device('cuda', 0)
    own = torch.zeros((4, 4), dtype=torch.int32, device=dev)
    out = adj.outputs(3, 8, dev, fill=FILL)
    fn = hip.load().nuhtc_territory_adjacency
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    good = dict(owner=vp(own), W=4, H=4, n=3, cap=8, edges=vp(out[0]), shared=vp(out[1]), degree=vp(out[2]))
    m = ctypes.c_int64(-7)
    call = lambda a, mp: fn(0, a['owner'], a['W'], a['H'], a['n'], a['cap'], a['edges'], a['shared'], a['degree'], mp, None)
    for change in (dict(W=0), dict(H=0), dict(W=-4), dict(W=1 << 15, H=(1 << 13) + 1), dict(n=-1), dict(n=(1 << 24) + 1), dict(cap=-1), dict(cap=1 << 31),
                   dict(owner=None), dict(degree=None), dict(edges=None), dict(shared=None)):
        assert call(dict(good, **change), ctypes.byref(m)) == hip.E_INVALID, change
    assert call(good, None) == hip.E_INVALID
    torch.cuda.synchronize()
    assert m.value == -7 and all((t == FILL).all().item() for t in out)
    assert call(dict(good, n=0, degree=None, cap=0, edges=None, shared=None), ctypes.byref(m)) == hip.E_INVALID      # owner 0 with n = 0
    assert call(good, ctypes.byref(m)) == hip.OK and m.value == 0                                                      # (the arguments as they are)


# ---- 8: end to end from points
def _cases():
    chain_p, chain_lab = PC.chain('shuffled')[:2]
    return {'patch 4': TC.patch(4), 'patch 1': TC.patch(1), 'ties 0': TC.ties(0), 'ties 1': TC.ties(1), 'labels': TC.labels_out_of_range(),
            'chain': (chain_p, chain_lab, 2, 8, 18), 'coincident': TC.coincident(2048),
            'uniform': TC.random_large('uniform') + (5,) + TC.LARGE_RS[0], 'clumps': TC.random_large('clumps') + (5,) + TC.LARGE_RS[1]}


def _built(case, win=None):
    p, lab, C, r, s = case
    return adj.build(p, lab, C, r / 2, s / 2, win=win, with_calls=True)


@pytest.mark.parametrize('name', list(_cases()))
def test_from_points_through_build(hip_device, name):
    case = _cases()[name]
    p, lab, C, r, s = case
    win = TC.default_window(case)
    graph, tallies, got_win, calls = _built(case)
    ref = tr.territory_reference(*case, win)
    want = adj.adjacency_reference(ref[0], len(p))
    assert got_win == win and calls in (1, 2)
    AC.equal(graph + (len(graph[0]),), want, name)
    TC.equal(tuple(ref[:2]) + tuple(tallies), ref, name + ': the tallies')
    assert np.array_equal(adj.contact_of(graph[0], graph[1], lab, C), tallies[3]), name    # the cross-check against the tally kernel
    again = _built(case)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(graph, again[0])) and all(a.tobytes() == b.tobytes() for a, b in zip(tallies, again[1]))
    if name in ('ties 0', 'uniform', 'patch 4'):                                           # the rows change with the order: against the reference on them
        order = np.random.default_rng(4).permutation(len(p))
        moved = (p[order], lab[order], C, r, s)
        graph = _built(moved)[0]
        AC.equal(graph + (len(graph[0]),), adj.adjacency_reference(tr.territory_reference(*moved, win)[0], len(p)), name + ', permuted rows')
    if name == 'patch 4':                                                                  # a sub-window: the edges visible in it
        sub = (win[0] + 5, win[1] + 3, win[2] - 9, win[3] - 7)
        graph = _built(case, sub)[0]
        AC.equal(graph + (len(graph[0]),), adj.adjacency_reference(ref[0][3:win[3] - 4, 5:win[2] - 4], len(p)), 'a sub-window')
    if name == 'coincident':
        assert want[3] == 0 and (ref[0] >= 0).any()
    elif name != 'chain':
        assert want[3] > len(np.unique(ref[0])) - 2 > 3


def test_a_second_call_when_the_first_guess_is_too_small(hip_device, monkeypatch):
    case = TC.patch(1)
    want = _built(case)
    monkeypatch.setattr(adj, 'first_edge_cap', lambda n: 2)
    graph, tallies, win, calls = _built(case)
    assert calls == 2 and len(graph[0]) > 2 and all(a.tobytes() == b.tobytes() for a, b in zip(graph, want[0]))
    with pytest.raises(ValueError, match='coarsen the pitch'):
        adj.build(np.array([[0, 0], [40000, 40000]], np.int32), [0, 1], 3, 4, 0.5)
    graph, tallies, win = adj.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, 4, 2)
    assert win == (0, 0, 1, 1) and graph[0].shape == (0, 2) and graph[1].shape == (0,) and graph[2].shape == (0,) and int(tallies[5]) == 1


# ---- 9: the profile
def test_profile_tags_of_one_call(hip_device):
    own, n = AC.stripes()[:2]
    hip.profile_enable(True)
    try:
        rc, m, got = _raw(own, n, 64)
        tags = {tag for tag in hip.profile_read() if tag.startswith('cell_adjacency')}
    finally:
        hip.profile_enable(False)
    assert rc == hip.OK and m == 32 and tags == {'cell_adjacency_count', 'cell_adjacency_insert', 'cell_adjacency_place'}, tags


# ---- 10: the tool
_run = points_util.run_tool


def test_cli_nuclei_adjacency(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-graph --nuclei-adjacency on the synthetic .npy slide of tests/points_util.py, with --merge: without the
    flag, with it, and with it on two ranks (three runs of the tool).  The folder gains exactly the one file, every other file is the same
    bytes as without the flag, the rows are those of <id>_nuclei_graph.npz, every integer equals the references on the file's own xy and
    label, every derived key equals `derive` of them, and the closing clause ends with the file's name."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-graph')
    flags = ['--nuclei-adjacency', '--adjacency-reach', '20', '--adjacency-pitch', '2.5']
    files = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d)))}
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    said = {'one': _run(base + flags + ['--save_dir', str(tmp_path / 'one'), '--merge'], env),
            'two': _run(base + flags + ['--save_dir', str(tmp_path / 'two'), '--merge', '--gpus', '2'], two)}
    z = {}
    for run in ('one', 'two'):
        assert 'territory borders between' in said[run] and 'closed territories, mean neighbours' in said[run]
        assert ') in s1_nuclei_adjacency.npz' in said[run], said[run][-400:]
        with_flag, without = files(run), files('merge0')
        assert sorted(with_flag) == sorted(list(without) + ['s1_nuclei_adjacency.npz']), run
        for f in without:
            assert with_flag[f] == without[f], (run, f)
        g = cellgraph.read_npz(str(folder(run) / 's1_nuclei_graph.npz'))
        z[run] = adj.read_npz(str(folder(run) / 's1_nuclei_adjacency.npz'))
        assert tuple(z[run]) == adj.NPZ_KEYS
        n = len(g['nuclei_id'])
        assert n > 10 and all(np.array_equal(z[run][k], g[k]) for k in ('nuclei_id', 'xy', 'label'))
        assert float(z[run]['reach_px']) == 20.0 and float(z[run]['pitch_px']) == 2.5
        pts = np.rint(2 * z[run]['xy']).astype(np.int32)
        win = tr.window(cellpoints.bounds_of(pts), 40, 5)
        assert z[run]['window'].tolist() == list(win)
        terr = tr.territory_reference(pts, z[run]['label'], 5, 40, 5, win)
        want = adj.adjacency_reference(terr[0], n)
        AC.equal(tuple(z[run][k] for k in adj.INT_NAMES) + (len(z[run]['edges']),), want, run)
        TC.equal(tuple(terr[:2]) + tuple(z[run][k] for k in tr.INT_NAMES), terr, run + ': the tallies')
        d = adj.derive(*want[:3], pts, z[run]['label'], 5, 5, terr[2], terr[4])
        for key in adj.DERIVED_KEYS:
            assert np.array_equal(z[run][key], d[key]) and z[run][key].dtype == d[key].dtype, (run, key)
        print(f"{run}: {n} nuclei, window {win}, {want[3]} edges, degree up to {int(want[2].max())}, closed {int(d['n_closed'].sum())}")
        assert want[3] > n
    for key in adj.NPZ_KEYS:
        assert np.array_equal(z['one'][key], z['two'][key]), key
