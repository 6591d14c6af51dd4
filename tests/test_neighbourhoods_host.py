"""The cellular neighbourhoods (nuhtc_amd/neighbourhoods.py) without a GPU: the argument limits, the reference's windows against a plain
loop over the graph, the generator against hand values and the library's host export, the seeding against cumsum / searchsorted, Lloyd
against a restatement in Python integers, the hand cases of tests/neighbourhoods_cases.py, `derive`, the file round trip and
`read_centres`' refusals, the row of the slide path's table, and the stand-alone host check under ASan and UBSan."""
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import neighbourhoods_cases as NC
from nuhtc_amd import cellgraph, slidepoints
from nuhtc_amd import neighbourhoods as nh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the arguments
def test_check_args_at_its_limits():
    for good in ((1, 1, 1, 1, 0, 1), (14, 16384, 32, 32, 2 ** 32 - 1, 1000), (5, 128, 10, 8, 0, 100)):
        nh.check_args(*good)
    for bad in ((0, 1, 1, 1, 0, 1), (15, 1, 1, 1, 0, 1), (1, 0, 1, 1, 0, 1), (1, 16385, 1, 1, 0, 1), (1, 1, 0, 1, 0, 1), (1, 1, 33, 1, 0, 1), (1, 1, 1, 0, 0, 1),
                (1, 1, 1, 33, 0, 1), (1, 1, 1, 1, -1, 1), (1, 1, 1, 1, 2 ** 32, 1), (1, 1, 1, 1, 0, 0), (1, 1, 1, 1, 0, 1001), (1, 1, 1.5, 1, 0, 1), (1, 1, 1, 2.5, 0, 1)):
        with pytest.raises(ValueError):
            nh.check_args(*bad)
    assert nh.as_centres([[0, 34000]], 1, 2).tolist() == [[0, 34000]]
    for bad in ([[0, 34001]], [[-1, 0]], [[0.5, 1]], [[0, 1, 2]], [[0, 1], [2, 3]]):
        with pytest.raises(ValueError):
            nh.as_centres(bad, 1, 2)


# ---- the windows against a plain loop over the graph
@pytest.mark.parametrize('name', ['sparse', 'one_class_one_neighbour', 'fourteen_classes_32_neighbours'])
def test_windows_against_a_plain_loop(name):
    p, lab, C, r, k, K, seed, max_iter = NC.point_cases()[name]
    nb = cellgraph.graph_reference(p, lab, C, r, k)[0].tolist()
    want = []
    for i, row in enumerate(nb):
        w = [0] * C
        for j in [i] + [j for j in row if j >= 0]:
            if 0 <= lab[j] < C:
                w[lab[j]] += 1
        want.append(w)
    got = NC.point_reference(name)[0]
    assert got.dtype == np.int32 and got.tolist() == want and max(map(sum, want)) <= k + 1
    with pytest.raises(ValueError):
        nh.windows_of([[1, 2], [0, -2]], [0, 1], 2)
    with pytest.raises(ValueError):
        nh.windows_of([[1, 2], [0, -1]], [0, 1], 2)


# ---- the generator
def test_generator_against_hand_values_and_the_library():
    fmix = lambda v: int(nh._fmix(v & 0xFFFFFFFF))
    assert fmix(0) == 0 and fmix(1) == 0x514E28B7 and fmix(0xFFFFFFFF) == 0x81F16F39               # murmur3's finaliser
    b = fmix(0x9E3779B9)
    assert nh.draws(0, 1) == [(fmix(b + 0x7F4A7C15) << 32) | fmix(b + 2 * 0x7F4A7C15)] == [17234813504040894259]
    b = fmix(0xFFFFFFFF + 0x9E3779B9 * 32)                                                         # wraps mod 2**32
    assert nh.draws(2 ** 32 - 1, 32)[31] == (fmix(b + 0x7F4A7C15) << 32) | fmix(b + 2 * 0x7F4A7C15)
    assert len(set(nh.draws(7, 32))) == 32 and nh.draws(7, 32)[:5] == nh.draws(7, 5) and all(0 <= u < 2 ** 64 for u in nh.draws(7, 32))
    for seed in (0, 1, 2024, 2 ** 32 - 1):
        assert nh.host_draws(seed, 32) == nh.draws(seed, 32), seed
    with pytest.raises(ValueError):
        nh.host_draws(0, 33)


def test_the_library_rules_on_the_host():
    prefix = np.cumsum([0, 3, 0, 4, 1, 0])
    assert [nh.host_rule('pick', prefix, t) for t in range(8)] == [nh.pick(prefix, t) for t in range(8)] == [1, 1, 1, 3, 3, 3, 3, 4]
    assert nh.host_rule('round', 1025, 2048) == 513 and nh.host_rule('round', 1023, 2048) == 512 and nh.host_rule('round', 0, 0, 99) == 99
    assert nh.host_rule('distance', [1, 2], [1000, 3000]) == 24 ** 2 + 952 ** 2
    assert nh.host_rule('distance', [33] + [0] * 13, [0] + [34000] * 13) == 33792 ** 2 + 13 * 34000 ** 2


# ---- the seeding against cumsum / searchsorted
@pytest.mark.parametrize('name', ['pick_t_is_prefix_minus_1', 'pick_t_is_prefix', 'one_past_a_block', 'a_type_loses_all_members', 'more_types_than_windows'])
def test_seeding_against_cumsum_and_searchsorted(name):
    nb, lab, C, K, seed, _, _ = NC.list_cases()[name]
    w = nh.windows_of(nb, lab, C).tolist()
    n, u = len(w), nh.draws(seed, K)
    d2 = lambda a, b: sum((x - y) ** 2 for x, y in zip(a, b))
    rows = [u[0] % n]
    for j in range(1, K):
        g = [min(d2(w[i], w[r]) for r in rows) for i in range(n)]
        T = sum(g)
        rows.append(rows[0] if T == 0 else int(np.searchsorted(np.cumsum(g), u[j] % T, side='right')))
    assert NC.list_reference(name)[5].tolist() == rows
    if name.startswith('pick_t'):                                   # the designed sides of the pick
        g = [d2(w[i], w[rows[0]]) for i in range(n)]
        prefix, t = np.cumsum(g), u[1] % sum(g)
        assert g[rows[1]] > 1 and (t == prefix[rows[1]] - 1 if name.endswith('minus_1') else t == prefix[rows[1] - 1] > 0)


# ---- Lloyd against a restatement in Python integers
def _lloyd(w, q, max_iter):
    K, C = len(q), len(q[0])
    before, t = [-1] * len(w), 0
    while True:
        t += 1
        D = [[sum((1024 * x - y) ** 2 for x, y in zip(row, centre)) for centre in q] for row in w]
        a = [d.index(min(d)) for d in D]                             # the first of equals
        if a == before or t == max_iter:
            break
        for j in range(K):
            mine = [row for row, at in zip(w, a) if at == j]
            if mine:
                q[j] = [(2 * 1024 * sum(col) + len(mine)) // (2 * len(mine)) for col in zip(*mine)]
        before = a
    return a, q, sum(min(d) for d in D), t, a == before


@pytest.mark.parametrize('name', ['pick_t_is_prefix', 'one_past_a_block', 'a_type_loses_all_members', 'half_rounds_up', 'fewer_rows_than_types', 'one_row'])
def test_lloyd_against_python_integers(name):
    nb, lab, C, K, seed, max_iter, _ = NC.list_cases()[name]
    window, hood, q, s, m, rows, inertia, n_iter, converged = NC.list_reference(name)
    w = window.tolist()
    a, centres, total, t, done = _lloyd(w, [[1024 * x for x in w[r]] for r in rows], max_iter)
    assert hood.tolist() == a and q.tolist() == centres and (inertia, n_iter, converged) == (total, t, done)
    assert s.tolist() == [[sum(w[i][c] for i in range(len(w)) if a[i] == j) for c in range(C)] for j in range(K)] and m.tolist() == [a.count(j) for j in range(K)]
    if n_iter > 2:                                                   # one iteration fewer: stopped by max_iter, on other centres
        short = NC.list_reference(name, n_iter - 1)
        a, centres, total, t, done = _lloyd(w, [[1024 * x for x in w[r]] for r in rows], n_iter - 1)
        assert short[1].tolist() == a and short[2].tolist() == centres and short[6:] == (total, n_iter - 1, False) and not done


def test_the_hand_cases():
    ref = NC.list_reference
    assert ref('half_rounds_up')[2].tolist() == [[513, 512]] and ref('half_rounds_up')[7:] == (2, True)
    tie = ref('tie_goes_to_the_smaller_type')
    assert tie[1].tolist() == [0, 0, 1] and tie[5].tolist() == [-1, -1, -1] and tie[6:] == (3 * 1024 ** 2, 0, True)
    dup = ref('duplicate_given_centres')
    assert dup[4][1] == 0 and dup[2].tolist() == [[1024, 0], [1024, 0], [0, 1024]] and dup[6] == 0 and set(dup[1].tolist()) == {0, 2}
    lost = ref('a_type_loses_all_members')
    assert lost[4].tolist() == [7, 2, 0] and lost[7:] == (3, True)
    assert ref('all_rows_equal')[5].tolist() == [120, 120, 120] and ref('all_rows_equal')[4].tolist() == [300, 0, 0]
    assert ref('one_row')[5].tolist() == [0] * 4 and ref('fewer_rows_than_types')[4].sum() == 3
    assert ref('pick_in_first_block')[5][1] < 256 and ref('pick_in_last_block')[5][1] >= 768
    zones = ref('zones_20000')
    assert zones[8] and 7 <= zones[7] <= 22
    empty = nh.neighbourhoods_reference(np.zeros((0, 2)), np.zeros(0), 3, 8, 5, 4)
    assert [np.shape(x) for x in empty[:6]] == [(0, 3), (0,), (4, 3), (4, 3), (4,), (4,)] and empty[5].tolist() == [-1] * 4 and empty[6:] == (0, 0, True)
    given = nh.neighbourhoods_reference(np.zeros((0, 2)), np.zeros(0), 3, 8, 5, 2, centres=[[1, 2, 3], [4, 5, 6]])
    assert given[2].tolist() == [[1, 2, 3], [4, 5, 6]] and given[2].dtype == np.int32


# ---- derive
def test_derive_on_hand_made_counts():
    hood = [0, 0, 2, 2, 2, 0]
    lab = [0, 1, 1, 7, 1, -1]
    s = np.array([[6, 3], [0, 0], [0, 6]])
    m = np.array([3, 0, 3])
    d = nh.derive(hood, s, m, 3 * 1024 ** 2, lab)
    assert set(d) == set(nh.DERIVED_KEYS) and all(np.isfinite(d[k]).all() for k in d)
    assert d['composition'].tolist() == [[2, 1], [0, 0], [0, 2]] and d['fraction'].tolist() == [[2 / 3, 1 / 3], [0, 0], [0, 1]]
    slide = np.array([6 / 15, 9 / 15])
    assert d['enrichment_log2'][0].tolist() == np.log2(np.array([2 / 3, 1 / 3]) / slide).tolist() and d['enrichment_log2'][1].tolist() == [0, 0]
    assert d['enrichment_log2'][2].tolist() == [0, float(np.log2(1 / slide[1]))]
    assert d['hood_class_count'].tolist() == [[1, 1], [0, 0], [0, 2]] and d['hood_class_count'].dtype == np.int64
    assert d['hood_size'].tolist() == [3, 0, 3] and d['order_by_size'].tolist() == [0, 2, 1] and float(d['inertia_per_nucleus']) == 0.5
    none = nh.derive([], np.zeros((2, 3), np.int64), [0, 0], 0, [])
    assert all(np.isfinite(none[k]).all() for k in none) and not none['composition'].any() and float(none['inertia_per_nucleus']) == 0
    assert none['order_by_size'].tolist() == [0, 1]
    with pytest.raises(ValueError):
        nh.derive(hood, s, m[:2], 0, lab)


# ---- the file
def test_npz_round_trip_and_read_centres(tmp_path):
    p, lab, C, r, k, K, seed, max_iter = NC.point_cases()['sparse']
    found = NC.point_reference('sparse')
    n = len(p)
    path = nh.write_npz(str(tmp_path / 's_nuclei_neighbourhoods.npz'), np.arange(n) * 2, p / 2, lab, *found, radius_px=r / 2, k=k, seed=seed, max_iter=max_iter)
    z = nh.read_npz(path)
    with np.load(path, allow_pickle=False) as plain:                 # nothing pickled, nothing beyond the keys
        assert set(plain.files) == set(nh.NPZ_KEYS)
    assert z['nuclei_id'].tolist() == list(range(0, 2 * n, 2)) and np.array_equal(z['xy'], p / 2) and np.array_equal(z['label'], lab)
    for key, want, t in zip(nh.INT_NAMES, found[:6], nh.INT_TYPES):
        assert np.array_equal(z[key], want) and z[key].dtype == t, key
    assert (int(z['inertia']), int(z['n_iter']), bool(z['converged'])) == found[6:] and z['inertia'].dtype == z['n_iter'].dtype == z['converged'].dtype == np.int64
    assert (float(z['radius_px']), int(z['k']), int(z['types']), int(z['seed']), int(z['max_iter']), int(z['centres_given'])) == (r / 2, k, K, seed, max_iter, 0)
    d = nh.derive(found[1], found[3], found[4], found[6], lab)
    for key in nh.DERIVED_KEYS:
        assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype, key
    with pytest.raises(ValueError):
        nh.write_npz(str(tmp_path / 'bad.npz'), np.arange(n - 1), p / 2, lab, *found, radius_px=r / 2, k=k)
    with pytest.raises(ValueError):
        nh.write_npz(str(tmp_path / 'bad.npz'), np.arange(n), p / 2, lab, found[0], found[1], found[2][:, :2], *found[3:], radius_px=r / 2, k=k)
    # the centres, for another slide
    q = nh.read_centres(path, k=k, radius_px=r / 2, num_classes=C)
    assert q.dtype == np.int32 and np.array_equal(q, found[2]) and np.array_equal(nh.read_centres(path), q)
    again = nh.neighbourhoods_reference(p, lab, C, r, k, K, seed, max_iter, centres=q)
    assert np.array_equal(again[1], found[1]) and again[7:] == (0, True) and again[6] == found[6]
    given = nh.write_npz(str(tmp_path / 'given.npz'), np.arange(n), p / 2, lab, *again, radius_px=r / 2, k=k)
    assert int(nh.read_npz(given)['centres_given']) == 1
    for wrong in (dict(k=k + 1), dict(radius_px=r / 2 + 0.5), dict(num_classes=C + 1)):
        with pytest.raises(ValueError, match='were fitted at'):
            nh.read_centres(path, **wrong)
    np.savez(str(tmp_path / 'other.npz'), centre_q=found[2])
    for no_file in (str(tmp_path / 'missing.npz'), str(tmp_path / 'other.npz')):
        with pytest.raises(ValueError, match='is no file of'):
            nh.read_centres(no_file)


# ---- the table of the slide path
@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('infer_wsi_for_neighbourhoods', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(tool, *flags):
    return tool.parse_args(['slide.npy', 'config.py', 'weights.pth', *flags])


@pytest.mark.parametrize('bad', [['--neighbourhood-k', '0'], ['--neighbourhood-k', '33'], ['--neighbourhood-radius', '0.25'], ['--neighbourhood-radius', '9000'],
                                 ['--neighbourhood-types', '0'], ['--neighbourhood-types', '33'], ['--neighbourhood-seed', '-1'],
                                 ['--neighbourhood-seed', str(2 ** 32)], ['--neighbourhood-iters', '0'], ['--neighbourhood-iters', '1001'],
                                 ['--neighbourhood-centres', '/nowhere/at_all.npz']])
def test_a_bad_argument_is_named_before_the_missing_gpu(tool, monkeypatch, bad):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SystemExit) as e:
        slidepoints.select(_args(tool, '--nuclei-neighbourhoods', *bad))
    assert str(e.value).startswith('--nuclei-neighbourhoods: ') and 'no GPU' not in str(e.value), str(e.value)


def test_the_flag_alone_reports_the_missing_gpu(tool, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SystemExit) as e:
        slidepoints.select(_args(tool, '--nuclei-neighbourhoods'))
    assert str(e.value) == '--nuclei-neighbourhoods: no GPU is visible (there is no fallback)'


def test_the_row_stands_behind_the_outlines_and_before_chance(tool, tmp_path):
    assert len(slidepoints.ANALYSES) == 6 and [a.module for a in slidepoints.OF_THE_COMPANY] == ['neighbourhoods']
    row = slidepoints.OF_THE_COMPANY[0]
    assert row._fields == slidepoints.ANALYSES[0]._fields and row.second is None and row.missing is None and row.order is None and row.more is None
    assert (row.cli, row.flag, row.suffix) == ('nuclei_neighbourhoods', '--nuclei-neighbourhoods', '_nuclei_neighbourhoods.npz')
    plain = _args(tool)
    assert plain.nuclei_neighbourhoods is False and plain.neighbourhood_centres is None
    assert (plain.neighbourhood_k, plain.neighbourhood_radius, plain.neighbourhood_types, plain.neighbourhood_seed, plain.neighbourhood_iters) == (10, 64.0, 8, 0, 100)
    chosen = slidepoints.select(_args(tool, '--nuclei-regions', str(tmp_path), '--nuclei-enrichment', '--nuclei-neighbourhoods', '--neighbourhood-k', '4',
                                      '--neighbourhood-radius', '12.5', '--neighbourhood-types', '3', '--neighbourhood-seed', '7', '--nuclei-outline',
                                      '--nuclei-graph'), need_gpu=False)
    assert [an.cli for an, _ in chosen] == ['nuclei_graph', 'nuclei_outline', 'nuclei_neighbourhoods', 'nuclei_enrichment', 'nuclei_regions']
    assert chosen[2][1] == (12.5, 4, 3, 7, 100, None)
    found = NC.point_reference('sparse')
    said = row.said(nh, found, (12.0, 4, 3, 5, 50, None))
    assert said == ('3 of 3 neighbourhood types in use (2 iterations, converged; seed 5; k 4, 12 px); the largest, type 1, holds 37 nuclei around class '
                    f'{int(found[3][1].argmax())}'), said
    # the centres of an earlier file: its number of types is taken; another k or radius is refused in the flag's name
    p, lab, C, r, k, K, seed, max_iter = NC.point_cases()['sparse']
    path = nh.write_npz(str(tmp_path / 'fit.npz'), np.arange(len(p)), p / 2, lab, *found, radius_px=r / 2, k=k, seed=seed, max_iter=max_iter)
    given = ['--nuclei-neighbourhoods', '--neighbourhood-centres', path, '--neighbourhood-types', '9']
    (an, params), = slidepoints.select(_args(tool, *given, '--neighbourhood-k', '4', '--neighbourhood-radius', '12'), need_gpu=False)
    assert params[:5] == (12.0, 4, 3, 0, 100) and np.array_equal(params[5], found[2])
    assert 'assigned to given centres' in an.said(nh, found[:7] + (0, True), params)
    for other in (['--neighbourhood-k', '5', '--neighbourhood-radius', '12'], ['--neighbourhood-k', '4', '--neighbourhood-radius', '12.5']):
        with pytest.raises(SystemExit) as e:
            slidepoints.select(_args(tool, *given, *other), need_gpu=False)
        assert str(e.value).startswith('--nuclei-neighbourhoods: ') and 'were fitted at' in str(e.value)


def test_no_flag_selects_nothing_and_imports_nothing(tool, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.delitem(sys.modules, 'nuhtc_amd.neighbourhoods', raising=False)
    assert slidepoints.select(_args(tool)) == ()
    assert 'nuhtc_amd.neighbourhoods' not in sys.modules


# ---- the plain-C++ rules under ASan and UBSan, in a program of their own
def test_the_host_check_is_clean_under_the_sanitizers(tmp_path):
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'a host C++ compiler builds tools/dev/cellhood_host_check.cpp'
    exe = str(tmp_path / 'cellhood_host_check')
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wno-unknown-pragmas', '-I',
                            os.path.join(ROOT, 'nuhtc_amd', 'csrc'), os.path.join(ROOT, 'tools', 'dev', 'cellhood_host_check.cpp'), '-o', exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith('cellhood host check ok') and not run.stderr, (run.stdout[-1000:], run.stderr[-2000:])
