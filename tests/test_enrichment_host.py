"""The neighbourhood enrichment (nuhtc_amd/enrichment.py) without a GPU: the argument limits, the permutation generator, the brute-force
reference on contacts written out by hand, `derive`, the null mean of the shuffles against the expectation under a uniform permutation,
the row of the slide path's table and the file round trip."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from nuhtc_amd import enrichment as en
from nuhtc_amd import slidepoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the arguments
def test_check_args_at_its_limits():
    for good in ((1, 1, 1, 0), (14, 16384, 1024, 2 ** 32 - 1), (5, 128, 1000, 0)):
        en.check_args(*good)
    for bad in ((0, 1, 1, 0), (15, 1, 1, 0), (1, 0, 1, 0), (1, 16385, 1, 0), (1, 1, 0, 0), (1, 1, 1025, 0), (1, 1, 1, -1), (1, 1, 1, 2 ** 32),
                (1, 1.5, 1, 0), (1, 1, 2.5, 0)):
        with pytest.raises(ValueError):
            en.check_args(*bad)
    with pytest.raises(ValueError):
        en.permutation(2 ** 24 + 1, 0, 1)
    with pytest.raises(ValueError):
        en.permutation(5, 0, 0)


# ---- the generator
@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 1025, 4097])
def test_permutation_is_a_bijection(n):
    seen = []
    for seed, p in ((0, 1), (0, 2), (2 ** 32 - 1, 1), (2024, 1024)):
        pi, steps = en.permutation(n, seed, p, with_steps=True)
        assert pi.dtype == np.int64 and np.array_equal(np.sort(pi), np.arange(n)), (n, seed, p)
        assert (steps >= 1).all() if n > 1 else (steps == 0).all()
        seen.append(pi.tolist())
    if n >= 16:                                                    # different p and different seeds give different shuffles
        assert len({tuple(s) for s in seen}) == 4, n


def test_permutation_is_the_identity_for_at_most_one_row_and_follows_the_definition():
    assert en.permutation(0, 3, 1).tolist() == [] and en.permutation(1, 3, 7).tolist() == [0]
    assert int(en._fmix(0)) == 0 and int(en._fmix(1)) == 0x514E28B7 and int(en._fmix(0xFFFFFFFF)) == 0x81F16F39   # murmur3's finaliser
    assert [en.half_bits(n) for n in (2, 4, 5, 16, 17, 1025, 4097, 2 ** 24)] == [1, 1, 2, 2, 3, 6, 7, 12]
    # the definition once more in plain Python integers, element by element
    n, seed, p = 37, 99, 5
    fmix = lambda v: int(en._fmix(v & 0xFFFFFFFF))
    h = 3
    mask = 7
    base = fmix(seed + 0x9E3779B9 * p)
    keys = [fmix(base + 0x7F4A7C15 * (k + 1)) for k in range(6)]
    assert keys == en.round_keys(seed, p)

    def F(x):
        L, R = x >> h, x & mask
        for k in range(6):
            L, R = R, L ^ (fmix(R + keys[k]) & mask)
        return (L << h) | R

    want = []
    for i in range(n):
        x = F(i)
        while x >= n:
            x = F(x)
        want.append(x)
    assert en.permutation(n, seed, p).tolist() == want


# ---- the reference against contacts written out by hand
def test_reference_on_a_hand_worked_case():
    p = np.array([[0, 0], [3, 4], [6, 8], [100, 100], [3, 4]])     # 0-1 and 1-2 are 5 apart, 0-2 is 10; 4 lies ON 1; 3 is alone
    lab = np.array([0, 1, 0, 1, 7])                                # 7: no class of C = 2, but its row is shuffled like the others
    near = [(0, 1), (1, 0), (1, 2), (2, 1), (0, 4), (4, 0), (4, 2), (2, 4), (1, 4), (4, 1)]        # r = 5, inclusive; coincident counts
    far = near + [(0, 2), (2, 0)]                                  # r = 10

    def by_hand(pairs, labels):
        t = np.zeros((2, 2), np.int64)
        for i, j in pairs:
            if labels[i] < 2 and labels[j] < 2:
                t[labels[i], labels[j]] += 1
        return t

    for r, pairs in ((5, near), (9, near), (10, far)):
        obs, perm, cn = en.enrichment_reference(p, lab, 2, r, 3, 11)
        assert obs.dtype == perm.dtype == cn.dtype == np.int64 and perm.shape == (3, 2, 2)
        assert np.array_equal(obs, by_hand(pairs, lab)) and cn.tolist() == [2, 2]
        for k in range(3):
            assert np.array_equal(perm[k], by_hand(pairs, lab[en.permutation(5, 11, k + 1)])), (r, k)
    obs = en.enrichment_reference(p, lab, 2, 5, 1, 0)[0]
    assert obs.tolist() == [[0, 2], [2, 0]] and en.enrichment_reference(p, lab, 2, 10, 1, 0)[0].tolist() == [[2, 2], [2, 0]]
    empty = en.enrichment_reference(np.zeros((0, 2)), np.zeros(0), 3, 4, 2, 0)
    assert [a.shape for a in empty] == [(3, 3), (2, 3, 3), (3,)] and not any(a.any() for a in empty)


# ---- derive
def test_derive_on_hand_made_counts():
    perm = np.zeros((4, 2, 2), np.int64)
    perm[:, 0, 0] = [1, 2, 3, 4]
    perm[:, 0, 1] = [5, 5, 5, 5]                                   # std 0
    perm[:, 1, 0] = [0, 10, 0, 10]
    obs = np.array([[3, 9], [12, 0]])
    d = en.derive(obs, perm)
    assert set(d) == set(en.DERIVED_KEYS) and all(d[k].dtype == np.float64 and d[k].shape == (2, 2) and np.isfinite(d[k]).all() for k in d)
    assert d['mean'].tolist() == [[2.5, 5.0], [5.0, 0.0]] and d['std'][0, 1] == 0 and d['std'][1, 0] == 5.0 and d['std'][0, 0] == np.sqrt(1.25)
    assert d['z'][0, 1] == 0 and d['z'][1, 1] == 0 and d['z'][1, 0] == 7 / 5 and d['z'][0, 0] == 0.5 / np.sqrt(1.25)
    assert d['p_enriched'].tolist() == [[3 / 5, 1 / 5], [1 / 5, 5 / 5]]     # (1 + #{perm >= observed}) / (P + 1)
    assert d['p_depleted'].tolist() == [[4 / 5, 5 / 5], [5 / 5, 5 / 5]]     # (1 + #{perm <= observed}) / (P + 1)
    with pytest.raises(ValueError):
        en.derive(obs, perm[:, :1])


def test_two_separate_blobs_are_enriched_within_and_depleted_between():
    rng = np.random.default_rng(3)
    p = np.concatenate([rng.integers(0, 60, (60, 2)), rng.integers(0, 60, (60, 2)) + 500])     # far beyond the radius: no contact between the blobs
    lab = np.repeat([0, 1], 60)
    order = rng.permutation(120)
    obs, perm, cn = en.enrichment_reference(p[order], lab[order], 2, 30, 200, 5)
    d = en.derive(obs, perm)
    assert cn.tolist() == [60, 60] and np.array_equal(obs, obs.T) and obs[0, 1] == 0 and obs[0, 0] > 0 and obs[1, 1] > 0
    assert (np.diag(d['z']) > 3).all() and d['z'][0, 1] < -3 and d['z'][1, 0] < -3
    assert (np.diag(d['p_enriched']) == 1 / 201).all() and d['p_depleted'][0, 1] == 1 / 201 and (np.diag(d['p_depleted']) == 1).all()
    assert (perm.sum(axis=(1, 2)) == obs.sum()).all()              # every label is known: a shuffle moves contacts between entries only


# ---- the null mean: a property of a uniform shuffle, so the bound is derived
def test_null_mean_matches_a_uniform_shuffle():
    """Under a uniform permutation with all labels known, E[count[a][b]] = M n_a n_b / (n (n - 1)) for a != b and M n_a (n_a - 1) /
    (n (n - 1)) for a = b, M the number of contacts.  Every entry's mean over P = 1024 permutations must lie within 5 standard errors
    (std with ddof 1, over sqrt(P)) of it."""
    rng = np.random.default_rng(7)
    n = 1500
    p = rng.integers(0, 2000, (n, 2))
    lab = rng.choice(4, n, p=[.5, .3, .15, .05])
    obs, perm, cn = en.enrichment_reference(p, lab, 4, 60, 1024, 2024)
    M = int(obs.sum())
    assert M > 0 and (perm.sum(axis=(1, 2)) == M).all() and cn.sum() == n
    na = cn.astype(np.float64)
    expect = M * (np.outer(na, na) - np.diag(na)) / (n * (n - 1.0))
    se = perm.std(axis=0, ddof=1) / np.sqrt(1024)
    dev = np.abs(perm.mean(axis=0) - expect) / se
    print('largest deviation of a null mean, in standard errors:', float(dev.max()))
    assert (se > 0).all() and (dev <= 5).all(), dev


# ---- the table of the slide path
@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('infer_wsi_for_enrichment', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(tool, *flags):
    return tool.parse_args(['slide.npy', 'config.py', 'weights.pth', *flags])


@pytest.mark.parametrize('bad', [['--enrichment-perms', '1025'], ['--enrichment-perms', '0'], ['--enrichment-radius', '0.25'],
                                 ['--enrichment-radius', '9000'], ['--enrichment-seed', '-1'], ['--enrichment-seed', str(2 ** 32)]])
def test_a_bad_argument_is_named_before_the_missing_gpu(tool, monkeypatch, bad):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SystemExit) as e:
        slidepoints.select(_args(tool, '--nuclei-enrichment', *bad))
    assert str(e.value).startswith('--nuclei-enrichment: ') and 'no GPU' not in str(e.value), str(e.value)


def test_the_flag_alone_reports_the_missing_gpu(tool, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SystemExit) as e:
        slidepoints.select(_args(tool, '--nuclei-enrichment'))
    assert str(e.value) == '--nuclei-enrichment: no GPU is visible (there is no fallback)'


def test_the_row_stands_between_the_six_and_regions(tool, tmp_path):
    assert len(slidepoints.ANALYSES) == 6 and 'enrichment' not in [a.module for a in slidepoints.ANALYSES]
    assert [a.module for a in slidepoints.AGAINST_CHANCE] == ['enrichment'] and slidepoints.AGAINST_CHANCE[0].second is None
    plain = _args(tool)
    assert plain.nuclei_enrichment is False and (plain.enrichment_radius, plain.enrichment_perms, plain.enrichment_seed) == (64.0, 1000, 0)
    chosen = slidepoints.select(_args(tool, '--nuclei-regions', str(tmp_path), '--nuclei-enrichment', '--enrichment-radius', '12.5', '--enrichment-perms',
                                      '16', '--enrichment-seed', '7', '--nuclei-density', '--nuclei-graph'), need_gpu=False)
    assert [an.cli for an, _ in chosen] == ['nuclei_graph', 'nuclei_density', 'nuclei_enrichment', 'nuclei_regions']
    assert chosen[2][1] == (12.5, 16, 7) and chosen[2][0].suffix == '_nuclei_enrichment.npz' and chosen[2][0].flag == '--nuclei-enrichment'
    obs = np.array([[4, 1], [1, 10]])
    perm = np.array([[[2, 3], [3, 8]], [[3, 2], [2, 9]]])
    said = chosen[2][0].said(en, (obs, perm, np.array([3, 5])), chosen[2][1])
    assert said == '16 contacts within 12.5 px against 16 label permutations (seed 7; largest |z|: class 0 next to class 0, z +3.00)', said


def test_no_flag_selects_nothing_and_imports_nothing(tool, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.delitem(sys.modules, 'nuhtc_amd.enrichment', raising=False)
    assert slidepoints.select(_args(tool)) == ()
    assert 'nuhtc_amd.enrichment' not in sys.modules


# ---- the file
def test_npz_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    p = rng.integers(0, 80, (40, 2))
    lab = rng.integers(0, 3, 40)
    found = en.enrichment_reference(p, lab, 3, 24, 5, 9)
    path = en.write_npz(str(tmp_path / 's_nuclei_enrichment.npz'), np.arange(40) * 2, p / 2, lab, *found, radius_px=12.0, seed=9)
    z = en.read_npz(path)
    with np.load(path, allow_pickle=False) as plain:               # nothing pickled, nothing beyond the keys
        assert set(plain.files) == set(en.NPZ_KEYS)
    assert z['nuclei_id'].tolist() == list(range(0, 80, 2)) and np.array_equal(z['xy'], p / 2) and np.array_equal(z['label'], lab)
    assert float(z['radius_px']) == 12.0 and int(z['perms']) == 5 and int(z['seed']) == 9 and z['perms'].dtype == z['seed'].dtype == np.int64
    for key, want in zip(('observed', 'perm_counts', 'class_n'), found):
        assert np.array_equal(z[key], want) and z[key].dtype == np.int64, key
    d = en.derive(found[0], found[1])
    for key in en.DERIVED_KEYS:
        assert np.array_equal(z[key], d[key]) and z[key].dtype == np.float64, key
    with pytest.raises(ValueError):
        en.write_npz(str(tmp_path / 'bad.npz'), np.arange(40), p / 2, lab, found[0], found[1][:, :2], found[2], radius_px=12.0, seed=9)
    with pytest.raises(ValueError):
        en.write_npz(str(tmp_path / 'bad.npz'), np.arange(39), p / 2, lab, *found, radius_px=12.0, seed=9)
