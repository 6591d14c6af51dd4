"""The designed sets of the cellular-neighbourhood tests (tests/test_neighbourhoods_host.py, tests/test_hip_neighbourhoods.py) and their
references, each computed once.  Two kinds: POINT cases (points, labels, C, r half pixels, k, K, seed, max_iter) go through the graph and
exercise the window; LIST cases (neighbors, labels, C, K, seed, max_iter, centres) hand a neighbour list to the clustering directly, so
the windows can be designed -- with every neighbour -1 a row's window is the one-hot of its own label.  Every comparison is `==`."""
import functools

import numpy as np

from nuhtc_amd import neighbourhoods as nh

NAMES = ('window', 'hood', 'centre_q', 'centre_sum', 'centre_n', 'seed_rows', 'inertia', 'n_iter', 'converged')


def equal(got, want, what):
    assert len(got) == len(want) == 9, what
    for name, g, w in zip(NAMES[:6], got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, f'{len(bad)} entries differ, first at {bad[0].tolist()}', int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))
    assert tuple(got[6:]) == tuple(want[6:]), (what, 'inertia, n_iter, converged', got[6:], want[6:])


# ---- point cases: the window
@functools.lru_cache(maxsize=None)
def point_cases():
    rng = np.random.default_rng(11)
    sparse = np.concatenate([rng.integers(0, 120, (60, 2)),                       # a loose cloud: most rows have fewer than k neighbours
                             np.full((5, 2), 60),                                 # five coincident rows inside it
                             rng.integers(0, 10, (4, 2)) + 5000,                  # four rows far away, all of unknown label: zero windows
                             np.array([[9000, 9000]])]).astype(np.int32)          # one row alone: the window is itself
    lab = rng.integers(0, 3, len(sparse)).astype(np.int32)
    lab[3], lab[17], lab[61] = -1, 3, 7                                           # unknown labels among rows that are neighbours of others
    lab[65:69] = -1
    dense = rng.integers(0, 80, (300, 2)).astype(np.int32)
    return dict(
        sparse=(sparse, lab, 3, 24, 4, 3, 5, 50),
        one_class_one_neighbour=(dense, rng.integers(-1, 2, 300).astype(np.int32), 1, 6, 1, 2, 1, 50),
        fourteen_classes_32_neighbours=(dense, rng.integers(-1, 15, 300).astype(np.int32), 14, 40, 32, 5, 2, 60),
    )


@functools.lru_cache(maxsize=None)
def point_reference(name):
    return nh.neighbourhoods_reference(*point_cases()[name])


# ---- list cases: seeding and Lloyd
def one_hot_rows(labels):
    """A neighbour list under which the window of row i is the one-hot of labels[i] (k = 1, every neighbour -1)."""
    return np.full((len(labels), 1), -1, np.int32), np.asarray(labels, np.int32)


def rows_with_windows(w):
    """A neighbour list and labels of two classes under which row i has the window w[i] (w[i] != (0, 0); both labels occur): a row is of
    class 0 when it counts one, and lists the first row of each class as often as its window says."""
    w = np.asarray(w, np.int64)
    lab = (w[:, 0] == 0).astype(np.int32)
    first = [int(np.flatnonzero(lab == c)[0]) for c in (0, 1)]
    nb = np.full((len(w), int(w.sum(1).max()) - 1), -1, np.int32)
    for i, (a, b) in enumerate(w.tolist()):
        listed = [first[0]] * (a - (lab[i] == 0)) + [first[1]] * (b - (lab[i] == 1))
        nb[i, :len(listed)] = listed
    assert np.array_equal(nh.windows_of(nb, lab, 2), w)
    return nb, lab


def zones(n, k, rng):
    """n rows in four composition zones of four classes: the neighbours of a row are k random rows of its zone."""
    comp = np.array([[.8, .1, .05, .05], [.1, .7, .1, .1], [.3, .3, .3, .1], [.05, .05, .2, .7]])
    zone = rng.integers(0, 4, n)
    lab = (rng.random(n)[:, None] > np.cumsum(comp, 1)[zone]).sum(1).astype(np.int32)
    members = [np.flatnonzero(zone == z) for z in range(4)]
    nb = np.zeros((n, k), np.int32)
    for z in range(4):
        nb[members[z]] = members[z][rng.integers(0, len(members[z]), (len(members[z]), k))]
    return nb, lab


def seed_where(make, wanted, tries=4000):
    """The smallest seed under which the case make(seed) has the property `wanted(reference)`; AssertionError when there is none."""
    for seed in range(tries):
        case = make(seed)
        if wanted(case):
            return seed
    raise AssertionError('no seed found')


def list_reference_of(case):
    nb, lab, C, K, seed, max_iter, centres = case
    w = nh.windows_of(nb, lab, C)
    return (w.astype(np.int32),) + nh.cluster_reference(w, K, seed, max_iter, centres)


def _pick_side(case, offset):
    """Does the second centre's draw fall on t == (inclusive prefix of the picked row) - 1 (offset 1: the last t that still picks it) or on
    t == the inclusive prefix of the row BEFORE the picked one with g > 0 (offset 0: the first t that no longer picks that one)?"""
    nb, lab, C, K, seed, _, _ = case
    w = nh.windows_of(nb, lab, C)
    u = nh.draws(seed, 2)
    g = ((w - w[u[0] % len(w)]) ** 2).sum(1)
    T = int(g.sum())
    if T == 0:
        return False
    prefix, t = np.cumsum(g), u[1] % T
    row = nh.pick(prefix, t)
    return t == prefix[row] - 1 and g[row] > 1 if offset else row > 0 and t == prefix[row - 1] and g[:row].any() and g[row] > 1


@functools.lru_cache(maxsize=None)
def list_cases():
    rng = np.random.default_rng(23)
    small = zones(40, 3, rng)
    three_blocks = np.zeros(3 * 256 + 17, np.int32)
    first, last = three_blocks.copy(), three_blocks.copy()
    first[[3, 100, 255]] = 1                                                     # every other row equals every other: g > 0 in block 0 only
    last[[768, 770, 784]] = 1                                                    # .. in the last, partly filled block only
    hood_small = lambda seed: small + (4, 3, seed, 50, None)
    cases = dict(
        pick_t_is_prefix_minus_1=hood_small(seed_where(hood_small, lambda c: _pick_side(c, 1))),
        pick_t_is_prefix=hood_small(seed_where(hood_small, lambda c: _pick_side(c, 0))),
        pick_in_first_block=one_hot_rows(first) + (2, 2, seed_where(lambda s: one_hot_rows(first) + (2, 2, s, 20, None), lambda c: 0 <= list_reference_of(c)[5][1] < 256
                                                                 and list_reference_of(c)[5][0] >= 256), 20, None),
        pick_in_last_block=one_hot_rows(last) + (2, 2, seed_where(lambda s: one_hot_rows(last) + (2, 2, s, 20, None), lambda c: list_reference_of(c)[5][1] >= 768
                                                               and list_reference_of(c)[5][0] < 768), 20, None),
        one_past_a_scan_chunk=one_hot_rows(rng.integers(0, 3, 256 * 1024 + 1)) + (3, 3, 4, 20, None),
        one_past_a_block=zones(257, 5, rng) + (4, 4, 1, 50, None),
        all_rows_equal=one_hot_rows(np.full(300, 2)) + (3, 3, 9, 20, None),      # T == 0 at every pick
        more_types_than_windows=one_hot_rows(rng.integers(0, 2, 500)) + (2, 4, 3, 20, None),
        fewer_rows_than_types=one_hot_rows([0, 1, 1]) + (2, 5, 7, 20, None),
        one_row=one_hot_rows([1]) + (3, 4, 0, 20, None),
        half_rounds_up=one_hot_rows(np.arange(2048) >= 1025) + (2, 1, 0, 20, None),     # one type of 2048 rows with sums 1025 and 1023
        most_types_most_classes=(rng.integers(-1, 3000, (3000, 8)).astype(np.int32), rng.integers(0, 14, 3000).astype(np.int32), 14, 32, 6, 100, None),
        tie_goes_to_the_smaller_type=one_hot_rows([0, 0, 1]) + (2, 3, 0, 20, np.array([[2048, 0], [0, 0], [1024, 2048]])),      # rows 0, 1: D = 1024^2 twice
        duplicate_given_centres=one_hot_rows(rng.integers(0, 2, 400)) + (2, 3, 0, 20, np.array([[1024, 0], [1024, 0], [0, 1024]])),
    )
    # found by a search over small windows: type 2 is seeded on a window of its own (so it holds that row at t = 1) and ends without a member
    cases['a_type_loses_all_members'] = rows_with_windows([[4, 2], [0, 3], [1, 0], [4, 3], [1, 1], [2, 2], [1, 4], [2, 3], [2, 3]]) + (2, 3, 1, 100, None)
    ref = list_reference_of(cases['a_type_loses_all_members'])
    assert ref[4].tolist() == [7, 2, 0] and len({tuple(ref[0][r]) for r in ref[5]}) == 3 and ref[7] == 3
    cases['zones_20000'] = zones(20000, 10, rng) + (4, 8, 0, 100, None)
    return cases


@functools.lru_cache(maxsize=None)
def list_reference(name, max_iter=None):
    case = list_cases()[name]
    return list_reference_of(case if max_iter is None else case[:5] + (max_iter,) + case[6:])
