"""Host-only checks of the density rasters (nuhtc_amd/density.py): `density_reference` against hand-written rasters and an independent
double loop in plain Python integers, `window` against the non-zero sites of the restatement (negative coordinates, one ring of zeros
around it), `derive` against its closed forms, `check_args` and the .npz round trip.  The device is compared with `density_reference` in
tests/test_hip_density.py."""
import numpy as np
import pytest

import density_cases as DC
from nuhtc_amd import cellpoints
from nuhtc_amd import density as dn


def double_loop(p, lab, C, h, s, win):
    """The definition word for word: Python integers, every site, every row."""
    gx0, gy0, W, H = win
    count, weight = np.zeros((C, H, W), np.int32), np.zeros((C, H, W), np.int64)
    for v in range(H):
        for u in range(W):
            qx, qy = (gx0 + u) * s, (gy0 + v) * s
            for (x, y), c in zip(p.tolist(), lab.tolist()):
                d2 = (qx - x) ** 2 + (qy - y) ** 2
                if 0 <= c < C and d2 <= h * h:
                    count[c, v, u] += 1
                    weight[c, v, u] += h * h - d2
    return count, weight


def _same(got, want, what):
    for name, g, w in zip(dn.INT_NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name)


def test_a_single_point_on_a_site():
    for h, s, at in ((9, 4, (5, -3)), (10, 5, (-2, 0)), (3, 1, (0, 0))):
        case = DC.single_point(h, s, at)
        win, count, weight = DC.single_point_expected(h, s, at)
        assert win == dn.window(cellpoints.bounds_of(case[0]), h, s)
        got = dn.density_reference(*case, win)
        _same(got, (count, weight), f'single point, h {h}, s {s}')
        k = h // s
        assert got[0][0, k, k] == 1 and got[1][0, k, k] == h * h and got[1][0, k, k + 1] == h * h - s * s


def test_three_four_five_and_the_ring_at_exactly_h():
    case = DC.three_four_five()
    count, weight = dn.density_reference(*case, (-5, -5, 11, 11))
    assert count[0, 4 + 5, 3 + 5] == 1 and weight[0, 4 + 5, 3 + 5] == 0                 # offset (3, 4): exactly h away
    assert count[0, 5 + 5, 3 + 5] == 0 and weight[0, 5 + 5, 3 + 5] == 0                 # offset (3, 5): 34 > 25
    assert count[0, 5, 5] == 1 and weight[0, 5, 5] == 25 and count[0, 5, 10] == 1 and weight[0, 5, 10] == 0
    count, weight = dn.density_reference(*DC.pythagorean_ring(), (0, 0, 1, 1))
    assert count[:, 0, 0].tolist() == [6, 6] and weight[:, 0, 0].tolist() == [0, 0]
    count, weight = dn.density_reference(*DC.pythagorean_ring()[:3], 24, 25, (0, 0, 1, 1))
    assert not count.any() and not weight.any()


@pytest.mark.parametrize('name', ['patch', 'mirrored', 'labels', 'sparse', 'unit', 'ring'])
def test_reference_equals_the_double_loop(name):
    case = dict(patch=DC.patch(), mirrored=DC.mirror(DC.patch()), labels=DC.labels_out_of_range(), sparse=DC.pitch_cases()['sparse'],
                unit=DC.pitch_cases()['unit'], ring=DC.pythagorean_ring())[name]
    win = DC.default_window(case)
    _same(dn.density_reference(*case, win, block=97), double_loop(*case, win), name)


def test_out_of_range_labels_land_nowhere():
    p, lab, C, h, s = DC.labels_out_of_range()
    win = DC.default_window((p, lab, C, h, s))
    count, weight = dn.density_reference(p, lab, C, h, s, win)
    keep = (lab >= 0) & (lab < C)
    one = dn.density_reference(p[keep], np.zeros(keep.sum(), np.int32), 1, h, s, win)
    assert np.array_equal(count.sum(0), one[0][0]) and np.array_equal(weight.sum(0), one[1][0]) and count.sum() < len(p) * 20


@pytest.mark.parametrize('seed', range(6))
def test_window_covers_exactly_the_non_zero_sites(seed):
    rng = np.random.default_rng(seed)
    n, h, s = int(rng.integers(1, 40)), int(rng.integers(1, 30)), int(rng.integers(1, 12))
    p = rng.integers(-300, 120, (n, 2)) + rng.integers(-500, 500, 2)
    gx0, gy0, W, H = dn.window(cellpoints.bounds_of(p), h, s)
    if W < 1 or H < 1:                                     # the pitch steps over every site in reach: nothing anywhere near
        count, _ = dn.density_reference(p, np.zeros(n), 1, h, s, (gx0 - 2, gy0 - 2, 5, 5))
        assert not count.any()
        return
    count, weight = dn.density_reference(p, np.zeros(n), 1, h, s, (gx0 - 1, gy0 - 1, W + 2, H + 2))
    ring = np.ones((H + 2, W + 2), bool)
    ring[1:-1, 1:-1] = False
    assert not count[0][ring].any() and not weight[0][ring].any()
    # the closed form is tight along each axis: the first and last column and row each hold a site within h of the box along that axis
    x_min, y_min, x_max, y_max = cellpoints.bounds_of(p)
    assert gx0 * s >= x_min - h > (gx0 - 1) * s and (gx0 + W - 1) * s <= x_max + h < (gx0 + W) * s
    assert gy0 * s >= y_min - h > (gy0 - 1) * s and (gy0 + H - 1) * s <= y_max + h < (gy0 + H) * s


def test_window_of_negative_coordinates_by_hand():
    assert dn.window((-10, -10, -10, -10), 3, 4) == (-3, -3, 2, 2)          # sites -12 and -8 lie within 3 of -10
    assert dn.window((0, 0, 0, 0), 3, 4) == (0, 0, 1, 1)
    assert dn.window((-13, 5, -7, 5), 1, 4) == (-3, 1, 2, 1) and dn.window((2, 2, 2, 2), 1, 4)[2:] == (0, 0)


def test_derive_closed_forms():
    h = 4
    count = np.array([[[1, 0, 2]], [[1, 0, 0]], [[0, 0, 0]]], np.int32)
    weight = np.array([[[16, 0, 8]], [[16, 0, 0]], [[0, 0, 0]]], np.int64)
    d = dn.derive(count, weight, h)
    assert tuple(d) == dn.DERIVED_KEYS
    assert np.array_equal(d['density_per_px2'], weight * 8 / (np.pi * 256.0)) and d['density_per_px2'].dtype == np.float64
    assert d['share'].tolist() == [[[0.5, 0.0, 1.0]], [[0.5, 0.0, 0.0]], [[0.0, 0.0, 0.0]]]
    assert d['class_total'].tolist() == [3, 1, 0] and d['class_total'].dtype == np.int64
    pa, pb = np.array([2 / 3, 0, 1 / 3]), np.array([1.0, 0, 0])
    mh = 2 * (pa * pb).sum() / ((pa * pa).sum() + (pb * pb).sum())
    assert np.allclose(d['colocalisation'], [[1, mh, 0], [mh, 1, 0], [0, 0, 0]], rtol=1e-15, atol=0)
    assert d['peak_site'].tolist() == [[0, 0], [0, 0], [-1, -1]] and d['peak_site'].dtype == np.int64
    # one nucleus per px^2 everywhere: a unit lattice of points at pitch 2 half pixels integrates to 1 per px^2 under the normalised kernel
    y, x = np.divmod(np.arange(41 * 41), 41)
    count, weight = dn.density_reference(np.stack([2 * x - 40, 2 * y - 40], 1), np.zeros(41 * 41), 1, 12, 1, (0, 0, 1, 1))
    assert abs(dn.derive(count, weight, 12)['density_per_px2'][0, 0, 0] - 1.0) < 0.02


def test_derive_on_random_rasters_and_on_empty_planes():
    p, lab = DC.random_large('clumps', 400)
    win = dn.window(cellpoints.bounds_of(p), 30, 16)
    count, weight = dn.density_reference(p, lab, 5, 30, 16, win)
    d = dn.derive(count, weight, 30)
    assert all(np.isfinite(v).all() for v in d.values())
    total = count.sum(0)
    assert np.allclose(d['share'].sum(0)[total > 0], 1.0, rtol=1e-14, atol=0) and not d['share'][:, total == 0].any()
    assert np.array_equal(d['colocalisation'], d['colocalisation'].T) and np.allclose(np.diag(d['colocalisation']), 1.0, rtol=1e-14, atol=0)
    assert (d['colocalisation'] >= 0).all() and (d['colocalisation'] <= 1 + 1e-14).all()
    for c in range(5):
        u, v = d['peak_site'][c]
        assert weight[c, v, u] == weight[c].max() and (weight[c].reshape(-1)[:v * win[2] + u] < weight[c].max()).all()
    empty = dn.derive(np.zeros((3, 4, 5), np.int32), np.zeros((3, 4, 5), np.int64), 7)
    assert all(np.isfinite(v).all() for v in empty.values()) and not empty['colocalisation'].any() and (empty['peak_site'] == -1).all()
    assert not empty['share'].any() and not empty['class_total'].any()


def test_no_points_and_refused_arguments():
    count, weight = dn.density_reference(np.zeros((0, 2)), [], 2, 5, 3, (4, -4, 3, 2))
    assert count.shape == (2, 2, 3) and count.dtype == np.int32 and weight.dtype == np.int64 and not count.any() and not weight.any()
    for C, h, s in ((0, 5, 3), (15, 5, 3), (3, 0, 3), (3, 16385, 3), (3, 5, 0), (3, 5, (1 << 20) + 1), (3, 5.5, 3)):
        with pytest.raises(ValueError):
            dn.check_args(C, h, s)
    dn.check_args(14, 16384, 1 << 20)
    for win in ((0, 0, 0, 1), (0, 0, 1, 0), (0, 0, (1 << 24) + 1, 1), (0, 0, 1 << 12, (1 << 12) + 1), (1 << 26, 0, 1, 1), (0, -(1 << 26), 1, 1),
                ((1 << 26) - 4, 0, 5, 1), (0, 0, 1)):
        with pytest.raises(ValueError):
            dn.check_args(3, 5, 4, win)
    dn.check_args(3, 5, 4, ((1 << 26) - 4, -(1 << 26) + 1, 4, 1 << 12))
    with pytest.raises(ValueError):
        dn.density_reference([[1 << 27, 0]], [0], 1, 5, 3, (0, 0, 1, 1))
    with pytest.raises(ValueError):
        dn.density_reference([[0, 0], [1, 1]], [0], 1, 5, 3, (0, 0, 1, 1))


def test_npz_round_trip(tmp_path):
    p, lab = DC.random_large('uniform', 200)
    h, s = 30, 16
    win = dn.window(cellpoints.bounds_of(p), h, s)
    count, weight = dn.density_reference(p, lab, 5, h, s, win)
    path = dn.write_npz(str(tmp_path / 'a_nuclei_density.npz'), np.arange(200) * 3, p / 2.0, lab, count, weight, win, h / 2, s / 2)
    z = dn.read_npz(path)
    assert tuple(z) == dn.NPZ_KEYS
    assert np.array_equal(z['count'], count) and z['count'].dtype == np.int32 and np.array_equal(z['weight'], weight) and z['weight'].dtype == np.int64
    assert float(z['bandwidth_px']) == 15.0 and float(z['pitch_px']) == 8.0 and z['window'].tolist() == list(win) and z['window'].dtype == np.int64
    assert z['origin_px'].tolist() == [win[0] * 8.0, win[1] * 8.0] and np.array_equal(z['nuclei_id'], np.arange(200) * 3)
    d = dn.derive(count, weight, h)
    for key in dn.DERIVED_KEYS:
        assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype, key
    with pytest.raises(ValueError):
        dn.write_npz(str(tmp_path / 'b.npz'), np.arange(200), p / 2.0, lab, count, weight, (win[0], win[1], win[2] + 1, win[3]), h / 2, s / 2)
    with pytest.raises(ValueError):
        dn.write_npz(str(tmp_path / 'b.npz'), np.arange(200), p / 2.0, lab, count, weight[:, :-1], win, h / 2, s / 2)
