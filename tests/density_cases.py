"""Designed inputs for the density rasters (nuhtc_amd/density.py), shared by tests/test_density_host.py (the restatement against
hand-written rasters and closed forms) and tests/test_hip_density.py (the device against the restatement).  A case is
(points int32 (n, 2) half pixels, labels int32 (n,), num_classes, h half pixels, s half pixels); its window is `density.window` of its
bounding box unless a test says otherwise."""
import numpy as np

from nuhtc_amd import cellpoints
from nuhtc_amd import density as dn


def _case(p, lab, C, h, s):
    p = np.asarray(p, np.int32).reshape(-1, 2)
    lab = np.zeros(len(p), np.int32) if lab is None else np.asarray(lab, np.int32).reshape(-1)
    assert len(lab) == len(p)
    return p, lab, C, h, s


def default_window(case):
    """The default window of a case, one site at least each way."""
    w = dn.window(cellpoints.bounds_of(case[0]), case[3], case[4])
    return w[0], w[1], max(w[2], 1), max(w[3], 1)


def translate(case, dx, dy):
    return (case[0] + np.array([dx, dy], np.int32),) + case[1:]


def mirror(case):
    return (-case[0],) + case[1:]


# ---- hand-written
def single_point(h=9, s=4, at=(5, -3)):
    """One point ON site `at`: the site has count 1 and weight h * h, the site at lattice offset (a, b) h * h - s * s * (a * a + b * b)
    while that is not negative."""
    return _case([[at[0] * s, at[1] * s]], [0], 1, h, s)


def single_point_expected(h=9, s=4, at=(5, -3)):
    """-> (window, count (1, H, W), weight (1, H, W)) written out by hand: the offsets (a, b) with s * s * (a * a + b * b) <= h * h."""
    k = h // s                                              # the farthest column and row in reach
    win = (at[0] - k, at[1] - k, 2 * k + 1, 2 * k + 1)
    count, weight = np.zeros((1, 2 * k + 1, 2 * k + 1), np.int32), np.zeros((1, 2 * k + 1, 2 * k + 1), np.int64)
    for b in range(-k, k + 1):
        for a in range(-k, k + 1):
            t = h * h - s * s * (a * a + b * b)
            if t >= 0:
                count[0, b + k, a + k], weight[0, b + k, a + k] = 1, t
    return win, count, weight


def three_four_five():
    """h = 5, s = 1, one point at the origin: the site at offset (3, 4) is exactly h away (count 1, weight 0), the site (3, 5) sees nothing."""
    return _case([[0, 0]], [0], 1, 5, 1)


RING_25 = [(25, 0), (-25, 0), (0, 25), (0, -25), (7, 24), (-7, 24), (24, -7), (-24, -7), (15, 20), (-15, -20), (20, -15), (-20, 15)]


def pythagorean_ring():
    """Twelve points at exactly h = 25 from the origin (0-25, 7-24, 15-20) and s = 25: the origin's site counts twelve with weight 0."""
    return _case(RING_25, np.arange(12) % 2, 2, 25, 25)


# ---- the designed sets of the device tests
def patch(s=4, seed=5):
    """40 points in a 60 x 60 half-pixel patch, h = 9, s = 4: the default window reaches past the box on all four sides.  With s = 1 the
    sites of a tile lie close enough for the staged kernel (15 s <= 2 h + side), with s = 4 every site walks its own cells."""
    rng = np.random.default_rng(seed)
    return _case(rng.integers(0, 60, (40, 2)), rng.integers(0, 3, 40), 3, 9, s)


def lattice(s, w=40, h=30, pitch=6, origin=(-777, 31)):
    """w x h points at pitch 6 (1200 of them) with a bandwidth of 9: cells of 9 against a pitch of 6; sites at pitch s."""
    y, x = np.divmod(np.arange(w * h), w)
    return _case(np.stack([origin[0] + pitch * x, origin[1] + pitch * y], 1), (x + 2 * y) % 3, 3, 9, s)


def coincident(s=16384, n=1500):
    """n coincident points on a site, h = 16384, one class: the site's weight is n * 2**28, above 2**32.  s divides 16384."""
    return _case([[3 * 16384, -2 * 16384]] * n, None, 1, 16384, s)


def crowded(h=8, n=1500, step=2):
    """n points on nine places in one or two cells (the proximity test's crowded set), sites at pitch 1: more records than one staging
    chunk of 256 with h = 8 (the staged kernel), a long walk for every site with h = 3 (the direct one)."""
    rng = np.random.default_rng(15)
    place = rng.integers(0, 9, n)
    return _case(np.stack([step * (place % 3) + 100, step * (place // 3) - 50], 1), rng.integers(0, 3, n), 3, h, 1)


def labels_out_of_range():
    """C = 3 with the labels -1, 0, 1, 2, 3 and 14 present."""
    rng = np.random.default_rng(8)
    return _case(rng.integers(-20, 40, (90, 2)), np.array([-1, 0, 1, 2, 3, 14])[np.arange(90) % 6], 3, 7, 3)


def pitch_cases():
    rng = np.random.default_rng(21)
    p, lab = rng.integers(-150, 150, (200, 2)), rng.integers(0, 2, 200)
    return dict(dense=_case(p[:60] // 4, lab[:60], 2, 3, 1), sparse=_case(p, lab, 2, 7, 50), unit=_case(p // 8, lab, 2, 1, 1))


def random_large(kind, n=3000):
    """3000 points, 5 classes (and a few labels outside them): uniform on a square of 400, or in 12 Gaussian clumps on the same square."""
    rng = np.random.default_rng(2026)
    if kind == 'uniform':
        p = rng.integers(0, 400, (n, 2))
    else:
        centre = rng.uniform(0, 400, (12, 2))
        p = np.clip(np.rint(centre[rng.integers(0, 12, n)] + rng.normal(0, 25, (n, 2))), 0, 399)
    return p.astype(np.int32), rng.integers(-1, 6, n).astype(np.int32)


LARGE_HS = [(20, 4), (30, 16), (5, 11)]                     # (h, s): sites far denser than the reach (staged), about as dense, and sparser


def staged(case, side=None):
    """Does the device stage this case through LDS?  The rule of csrc/cellgrid_host.h (site_route_staged) restated: 15 s <= 2 h + side, the
    cell side being h for every box of these tests (fewer than 2**22 cells of side h)."""
    return 15 * case[4] <= 2 * case[3] + (case[3] if side is None else side)
