"""Designed inputs for the nucleus territories (nuhtc_amd/territory.py), shared by tests/test_territory_host.py (the restatement against
hand-written rasters, a double loop and closed forms) and tests/test_hip_territory.py (the device against the restatement).  A case is
(points int32 (n, 2) half pixels, labels int32 (n,), num_classes, R half pixels, s half pixels), the shape of the cases of
tests/density_cases.py with the reach in place of the bandwidth -- its generators serve here as they are; the window of a case is
`territory.window` of its bounding box unless a test says otherwise."""
import numpy as np

import density_cases as DC
from density_cases import (_case, coincident, crowded, default_window, labels_out_of_range, lattice, mirror, patch, pitch_cases,  # noqa: F401
                           random_large, single_point, single_point_expected, staged, three_four_five, translate)
from nuhtc_amd import territory as tr

LARGE_RS = DC.LARGE_HS                                     # (R, s): sites far denser than the reach (staged), about as dense, and sparser
NAMES = tr.MAP_NAMES + tr.INT_NAMES


def equal(got, want, what):
    """Every one of the eight outputs: same dtype, same shape, same entries."""
    assert len(got) == len(want) == len(NAMES), (what, len(got), len(want))
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, f'{len(bad)} entries differ, first at {bad[0].tolist()}', int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


def bisector(swapped=False):
    """Two points 8 apart on a row of sites at pitch 4, R = 10: the sites of the column x = 4 are as far from one as from the other (d2 16 +
    y * y) and go to the smaller ROW -- the left point as given, the right one once the rows are swapped."""
    p = [[8, 0], [0, 0]] if swapped else [[0, 0], [8, 0]]
    return _case(p, [0, 1], 2, 10, 4)


def on_sites(k=3, s=2, m=5, classes=2, origin=(-3, 7)):
    """m x m points on a lattice of spacing k * s (k odd), every one ON a site (the origin is given in lattice units), R = k * s; the
    labels are a checkerboard (classes = 2) or all 0.  Inside the points' own box every site is owned, the territory of an interior point
    is the k x k sites around it (k odd: no site lies on a bisector) and is closed."""
    assert k % 2 == 1
    y, x = np.divmod(np.arange(m * m), m)
    p = np.stack([(origin[0] + k * x) * s, (origin[1] + k * y) * s], 1)
    return _case(p, (x + y) % 2 if classes == 2 else None, classes, k * s, s)


def on_sites_window(k=3, m=5, origin=(-3, 7)):
    """The window that is exactly the box of `on_sites`: (m - 1) k + 1 sites each way."""
    return origin[0], origin[1], (m - 1) * k + 1, (m - 1) * k + 1


def ties(seed, n=400, grid=6, extent=40, C=3):
    """n points on a coarse grid of `grid` half pixels (many coincident, many equidistant from a site), labels -1 .. C (some do not compete),
    R = 15 and sites at pitch 3, which divides the grid: bisectors run through sites everywhere."""
    rng = np.random.default_rng(seed)
    return _case(grid * rng.integers(0, extent, (n, 2)) - 77, rng.integers(-1, C + 1, n), C, 15, 3)


def two_cells(n=1500):
    """n points on nine places in one or two cells (density's crowded set) with R = 8 and sites at pitch 1: more records in a cell row than one
    staging chunk of 256, and every place many times over -- the smallest row of a place owns its sites."""
    return crowded(8, n)
