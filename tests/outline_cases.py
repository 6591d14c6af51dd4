"""Designed point sets for the alpha-shape outline (nuhtc_amd/outline.py), shared by tests/test_outline_host.py and
tests/test_hip_outline.py.  A case is (points int32 (n, 2) half pixels, labels int32 (n,), C, r in HALF pixels, by_class), as in
tests/alpha_cases.py; `complex_of` is its alpha complex from the brute-force restatement, `reference` the outline walk on that."""
import numpy as np

from nuhtc_amd import alphacomplex as ax
from nuhtc_amd import outline as ol

NAMES = ol.INT_NAMES + ('h', 'R', 'K')


def _case(p, lab, C, r, by_class=0):
    p = np.asarray(p, np.int32).reshape(-1, 2)
    lab = np.zeros(len(p), np.int32) if lab is None else np.asarray(lab, np.int32).reshape(-1)
    assert len(lab) == len(p)
    return p, lab, C, r, by_class


def complex_of(case):
    """-> (edges, edge_d2, apex) of alpha_reference."""
    return ax.alpha_reference(*case)[:3]


def reference(case, alpha=None):
    p, lab, C, r, by = case
    e, d2, ap = complex_of(case) if alpha is None else alpha[:3]
    return ol.outline_reference(p, lab, e, d2, ap, by)


def equal(got, want, what):
    """Every one of the nine results: same dtype, same shape, same values."""
    for name, g, w, t in zip(NAMES, got, want, ol.INT_TYPES + (None,) * 3):
        if t is None:
            assert int(g) == int(w), (what, name, g, w)
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype == np.dtype(t) and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f'{what}: {name} differs at {len(bad)} places, first {bad[:5].tolist()}: got {g[bad[:5]].tolist()}, want {w[bad[:5]].tolist()}')


def expected(rings, area2, comp_of_ring, component, labels):
    """Hand-written rings -> the nine results."""
    start = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
    vertex = np.asarray([v for r in rings for v in r], np.int32).reshape(-1)
    return (vertex, start, np.asarray(area2, np.int64).reshape(-1), np.asarray(comp_of_ring, np.int32).reshape(-1), np.asarray(component, np.int32).reshape(-1),
            np.asarray(labels, np.int32).reshape(-1), len(vertex), len(rings), len(labels))


# ---- one triangle beside the radius: (0, 0), (8, 0) and (4, 8) lie on the circle of radius 5 about (4, 3)
def triangle(top=8, r=5):
    """top = 8: the circumradius is exactly r = 5, the triangle is there.  top = 9, one half-pixel step over: the circumradius is 5.39, the
    three edges stay (each has an empty disc of radius <= 5 of its own) and none has an apex."""
    return _case([[0, 0], [8, 0], [4, top]], None, 1, r)


# edge 0 = (0, 1) has row 2 on its left: the half-edge 0 -> 1 leads; twice the area is 8 * 8
TRIANGLE = expected([[0, 1, 2]], [64], [0], [0, 0, 0], [-1])
NOTHING_3 = expected([], [], [], [-1, -1, -1], [])


def two_triangles():
    """(0, 0), (8, 0), (4, 8), (4, -8): two triangles over the interior edge (0, 1)."""
    return _case([[0, 0], [8, 0], [4, 8], [4, -8]], None, 1, 5)


# edges (0,1) (0,2) (0,3) (1,2) (1,3) = ids 0..4; the smallest outline id is 1 = (0, 2), with row 1 on its right: the half-edge 2 -> 0
TWO_TRIANGLES = expected([[2, 0, 3, 1]], [128], [0], [0, 0, 0, 0], [-1])


def bow_tie():
    """Two triangles that share row 0 and nothing else: two rings, two components, two out-half-edges at row 0."""
    return _case([[0, 0], [8, -3], [8, 3], [-8, -3], [-8, 3]], None, 1, 5)


# edges (0,1) (0,2) (0,3) (0,4) (1,2) (3,4) = ids 0..5.  id 0 = (0, 1): row 2 on the left, 0 -> 1, ring 0 1 2.  id 2 = (0, 3): row 4 on the
# right, 3 -> 0, ring 3 0 4.  The component of an edge is the rank of its smallest edge: ring 0 in 0, ring 1 in 1; row 0 takes the smaller
BOW_TIE = expected([[0, 1, 2], [3, 0, 4]], [48, 48], [0, 1], [0, 0, 0, 1, 1], [-1, -1])


def lattice(w, h, s=10, r=8, without=(), origin=(0, 0), lab=None, C=1, by_class=0):
    """w x h points at spacing s (row-major) without the sites `without` = ((ix, iy), ..).  With r = 8 and s = 10 every cell is a square of
    circumradius 7.07 with both diagonals kept (four cocircular points); a cell with one corner missing keeps the triangle of the other
    three; the diamond around a missing site has the circumradius 10 and stays empty."""
    sites = [(ix, iy) for iy in range(h) for ix in range(w) if (ix, iy) not in set(without)]
    p = np.asarray(sites, np.int64).reshape(-1, 2) * s + np.asarray(origin)
    return _case(p, lab, C, r, by_class)


def annulus():
    """5 x 5 sites without the middle one: an outer ring of 16 places and the diamond hole around the missing site."""
    return lattice(5, 5, without=((2, 2),))


def pinched():
    """5 x 4 sites without (2, 1): the diamond around it touches the bottom row at (2, 0), so the ONE ring runs through that row twice --
    along the bottom, up round the diamond, and on along the bottom."""
    return lattice(5, 4, without=((2, 1),))


def island():
    """A frame two sites wide around an empty middle of 60 x 60 (less the triangles its corner cells keep), and one small triangle in the
    middle, out of the frame's reach: three rings, two components, the second inside the first's hole."""
    frame = lattice(9, 9, without=tuple((ix, iy) for ix in range(2, 7) for iy in range(2, 7)))[0]
    return _case(np.concatenate([frame, [[36, 36], [44, 36], [40, 43]]]), None, 1, 8)


def square():
    return _case([[0, 0], [10, 0], [0, 10], [10, 10]], None, 1, 8)


def circle_of_twelve(scale=2):
    """The twelve lattice points on the circle of radius 5, scaled: all cocircular, every pair an edge, one ring of twelve and no hole."""
    pts = [(5, 0), (4, 3), (3, 4), (0, 5), (-3, 4), (-4, 3), (-5, 0), (-4, -3), (-3, -4), (0, -5), (3, -4), (4, -3)]
    order = [7, 2, 9, 0, 5, 11, 4, 1, 10, 3, 8, 6]                                # rows in no order of angle
    return _case(np.asarray([pts[k] for k in order]) * scale, None, 1, 5 * scale)


def coincident_corner():
    """A triangle whose corner (0, 0) holds three rows, the smallest of them not the first row of the set."""
    return _case([[4, 8], [0, 0], [8, 0], [0, 0], [0, 0]], None, 1, 5)


# the representatives are rows 0, 1, 2: edges (0,1) (0,2) (0,3) (0,4) (1,2) (1,3) (1,4) (2,3) (2,4) (3,4) = ids 0..9; (0, 1) = (4,8)-(0,0)
# has row 2 on its left: 0 -> 1, ring 0 1 2.  Rows 3 and 4 take row 1's component
COINCIDENT_CORNER = expected([[0, 1, 2]], [64], [0], [0, 0, 0, 0, 0], [-1])


def path():
    """Seven points in a line and a bend: singular edges only."""
    return _case([[0, 0], [8, 0], [16, 0], [24, 0], [24, 9], [24, 18], [33, 18]], None, 1, 5)


def two_classes(by_class):
    """Two 4 x 4 lattices laid over each other, half a cell apart, labels 0 and 1: by class each is its own square; with `any` they are one
    finer complex."""
    a, b = lattice(4, 4)[0], lattice(4, 4, origin=(5, 5))[0]
    return _case(np.concatenate([a, b]), [0] * 16 + [1] * 16, 2, 8, by_class)


def strip(n=20000, order='ascending', s=10, top=8, r=8):
    """A zigzag strip of n points: the bottom row at (s k, 0) and the top row at (s k + s / 2, top), triangles of circumradius 5.56 between
    them.  ONE ring of n half-edges (all of the bottom and the top edges and the two ends).  The rows in place order (bottom and top
    alternating), backwards, or shuffled."""
    k = np.arange(n)
    p = np.stack([(k // 2) * s + (k % 2) * (s // 2), (k % 2) * top], 1)
    if order == 'descending':
        p = p[::-1]
    elif order == 'shuffled':
        p = p[np.random.default_rng(7).permutation(n)]
    return _case(p, None, 1, r)


def many_triangles(count=5000):
    """`count` triangles 40 apart on a grid 100 wide: as many rings and components."""
    k = np.arange(count)
    o = np.stack([(k % 100) * 40, (k // 100) * 40], 1)
    p = (o[:, None, :] + np.asarray([[0, 0], [8, 0], [4, 8]])[None]).reshape(-1, 2)
    return _case(p, k.repeat(3) % 3, 3, 5)


def coarse(by_class=0, n=300, side=41, r=4, seed=12):
    """n points on a coarse lattice with the coordinates 0 .. side - 1: full of collinear, cocircular and coincident points."""
    rng = np.random.default_rng(seed)
    return _case(rng.integers(0, side, (n, 2)), rng.integers(-1, 4, n), 3, r, by_class)


def scattered(n=400, extent=300, r=14, seed=5, by_class=0):
    """Random points without two on one place; with these sizes no four cocircular in an empty circle (n_degenerate == 0 is asserted
    where it matters)."""
    rng = np.random.default_rng(seed)
    p = np.unique(rng.integers(0, extent, (n, 2)), axis=0)
    p = p[rng.permutation(len(p))]
    return _case(p, rng.integers(0, 3, len(p)), 3, r, by_class)


def permuted(case, seed=4):
    order = np.random.default_rng(seed).permutation(len(case[0]))                  # new row k is old row order[k]
    return (case[0][order], case[1][order]) + case[2:]


def small_cases():
    return dict(triangle_at_r=triangle(8), triangle_over_r=triangle(9), two_triangles=two_triangles(), bow_tie=bow_tie(), annulus=annulus(), pinched=pinched(),
                island=island(), square=square(), circle_of_twelve=circle_of_twelve(), lattice_6=lattice(6, 6), coincident_corner=coincident_corner(),
                path=path(), none=_case(np.zeros((0, 2)), None, 1, 5), one=_case([[3, 4]], None, 1, 5), two=_case([[0, 0], [6, 0]], None, 1, 5),
                two_classes_any=two_classes(0), two_classes_class=two_classes(1), strip_41=strip(41), coarse_any=coarse(0), coarse_class=coarse(1),
                coarse_any_r5=coarse(0, r=5, seed=17), scattered=scattered(), scattered_class=scattered(by_class=1, seed=6))


# what the small cases are for: (rings, holes, components) each
SHAPES = dict(triangle_at_r=(1, 0, 1), triangle_over_r=(0, 0, 0), two_triangles=(1, 0, 1), bow_tie=(2, 0, 2), annulus=(2, 1, 1), pinched=(1, 0, 1),
              island=(3, 1, 2), square=(1, 0, 1), circle_of_twelve=(1, 0, 1), lattice_6=(1, 0, 1), coincident_corner=(1, 0, 1), path=(0, 0, 0),
              none=(0, 0, 0), one=(0, 0, 0), two=(0, 0, 0), two_classes_any=(1, 0, 1), two_classes_class=(2, 0, 2), strip_41=(1, 0, 1))
HAND_WRITTEN = dict(triangle_at_r=TRIANGLE, triangle_over_r=NOTHING_3, two_triangles=TWO_TRIANGLES, bow_tie=BOW_TIE, coincident_corner=COINCIDENT_CORNER)
