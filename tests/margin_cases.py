"""Designed inputs for the margin bands (nuhtc_amd/margin.py), shared by tests/test_margin_host.py (the restatement against a double loop
in Python integers and hand-written rows) and tests/test_hip_margin.py (the device against the restatement).  A case is (points int32
(n, 2) half pixels, labels int32 (n,), num_classes, edges int32 (E, 4), edge_region int32 (E,), G, thresholds int32 (B,)).  Regions are
written as lists of rings of half-pixel vertices and turned into the edge table by `regions_cases.table`."""
import numpy as np

import regions_cases as RC
from regions_cases import lattice, rect

TRIPLES = ((3, 4, 5), (119, 120, 169))
# the pair that the float64 restatement (project onto the segment, compare hypot with e) decides wrongly: direction 119:120:169, the
# distance is exactly 3549
F64_EDGE, F64_POINT, F64_E = ((-4576275, 3091603), (23000071, 30899683)), (2840736, 10575982), 3549


def _case(p, lab, C, regions, thresholds):
    return RC._case(p, lab, C, regions) + (np.ascontiguousarray(thresholds, np.int32),)


def permuted(case, seed=4):
    order = np.random.default_rng(seed).permutation(len(case[0]))
    return (case[0][order], case[1][order]) + case[2:], order


# ---- points exactly on every threshold of a B = 32 row, and one half-pixel step beyond it
def pythagorean(triple, length=40):
    """One edge from the origin along (a, b) of a Pythagorean triple (a, b, c), as a ring of two vertices (region 0 holds nothing), and the
    thresholds c, 2 c, .., 32 c.  For k = 1..32 and for feet at the start, inside and at the end of the edge: the point k unit normals
    from the foot (distance exactly k c: band k - 1) and the same point one step farther out in x (band k, or 32 = none).  Both sides of
    the edge.  -> (case, expected band int32 (n,))."""
    a, b, c = triple
    pts, want = [], []
    for k in range(1, 33):
        for along in (0, 7, length):
            for sign in (1, -1):
                x, y = along * a - sign * k * b, along * b + sign * k * a
                pts += [(x, y), (x - sign, y)]
                want += [k - 1, k]
    return _case(pts, None, 1, [[[(0, 0), (length * a, length * b)]]], c * np.arange(1, 33)), np.asarray(want, np.int32)


def float64_pair():
    """The failing pair of the issue between thresholds one below and one above: rows 0 (exactly 3549 away: band 1), 1 (one half-pixel step
    in x farther out: band 2) and 2 (one step nearer: band 1 still -- 3548 is a whole half pixel closer)."""
    (a, b), p = F64_EDGE, F64_POINT
    return _case([p, (p[0] - 1, p[1]), (p[0] + 1, p[1])], None, 1, [[[a, b]]], (F64_E - 1, F64_E, F64_E + 1))


# ---- the three regimes of near, by hand
REGIME_ROWS = [  # (point, band of region 0 = the edge (0, 0) -> (10, 0), thresholds 1 2 3 5)
    ((0, 5), 3), ((0, 6), 4), ((10, 5), 3), ((10, 6), 4),                  # s == 0 and s == L2 exactly: the end regimes, inclusive
    ((-3, 4), 3), ((-3, 5), 4), ((13, -4), 3), ((14, 4), 4),               # past either end: the distance to the vertex
    ((5, 0), 0), ((0, 0), 0), ((10, 0), 0),                                # on the edge and on its vertices
    ((5, 1), 0), ((5, -2), 1), ((4, 3), 2), ((6, -4), 3), ((5, 5), 3), ((5, 6), 4),
]


def regimes():
    """Region 0: the edge (0, 0) -> (10, 0) as a ring of two vertices.  Region 1: a zero-length edge at (40, 40).  Region 2: the square
    (100, 0) .. (110, 10), with points on its sides and corners: band 0, and the side the half-open rule gives."""
    pts = [p for p, _ in REGIME_ROWS] + [(40, 40), (43, 44), (43, 45), (105, 0), (105, 10), (100, 5), (110, 5), (100, 0), (110, 10), (105, 5), (105, 13), (113, 14), (114, 14)]
    return _case(pts, [0, 1] * (len(pts) // 2) + [0] * (len(pts) % 2), 2, [[[(0, 0), (10, 0)]], [[(40, 40)]], [rect(100, 0, 110, 10)]], (1, 2, 3, 5))


REGIME_SQUARE = {(105, 0): (0, 1), (105, 10): (0, 0), (100, 5): (0, 1), (110, 5): (0, 0), (100, 0): (0, 1), (110, 10): (0, 0), (105, 5): (3, 1), (105, 13): (2, 0),
                 (113, 14): (3, 0), (114, 14): (4, 0)}                      # point -> (band, inside) of region 2


# ---- holes, nesting, multipolygons, shared edges
def holes_and_nested():
    """Region 0: a ring, a hole in it and an island in the hole.  Region 1: two separate squares (a MultiPolygon).  Region 2: a square nested
    in the island of region 0.  Every lattice point of the frame."""
    rings = [rect(0, 0, 40, 40), rect(8, 8, 32, 32), rect(14, 14, 26, 26)]
    return _case(lattice(-6, -6, 80, 46), None, 1, [rings, [rect(50, 0, 58, 8), rect(64, 4, 72, 12)], [rect(17, 17, 23, 23)]], (1, 2, 3, 5))


def shared_edge():
    """Two rectangles that share the side x == 12: every point on it is in band 0 of both and inside exactly one."""
    return _case(lattice(-4, -4, 28, 12), None, 1, [[rect(0, 0, 12, 8)], [rect(12, 0, 24, 8)]], (1, 2, 4))


# ---- edges around the points' box, within R and beyond it
def around_the_box():
    """Points on the lattice of (0, 0) .. (60, 40), R = 20.  Eight squares outside the box: above, below, left and right of it at a gap of 10
    (within R) and of 30 (beyond it), and region 8, which contains the whole box from far away (only the parity sees it)."""
    sq = [rect(20, -20, 30, -10), rect(20, 50, 30, 60), rect(-20, 15, -10, 25), rect(70, 15, 80, 25),
          rect(20, -45, 30, -30), rect(20, 70, 30, 85), rect(-45, 15, -30, 25), rect(90, 15, 105, 25), rect(-300, -300, 400, 400)]
    p = lattice(0, 0, 60, 40, 2)
    return _case(p, np.arange(len(p)) % 3, 3, [[r] for r in sq], (5, 10, 20))


def empty_slab():
    """Three groups of points 500 apart in y and regions near the outer two only, R = 20: at slab heights 1 and 7 the middle group's slabs
    hold points but no edge record."""
    rng = np.random.default_rng(5)
    group = lambda y: np.stack([rng.integers(0, 200, 120), rng.integers(y, y + 6, 120)], 1)
    return _case(np.concatenate([group(0), group(500), group(1000)]), rng.integers(0, 2, 360), 2,
                 [[rect(50, -10, 150, 12)], [[(20, 990), (180, 1000), (90, 1030)]]], (4, 9, 20))


# ---- staging
def staging():
    """700 points in a band ten half pixels tall, 600 coincident points and 300 points over a box 2000 tall.  Region 0: a star of exactly 256
    vertices around the band -- with one slab (height 16384) its 256 records fill the first staging pass, so the region changes exactly on
    the 256-record boundary.  Region 1: a star of 600 vertices (more records in a slab than a pass holds).  Region 2: a tall triangle whose
    long edges span every slab (every edge of the set is within R of the box: one record each with one slab).  Region 3 contains the whole box."""
    rng = np.random.default_rng(19)
    band = np.stack([rng.integers(0, 301, 700), rng.integers(100, 111, 700)], 1)
    tall = np.stack([rng.integers(0, 301, 300), rng.integers(0, 2001, 300)], 1)
    p = np.concatenate([band, np.full((600, 2), (150, 105)), tall, [[0, 0], [300, 2000]]], 0)

    def star(k, r0):
        t = 2 * np.pi * np.arange(k) / k
        rad = r0 + 30 * (np.arange(k) % 2) + rng.integers(0, 8, k)
        return np.rint(np.stack([150 + rad * np.cos(t), 105 + rad * np.sin(t)], 1)).astype(np.int64).tolist()
    regions = [[star(256, 60)], [star(600, 45)], [[(-50, -1000), (400, 2040), (-50, 2040)]], [rect(-10, -10, 310, 2010)]]
    return _case(p, rng.integers(-1, 5, len(p)), 4, regions, (3, 6, 12, 25, 50))


# ---- the walk of a workgroup through its slabs, at ONE slab height
SLAB_WALK_SLAB = RC.SLAB_WALK_SLAB


def slab_walk():
    """`regions_cases.slab_walk` under thresholds up to R = 20: the records per slab are the census's (no grown y-range reaches another
    slab), the middle slab of the first workgroup has none, and region 2 is farther than R from every point."""
    return RC.slab_walk() + (np.asarray([3, 8, 20], np.int32),)


# ---- many ties
def random_lattice(seed, n=2000, regions=10):
    """`regions_cases.random_lattice` (everything on multiples of 4 within a square of 240, labels partly outside the classes) under
    thresholds that are 4 times the hypotenuses and legs of small Pythagorean triples: very many pairs lie exactly at a threshold."""
    return RC.random_lattice(seed, n, regions) + (np.asarray([4, 8, 12, 16, 20, 40, 52, 60, 68], np.int32),)


def empty_cases():
    some = regimes()
    none = np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
    return dict(no_points=none + some[2:], no_regions=some[:3] + RC.table([]) + some[6:], neither=none + (2,) + RC.table([]) + some[6:],
                regions_without_edges=some[:3] + RC.table([])[:2] + (3,) + some[6:])


def all_cases():
    """name -> case: every designed set, for the tests that run each one through the same check."""
    cases = dict(regimes=regimes(), float64_pair=float64_pair(), holes_and_nested=holes_and_nested(), shared_edge=shared_edge(),
                 around_the_box=around_the_box(), empty_slab=empty_slab(), staging=staging(), random_lattice_1=random_lattice(1),
                 random_lattice_2=random_lattice(2, 1200, 30))
    cases.update({f'pythagorean_{c}': pythagorean((a, b, c))[0] for a, b, c in TRIPLES})
    cases.update(empty_cases())
    return cases
