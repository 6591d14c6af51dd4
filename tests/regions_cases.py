"""Designed inputs for the region census (nuhtc_amd/regions.py), shared by tests/test_regions_host.py (the restatement against a double loop
in Python integers, hand-written rows, the tiling property and matplotlib) and tests/test_hip_regions.py (the device against the
restatement).  A case is (points int32 (n, 2) half pixels, labels int32 (n,), num_classes, edges int32 (E, 4), edge_region int32 (E,), G).
Regions are written here as lists of rings of half-pixel vertices and turned into the edge table by `table`, independently of the module's
own GeoJSON reader."""
import numpy as np

import proximity_cases as PC

P = (1 << 27) - 1


def table(regions):
    """regions: per region a list of rings, each a list of (x, y) half-pixel vertices without the closing repeat -> (edges, edge_region, G)."""
    edges, region = [], []
    for g, rings in enumerate(regions):
        for ring in rings:
            v = np.asarray(ring, np.int64).reshape(-1, 2)
            edges.append(np.concatenate([v, np.roll(v, -1, 0)], 1))
            region.append(np.full(len(v), g))
    e = np.concatenate(edges, 0) if edges else np.zeros((0, 4))
    return np.ascontiguousarray(e, np.int32).reshape(-1, 4), np.ascontiguousarray(np.concatenate(region) if region else np.zeros(0), np.int32), len(regions)


def _case(p, lab, C, regions):
    p = np.ascontiguousarray(np.asarray(p, np.int64).reshape(-1, 2), np.int32)
    lab = np.zeros(len(p), np.int32) if lab is None else np.ascontiguousarray(np.asarray(lab).reshape(-1), np.int32)
    assert len(lab) == len(p)
    return (p, lab, C) + table(regions)


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def lattice(x0, y0, x1, y1, step=1):
    y, x = np.mgrid[y0:y1 + 1:step, x0:x1 + 1:step]
    return np.stack([x.ravel(), y.ravel()], 1)


def permuted(case, seed=4):
    order = np.random.default_rng(seed).permutation(len(case[0]))
    return (case[0][order], case[1][order]) + case[2:], order


# ---- the unit rectangle, by hand
RECT_POINTS = [(0, 0), (10, 0), (10, 6), (0, 6), (5, 0), (10, 3), (5, 6), (0, 3), (5, 3), (12, 3), (-2, 3)]
RECT_REGION = [0, -1, -1, -1, 0, -1, -1, 0, 0, -1, -1]       # the min-x and min-y sides belong to it, the max sides do not
RECT_ON = [1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0]


def unit_rectangle():
    return _case(RECT_POINTS, [0, 1] * 5 + [0], 2, [[rect(0, 0, 10, 6)]])


def unit_rectangle_expected():
    region = np.asarray(RECT_REGION, np.int32)
    census = np.zeros((1, 2), np.int64)
    np.add.at(census, (0, np.asarray([0, 1] * 5 + [0])[region == 0]), 1)
    return region, (region == 0).astype(np.int32), np.asarray(RECT_ON, np.uint8), census


# ---- tiling: two rectangles that share a side, four triangles that share an apex at a lattice point
def tiling():
    tri = [[(20, 0), (28, 0), (24, 4)], [(28, 0), (28, 8), (24, 4)], [(28, 8), (20, 8), (24, 4)], [(20, 8), (20, 0), (24, 4)]]
    return _case(lattice(-2, -2, 31, 10), None, 1, [[rect(0, 0, 6, 4)], [rect(6, 0, 12, 4)]] + [[t] for t in tri])


def tiling_union(p):
    """bool (n,): the points of the union of the pieces, half-open as the definition makes it."""
    x, y = p[:, 0], p[:, 1]
    return ((x >= 0) & (x < 12) & (y >= 0) & (y < 4)) | ((x >= 20) & (x < 28) & (y >= 0) & (y < 8))


# ---- rays through vertices and along edges
def notch():
    """A box with a notch cut from its top: (6, 4) is a local extremum of the boundary (both notch sides rise from it), (13, 5) a vertex of
    a monotone chain on the right side; the top sides and the bottom are horizontal edges.  Points on the rows y = 4, 5, 10 and 0 send
    their rays through those vertices and along those edges; (6, 4), (13, 5) and (0, 0) are ON vertices."""
    ring = [(0, 0), (12, 0), (13, 5), (12, 10), (8, 10), (6, 4), (4, 10), (0, 10)]
    pts = [(x, y) for y in (0, 4, 5, 10) for x in range(-3, 16)] + [(6, 5), (6, 3), (5, 7), (7, 7), (6, 9)]
    return _case(pts, None, 1, [[ring]])


NOTCH_HAND = {(2, 4): 0, (6, 4): 0, (7, 4): 0, (-3, 4): -1, (12, 4): 0, (13, 4): -1, (2, 5): 0, (6, 5): -1, (12, 5): 0, (13, 5): -1, (5, 10): -1, (2, 10): -1, (-2, 10): -1,
              (3, 0): 0, (-1, 0): -1, (12, 0): -1, (6, 3): 0, (6, 9): -1, (5, 7): -1}


# ---- holes, orientation, multipolygon
def holes(flip=(False, False, False)):
    """Region 0: a ring, a hole in it and an island in the hole, each reversed where `flip` says; region 1: two separate squares (a
    MultiPolygon).  Every lattice point of the frame."""
    rings = [rect(0, 0, 20, 20), rect(4, 4, 16, 16), rect(8, 8, 12, 12)]
    rings = [r[::-1] if f else r for r, f in zip(rings, flip)]
    return _case(lattice(-1, -1, 47, 21), None, 1, [rings, [rect(30, 0, 36, 6), rect(40, 2, 46, 8)]])


# ---- overlap
OVERLAP_RECTS = [(0, 0, 30, 30), (5, 5, 25, 25), (10, 10, 15, 15), (20, 20, 40, 40)]


def overlap(labels='in'):
    p = lattice(-1, -1, 41, 41)
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 3, len(p)) if labels == 'in' else np.array([-1, 0, 1, 2, 3, 14])[np.arange(len(p)) % 6]
    return _case(p, lab, 3, [[rect(*r)] for r in OVERLAP_RECTS])


def overlap_features():
    """The rectangles of `overlap` as GeoJSON features in px (half the half-pixel numbers), small ones first: order='area' must put them back."""
    def feat(r, name):
        x0, y0, x1, y1 = (v / 2 for v in r)
        ring = [[x0, y0], [x1, y0], [x1, y1], [x0, y1], [x0, y0]]
        return dict(type='Feature', geometry=dict(type='Polygon', coordinates=[ring]), properties=dict(classification=dict(name=name)))
    return [feat(OVERLAP_RECTS[2], 'small'), feat(OVERLAP_RECTS[3], 'other'), feat(OVERLAP_RECTS[1], 'mid'), feat(OVERLAP_RECTS[0], 'big')]


# ---- degenerate rings
def degenerate():
    """Region 0: a ring of one vertex (one zero-length edge).  Region 1: a square with a repeated vertex.  Region 2: a ring of two points
    (area 0: it contains nothing and touches the points on it)."""
    return _case(lattice(-1, -1, 16, 8), None, 1, [[[(3, 3)]], [[(0, 0), (6, 0), (6, 0), (6, 6), (0, 6)]], [[(10, 0), (14, 4)]]])


# ---- the bit budget
def bit_budget():
    """A thin triangle whose long edge A -> B has u = (2**28 - 3, 2**28 - 7): the lattice points nearest to it have cross products +1 and -1
    against products of 1.5 * 2**55.  -> (case, (row of the +1 point, row of the -1 point), (A, B))."""
    a, b = (1 << 28) - 3, (1 << 28) - 7
    A = (-P, -P)
    B = (A[0] + a, A[1] + b)
    w1 = ((1 + 3 * a) // 4, (1 + 3 * a) // 4 - 3)
    w2 = (a - w1[0], b - w1[1])
    assert a * w1[1] - b * w1[0] == 1 and a * w2[1] - b * w2[0] == -1 and a * w1[1] > 1 << 55
    p1, p2 = (A[0] + w1[0], A[1] + w1[1]), (A[0] + w2[0], A[1] + w2[1])
    pts = [p1, p2, A, B, (B[0], B[1] + 4), (0, 0), (p1[0] - 1, p1[1]), (p1[0] + 1, p1[1]), (p2[0], p2[1] + 1), (P, -P), (-P, P)]
    return _case(pts, None, 1, [[[A, B, (B[0], B[1] + 4)]]]), (0, 1), (A, B)


# ---- staging and slabs
def staging():
    """700 points in a band ten half pixels tall, 1500 coincident points and 300 points over a box 2000 tall.  Region 0: a tall triangle whose
    long edges span every slab.  Region 1: a star of 600 vertices around the band (more edge records in a slab than one staging pass
    holds).  Regions 2..5: squares wholly left, right, above and below the points' box.  Region 6 contains the whole box."""
    rng = np.random.default_rng(19)
    band = np.stack([rng.integers(0, 301, 700), rng.integers(100, 111, 700)], 1)
    tall = np.stack([rng.integers(0, 301, 300), rng.integers(0, 2001, 300)], 1)
    p = np.concatenate([band, np.full((1500, 2), (150, 105)), tall, [[0, 0], [300, 2000]]], 0)
    t = 2 * np.pi * np.arange(600) / 600
    rad = 45 + 30 * (np.arange(600) % 2) + rng.integers(0, 8, 600)
    star = np.rint(np.stack([150 + rad * np.cos(t), 105 + rad * np.sin(t)], 1)).astype(np.int64)
    regions = [[[(-50, -1000), (400, 3000), (-50, 3000)]], [star.tolist()], [rect(-90, 500, -20, 600)], [rect(320, 500, 390, 600)],
               [rect(100, -90, 200, -20)], [rect(100, 2020, 200, 2090)], [rect(-10, -10, 310, 2010)]]
    return _case(p, rng.integers(0, 4, len(p)), 4, regions)


# ---- the walk of a workgroup through its slabs (csrc/celledges.h rg_walk), at ONE slab height
SLAB_WALK_SLAB = 200


def slab_walk():
    """300 points on a box 1000 x 599 at slab height 200: 100 in slab 0, 60 in slab 1, 140 in slab 2, so the first workgroup of 256 records
    lies in three slabs and the second one is partial.  Region 0: a square in slab 0 and a zigzag ring of 256 vertices in slab 2; region
    1: a zigzag ring of 260 vertices inside it; region 2: a rectangle wholly right of the box beside slab 2 (kept for the parity; farther
    than 20 from every point).  Every edge keeps 30 from the rows of slab 1, which has no edge record at all -- also with the y-ranges
    grown by 20 (tests/margin_cases.py) -- and the records of slab 2 number 256 + 260 + 4: the region changes at record 256, exactly
    between two staging passes, and at record 516, inside the last, partial pass."""
    rng = np.random.default_rng(23)
    cloud = lambda k, y0, y1: np.stack([rng.integers(0, 1001, k), rng.integers(y0, y1 + 1, k)], 1)

    def ring(k, cy, rx, ry):
        t = 2 * np.pi * np.arange(k) / k
        wob = 1 + 0.15 * (np.arange(k) % 2)
        return np.rint(np.stack([500 + rx * wob * np.cos(t), cy + ry * wob * np.sin(t)], 1)).astype(np.int64).tolist()
    outer, inner = ring(256, 500, 400, 60), ring(260, 500, 200, 35)
    on_ring = [outer[0], outer[64], inner[1], inner[131]]                                   # points ON vertices of both rings
    p = np.concatenate([[[0, 0]], cloud(95, 0, 199), [[400, 40], [600, 150], [400, 95], [503, 150]], cloud(60, 200, 399),
                        on_ring, cloud(135, 400, 599), [[1000, 599]]], 0)
    return _case(p, rng.integers(-1, 4, len(p)), 3, [[rect(400, 40, 600, 150), outer], [inner], [rect(1100, 450, 1200, 550)]])


def slab_layout(case, slab, grow=0):
    """What a workgroup walks through, by a direct loop: (the points per slab, and per slab the regions of its edge records in edge
    order) at slab height `slab` with every edge's y-range grown by `grow`.  For a box small enough that the cell side IS the slab."""
    p, edges, er = case[0].astype(np.int64), case[3].astype(np.int64), case[4]
    x_min, y_min, y_max = p[:, 0].min(), p[:, 1].min(), p[:, 1].max()
    rows = (y_max - y_min) // slab + 1
    records = [[] for _ in range(rows)]
    for (ax, ay, bx, by), g in zip(edges.tolist(), er.tolist()):
        if ax < x_min - grow and bx < x_min - grow:
            continue
        for s in range(rows):
            if max(ay, by) + grow >= y_min + s * slab and min(ay, by) - grow <= min(y_min + (s + 1) * slab - 1, y_max):
                records[s].append(g)
    return np.bincount((p[:, 1] - y_min) // slab, minlength=rows).tolist(), records


# ---- scale
def chain(order):
    """The chain of tests/proximity_cases.py (20 000 points 8 apart on the line y = 11) under four regions: a long rectangle, a triangle whose
    slanted side cuts the line, a rectangle whose min-y side IS the line and one whose max-y side is."""
    p, lab = PC.chain(order)[:2]
    regions = [[rect(1000, 0, 50001, 22)], [[(60000, -100), (90000, 11), (60000, 300)]], [rect(100000, 11, 120000, 40)], [rect(130000, -40, 150000, 11)]]
    return _case(p, lab, 2, regions)


def random_lattice(seed, n=3000, regions=12):
    """n points and `regions` random regions of one or two rings of 3..9 vertices, everything on multiples of 4 within a square of 240: many
    points on edges and on vertices, overlapping regions, labels partly outside the classes.  A ring's vertices are distinct and sorted by
    angle (then distance) about their mean, which makes it simple: matplotlib's winding rule and even-odd then agree."""
    rng = np.random.default_rng(seed)

    def ring():
        v = np.unique(4 * rng.integers(0, 61, (int(rng.integers(3, 10)), 2)), axis=0)
        d = v - v.mean(0)
        return [tuple(q) for q in v[np.lexsort((np.hypot(d[:, 0], d[:, 1]), np.arctan2(d[:, 1], d[:, 0])))].tolist()]
    rings = [[ring() for _ in range(int(rng.integers(1, 3)))] for _ in range(regions)]
    return _case(4 * rng.integers(0, 61, (n, 2)), rng.integers(-1, 5, n), 4, rings)


def empty_cases():
    some = unit_rectangle()
    none = np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
    return dict(no_points=none + some[2:], no_regions=some[:3] + table([]), neither=none + (2,) + table([]),
                region_without_edges=some[:3] + (some[3], some[4] + 1, 3))


def all_cases():
    """name -> case: every designed set, for the tests that run each one through the same check."""
    cases = dict(unit_rectangle=unit_rectangle(), tiling=tiling(), notch=notch(), holes=holes(), holes_all_reversed=holes((True, True, True)),
                 holes_some_reversed=holes((False, True, False)), overlap=overlap(), labels_out_of_range=overlap('out'), degenerate=degenerate(),
                 bit_budget=bit_budget()[0], staging=staging(), random_lattice_1=random_lattice(1), random_lattice_2=random_lattice(2, 1500, 40))
    cases.update({'chain_' + order: chain(order) for order in ('ascending', 'descending', 'shuffled')})
    cases.update(empty_cases())
    return cases
