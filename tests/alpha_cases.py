"""Designed point sets for the alpha complex (nuhtc_amd/alphacomplex.py), shared by tests/test_alpha_host.py (the restatement against a
loop in Python fractions, hand-written lists, closed forms, scipy's Delaunay, the Gabriel graph and the forest) and
tests/test_hip_alpha.py (the device against the restatement).  A case is (points int (n, 2) half pixels, labels (n,), num_classes, r half
pixels, by_class); D = 2 r is the diameter.  `small_cases` are few enough points for the loop in fractions; the others are sized to what
can go wrong on the device only (rows over two scan chunks, a cell fuller than a workgroup, more edges than the first call has room for).
`expected` turns hand-written rows (i, j, d2, apex0, apex1, gabriel) into the seven results of alpha_reference."""
from fractions import Fraction

import numpy as np

NAMES = ('edges', 'edge_d2', 'apex', 'edge_gabriel', 'degree', 'm', 'm_gabriel')


def _case(p, lab, C, r, by_class=0):
    p = np.asarray(p, np.int32).reshape(-1, 2)
    lab = np.zeros(len(p), np.int32) if lab is None else np.asarray(lab, np.int32).reshape(-1)
    assert len(lab) == len(p)
    return p, lab, C, r, by_class


def expected(n, rows):
    """rows: (i, j, d2, apex0, apex1, gabriel) in any order -> the seven results of alpha_reference."""
    e = np.asarray(sorted(rows), np.int64).reshape(-1, 6)
    gab = e[:, 5].astype(bool)
    edges = e[:, :2].astype(np.int32).reshape(-1, 2)
    degree = np.stack([np.bincount(edges.reshape(-1), minlength=n), np.bincount(edges[gab].reshape(-1), minlength=n)], 1).astype(np.int32).reshape(n, 2)
    return edges, e[:, 2].astype(np.int32), e[:, 3:5].astype(np.int32).reshape(-1, 2), gab.astype(np.uint8), degree, len(e), int(gab.sum())


def equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        if name in ('m', 'm_gabriel'):
            assert int(g) == int(w), (what, name, int(g), int(w))
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, f'{len(bad)} entries differ, first at {bad[0].tolist()}', int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


def fraction_loop(p, lab, C, r, by_class):
    """The definition word for word: Python integers and fractions, every pair, EVERY other row as a witness (none passed over for its
    distance) -> the seven results as lists."""
    p, lab, n = [(int(x), int(y)) for x, y in p], [int(v) for v in lab], len(p)
    D2 = 4 * r * r
    edges, dist, apexes, flags, degree = [], [], [], [], [[0, 0] for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            qx, qy = p[j][0] - p[i][0], p[j][1] - p[i][1]
            d2 = qx * qx + qy * qy
            if d2 > D2 or (by_class and lab[i] != lab[j]):
                continue
            hi = lo = None
            hk = lk = -1
            blocked, gabriel = False, True
            if d2 > 0:
                T2 = Fraction(D2 - d2, d2)
                le_T = lambda t: t <= 0 or t * t <= T2
                ge_neg_T = lambda t: t >= 0 or t * t <= T2
                for k in range(n):
                    if k == i or k == j or (by_class and lab[k] != lab[i]):
                        continue
                    rx, ry = p[k][0] - p[i][0], p[k][1] - p[i][1]
                    s, m = qx * ry - qy * rx, rx * (rx - qx) + ry * (ry - qy)
                    if m < 0:
                        gabriel = False
                    if s == 0:
                        blocked = blocked or m < 0
                    elif s > 0 and (hi is None or Fraction(m, s) < hi):          # k ascends: the first row that attains a bound is the smallest
                        hi, hk = Fraction(m, s), k
                    elif s < 0 and (lo is None or Fraction(m, s) > lo):
                        lo, lk = Fraction(m, s), k
                if blocked or (hi is not None and not ge_neg_T(hi)) or (lo is not None and not le_T(lo)) or (hi is not None and lo is not None and lo > hi):
                    continue
                hk = hk if hi is not None and le_T(hi) else -1
                lk = lk if lo is not None and ge_neg_T(lo) else -1
            edges.append([i, j]); dist.append(d2); apexes.append([hk, lk]); flags.append(int(gabriel))
            for end in (i, j):
                degree[end][0] += 1
                degree[end][1] += int(gabriel)
    return edges, dist, apexes, flags, degree, len(edges), sum(flags)


# ---- on and beside the diameter
def two_points(d2_over):
    """Two points (0, 0) and (6, 8 + d2_over) at r = 5, D = 10: d2 = 100 = D * D is an edge (T = 0: the diametral circle alone), d2 = 117 is none;
    and (10, 1) at d2 = D * D + 1 = 101 in `two_points_one_over`."""
    return _case([[0, 0], [6, 8 + d2_over]], [0, 1], 2, 5)


TWO_AT_D = [(0, 1, 100, -1, -1, 1)]


def two_points_one_over():
    return _case([[0, 0], [10, 1]], [0, 1], 2, 5)


# ---- the right triangle 6-8-10: its circumcircle is the diametral circle of the hypotenuse, radius 5
def right_triangle(r):
    return _case([[0, 0], [6, 0], [0, 8]], None, 1, r)


# r = 5: edge (0, 1) has row 2 on the left at t = 64 / 48 = 4 / 3 = T exactly; (0, 2) has row 1 on the right at -3 / 4 = -T; the hypotenuse
# (1, 2) at d2 = D * D has T = 0 and row 0 ON its diametral circle (t = 0, m = 0: Gabriel stays)
RIGHT_5 = [(0, 1, 36, 2, -1, 1), (0, 2, 64, -1, 1, 1), (1, 2, 100, 0, -1, 1)]
# r = 4: the circumradius 5 is out of reach -- the two legs stay by their diametral discs, without apexes; the hypotenuse is no candidate
RIGHT_4 = [(0, 1, 36, -1, -1, 1), (0, 2, 64, -1, -1, 1)]


# ---- cocircular points: the circle of radius 25 about the lattice point (100, -50)
ON_CIRCLE = [(25, 0), (7, 24), (-15, 20), (-24, -7), (0, -25), (20, -15), (-7, -24)]


def cocircular(k, r=25):
    assert all(x * x + y * y == 625 for x, y in ON_CIRCLE)
    return _case([[100 + x, -50 + y] for x, y in ON_CIRCLE[:k]], np.arange(k) % 2, 2, r)


# ---- collinear points
def collinear():
    """Rows 0-2 at x = 0, 5, 10: (0, 2) is blocked by row 1 strictly between its ends.  Rows 3-5 at x = 100, 105, 112 with the pair
    (3, 4) and row 5 collinear OUTSIDE the segment: it does not bind ((3, 5) is blocked by row 4)."""
    return _case([[0, 0], [5, 0], [10, 0], [100, 3], [105, 3], [112, 3]], None, 1, 10)


COLLINEAR = [(0, 1, 25, -1, -1, 1), (1, 2, 25, -1, -1, 1), (3, 4, 25, -1, -1, 1), (4, 5, 49, -1, -1, 1)]


# ---- on and inside the diametral circle: groups 1000 apart, r = 20
def diametral():
    """Rows 0-1 of every group are (0, 0) and (10, 0), d2 = 100; row 2 is the witness.
    group 0  (5, 5): ON the diametral circle (m = 0): Gabriel stays, and the witness is the apex of the left side at t = 0
    group 1  (5, 4): one half-pixel step inside (m = -9 < 0): the Gabriel flag drops and the edge SURVIVES -- the circles t <= -9 / 40 avoid it"""
    p = []
    for g, w in enumerate(((5, 5), (5, 4))):
        p += [[1000 * g, 0], [1000 * g + 10, 0], [1000 * g + w[0], w[1]]]
    return _case(p, None, 1, 20)


DIAMETRAL = [(0, 1, 100, 2, -1, 1), (0, 2, 50, -1, 1, 1), (1, 2, 50, 0, -1, 1),
             (3, 4, 100, 5, -1, 0), (3, 5, 41, -1, 4, 1), (4, 5, 41, 3, -1, 1)]


# ---- a binding witness farther from i than j is
def far_witness():
    """i = (0, 0), j = (4, 0), r = 10: T**2 = 24.  Row 2 at (10, 6) is sqrt(136) from i (j is 4 away) and binds at t = 96 / 24 = 4 <= T: the
    proximity kernel's witness window (nearer to i than j is) would miss it."""
    return _case([[0, 0], [4, 0], [10, 6]], None, 1, 10)


# ---- the lattice: closed form
def lattice(r, w=4, h=4, s=10, origin=(0, 0)):
    """w x h points at spacing s, row y * w + x.  A cell's circumradius is s / sqrt(2): with D < s * sqrt(2) the sides are the edges (no
    apex: every bound lies beyond T), from D >= s * sqrt(2) on BOTH diagonals of every cell join them (four cocircular points)."""
    y, x = np.divmod(np.arange(w * h), w)
    return _case(np.stack([origin[0] + s * x, origin[1] + s * y], 1), (x + y) % 2, 2, r)


def lattice_edges(w, h, diagonals):
    return w * (h - 1) + h * (w - 1) + (2 * (w - 1) * (h - 1) if diagonals else 0)


# ---- witnesses and pairs across cell borders
def borders():
    """r = 5, D = 10, the box starts at (0, 0): cells are 10 wide.  Rows 0-1 pin the box.  Rows 2-4: (11, 15) and (3, 15) are a pair across
    a cell border, the witness (7, 15) between them sits in the SIDE cell.  Rows 5-7: (31, 31) and (25, 25), the witness (28, 28) in the
    CORNER cell.  Rows 8-10: (62, 20) and (68, 20) in one cell with the binding witness (65, 13) in the cell BELOW.  Rows 11-13: (80, 45)
    and (89, 45) with (84, 44) just inside their diametral circle, which no circle of radius <= 5 through both avoids."""
    p = [[0, 0], [99, 59], [11, 15], [3, 15], [7, 15], [31, 31], [25, 25], [28, 28], [62, 20], [68, 20], [65, 13], [80, 45], [89, 45], [84, 44]]
    return _case(p, None, 1, 5)


def cell_boundaries_negative():
    """150 random points on [-40, 40]^2 with r = 5: the grid starts at a negative corner, cells are 10 wide, and every tenth point is
    moved onto a multiple of 10 from that corner -- the first coordinate of a cell -- with a partner one half pixel below it."""
    rng = np.random.default_rng(31)
    p = rng.integers(-40, 41, (150, 2))
    p[0] = [-40, -40]
    p[5::10] = (p[5::10] + 40) // 10 * 10 - 40
    p[6::10] = p[5::10] - 1
    p = np.clip(p, -40, 40)
    return _case(p, rng.integers(0, 3, 150), 3, 5)


# ---- the two label modes
def other_label_witness(by_class):
    """Rows 0-1 of label 0 at (0, 0) and (10, 0), row 2 of label 1 at their midpoint: it blocks under `any` and not under `class`.  Rows 3-5
    the same far away with the labels -1, -1 and 7 (outside 0..C-1: compared by plain equality)."""
    return _case([[0, 0], [10, 0], [5, 0], [500, 0], [510, 0], [505, 0]], [0, 0, 1, -1, -1, 7], 2, 6, by_class)


OTHER_LABEL = {0: [(0, 2, 25, -1, -1, 1), (1, 2, 25, -1, -1, 1), (3, 5, 25, -1, -1, 1), (4, 5, 25, -1, -1, 1)],
               1: [(0, 1, 100, -1, -1, 1), (3, 4, 100, -1, -1, 1)]}


def labels_out_of_range(by_class):
    """C = 3 with labels -1, 7 and 1 on forty nearby points."""
    rng = np.random.default_rng(8)
    return _case(rng.integers(0, 14, (40, 2)), np.array([-1, 7, 1])[np.arange(40) % 3], 3, 4, by_class)


# ---- ties
def coarse(by_class=0, n=300, side=41, r=4, seed=12):
    """n points on a coarse lattice with the coordinates 0 .. side - 1: full of collinear, cocircular and coincident points."""
    rng = np.random.default_rng(seed)
    return _case(rng.integers(0, side, (n, 2)), rng.integers(-1, 4, n), 3, r, by_class)


def random_small(by_class, r=9):
    rng = np.random.default_rng(77)
    return _case(rng.integers(0, 90, (160, 2)), rng.integers(-1, 4, 160), 3, r, by_class)


# ---- the largest diameter
def largest(seed=3):
    """r = 512, D = 1024.  Rows 0-1 one half pixel apart (T**2 = 2**20 - 1) with witnesses at the largest offsets that still bind: 1023 straight
    above and below either end (m = 1023**2, s = +-1023, t = +-1023 < T, two rows tied on each side), and one beyond D from both ends (passed
    over by the restatement, not by the loop in fractions: its bound lies beyond T).  Rows 7-8 exactly D apart (T = 0) with one witness ON
    their diametral circle and one a step outside it.  Then 50 random rows on a box that D reaches across."""
    rng = np.random.default_rng(seed)
    p = [[0, 0], [1, 0], [0, 1023], [1, -1023], [0, -1023], [1, 1023], [0, 1025],
         [3000, 0], [3000 + 1024, 0], [3512, 512], [3512, -513], [3000 + 600, 0 + 5000], [3000, 5000]]
    p += (rng.integers(0, 700, (50, 2)) + [6000, 6000]).tolist()
    return _case(p, rng.integers(0, 2, len(p)), 2, 512)


def general_position(n=120, seed=5, extent=700):
    """Random points on a box small enough for D = 1024 to reach across it, no two coincident."""
    rng = np.random.default_rng(seed)
    p = np.unique(rng.integers(0, extent, (n, 2)), axis=0)
    return rng.permutation(p)


def small_cases():
    return dict(two_at_D=two_points(0), two_beyond=two_points(1), two_one_over=two_points_one_over(), right_5=right_triangle(5), right_4=right_triangle(4),
                circle_3=cocircular(3), circle_5=cocircular(5), circle_7=cocircular(7), circle_3_r24=cocircular(3, 24), circle_5_r24=cocircular(5, 24),
                collinear=collinear(), diametral=diametral(), far_witness=far_witness(), lattice_14=lattice(7), lattice_16=lattice(8),
                lattice_28=lattice(14, s=20), lattice_30=lattice(15, s=20), lattice_3x2=lattice(4, 3, 2, 5, (-17, 9)), borders=borders(),
                cell_boundaries_negative=cell_boundaries_negative(), other_label_any=other_label_witness(0), other_label_class=other_label_witness(1),
                out_of_range_any=labels_out_of_range(0), out_of_range_class=labels_out_of_range(1), coarse_any=coarse(0, 120, 9, 4),
                coarse_class=coarse(1, 120, 9, 4), random_any=random_small(0), random_class=random_small(1), largest=largest(),
                one_point=_case([[123456, -7890]], [2], 3, 8), two_coincident=_case([[4, 4], [4, 4]], [0, 1], 2, 1),
                radius_one=_case([[0, 0], [1, 0], [1, 1], [2, 1], [3, 1]], None, 1, 1), short_chain_shuffled=chain('shuffled', 40),
                crowded_small=crowded(70), coincident_small=coincident(12))


def translate(case, dx, dy):
    return (case[0] + np.array([dx, dy], np.int32),) + case[1:]


# ---- device-sized
def coincident(n=300):
    """n coincident points (a clique of n (n - 1) / 2 edges of d2 = 0, no apexes, all Gabriel: more than the first call has room for) and
    five others."""
    p = [[5000, 5000]] * n + [[5000 + 3 * k, 4990 + 5 * k] for k in range(5)]
    return _case(p, np.arange(n + 5) % 3, 3, 8)


def chain(order, n=20000, r=8):
    """n points D / 2 = r apart on a line, wherever `order` ('ascending', 'descending', 'shuffled') puts the rows: every point has four
    candidates (one and two places away on either side); the links between neighbouring places are the edges, places two apart are
    blocked by the place between them."""
    k = dict(ascending=np.arange(n), descending=np.arange(n)[::-1], shuffled=np.random.default_rng(3).permutation(n))[order]
    return _case(np.stack([k * r - 7, np.full(n, 11)], 1), k % 2, 2, r)


def chain_expected(case):
    p, r = case[0], case[3]
    at = np.argsort((p[:, 0] + 7) // r)                     # the row at every place
    e = np.sort(np.stack([at[:-1], at[1:]], 1), 1)
    return expected(len(p), [(int(i), int(j), r * r, -1, -1, 1) for i, j in e])


def crowded(n=1500, s=2, r=2):
    """n points thrown on the 3 x 3 lattice at spacing s (D = 2 r = 2 s: the sites two apart are candidates that the site between them
    blocks), all in one or two cells: about n / 9 coincident points per site, a cell fuller than a workgroup, and hundreds of thousands
    of edges -- two rows are joined when they share a site or sit on the two ends of a side or of a diagonal of a cell."""
    rng = np.random.default_rng(15)
    site = rng.integers(0, 9, n)
    return _case(np.stack([s * (site % 3) + 100, s * (site // 3) - 50], 1), rng.integers(0, 3, n), 3, r)


def crowded_expected(case):
    """The seven results for points with many repeats (by_class 0), from the complex of the DISTINCT sites in fractions: rows on one
    site are joined (d2 = 0, no apex, Gabriel) and never bind each other, so a pair of rows on two sites has the bounds of the two sites,
    and its apex is the smallest row on any site that attains the bound."""
    p, r = case[0].astype(np.int64), case[3]
    assert case[4] == 0
    sites, site_of = np.unique(p, axis=0, return_inverse=True)
    site_of = site_of.reshape(-1)
    S, D2 = len(sites), 4 * r * r
    first = np.full(S, len(p), np.int64)
    np.minimum.at(first, site_of, np.arange(len(p)))
    edge, gab = np.zeros((S, S), bool), np.ones((S, S), bool)
    apex = np.full((S, S, 2), -1, np.int64)
    P = [(int(x), int(y)) for x, y in sites]
    for A in range(S):
        for B in range(S):
            qx, qy = P[B][0] - P[A][0], P[B][1] - P[A][1]
            d2 = qx * qx + qy * qy
            if A == B or d2 > D2:
                continue
            T2, hi, lo, at_hi, at_lo, blocked = Fraction(D2 - d2, d2), None, None, [], [], False
            for K in range(S):
                if K in (A, B):
                    continue
                rx, ry = P[K][0] - P[A][0], P[K][1] - P[A][1]
                s, m = qx * ry - qy * rx, rx * (rx - qx) + ry * (ry - qy)
                gab[A, B] &= m >= 0
                if s == 0:
                    blocked |= m < 0
                elif s > 0 and (hi is None or Fraction(m, s) <= hi):
                    at_hi = at_hi + [K] if hi == Fraction(m, s) else [K]
                    hi = Fraction(m, s)
                elif s < 0 and (lo is None or Fraction(m, s) >= lo):
                    at_lo = at_lo + [K] if lo == Fraction(m, s) else [K]
                    lo = Fraction(m, s)
            le_T = lambda t: t <= 0 or t * t <= T2
            ge_neg_T = lambda t: t >= 0 or t * t <= T2
            if blocked or (hi is not None and not ge_neg_T(hi)) or (lo is not None and not le_T(lo)) or (hi is not None and lo is not None and lo > hi):
                continue
            edge[A, B] = True
            if hi is not None and le_T(hi):
                apex[A, B, 0] = min(first[K] for K in at_hi)
            if lo is not None and ge_neg_T(lo):
                apex[A, B, 1] = min(first[K] for K in at_lo)
    same = site_of[:, None] == site_of[None, :]
    i, j = np.nonzero(np.triu(same | edge[site_of[:, None], site_of[None, :]], 1))
    A, B = site_of[i], site_of[j]
    d2 = ((p[i] - p[j]) ** 2).sum(1)
    rows = np.column_stack([i, j, d2, np.where(A == B, -1, apex[A, B, 0]), np.where(A == B, -1, apex[A, B, 1]), np.where(A == B, True, gab[A, B])])
    return expected(len(p), [tuple(int(v) for v in row) for row in rows])


def side_and_corner_cells():
    """r = 8, D = 16, the box pinned to (0, 0) .. (159, 159): cells are 16 wide.  300 points around the corner where four cells meet, within
    12 of it: nearly every pair has its witnesses in the side and corner cells of its smaller row's cell."""
    rng = np.random.default_rng(21)
    p = np.concatenate([[[0, 0], [159, 159]], 80 + rng.integers(-12, 13, (300, 2))])
    return _case(p, rng.integers(0, 3, len(p)), 3, 8)


def random_large(kind, r, by_class=0, n=3000):
    """3000 points on small integer coordinates (many equal distances and right angles), 12 blocks of threads: uniform on a square of 400,
    or in 12 Gaussian clumps on the same square (many coincident points)."""
    rng = np.random.default_rng(2026)
    if kind == 'uniform':
        p = rng.integers(0, 400, (n, 2))
    else:
        centre = rng.uniform(0, 400, (12, 2))
        p = np.clip(np.rint(centre[rng.integers(0, 12, n)] + rng.normal(0, 25, (n, 2))), 0, 399)
    return _case(p, rng.integers(-1, 5, n), 4, r, by_class)
