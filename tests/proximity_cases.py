"""Designed point sets for the proximity graphs (nuhtc_amd/proximity.py), shared by tests/test_proximity_host.py (the restatement against
a triple loop, closed forms, the forest and Delaunay) and tests/test_hip_proximity.py (the device against the restatement).  A case is
(points int (n, 2) half pixels, labels (n,), num_classes, r half pixels, by_class).  `small_cases` are few enough points for a Python
triple loop; the others are sized to what can go wrong on the device only (rows over two scan chunks, a cell fuller than a workgroup, more
edges than the first call has room for) and come with their expected arrays in closed form."""
import numpy as np


def _case(p, lab, C, r, by_class=0):
    p = np.asarray(p, np.int32).reshape(-1, 2)
    lab = np.zeros(len(p), np.int32) if lab is None else np.asarray(lab, np.int32).reshape(-1)
    assert len(lab) == len(p)
    return p, lab, C, r, by_class


def _expected(n, rows):
    """rows: (i, j, d2, rng) in any order -> the six results of proximity_reference."""
    e = np.asarray(sorted(rows), np.int64).reshape(-1, 4)
    return _from_arrays(n, e[:, 0], e[:, 1], e[:, 2], e[:, 3])


def _from_arrays(n, i, j, d2, rng):
    """i < j, d2, rng as arrays in any order -> the six results of proximity_reference."""
    order = np.lexsort((j, i))
    i, j, d2, rng = i[order], j[order], d2[order], rng[order].astype(bool)
    edges = np.stack([i, j], 1).astype(np.int32).reshape(-1, 2)
    degree = np.stack([np.bincount(edges.reshape(-1), minlength=n), np.bincount(edges[rng].reshape(-1), minlength=n)], 1).astype(np.int32).reshape(n, 2)
    return edges, d2.astype(np.int32), rng.astype(np.uint8), degree, len(i), int(rng.sum())


# ---- on and beside the circle, on and beside the radius: four groups of three rows, 1000 apart, r = 20
def circles():
    """Rows 0-1 of every group are (0, 0) and (10, 0), d2 = 100; row 2 is the witness.
    group 0  (5, 5): a right angle at the witness, sum == 100: the Gabriel edge stays (max 50 < 100: not an RNG edge)
    group 1  (5, 4): one half-pixel step inwards, sum 82: the edge goes
    group 2  (6, 8): as far from row 0 as row 1 is (100), 80 from row 1: the RNG edge stays
    group 3  (6, 7): one step nearer (85 and 65): the RNG edge goes, the Gabriel edge stays (150 >= 100)"""
    p = []
    for g, w in enumerate(((5, 5), (5, 4), (6, 8), (6, 7))):
        p += [[1000 * g, 0], [1000 * g + 10, 0], [1000 * g + w[0], w[1]]]
    return _case(p, None, 1, 20)


CIRCLES = [(0, 1, 100, 0), (0, 2, 50, 1), (1, 2, 50, 1),
           (3, 5, 41, 1), (4, 5, 41, 1),
           (6, 7, 100, 1), (6, 8, 100, 1), (7, 8, 80, 1),
           (9, 10, 100, 0), (9, 11, 85, 1), (10, 11, 65, 1)]


def radius():
    """r = 10: rows 0-1 have d2 = 100 = r * r (an edge), rows 2-3 are (r, 1) apart, d2 = 101 (none), rows 4-5 |dx| = |dy| = 9 <= r but
    d2 = 162 (none)."""
    return _case([[0, 0], [6, 8], [100, 0], [110, 1], [200, 0], [209, 9]], [0, 1, 0, 1, 0, 1], 2, 10)


RADIUS = [(0, 1, 100, 1)]


# ---- the lattice: closed form
def lattice(w=7, h=5, s=10, r=15, origin=(0, 0)):
    """w x h points at spacing s, row y * w + x; 2 s > r >= s * sqrt(2), so the sides and the diagonals of every cell are candidates and
    nothing longer is."""
    assert 4 * s * s > r * r >= 2 * s * s
    y, x = np.divmod(np.arange(w * h), w)
    return _case(np.stack([origin[0] + s * x, origin[1] + s * y], 1), (x + y) % 2, 2, r)


def lattice_expected(w=7, h=5, s=10):
    """Gabriel = the sides plus BOTH diagonals of every cell (the other two corners lie ON the circle), RNG = the sides only (the other two
    corners are nearer to both ends than the diagonal is long): w (h - 1) + h (w - 1) sides and 2 (w - 1)(h - 1) diagonals."""
    rows = []
    for y in range(h):
        for x in range(w):
            k = y * w + x
            if x < w - 1:
                rows.append((k, k + 1, s * s, 1))
            if y < h - 1:
                rows.append((k, k + w, s * s, 1))
            if x < w - 1 and y < h - 1:
                rows.append((k, k + w + 1, 2 * s * s, 0))
                rows.append((k + 1, k + w, 2 * s * s, 0))
    assert len(rows) == w * (h - 1) + h * (w - 1) + 2 * (w - 1) * (h - 1)
    return _expected(w * h, rows)


# ---- witnesses and pairs across cell borders
def borders():
    """r = 10, the box starts at (0, 0): cells are 10 wide.  Rows 0-1 pin the box.  Rows 2-4: (11, 15) and (3, 15) are a pair across a cell
    border, the witness (7, 15) between them sits in the SIDE cell.  Rows 5-7: (31, 31) and (25, 25), the witness (28, 28) in the CORNER
    cell.  Rows 8-10: (60, 20) and (69, 20), d2 81; (58, 20) is 4 from row 8 and 11 > r along x from row 9 -- outside its reach box, and
    it does not block.  Rows 11-13: (80, 45) and (89, 45) with the blocker (84, 44) in their own cell."""
    p = [[0, 0], [99, 59], [11, 15], [3, 15], [7, 15], [31, 31], [25, 25], [28, 28], [60, 20], [69, 20], [58, 20], [80, 45], [89, 45], [84, 44]]
    return _case(p, None, 1, 10)


def cell_boundaries_negative():
    """150 random points on [-40, 40]^2 with r = 10: the grid starts at a negative corner, cells are 10 wide, and every tenth point is
    moved onto a multiple of 10 from that corner -- the first coordinate of a cell -- with a partner one half pixel below it."""
    rng = np.random.default_rng(31)
    p = rng.integers(-40, 41, (150, 2))
    p[0] = [-40, -40]
    p[5::10] = (p[5::10] + 40) // 10 * 10 - 40
    p[6::10] = p[5::10] - 1
    p = np.clip(p, -40, 40)
    return _case(p, rng.integers(0, 3, 150), 3, 10)


# ---- the two label modes
def other_label_witness(by_class):
    """Rows 0-1 of label 0 at (0, 0) and (10, 0), row 2 of label 1 at their midpoint: it blocks under `any` and not under `class`.  Rows 3-5
    the same far away with the labels -1, -1 and 7 (outside 0..C-1: compared by plain equality)."""
    return _case([[0, 0], [10, 0], [5, 0], [500, 0], [510, 0], [505, 0]], [0, 0, 1, -1, -1, 7], 2, 12, by_class)


OTHER_LABEL = {0: [(0, 2, 25, 1), (1, 2, 25, 1), (3, 5, 25, 1), (4, 5, 25, 1)], 1: [(0, 1, 100, 1), (3, 4, 100, 1)]}


def labels_out_of_range(by_class):
    """C = 3 with labels -1, 7 and 1 on forty nearby points."""
    rng = np.random.default_rng(8)
    return _case(rng.integers(0, 14, (40, 2)), np.array([-1, 7, 1])[np.arange(40) % 3], 3, 7, by_class)


# ---- ties
def random_ties(by_class=0, n=300, side=12, r=4):
    """n points on a side x side lattice of half pixels: many coincident points, right angles and equal distances."""
    rng = np.random.default_rng(12)
    return _case(rng.integers(0, side, (n, 2)), rng.integers(-1, 4, n), 3, r, by_class)


def random_small(by_class):
    rng = np.random.default_rng(77)
    return _case(rng.integers(0, 90, (160, 2)), rng.integers(-1, 4, 160), 3, 14, by_class)


def small_cases():
    return dict(circles=circles(), radius=radius(), lattice=lattice(), lattice_3x2=lattice(3, 2, 5, 8, (-17, 9)), borders=borders(),
                cell_boundaries_negative=cell_boundaries_negative(), other_label_any=other_label_witness(0), other_label_class=other_label_witness(1),
                out_of_range_any=labels_out_of_range(0), out_of_range_class=labels_out_of_range(1), ties_any=random_ties(0, 120, 8, 4),
                ties_class=random_ties(1, 120, 8, 4), random_any=random_small(0), random_class=random_small(1),
                one_point=_case([[123456, -7890]], [2], 3, 8), two_points=_case([[0, 0], [3, 4]], [0, 1], 2, 5),
                two_points_apart=_case([[0, 0], [3, 5]], [0, 1], 2, 5), two_coincident=_case([[4, 4], [4, 4]], [0, 1], 2, 1),
                radius_one=_case([[0, 0], [1, 0], [1, 1], [3, 1]], None, 1, 1), short_chain_shuffled=chain('shuffled', 40),
                crowded_small=crowded(70))


def translate(case, dx, dy):
    return (case[0] + np.array([dx, dy], np.int32),) + case[1:]


# ---- device-sized, with closed forms
def coincident(n=300):
    """n coincident points (a clique of n (n - 1) / 2 edges of d2 = 0, all RNG: more than the first call has room for) and five others."""
    p = [[5000, 5000]] * n + [[5000 + 3 * k, 4990 + 5 * k] for k in range(5)]
    return _case(p, np.arange(n + 5) % 3, 3, 16)


def chain(order, n=20000, r=16):
    """n points r / 2 apart on a line, wherever `order` ('ascending', 'descending', 'shuffled') puts the rows: the links between
    neighbouring places are the edges (d2 = r * r / 4, RNG); places two apart are candidates (d2 = r * r) that the place between them
    blocks in both graphs."""
    k = dict(ascending=np.arange(n), descending=np.arange(n)[::-1], shuffled=np.random.default_rng(3).permutation(n))[order]
    return _case(np.stack([k * (r // 2) - 7, np.full(n, 11)], 1), k % 2, 2, r)


def chain_expected(case):
    p, r = case[0], case[3]
    at = np.argsort((p[:, 0] + 7) // (r // 2))              # the row at every place
    e = np.sort(np.stack([at[:-1], at[1:]], 1), 1)
    n = len(p)
    return _from_arrays(n, e[:, 0], e[:, 1], np.full(n - 1, r * r // 4), np.ones(n - 1, bool))


def crowded(n=1500, s=2, r=3):
    """n points thrown on the 3 x 3 lattice at spacing s (2 s > r >= s * sqrt(2)), all in one or two cells: about n / 9 coincident points
    per site, a cell fuller than a workgroup, and hundreds of thousands of edges."""
    rng = np.random.default_rng(15)
    site = rng.integers(0, 9, n)
    return _case(np.stack([s * (site % 3) + 100, s * (site // 3) - 50], 1), rng.integers(0, 3, n), 3, r)


def crowded_expected(case, s=2):
    """The lattice's closed form with repeats: two rows are joined when they share a site (d2 = 0, RNG), sit on the two ends of a side
    (s * s, RNG) or of a diagonal (2 s * s, Gabriel only) -- the repeats of an end never block, every other site blocks as on the lattice."""
    p = case[0].astype(np.int64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(2)
    i, j = np.nonzero(np.triu(d2 <= 2 * s * s, 1))
    return _from_arrays(len(p), i, j, d2[i, j], d2[i, j] <= s * s)


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
