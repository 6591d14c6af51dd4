"""Designed point sets for the minimum spanning forest (nuhtc_amd/mst.py), shared by tests/test_mst_host.py (the restatement against Prim,
scipy and hand-written forests) and tests/test_hip_mst.py (the device against the restatement).  A case is (points int (n, 2) half pixels,
labels (n,), num_classes, r half pixels, by_class).  `small_cases` are few enough points for a Python double loop; the others are sized to
what can go wrong on the device only (a union 20000 deep, rows over two scan chunks, a cell fuller than a workgroup, ten rounds)."""
import numpy as np


def _case(p, lab, C, r, by_class=0):
    p = np.asarray(p, np.int32).reshape(-1, 2)
    lab = np.zeros(len(p), np.int32) if lab is None else np.asarray(lab, np.int32).reshape(-1)
    assert len(lab) == len(p)
    return p, lab, C, r, by_class


def edge_pairs():
    """r = 10: rows 0-1 have d2 = 100 = r * r (joined), rows 2-3 d2 = 101 (not), rows 4-5 |dx| = |dy| = 9 <= r but d2 = 162 (not)."""
    return _case([[0, 0], [6, 8], [100, 0], [110, 1], [200, 0], [209, 9]], [0, 1, 0, 1, 0, 1], 2, 10)


def lattice():
    """The 8 x 8 lattice at spacing 3 with r = 3: every edge has d2 = 9, so the tie-break (i, j) alone decides the forest."""
    y, x = np.divmod(np.arange(64), 8)
    return _case(np.stack([3 * x, 3 * y], 1), np.arange(64) % 3, 3, 3)


def equidistant():
    """r = 5.  Rows 0..2: row 0 between rows 1 and 2, both 5 away and 10 from each other -- two edges that share (d2, lo) and differ in hi.
    Rows 3..5, far away, the mirror image in the key: row 5 between rows 3 and 4 -- two edges that share (d2, hi) and differ in lo."""
    return _case([[0, 0], [5, 0], [-5, 0], [1005, 0], [995, 0], [1000, 0]], None, 1, 5)


EQUIDISTANT_FOREST = ([[0, 1], [0, 2], [3, 5], [4, 5]], [25, 25, 25, 25], [0, 0, 0, 1, 1, 1])


def collinear():
    """Three points with gaps 2 and 3, r = 3: rows 0 and 1 pick each other (a mutual pick), row 2 picks (1, 2) alone -- in one round."""
    return _case([[0, 0], [2, 0], [5, 0]], None, 1, 3)


COLLINEAR_FOREST = ([[0, 1], [1, 2]], [4, 9], [0, 0, 0])


def coincident(n=300):
    """n coincident points (rows 0 .. n - 1: a cell fuller than a workgroup, and a star of d2 = 0 edges on row 0) and five others around."""
    p = [[5000, 5000]] * n + [[5000 + 3 * k, 4990 + 5 * k] for k in range(5)]
    return _case(p, np.arange(n + 5) % 3, 3, 16)


def groups():
    """r = 5: rows 0..2 a right triangle 3-4-5, rows 3-4 a pair at d2 = 25, row 5 alone: T = 3, the last a tree of size 1."""
    return _case([[0, 0], [3, 0], [3, 4], [100, 0], [100, 5], [50, 50]], None, 1, 5)


GROUPS_FOREST = ([[0, 1], [1, 2], [3, 4]], [9, 16, 25], [0, 0, 0, 1, 1, 2])


def interleaved_classes(by_class):
    """Ten positions 4 apart, a class-0 and a class-1 point on each; r 5.  `any`: one tree, the coincident pairs joined at d2 = 0;
    `class`: two trees of nine d2 = 16 edges each."""
    p = np.repeat(np.stack([np.arange(10) * 4, np.zeros(10, int)], 1), 2, 0)
    return _case(p, np.arange(20) % 2, 2, 5, by_class)


def ruler(n=1024):
    """n points on a line, rows in line order, the gap between places k - 1 and k being 2 + (the number of times 2 divides k); r = the
    largest gap.  Every round joins the components in pairs: exactly log2 n rounds (n a power of two)."""
    k = np.arange(1, n)
    gap = 2 + np.array([(int(v) & -int(v)).bit_length() - 1 for v in k])
    x = np.concatenate([[0], np.cumsum(gap)])
    return _case(np.stack([x - 300, np.full(n, 7)], 1), np.arange(n) % 2, 2, int(gap.max()))


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


def labels_out_of_range(by_class):
    """C = 3 with labels -1, 7 and 1 on thirty nearby points: in `class` mode each label is joined among its equals only."""
    rng = np.random.default_rng(8)
    return _case(rng.integers(0, 12, (30, 2)), np.array([-1, 7, 1])[np.arange(30) % 3], 3, 6, by_class)


def random_small(by_class):
    rng = np.random.default_rng(77)
    return _case(rng.integers(0, 120, (220, 2)), rng.integers(-1, 4, 220), 3, 12, by_class)


def small_cases():
    return dict(edge_pairs=edge_pairs(), lattice=lattice(), equidistant=equidistant(), collinear=collinear(), coincident=coincident(),
                groups=groups(), interleaved_any=interleaved_classes(0), interleaved_class=interleaved_classes(1), ruler_256=ruler(256),
                cell_boundaries_negative=cell_boundaries_negative(), out_of_range_any=labels_out_of_range(0),
                out_of_range_class=labels_out_of_range(1), random_any=random_small(0), random_class=random_small(1),
                one_point=_case([[123456, -7890]], [2], 3, 8), two_points=_case([[0, 0], [3, 4]], [0, 1], 2, 5),
                two_points_apart=_case([[0, 0], [3, 5]], [0, 1], 2, 5), radius_one=_case([[0, 0], [1, 0], [1, 1], [3, 1]], None, 1, 1),
                short_chain_shuffled=chain('shuffled', 40))


def translate(case, dx, dy):
    return (case[0] + np.array([dx, dy], np.int32),) + case[1:]


# ---- device-sized
def chain(order, n=20000, r=16):
    """n points r apart on a line: every link has d2 = r * r exactly and the whole line is one tree, wherever `order` ('ascending',
    'descending', 'shuffled') puts the rows.  In ascending order every point but the first picks the link behind it: one round, and a
    union n deep."""
    k = dict(ascending=np.arange(n), descending=np.arange(n)[::-1], shuffled=np.random.default_rng(3).permutation(n))[order]
    return _case(np.stack([k * r - 7, np.full(n, 11)], 1), k % 2, 2, r)


def chain_forest(case):
    """The forest of a `chain` case in closed form, from the place of every row along the line: the links between neighbouring places."""
    p, r = case[0], case[3]
    at = np.argsort((p[:, 0] + 7) // r)                     # the row at every place
    e = np.sort(np.stack([at[:-1], at[1:]], 1), 1)
    e = e[np.lexsort((e[:, 1], e[:, 0]))]
    n = len(p)
    return e.astype(np.int32), np.full(n - 1, r * r, np.int32), np.zeros(n, np.int32), n - 1, 1


def random_large(kind, r, by_class=0, n=3000):
    """3000 points on small integer coordinates (many equal distances), 12 blocks of threads: uniform on a square of 400, or in 12
    Gaussian clumps on the same square (many coincident points)."""
    rng = np.random.default_rng(2026)
    if kind == 'uniform':
        p = rng.integers(0, 400, (n, 2))
    else:
        centre = rng.uniform(0, 400, (12, 2))
        p = np.clip(np.rint(centre[rng.integers(0, 12, n)] + rng.normal(0, 25, (n, 2))), 0, 399)
    return _case(p, rng.integers(-1, 5, n), 4, r, by_class)
