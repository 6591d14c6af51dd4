"""Designed point sets for the nucleus clusters (nuhtc_amd/clusters.py), shared by tests/test_clusters_host.py (the restatement against a
double loop) and tests/test_hip_clusters.py (the device against the restatement).  A case is (points int (n, 2) half pixels, labels (n,),
num_classes, r half pixels, min_pts, by_class).  `small_cases` are few enough points for a Python double loop; the others are sized to
what can go wrong on the device only (deep parent trees, a cell fuller than a workgroup, several blocks of threads)."""
import numpy as np


def _case(p, lab, C, r, min_pts, by_class=0):
    p = np.asarray(p, np.int32).reshape(-1, 2)
    lab = np.zeros(len(p), np.int32) if lab is None else np.asarray(lab, np.int32).reshape(-1)
    assert len(lab) == len(p)
    return p, lab, C, r, min_pts, by_class


def edge_pairs():
    """r = 10: (0, 0) - (6, 8) has d2 = 100 = r * r (adjacent), (100, 0) - (106, 9) has d2 = 117 (not).  min_pts 2."""
    return _case([[0, 0], [6, 8], [100, 0], [106, 9]], [0, 1, 0, 1], 2, 10, 2)


def one_above_the_radius():
    """r = 10: (0, 0) - (10, 1) has d2 = 101 = r * r + 1 (not adjacent), (100, 0) - (100, 10) has d2 = r * r (adjacent).  min_pts 2."""
    return _case([[0, 0], [10, 1], [100, 0], [100, 10]], [0, 1, 0, 1], 2, 10, 2)


def min_pts_threshold():
    """min_pts 4, r 10, three stars whose arms are 10 from the centre and more than 10 from each other: a centre with 2 others (degree 3:
    one below), with 3 others (degree 4: at the threshold, core, its arms border points) and with 4 others (degree 5)."""
    star = lambda cx, arms: [[cx, 0]] + [[cx + 10, 0], [cx, 10], [cx - 10, 0], [cx, -10]][:arms]
    return _case(star(0, 2) + star(1000, 3) + star(2000, 4), None, 1, 10, 4)


def _two_blobs_and_a_bridge(bridge, r, order):
    """Two clusters of five core points each -- one point at (0, 0) with four at (-5, 0), one at (20, 0) with four at (25, 0) -- and one
    point between them that reaches only (0, 0) and (20, 0): degree 3 < min_pts 5, a border point of both and a bridge of neither."""
    p = np.array([[0, 0]] + [[-5, 0]] * 4 + [[20, 0]] + [[25, 0]] * 4 + [bridge])
    return _case(p[order], (np.arange(11) % 3)[order], 3, r, 5)


def bridge_equidistant():
    """The bridge (10, 0) is 10 from (0, 0) and from (20, 0).  Rows: (20, 0) is row 1, (0, 0) is row 2, and row 0 belongs to the left blob:
    the bridge goes to the smaller INDEX, row 1, which is in the cluster with the LARGER number."""
    return _two_blobs_and_a_bridge([10, 0], 10, [1, 5, 0, 2, 3, 4, 6, 7, 8, 9, 10])


def bridge_nearer_later():
    """The bridge (11, 0) with r = 11: d2 = 121 to (0, 0), row 0, and 81 to (20, 0), row 5: it goes to the nearer one, in the later cluster."""
    return _two_blobs_and_a_bridge([11, 0], 11, np.arange(11))


def cell_boundaries_negative():
    """150 random points on [-40, 40]^2 with r = 10: the grid starts at a negative corner, cells are 10 wide, and every fifth point is
    moved onto a multiple of 10 from that corner -- the first coordinate of a cell -- with a partner one half pixel below it."""
    rng = np.random.default_rng(31)
    p = rng.integers(-40, 41, (150, 2))
    p[0] = [-40, -40]
    p[5::10] = (p[5::10] + 40) // 10 * 10 - 40
    p[6::10] = p[5::10] - 1
    p = np.clip(p, -40, 40)
    return _case(p, rng.integers(0, 3, 150), 3, 10, 4)


def interleaved_classes(by_class):
    """Ten positions 4 apart, a class-0 and a class-1 point on each; r 5, min_pts 3.  `class`: two clusters (the ends are border points);
    `any`: one."""
    p = np.repeat(np.stack([np.arange(10) * 4, np.zeros(10, int)], 1), 2, 0)
    return _case(p, np.arange(20) % 2, 2, 5, 3, by_class)


def labels_out_of_range(by_class):
    """C = 3 with labels -1, 7 and 1 on three nearby groups: in `class` mode each label clusters among its equals; -1 and 7 are counted in
    no class column."""
    rng = np.random.default_rng(8)
    p = rng.integers(0, 12, (30, 2))
    return _case(p, np.array([-1, 7, 1])[np.arange(30) % 3], 3, 6, 3, by_class)


def random_small(by_class):
    rng = np.random.default_rng(77)
    return _case(rng.integers(0, 200, (220, 2)), rng.integers(-1, 4, 220), 3, 12, 4, by_class)


def small_cases():
    one = _case([[123456, -7890]], [2], 3, 8, 1)
    return dict(edge_pairs=edge_pairs(), one_above_the_radius=one_above_the_radius(), min_pts_threshold=min_pts_threshold(), bridge_equidistant=bridge_equidistant(),
                bridge_nearer_later=bridge_nearer_later(), cell_boundaries_negative=cell_boundaries_negative(),
                interleaved_any=interleaved_classes(0), interleaved_class=interleaved_classes(1),
                out_of_range_any=labels_out_of_range(0), out_of_range_class=labels_out_of_range(1),
                random_any=random_small(0), random_class=random_small(1),
                one_point=one, one_point_alone_is_noise=one[:4] + (2, 0),
                two_points=_case([[0, 0], [3, 4]], [0, 1], 2, 5, 2), two_points_apart=_case([[0, 0], [3, 5]], [0, 1], 2, 5, 2),
                min_pts_above_n=random_small(0)[:4] + (221, 0), components=random_small(0)[:4] + (1, 0))


def translate(case, dx, dy):
    return (case[0] + np.array([dx, dy], np.int32),) + case[1:]


# ---- device-sized
def chain(order, n=20000, r=16):
    """n points r apart on a line: every link has d2 = r * r exactly, min_pts 2 makes every point a core point, and the whole line is one
    cluster whose root is row 0 wherever `order` ('ascending', 'descending', 'shuffled') puts it."""
    k = dict(ascending=np.arange(n), descending=np.arange(n)[::-1], shuffled=np.random.default_rng(3).permutation(n))[order]
    return _case(np.stack([k * r - 7, np.full(n, 11)], 1), k % 2, 2, r, 2)


def crowded_cell():
    """3000 coincident points -- more than any workgroup has threads -- with 40 others in the cells around, none within r = 50 of the
    pile: every point of the pile has degree 3000 = min_pts exactly."""
    rng = np.random.default_rng(12)
    ang = rng.uniform(0, 2 * np.pi, 40)
    rad = rng.integers(52, 120, 40)
    others = np.rint(np.stack([5000 + rad * np.cos(ang), 5000 + rad * np.sin(ang)], 1)).astype(np.int64)
    p = np.concatenate([np.full((3000, 2), 5000), others])
    order = rng.permutation(len(p))
    return _case(p[order], rng.integers(0, 3, len(p))[order], 3, 50, 3000)


def random_large(kind, r, min_pts, by_class=0, n=5000):
    """5000 points, 20 blocks of threads: uniform on a square, or in 12 Gaussian clumps on the same square."""
    rng = np.random.default_rng(2025)
    if kind == 'uniform':
        p = rng.integers(0, 3000, (n, 2))
    else:
        centre = rng.uniform(0, 3000, (12, 2))
        p = np.clip(np.rint(centre[rng.integers(0, 12, n)] + rng.normal(0, 90, (n, 2))), 0, 2999)
    return _case(p, rng.integers(-1, 5, n), 4, r, min_pts, by_class)
