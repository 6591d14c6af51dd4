"""Designed owner maps for the territory adjacency (nuhtc_amd/adjacency.py), shared by tests/test_adjacency_host.py (the restatement against
edges written out by hand) and tests/test_hip_adjacency.py (the device against the restatement).  A map case is (owner int32 (H, W), n,
edges, shared): the expected edges as a list of (i, j) in ascending order with their shared, or None where only the restatement says.  The
cases from points are those of tests/territory_cases.py."""
import numpy as np

from nuhtc_amd import adjacency as adj

NAMES = adj.INT_NAMES + ('m',)


def equal(got, want, what):
    """edges, shared, degree and m: same dtype, same shape, same entries, same order."""
    assert len(got) == len(want) == len(NAMES), (what, len(got), len(want))
    for name, g, w in zip(NAMES[:3], got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, f'{len(bad)} entries differ, first at {bad[0].tolist()}', int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))
    assert int(got[3]) == int(want[3]) == len(want[0]), (what, 'm', got[3], want[3])


def _map(rows):
    return np.ascontiguousarray(np.asarray(rows, np.int32))


def smallest():
    """-> {name: case}: one site, two sites with two owners, two owners with a free column between them, nobody's, a diagonal meeting, and a
    row that appears in the map's range but owns nothing."""
    return {'one site': (_map([[0]]), 1, [], []),
            'two owners': (_map([[0, 1]]), 2, [(0, 1)], [1]),
            'two owners, one above the other': (_map([[1], [0]]), 2, [(0, 1)], [1]),
            'a free column between': (_map([[0, -1, 1], [0, -1, 1]]), 2, [], []),
            'nobody': (np.full((5, 7), -1, np.int32), 3, [], []),
            'a diagonal meeting': (_map([[0, -1], [-1, 1]]), 2, [], []),
            'four quadrants': (_map([[0, 0, 1, 1], [0, 0, 1, 1], [2, 2, 4, 4]]), 5, [(0, 1), (0, 2), (1, 4), (2, 4)], [2, 2, 2, 1])}


def checkerboard(k=17):
    """k x k sites of two owners in a checkerboard: EVERY site pair has the owners {0, 1}: one edge, shared 2 k (k - 1)."""
    y, x = np.divmod(np.arange(k * k), k)
    return _map(((x + y) % 2).reshape(k, k)), 2, [(0, 1)], [2 * k * (k - 1)]


def stripes(W=33, H=18):
    """W columns, each a territory of its own: W - 1 edges of shared H, across two tile columns and two tile rows."""
    return _map(np.tile(np.arange(W), (H, 1))), W, [(u, u + 1) for u in range(W - 1)], [H] * (W - 1)


def far_apart():
    """40 x 40 sites, nobody's but for rows 3 and 5, which meet in the first tile, in the last one, and once across a tile border: ONE edge,
    the records of three tiles merged."""
    own = np.full((40, 40), -1, np.int32)
    own[2, 2], own[2, 3] = 3, 5                            # tile (0, 0)
    own[35, 36], own[36, 36] = 5, 3                        # tile (2, 2), one above the other
    own[20, 15], own[20, 16] = 3, 5                        # across the border of tiles (0, 1) and (1, 1): the left tile's pair
    return own, 7, [(3, 5)], [3]


def long_row(descending=False, upright=False):
    """601 sites in a line: the hub between every two of 300 other rows, each of them its neighbour with shared 2 -- more neighbours than a
    workgroup has threads.  As given the hub is row 0 and the others 1 .. 300 (a segment of 300 to rank); `descending` renumbers row k as
    300 - k: the hub is the LARGER end of every edge, and the edges' output order is the reverse of the order of the sites."""
    line = np.zeros(601, np.int64)
    line[1::2] = np.arange(1, 301)
    if descending:
        line = 300 - line
    edges = [(k, 300) for k in range(300)] if descending else [(0, k) for k in range(1, 301)]
    return _map(line.reshape((601, 1) if upright else (1, 601))), 301, edges, [2] * 300


def random_map(W, H, n, seed=0, free=0.0):
    """Independent owners out of n per site (a share `free` of them nobody's): almost every site pair is an edge of its own."""
    rng = np.random.default_rng(seed)
    own = rng.integers(0, n, (H, W))
    own[rng.random((H, W)) < free] = -1
    return _map(own), n, None, None


def wide(W=70000, H=2, n=1000, seed=5):
    """A window of 4 375 tiles in x and one in y: runs of 1 .. 6 sites of one owner in either row."""
    rng = np.random.default_rng(seed)
    own = np.stack([np.repeat(rng.integers(-1, n, W), rng.integers(1, 7, W))[:W] for _ in range(H)])
    return _map(own), n, None, None


def as_arrays(case):
    """The hand-written expectation of a case in the reference's form."""
    own, n, edges, shared = case
    e = np.asarray(edges, np.int32).reshape(-1, 2)
    return e, np.asarray(shared, np.int32), np.bincount(e.reshape(-1), minlength=n).astype(np.int32), len(e)
