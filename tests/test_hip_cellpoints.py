"""GPU tests of what the three per-slide point analyses share (nuhtc_amd/cellpoints.py; csrc/cellbin.h: the binning, the 3 x 3 sweep, the
scan, the epilogue): the cell graph, the spatial statistics and the clusters of ONE point set agree with each other where their definitions
overlap, each equals its own brute-force reference, and the clusters' root numbering is right where the roots lie in more than one chunk
of the scan."""
import numpy as np
import pytest

from nuhtc_amd import cellgraph as cg
from nuhtc_amd import clusters as cl
from nuhtc_amd import spatial as sp

pytestmark = pytest.mark.gpu

N, C, R, K, MIN_PTS, SEED = 600, 4, 24, 4, 10, 0          # R in half pixels: 17 x 13 cells of side R, three blocks of 256 threads


@pytest.fixture(scope='module')
def one_set():
    """About 600 points on a 400 x 300 half-pixel window, labels 0..3 with six at -1 and six at 9, and the three references on the CPU."""
    rng = np.random.default_rng(SEED)
    p = np.stack([rng.integers(0, 400, N), rng.integers(0, 300, N)], 1).astype(np.int32)
    lab = rng.integers(0, C, N).astype(np.int32)
    odd = rng.choice(N, 12, replace=False)
    lab[odd[:6]], lab[odd[6:]] = -1, 9
    ref = dict(graph=cg.graph_reference(p, lab, C, R, K), spatial=sp.spatial_reference(p, lab, C, [R]),
               clusters=cl.cluster_reference(p, lab, C, R, MIN_PTS, 0))
    d = p.astype(np.int64)[:, None, :] - p.astype(np.int64)[None, :, :]
    near = (d * d).sum(-1) <= R * R
    np.fill_diagonal(near, False)
    unknown = (lab < 0) | (lab >= C)
    return p, lab, ref, (near & unknown[None, :]).sum(1)                       # the last: the neighbours no class counts


def test_the_three_analyses_agree_on_one_set(hip_device, one_set):
    p, lab, ref, unknown_near = one_set
    nb, d2, cc = ref['graph']
    cluster, core = ref['clusters'][0], ref['clusters'][1].astype(bool)
    # the set is not degenerate: clusters, noise and border points, an empty neighbour list and a full one, out-of-range neighbours
    assert len(ref['clusters'][3]) > 1 and (cluster < 0).any() and ((cluster >= 0) & ~core).any() and core.any()
    assert (nb[:, 0] < 0).any() and (nb[:, K - 1] >= 0).any() and 0 < (unknown_near > 0).sum() < N
    assert (p.max(0) - p.min(0)).min() // R >= 3 and N > 2 * 256
    graph = cg.build(p, lab, C, R / 2, K)
    spatial = sp.build(p, lab, C, [R])
    clusters = cl.build(p, lab, C, R / 2, MIN_PTS, 0)
    for name, got in (('graph', graph), ('spatial', spatial), ('clusters', clusters)):
        assert len(got) == len(ref[name])
        for i, (g, w) in enumerate(zip(got, ref[name])):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, i)
    deg = graph[2].sum(1) + unknown_near                                       # every neighbour within the radius, whatever its label
    assert np.array_equal(clusters[2], deg + 1)                                # the clusters' degree counts the point itself
    # the nearest neighbour, from the nearest of every class: the same d2 wherever every neighbour is of some class; with a neighbour of
    # no class the graph's nearest can only be nearer
    nn = spatial[1].astype(np.int64)
    nearest = np.where(nn >= 0, nn, np.iinfo(np.int64).max).min(1)
    nearest = np.where((nn >= 0).any(1), nearest, -1)
    clean = unknown_near == 0
    assert clean.sum() > N // 2 and np.array_equal(nearest[clean], graph[1][clean, 0])
    assert (graph[1][~clean, 0] >= 0).all() and (graph[1][~clean, 0] <= np.where(nearest[~clean] >= 0, nearest[~clean], R * R)).all()
    assert np.array_equal(spatial[0].sum(2), _pairs_by_class(graph[2], lab))   # bin 0 of edges = [r] is the graph's disc, summed by class


def _pairs_by_class(class_count, lab):
    out = np.zeros((C, C), np.int64)
    for a in range(C):
        out[a] = class_count[lab == a].sum(0)
    return out


def test_the_root_numbering_crosses_scan_chunks(hip_device):
    """n = 2 * 16384 + 3 points on a lattice of spacing 3 r, rows shuffled, min_pts = 1: every point is a core point and its own cluster,
    so cluster i is row i and the roots lie in three chunks of the scan (tests/test_clusters_host.py pins on 40 points that the definition
    says so).  The expected values follow from the definition: no O(n^2) reference."""
    n, r = 2 * 16384 + 3, 8
    at = np.arange(n)
    p = (np.stack([at % 200, at // 200], 1) * 3 * r - 1000).astype(np.int32)
    p = p[np.random.default_rng(5).permutation(n)]
    lab = (np.arange(n) % 3).astype(np.int32)
    cluster, core, degree, size, n_core, class_count, sum_xy, bbox = cl.build(p, lab, 3, r / 2, 1, 0)
    assert len(size) == n
    assert np.array_equal(cluster, np.arange(n)) and core.all() and (degree == 1).all()
    assert (size == 1).all() and (n_core == 1).all() and np.array_equal(class_count, np.eye(3, dtype=np.int32)[lab])
    assert np.array_equal(sum_xy, p.astype(np.int64)) and np.array_equal(bbox, np.concatenate([p, p], 1))
