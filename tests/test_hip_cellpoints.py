"""GPU tests of what the three per-slide point analyses share (nuhtc_amd/cellpoints.py; csrc/cellbin.h: the binning, the 3 x 3 sweep, the
scan, the epilogue): the cell graph, the spatial statistics and the clusters of ONE point set agree with each other where their definitions
overlap, each equals its own brute-force reference, and the clusters' root numbering is right where the roots lie in more than one chunk
of the scan.  And the loop that runs all six for the slide path (nuhtc_amd/slidepoints.py) on one hand-placed set of boxes."""
import argparse
import os

import numpy as np
import pytest

from nuhtc_amd import cellgraph as cg
from nuhtc_amd import clusters as cl
from nuhtc_amd import density, mst, proximity, slidepoints
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


def _placed_boxes():
    """60 boxes of 6 x 4 px, 5 classes: 56 on a jittered 8 x 7 lattice of 9 px whose centres fall on whole and half pixels, two with the centre
    (120, 40) and one label, and two of one label exactly 10 px apart -- (200, 100) and (206, 108) -- away from the rest."""
    at = np.arange(56)
    cx = np.concatenate([20 + 9.0 * (at % 8) + (at * 7 % 5) * 0.5, [120, 120, 200, 206]])
    cy = np.concatenate([15 + 9.0 * (at // 8) + (at * 3 % 4) * 0.5, [40, 40, 100, 108]])
    lab = np.concatenate([(at // 8 + (at % 8 >= 5)) % 5, [1, 1, 2, 2]]).astype(np.int64)     # runs along the rows: `class` mode keeps edges
    return np.stack([cx - 3, cy - 2, cx + 3, cy + 2], 1), lab


def test_the_loop_of_the_slide_path_runs_all_six_on_one_set_of_boxes(hip_device, tmp_path):
    """slidepoints.run, as tools/infer_wsi.py calls it, with every analysis selected at a radius of 10 px (not a default) and `class` mode
    where there is one: exactly the six files, one header, each file's integers equal to its module's reference on the file's own xy and
    label, the clauses in table order; and a selection of the last entry alone writes one file."""
    boxes, lab = _placed_boxes()
    rows = 2 * np.arange(len(lab), dtype=np.int64) + 1
    args = argparse.Namespace(nuclei_graph=True, graph_radius=10.0, graph_k=3, nuclei_spatial=True, spatial_step=2.5, spatial_bins=4,
                              nuclei_clusters=True, cluster_radius=10.0, cluster_min=2, cluster_by='class', nuclei_mst=True, mst_radius=10.0,
                              mst_by='class', nuclei_proximity=True, proximity_radius=10.0, proximity_by='class', nuclei_density=True,
                              density_bandwidth=10.0, density_pitch=7.5)
    chosen = slidepoints.select(args)
    assert [an for an, _ in chosen] == list(slidepoints.ANALYSES)
    all_dir, one_dir = tmp_path / 'all', tmp_path / 'one'
    os.makedirs(all_dir), os.makedirs(one_dir)
    said = slidepoints.run(chosen, rows, boxes, lab, 5, str(all_dir), 't', 0, dict(tiles_area_px=6 * 48.0 ** 2))
    assert sorted(os.listdir(all_dir)) == sorted('t' + an.suffix for an in slidepoints.ANALYSES)
    assert len(said) == 6 and all(clause.endswith(f' in t{an.suffix}') for clause, an in zip(said, slidepoints.ANALYSES)), said
    z = {an.module: slidepoints.module_of(an).read_npz(str(all_dir / ('t' + an.suffix))) for an in slidepoints.ANALYSES}
    xy = np.stack([(boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2], 1)
    for name, f in z.items():
        assert np.array_equal(f['nuclei_id'], rows) and np.array_equal(f['xy'], xy) and np.array_equal(f['label'], lab), name
        assert f['nuclei_id'].dtype == np.int64 and f['xy'].dtype == np.float64 and f['label'].dtype == np.int64, name
    p = np.rint(2 * xy).astype(np.int32)
    assert (p % 2 == 1).any() and np.array_equal(p[56], p[57]) and ((p[58] - p[59]) ** 2).sum() == 20 * 20      # the set is what it says

    def same(name, got, want):
        assert len(got) == len(want), name
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.asarray(g).dtype == np.asarray(w).dtype and np.array_equal(g, w), (name, i)
    nb, d2, cc = cg.graph_reference(p, lab, 5, 20, 3)
    same('graph', [z['cellgraph'][k] for k in ('neighbors', 'dist', 'class_count')], [nb, cg.distances_px(d2), cc])
    edges = sp.edges_from_step(2.5, 4)
    same('spatial', [z['spatial'][k] for k in ('pair_hist', 'nn_d2', 'class_n')], sp.spatial_reference(p, lab, 5, edges))
    assert float(z['spatial']['tiles_area_px']) == 6 * 48.0 ** 2 and z['spatial']['edges_px'].tolist() == [2.5, 5.0, 7.5, 10.0]
    same('clusters', [z['clusters'][k] for k in cl.INT_NAMES], cl.cluster_reference(p, lab, 5, 20, 2, 1))
    want = mst.mst_reference(p, lab, 5, 20, 1)
    same('mst', [z['mst'][k] for k in mst.INT_NAMES], want[:3])
    assert (int(z['mst']['n_edges']), int(z['mst']['n_trees'])) == want[3:]
    forest = {tuple(e): int(d) for e, d in zip(z['mst']['edges'].tolist(), z['mst']['edge_d2'].tolist())}
    assert forest[(56, 57)] == 0 and forest[(58, 59)] == 400                  # the coincident pair, and the pair AT the radius: inclusive
    want = proximity.proximity_reference(p, lab, 5, 20, 1)
    same('proximity', [z['proximity'][k] for k in proximity.INT_NAMES], want[:4])
    assert (int(z['proximity']['n_edges']), int(z['proximity']['n_rng'])) == want[4:]
    win = tuple(int(v) for v in z['density']['window'])
    assert win == density.window((int(p[:, 0].min()), int(p[:, 1].min()), int(p[:, 0].max()), int(p[:, 1].max())), 20, 15)
    same('density', [z['density'][k] for k in density.INT_NAMES], density.density_reference(p, lab, 5, 20, 15, win))
    assert len(z['clusters']['size']) > 1 and (z['clusters']['cluster'] < 0).any() and int(z['mst']['n_edges']) > 10 and int(z['proximity']['n_edges']) > 10
    assert int(z['clusters']['by_class']) == int(z['mst']['by_class']) == int(z['proximity']['by_class']) == 1
    last = slidepoints.run(chosen[-1:], rows, boxes, lab, 5, str(one_dir), 't', 0, dict(tiles_area_px=6 * 48.0 ** 2))
    assert os.listdir(one_dir) == ['t' + slidepoints.ANALYSES[-1].suffix] and last == said[-1:]
    assert open(one_dir / 't_nuclei_density.npz', 'rb').read() == open(all_dir / 't_nuclei_density.npz', 'rb').read()
