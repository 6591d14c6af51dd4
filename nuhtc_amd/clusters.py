"""Nucleus clusters of a slide: which nuclei belong together (tumour nests, lymphocyte aggregates), how many nuclei each group holds and
of which classes, and which nuclei are isolated -- DBSCAN over the nodes the slide path already writes, with one rule added so that the
result is a pure function of the input.  Computed on the GPU (csrc/cellcluster.hip, `nuhtc_cell_clusters`); tools/infer_wsi.py
--nuclei-clusters writes it as <id>_nuclei_clusters.npz.  Not in the reference.

Definition.

Inputs.  n points in HALF pixels, int32 (n, 2), from `cellgraph.quantize_centres`, with |p| < 2**27 and n <= 2**24; labels, int32, one per
point; C classes, 1 <= C <= 14; a radius r in half pixels, an integer with 1 <= r <= 16384; min_pts >= 1; by_class in {0, 1}.  All geometry
is integer arithmetic.

Rules.
  * adj(i, j) holds when dx * dx + dy * dy <= r * r.  The radius is inclusive.  With by_class, adj also requires labels[i] == labels[j]:
    plain equality, the same for labels outside 0..C-1.  adj(i, i) holds; coincident points are adjacent.
  * degree[i] is the number of j with adj(i, j).  It counts i itself (scikit-learn's convention for min_samples).
  * i is a CORE point when degree[i] >= min_pts.
  * Clusters are the connected components of adj restricted to core-core pairs.  The ROOT of a cluster is its smallest core row index.
  * A non-core point with at least one adjacent core point is a BORDER point.  It joins the cluster of the adjacent core point with the
    smallest key (d2, j).  DBSCAN proper leaves that choice to the visiting order; this rule does not, and a border point never joins two
    clusters (nor does it connect them).
  * Every other point is NOISE and gets cluster -1.
  * Clusters are numbered 0..m-1 by ascending root.

Outputs, integers only.
  per nucleus   cluster int32 (n,), core uint8 (n,), degree int32 (n,)
  per cluster   size int32 (m,), n_core int32 (m,), class_count int32 (m, C) (a label outside 0..C-1 is counted in no class),
                sum_xy int64 (m, 2) in half pixels, bbox int32 (m, 4): x_min, y_min, x_max, y_max in half pixels

`cluster_reference` is the brute-force int64 restatement (every pair, no grid): the oracle the device result must EQUAL.  The device bins
the points into the cell graph's grid (`cellgraph.cell_side`: the smallest multiple of r with at most 2**22 cells over the bounding box,
computed here on the host and passed in), finds degrees with one 3 x 3 sweep, unites adjacent core points in a lock-free union-find whose
parent never exceeds its child -- so the smallest row of a component is its root, with no relabelling pass -- and numbers the roots with a
scan.  `derive` makes the float64 side on the host: centroids and boxes in px, class fractions per cluster, and the slide's counts."""
import numpy as np

from . import cellpoints
from .cellgraph import cell_side  # noqa: F401 (the cell graph's grid, re-exported)
from .cellpoints import COORD_LIMIT, MAX_CLASSES, MAX_POINTS, MAX_R, centres, half_pixel_radius, quantize_centres  # noqa: F401 (re-exported)

MAX_MIN_PTS = (1 << 31) - 1
INT_NAMES = ('cluster', 'core', 'degree', 'size', 'n_core', 'class_count', 'sum_xy', 'bbox')
DERIVED_KEYS = ('centroid_px', 'bbox_px', 'class_fraction', 'n_clusters', 'n_noise', 'class_n', 'class_clustered', 'class_clustered_share')
NPZ_KEYS = ('nuclei_id', 'xy', 'label') + INT_NAMES + DERIVED_KEYS + ('radius_px', 'min_pts', 'by_class')
BY = {'any': 0, 'class': 1}


def check_args(num_classes, r, min_pts, by_class):
    """num_classes 1..14, r 1..16384 half pixels, min_pts >= 1, by_class 0 or 1: ValueError otherwise."""
    whole = all(float(v) == int(v) for v in (num_classes, r, min_pts, by_class))
    if not (whole and 1 <= int(num_classes) <= MAX_CLASSES and 1 <= int(r) <= MAX_R and 1 <= int(min_pts) <= MAX_MIN_PTS and int(by_class) in (0, 1)):
        raise ValueError(f'clusters: num_classes 1..{MAX_CLASSES}, r 1..{MAX_R} half pixels, min_pts >= 1, by_class 0 or 1 '
                         f'(got num_classes={num_classes}, r={r}, min_pts={min_pts}, by_class={by_class})')


def _tables(p, lab, C, cluster, core, m):
    """The per-cluster integers of an assignment: p int64 (n, 2), cluster int (n,) with -1 for noise."""
    inside = cluster >= 0
    c, q = cluster[inside], p[inside]
    size = np.bincount(c, minlength=m).astype(np.int32)
    n_core = np.bincount(cluster[inside & core], minlength=m)
    class_count = np.zeros((m, C), np.int32)
    known = inside & (lab >= 0) & (lab < C)
    np.add.at(class_count, (cluster[known], lab[known]), 1)
    sum_xy = np.zeros((m, 2), np.int64)
    np.add.at(sum_xy, c, q)
    bbox = np.empty((m, 4), np.int64)
    bbox[:, :2], bbox[:, 2:] = np.iinfo(np.int64).max, np.iinfo(np.int64).min
    np.minimum.at(bbox[:, 0], c, q[:, 0]); np.minimum.at(bbox[:, 1], c, q[:, 1])
    np.maximum.at(bbox[:, 2], c, q[:, 0]); np.maximum.at(bbox[:, 3], c, q[:, 1])
    return size, n_core.astype(np.int32), class_count, sum_xy, bbox.astype(np.int32)


def cluster_reference(points, labels, num_classes, r, min_pts, by_class):
    """The definition, pair by pair in int64: points int (n, 2) half pixels, labels int (n,), r in HALF pixels ->
    (cluster int32 (n,), core uint8 (n,), degree int32 (n,), size int32 (m,), n_core int32 (m,), class_count int32 (m, C),
    sum_xy int64 (m, 2), bbox int32 (m, 4)).  O(n^2) time, rows in blocks of 256, and memory for the list of ALL adjacent ordered pairs
    (24 bytes each): meant for a few thousand points, or more where few are adjacent.  The components come from that list by repeated
    minimum over the core-core pairs and pointer jumping, with no grid and no tree."""
    check_args(num_classes, r, min_pts, by_class)
    p, lab = cellpoints.reference_points(points, labels, 'cluster_reference')
    n, C, r, min_pts, by_class = len(p), int(num_classes), int(r), int(min_pts), int(by_class)
    idx = np.arange(n, dtype=np.int64)
    none = np.iinfo(np.int64).max
    degree = np.zeros(n, np.int64)
    ii, jj, dd = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]      # every adjacent ordered pair and its d2
    for rows, d2 in cellpoints.pair_blocks(p, 256):
        adj = d2 <= r * r
        if by_class:
            adj &= lab[rows, None] == lab[None, :]
        degree[rows] = adj.sum(axis=1)                                       # i itself is among them
        i, j = np.nonzero(adj)
        ii.append(rows[i]); jj.append(j); dd.append(d2[i, j])
    ii, jj, dd = np.concatenate(ii), np.concatenate(jj), np.concatenate(dd)
    core = degree >= min_pts
    to_core = core[jj] if n else np.zeros(0, bool)
    nearest = np.full(n, none, np.int64)                                     # the least (d2, j) over the adjacent core points j
    np.minimum.at(nearest, ii[to_core], (dd[to_core] << 32) | jj[to_core])
    both = to_core & core[ii] if n else to_core
    pairs = np.stack([ii[both], jj[both]], 1)
    root = idx.copy()                                                        # of core points: the smallest core row of the component
    while True:
        new = root.copy()
        np.minimum.at(new, pairs[:, 0], root[pairs[:, 1]])
        np.minimum.at(new, root[pairs[:, 0]], root[pairs[:, 1]])
        while True:
            hop = new[new]
            if np.array_equal(hop, new):
                break
            new = hop
        if np.array_equal(new, root):
            break
        root = new
    border = ~core & (nearest != none)
    root = np.where(core, root, np.where(border, root[np.where(border, nearest & 0xffffffff, 0)], -1))
    roots = np.unique(root[root >= 0])                                       # ascending: the numbering
    cluster = np.where(root >= 0, np.searchsorted(roots, np.maximum(root, 0)), -1)
    return (cluster.astype(np.int32), core.astype(np.uint8), degree.astype(np.int32)) + _tables(p, lab, C, cluster, core, len(roots))


def call(points, labels, num_classes, r, min_pts, by_class, cluster, core, degree, size, n_core, class_count, sum_xy, bbox, bounds=None, device=0):
    """nuhtc_cell_clusters on torch tensors of cuda:`device` (points, labels, cluster, degree, size, n_core, class_count, bbox int32; core
    uint8; sum_xy int64; contiguous; the per-cluster tensors with n rows; r in HALF pixels) -> (the library's return code, m), nothing
    raised: the code is 0 or hip.E_INVALID / hip.E_HIP, m the number of clusters (None unless the code is 0).  bounds = (x_min, y_min,
    x_max, y_max) of the points, computed on the host when not given."""
    import ctypes
    m = ctypes.c_int64(-1)
    rc = cellpoints.launch('nuhtc_cell_clusters', device, points, labels, (int(num_classes), int(r), int(min_pts), int(by_class)),
                           (cluster, core, degree, size, n_core, class_count, sum_xy, bbox), bounds, extra=(ctypes.byref(m),))
    return rc, (int(m.value) if rc == 0 else None)


def outputs(n, num_classes, device, fill=0):
    """The eight output tensors of `call` for n points on `device`, every entry `fill`."""
    import torch
    i32 = torch.int32
    shapes = (((n,), i32), ((n,), torch.uint8), ((n,), i32), ((n,), i32), ((n,), i32), ((n, int(num_classes)), i32), ((n, 2), torch.int64), ((n, 4), i32))
    return [torch.full(s, fill, dtype=d, device=device) for s, d in shapes]


def build(points, labels, num_classes, radius_px, min_pts, by_class=0, device=0):
    """The clusters of `points` (int (n, 2) half pixels, see cellpoints.quantize_centres) with `labels` (n,) on cuda:`device`: numpy in,
    the eight arrays of `cluster_reference` out (the per-cluster ones cut to their m rows).  There is no host route: without the library or
    a GPU this raises."""
    C, r = int(num_classes), half_pixel_radius(radius_px)
    check_args(C, r, min_pts, by_class)
    p, lab, dev, p_d, lab_d, bounds = cellpoints.resident(points, labels, 'clusters', device)
    n = len(p)
    out = outputs(n, C, dev)
    rc, m = call(p_d, lab_d, C, r, int(min_pts), int(by_class), *out, bounds=bounds, device=device)
    cellpoints.raise_for(rc, 'nuhtc_cell_clusters')
    return tuple(t.cpu().numpy() for t in out[:3]) + tuple(t[:m].cpu().numpy() for t in out[3:])


def derive(cluster, labels, num_classes, size, class_count, sum_xy, bbox):
    """The float64 side of the integers -> dict:
      centroid_px    float64 (m, 2)  sum_xy / (2 size): the mean centre of the cluster's nuclei in px
      bbox_px        float64 (m, 4)  bbox / 2
      class_fraction float64 (m, C)  class_count / size (the rows sum to less than 1 where labels lie outside 0..C-1)
      n_clusters, n_noise            int64 0-d: m, and the nuclei with cluster -1
      class_n, class_clustered       int64 (C,): the nuclei of each class, and those of them that lie in some cluster
      class_clustered_share          float64 (C,): class_clustered / class_n; 0, never NaN, for a class without nuclei."""
    cl = np.asarray(cluster, np.int64).reshape(-1)
    lab = np.asarray(labels, np.int64).reshape(-1)
    C = int(num_classes)
    size = np.asarray(size, np.int64).reshape(-1)
    m = len(size)
    cc = np.asarray(class_count, np.int64).reshape(m, C)
    sxy = np.asarray(sum_xy, np.int64).reshape(m, 2)
    bb = np.asarray(bbox, np.int64).reshape(m, 4)
    if len(cl) != len(lab) or (size < 1).any():
        raise ValueError('derive: one label per nucleus, and no empty cluster')
    known = (lab >= 0) & (lab < C)
    class_n = np.bincount(lab[known], minlength=C).astype(np.int64)
    class_clustered = np.bincount(lab[known & (cl >= 0)], minlength=C).astype(np.int64)
    share = np.divide(class_clustered.astype(np.float64), class_n.astype(np.float64), out=np.zeros(C), where=class_n > 0)
    return dict(centroid_px=sxy.astype(np.float64) / (2.0 * size.astype(np.float64))[:, None], bbox_px=bb.astype(np.float64) / 2.0,
                class_fraction=cc.astype(np.float64) / size.astype(np.float64)[:, None], n_clusters=np.asarray(m, np.int64),
                n_noise=np.asarray(int((cl < 0).sum()), np.int64), class_n=class_n, class_clustered=class_clustered, class_clustered_share=share)


def write_npz(path, nuclei_id, xy, label, cluster, core, degree, size, n_core, class_count, sum_xy, bbox, radius_px, min_pts, by_class):
    """<id>_nuclei_clusters.npz, row i for the i-th row of <id>_nuclei_graph.npz / <id>_nuclei_feat.npz:
      nuclei_id int64 (n,), xy float64 (n, 2) (the unquantised centre in slide px), label int64 (n,)
      cluster int32 (n,) (-1: noise), core uint8 (n,), degree int32 (n,)
      size, n_core int32 (m,), class_count int32 (m, C), sum_xy int64 (m, 2), bbox int32 (m, 4): the integers of the definition
      the arrays of `derive` (DERIVED_KEYS), and radius_px float64, min_pts int64, by_class int64 as 0-d arrays."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    n = len(head['label'])
    cluster = np.ascontiguousarray(cluster, np.int32).reshape(-1)
    core = np.ascontiguousarray(core, np.uint8).reshape(-1)
    degree = np.ascontiguousarray(degree, np.int32).reshape(-1)
    size = np.ascontiguousarray(size, np.int32).reshape(-1)
    m = len(size)
    n_core = np.ascontiguousarray(n_core, np.int32).reshape(-1)
    class_count = np.ascontiguousarray(class_count, np.int32)
    sum_xy = np.ascontiguousarray(sum_xy, np.int64).reshape(-1, 2)
    bbox = np.ascontiguousarray(bbox, np.int32).reshape(-1, 4)
    if not (len(cluster) == len(core) == len(degree) == n):
        raise ValueError('write_npz: one row per nucleus in every per-nucleus field')
    if class_count.ndim != 2 or not (len(n_core) == len(class_count) == len(sum_xy) == len(bbox) == m):
        raise ValueError('write_npz: one row per cluster in every per-cluster field')
    if n and cluster.max() >= m:
        raise ValueError('write_npz: a nucleus lies in a cluster the tables do not hold')
    check_args(class_count.shape[1], half_pixel_radius(radius_px), min_pts, by_class)
    d = derive(cluster, head['label'], class_count.shape[1], size, class_count, sum_xy, bbox)
    with open(path, 'wb') as f:
        np.savez(f, **head, cluster=cluster, core=core, degree=degree, size=size, n_core=n_core,
                 class_count=class_count, sum_xy=sum_xy, bbox=bbox, radius_px=np.asarray(float(radius_px), np.float64),
                 min_pts=np.asarray(int(min_pts), np.int64), by_class=np.asarray(int(by_class), np.int64), **d)
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)
