"""Minimum spanning forest of a slide's nuclei: the third classic family of architectural descriptors of a tissue section beside Voronoi
cells and Delaunay edges -- edge-length mean, standard deviation, min / max ratio and disorder, the same per tree, and which classes the
edges join -- and, at the same time, the single-linkage dendrogram of the slide: cutting the forest at any length t <= r gives the
connected components of the t-radius graph, so one call answers "which nuclei hang together" for every radius at once.  Computed on the
GPU (csrc/cellmst.hip, `nuhtc_cell_mst`); tools/infer_wsi.py --nuclei-mst writes it as <id>_nuclei_mst.npz.  Not in the reference.

Definition.

Inputs.  n points in HALF pixels, int32 (n, 2), from `cellpoints.quantize_centres`, with |p| < 2**27 and n <= 2**24; labels, int32, one per
point; C classes, 1 <= C <= 14; a radius r in half pixels, an integer with 1 <= r <= 16384; by_class in {0, 1}.  All geometry is integer
arithmetic.

Rules.
  * An EDGE is an unordered pair i < j with dx * dx + dy * dy <= r * r.  The radius is inclusive.  With by_class, an edge also needs
    labels[i] == labels[j]: plain equality, the same for labels outside 0..C-1.  Coincident points are joined by an edge with d2 = 0.
  * Edges are ordered by the key (d2, i, j), lexicographically.  This is a strict total order, so the minimum spanning forest of the edge
    set is UNIQUE: it is what Kruskal's algorithm returns when it takes the edges in ascending key order.  That forest is the result.
    Nothing depends on visiting order.

Outputs, integers only.
  edges    int32 (m, 2)  the forest's edges (i, j) with i < j, in ascending (i, j) order
  edge_d2  int32 (m,)    the squared length of each edge, half pixels squared
  tree     int32 (n,)    the tree of every point, numbered 0..T-1 by ascending smallest row; an isolated point is a tree of size 1, so no
                         entry is -1
  m, T (m = n - T), and `rounds`: the number of Boruvka rounds of the device that added at least one edge.

`mst_reference` is the brute-force int64 restatement (every pair, no grid; Kruskal with a textbook union-find): the oracle the device
result must EQUAL.  The device bins the points into the cell graph's grid and runs Boruvka rounds over it: every component picks its
smallest edge out under the same key (a 64-bit atomic minimum over (d2, i) and a second one over j), the picks are united in the lock-free
union-find of the clusters, and the edges are put in (i, j) order by counting, not sorting.  `derive` makes the float64 side on the host:
edge lengths in px, node degrees, tree sizes and lengths, the class-pair census of the edges and the slide's edge-length statistics."""
import numpy as np

from . import cellpoints
from .cellpoints import COORD_LIMIT, MAX_CLASSES, MAX_POINTS, MAX_R, centres, half_pixel_radius, quantize_centres  # noqa: F401 (re-exported)

INT_NAMES = ('edges', 'edge_d2', 'tree')
DERIVED_KEYS = ('edge_len_px', 'mst_degree', 'tree_size', 'tree_length_px', 'edge_class_count', 'n_trees', 'n_edges',
                'length_mean_px', 'length_std_px', 'length_min_max_ratio', 'length_disorder')
NPZ_KEYS = ('nuclei_id', 'xy', 'label') + INT_NAMES + DERIVED_KEYS + ('radius_px', 'by_class')
BY = {'any': 0, 'class': 1}


def check_args(num_classes, r, by_class):
    """num_classes 1..14, r 1..16384 half pixels, by_class 0 or 1: ValueError otherwise."""
    cellpoints.check_radius_args('mst', num_classes, r, by_class)


def mst_reference(points, labels, num_classes, r, by_class):
    """The definition, pair by pair in int64: points int (n, 2) half pixels, labels int (n,), r in HALF pixels ->
    (edges int32 (m, 2), edge_d2 int32 (m,), tree int32 (n,), m, T).  O(n^2) time, rows in blocks of 256, and memory for the list of ALL
    edges (24 bytes each): meant for a few thousand points, or more where few are joined.  The edges are sorted by (d2, i, j) and taken by
    Kruskal's algorithm with a union-find (path compression, the smaller root on top); no grid and no rounds."""
    check_args(num_classes, r, by_class)
    p, lab = cellpoints.reference_points(points, labels, 'mst_reference')
    n, r, by_class = len(p), int(r), int(by_class)
    ii, jj, dd = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]      # every edge i < j and its d2
    for rows, d2 in cellpoints.pair_blocks(p, 256):
        adj = d2 <= r * r
        if by_class:
            adj &= lab[rows, None] == lab[None, :]
        adj &= rows[:, None] < np.arange(n, dtype=np.int64)[None, :]
        i, j = np.nonzero(adj)
        ii.append(rows[i]); jj.append(j); dd.append(d2[i, j])
    ii, jj, dd = np.concatenate(ii), np.concatenate(jj), np.concatenate(dd)
    order = np.lexsort((jj, ii, dd))                                          # ascending (d2, i, j)
    parent = list(range(n))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root
    taken = []
    for e, i, j in zip(order.tolist(), ii[order].tolist(), jj[order].tolist()):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)                                     # the root of a tree is its smallest row
            taken.append(e)
    taken = np.asarray(taken, np.int64)
    ei, ej, ed = ii[taken], jj[taken], dd[taken]
    by_rows = np.lexsort((ej, ei))                                            # ascending (i, j)
    root = np.asarray([find(x) for x in range(n)], np.int64)
    roots = np.unique(root)                                                   # ascending: the numbering
    tree = np.searchsorted(roots, root)
    edges = np.stack([ei[by_rows], ej[by_rows]], 1).astype(np.int32).reshape(-1, 2)
    return edges, ed[by_rows].astype(np.int32), tree.astype(np.int32), len(taken), len(roots)


def call(points, labels, num_classes, r, by_class, edges, edge_d2, tree, bounds=None, device=0):
    """nuhtc_cell_mst on torch tensors of cuda:`device` (all int32, contiguous; edges (n, 2), edge_d2 and tree (n,); r in HALF pixels) ->
    (the library's return code, m, T, rounds), nothing raised: the code is 0 or hip.E_INVALID / hip.E_HIP; m edges, T trees and the rounds
    that added an edge are None unless the code is 0.  bounds = (x_min, y_min, x_max, y_max) of the points, computed on the host when not
    given."""
    import ctypes
    m, t, rounds = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = cellpoints.launch('nuhtc_cell_mst', device, points, labels, (int(num_classes), int(r), int(by_class)),
                           (edges, edge_d2, tree), bounds, extra=(ctypes.byref(m), ctypes.byref(t), ctypes.byref(rounds)))
    return (rc,) + (tuple(int(v.value) for v in (m, t, rounds)) if rc == 0 else (None, None, None))


def outputs(n, device, fill=0):
    """The three output tensors of `call` for n points on `device`, every entry `fill`."""
    import torch
    return [torch.full(s, fill, dtype=torch.int32, device=device) for s in ((n, 2), (n,), (n,))]


def build(points, labels, num_classes, radius_px, by_class=0, device=0, with_rounds=False):
    """The forest of `points` (int (n, 2) half pixels, see cellpoints.quantize_centres) with `labels` (n,) on cuda:`device`: numpy in, the
    five results of `mst_reference` out (edges and edge_d2 cut to their m rows), and the device's `rounds` behind them when `with_rounds`.
    There is no host route: without the library or a GPU this raises."""
    C, r = int(num_classes), half_pixel_radius(radius_px)
    check_args(C, r, by_class)
    p, lab, dev, p_d, lab_d, bounds = cellpoints.resident(points, labels, 'mst', device)
    n = len(p)
    out = outputs(n, dev)
    rc, m, t, rounds = call(p_d, lab_d, C, r, int(by_class), *out, bounds=bounds, device=device)
    cellpoints.raise_for(rc, 'nuhtc_cell_mst')
    got = (out[0][:m].cpu().numpy(), out[1][:m].cpu().numpy(), out[2].cpu().numpy(), m, t)
    return got + (rounds,) if with_rounds else got


def derive(edges, edge_d2, tree, labels, num_classes):
    """The float64 side of the integers -> dict:
      edge_len_px           float64 (m,)    sqrt(edge_d2) / 2
      mst_degree            int32 (n,)      the forest's edges at every nucleus
      tree_size             int32 (T,)      the nuclei of every tree
      tree_length_px        float64 (T,)    the sum of its edge lengths (0 for a single nucleus)
      edge_class_count      int64 (C, C)    the edges by [min label, max label] of their ends (upper triangle); an edge touching a label
                                            outside 0..C-1 is counted nowhere
      n_trees, n_edges      int64 0-d       T, m
      length_mean_px, length_std_px         float64 0-d: over the edges (the population standard deviation)
      length_min_max_ratio  float64 0-d     the shortest edge over the longest
      length_disorder       float64 0-d     1 - 1 / (1 + std / mean)
    The last four are 0, never NaN, when there is no edge (and a ratio is 0 where its denominator is)."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    d2 = np.asarray(edge_d2, np.int64).reshape(-1)
    tr = np.asarray(tree, np.int64).reshape(-1)
    lab = np.asarray(labels, np.int64).reshape(-1)
    C, n, m = int(num_classes), len(tr), len(d2)
    if len(e) != m or len(lab) != n or (m and (e.min() < 0 or e.max() >= n)) or (n and tr.min() < 0) or (d2 < 0).any():
        raise ValueError('derive: one d2 per edge, one label and one tree per nucleus, edges between rows')
    t = int(tr.max()) + 1 if n else 0
    length = np.sqrt(d2.astype(np.float64)) / 2
    degree = np.bincount(e.reshape(-1), minlength=n).astype(np.int32)
    tree_size = np.bincount(tr, minlength=t).astype(np.int32)
    tree_length = np.bincount(tr[e[:, 0]], weights=length, minlength=t).astype(np.float64) if m else np.zeros(t, np.float64)
    census = cellpoints.class_pair_census(lab[e[:, 0]], lab[e[:, 1]], C)
    mean = float(length.mean()) if m else 0.0
    std = float(length.std()) if m else 0.0
    longest = float(length.max()) if m else 0.0
    ratio = float(length.min()) / longest if longest > 0 else 0.0
    disorder = 1.0 - 1.0 / (1.0 + std / mean) if mean > 0 else 0.0
    f8 = lambda v: np.asarray(v, np.float64)
    return dict(edge_len_px=length, mst_degree=degree, tree_size=tree_size, tree_length_px=tree_length, edge_class_count=census,
                n_trees=np.asarray(t, np.int64), n_edges=np.asarray(m, np.int64), length_mean_px=f8(mean), length_std_px=f8(std),
                length_min_max_ratio=f8(ratio), length_disorder=f8(disorder))


def write_npz(path, nuclei_id, xy, label, edges, edge_d2, tree, num_classes, radius_px, by_class):
    """<id>_nuclei_mst.npz, row i for the i-th row of <id>_nuclei_graph.npz / <id>_nuclei_feat.npz:
      nuclei_id int64 (n,), xy float64 (n, 2) (the unquantised centre in slide px), label int64 (n,)
      edges int32 (m, 2) (rows of this file), edge_d2 int32 (m,), tree int32 (n,): the integers of the definition
      the arrays of `derive` (DERIVED_KEYS), and radius_px float64, by_class int64 as 0-d arrays."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    n = len(head['label'])
    edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
    edge_d2 = np.ascontiguousarray(edge_d2, np.int32).reshape(-1)
    tree = np.ascontiguousarray(tree, np.int32).reshape(-1)
    if len(tree) != n or len(edges) != len(edge_d2):
        raise ValueError('write_npz: one tree per nucleus and one d2 per edge')
    cellpoints.check_edge_rows(edges, n)
    check_args(num_classes, half_pixel_radius(radius_px), by_class)
    d = derive(edges, edge_d2, tree, head['label'], num_classes)
    with open(path, 'wb') as f:
        np.savez(f, **head, edges=edges, edge_d2=edge_d2, tree=tree, radius_px=np.asarray(float(radius_px), np.float64),
                 by_class=np.asarray(int(by_class), np.int64), **d)
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)
