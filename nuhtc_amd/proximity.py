"""Proximity graphs of a slide's nuclei: the Gabriel graph and the relative neighbourhood graph (RNG) -- the parameter-free "who touches
whom" relations that cell-graph work in pathology counts contacts between cell types on (lymphocyte next to tumour, stroma next to
tumour).  The other per-slide analyses take a parameter that decides who is a neighbour (k, eps, min_pts) or, like the forest of mst.py,
keep n - 1 edges only.  Both graphs are subgraphs of the Delaunay graph and supergraphs of the minimum spanning forest at the same radius
(MSF in RNG in Gabriel), and unlike a Delaunay or Voronoi build both are decided by three squared distances in int32, are local, and are
unique without a tie rule.  Computed on the GPU (csrc/cellprox.hip, `nuhtc_cell_proximity`); tools/infer_wsi.py --nuclei-proximity writes
them as <id>_nuclei_proximity.npz.  Not in the reference.

Definition.

Inputs.  n points in HALF pixels, int32 (n, 2), from `cellpoints.quantize_centres`, with |p| < 2**27 and n <= 2**24; labels, int32, one per
point; C classes, 1 <= C <= 14; a radius r in half pixels, an integer with 1 <= r <= 16384; by_class in {0, 1}.  All geometry is integer
arithmetic; write d2(a, b) for the squared distance of two rows.

Rules.
  * A CANDIDATE is an unordered pair i < j with d2(i, j) <= r * r.  The radius is inclusive.  With by_class, a candidate also needs
    labels[i] == labels[j]: plain equality, the same for labels outside 0..C-1.
  * A WITNESS for a candidate is any other row k (k != i, k != j), at any distance.  With by_class, k must have the label of i and j, so the
    by_class result is the union of the graphs of the label subsets.
  * The candidate is a GABRIEL edge when no witness has d2(i, k) + d2(j, k) < d2(i, j): no witness strictly inside the disc whose diameter
    is ij.  A witness ON the circle (a right angle at k) does not block.
  * It is an RNG edge when no witness has max(d2(i, k), d2(j, k)) < d2(i, j).  Strict: a witness as far from an end as the other end is
    does not block.
  * Every RNG edge is a Gabriel edge (two non-negative terms with a sum below d2(i, j) are each below it).  Coincident points are joined by
    an edge with d2 = 0 and rng = 1, and a point coincident with an end never blocks.  m coincident points are a clique of m (m - 1) / 2
    edges: the edge count is not bounded by a multiple of n.
  * A blocking witness has d2(i, k) < d2(i, j) <= r * r, so the device finds it in the 3 x 3 grid cells around i; the restatement below
    looks at every row.
  * Every sum is at most 2**29: int32 throughout on the device (csrc/cellgrid_host.h has the argument), int64 here.

Outputs, integers only.
  edges     int32 (m, 2)  the Gabriel edges (i, j) with i < j, in ascending (i, j) order
  edge_d2   int32 (m,)    the squared length of each edge, half pixels squared
  edge_rng  uint8 (m,)    1 where the Gabriel edge is an RNG edge too
  degree    int32 (n, 2)  the Gabriel and the RNG edges at every row
  m, m_rng

`proximity_reference` is the brute-force int64 restatement (every pair against every row, no grid): the oracle the device result must EQUAL.
`derive` makes the float64 side on the host: edge lengths in px, the class-pair census of both graphs, each nucleus's mean edge length and
share of neighbours of another label, and the census over what shuffled labels would give on the same graph."""
import numpy as np

from . import cellpoints
from .cellpoints import COORD_LIMIT, MAX_CLASSES, MAX_POINTS, MAX_R, centres, half_pixel_radius, quantize_centres  # noqa: F401 (re-exported)

INT_NAMES = ('edges', 'edge_d2', 'edge_rng', 'degree')
DERIVED_KEYS = ('edge_len_px', 'gabriel_class_count', 'rng_class_count', 'mean_len_px', 'other_class_share', 'gabriel_class_enrichment',
                'n_edges', 'n_rng')
NPZ_KEYS = ('nuclei_id', 'xy', 'label') + INT_NAMES + DERIVED_KEYS + ('radius_px', 'by_class')
BY = {'any': 0, 'class': 1}


def check_args(num_classes, r, by_class):
    """num_classes 1..14, r 1..16384 half pixels, by_class 0 or 1: ValueError otherwise."""
    cellpoints.check_radius_args('proximity', num_classes, r, by_class)


def first_edge_cap(n):
    """The rows of capacity of `build`'s first call: a planar graph has fewer than 3 n edges, coincident points add to that."""
    return cellpoints.first_edge_cap(n, 4)


def proximity_reference(points, labels, num_classes, r, by_class):
    """The definition in int64: points int (n, 2) half pixels, labels int (n,), r in HALF pixels ->
    (edges int32 (m, 2), edge_d2 int32 (m,), edge_rng uint8 (m,), degree int32 (n, 2), m, m_rng).  Every candidate against EVERY row as a
    witness, no grid: O(candidates x n) time, rows in blocks of 256 and the candidates of a block 1024 at a time (three (1024, n) int64
    temporaries).  Meant for a few thousand points."""
    check_args(num_classes, r, by_class)
    p, lab = cellpoints.reference_points(points, labels, 'proximity_reference')
    n, r, by_class = len(p), int(r), int(by_class)
    idx = np.arange(n, dtype=np.int64)
    ii, jj, dd, rr = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, bool)]
    for rows, d2 in cellpoints.pair_blocks(p, 256):
        cand = d2 <= r * r
        if by_class:
            cand &= lab[rows, None] == lab[None, :]
        cand &= rows[:, None] < idx[None, :]
        a, j = np.nonzero(cand)                                               # row-major: ascending (i, j)
        for c0 in range(0, len(a), 1024):
            ac, jc = a[c0:c0 + 1024], j[c0:c0 + 1024]
            i = rows[ac]
            dij = d2[ac, jc][:, None]
            dik = d2[ac]                                                      # (e, n): from i to every row
            djk = ((p[jc, None, :] - p[None, :, :]) ** 2).sum(2)              # (e, n): from j to every row
            witness = (idx[None, :] != i[:, None]) & (idx[None, :] != jc[:, None])
            if by_class:
                witness &= lab[None, :] == lab[i, None]
            gabriel = ~((dik + djk < dij) & witness).any(1)
            rng = ~((np.maximum(dik, djk) < dij) & witness).any(1)
            ii.append(i[gabriel]); jj.append(jc[gabriel]); dd.append(dij[gabriel, 0]); rr.append(rng[gabriel])
    ii, jj, dd, rr = np.concatenate(ii), np.concatenate(jj), np.concatenate(dd), np.concatenate(rr)
    edges = np.stack([ii, jj], 1).astype(np.int32).reshape(-1, 2)
    degree = np.stack([np.bincount(edges.reshape(-1), minlength=n), np.bincount(edges[rr].reshape(-1), minlength=n)], 1).astype(np.int32).reshape(n, 2)
    return edges, dd.astype(np.int32), rr.astype(np.uint8), degree, len(ii), int(rr.sum())


def call(points, labels, num_classes, r, by_class, edge_cap, edges, edge_d2, edge_rng, degree, bounds=None, device=0):
    """nuhtc_cell_proximity on torch tensors of cuda:`device` (contiguous; edges int32 (edge_cap, 2), edge_d2 int32 and edge_rng uint8
    (edge_cap,), degree int32 (n, 2); r in HALF pixels) -> (the library's return code, m, m_rng), nothing raised: the code is 0 or
    hip.E_INVALID / hip.E_HIP; m and m_rng are None unless the code is 0.  With m > edge_cap the three edge arrays are untouched (degree
    is written): call again with edge_cap >= m.  bounds = (x_min, y_min, x_max, y_max) of the points, computed on the host when not given."""
    import ctypes
    m, m_rng = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = cellpoints.launch('nuhtc_cell_proximity', device, points, labels, (int(num_classes), int(r), int(by_class), int(edge_cap)),
                           (edges, edge_d2, edge_rng, degree), bounds, extra=(ctypes.byref(m), ctypes.byref(m_rng)))
    return (rc,) + ((int(m.value), int(m_rng.value)) if rc == 0 else (None, None))


def outputs(n, edge_cap, device, fill=0):
    """The four output tensors of `call` for n points and edge_cap rows of capacity on `device` (one row at least each), every entry `fill`."""
    import torch
    cap, n = max(int(edge_cap), 1), max(int(n), 1)
    return [torch.full(s, fill, dtype=t, device=device) for s, t in (((cap, 2), torch.int32), ((cap,), torch.int32), ((cap,), torch.uint8), ((n, 2), torch.int32))]


def build(points, labels, num_classes, radius_px, by_class=0, device=0, with_calls=False):
    """The two graphs of `points` (int (n, 2) half pixels, see cellpoints.quantize_centres) with `labels` (n,) on cuda:`device`: numpy in,
    the six results of `proximity_reference` out, and the number of device calls it took behind them when `with_calls`.  The first call has
    room for `first_edge_cap(n)` edges; when there are more (many coincident points) the device says how many and writes no edge, and ONE
    second call has room for exactly that many.  There is no host route: without the library or a GPU this raises."""
    C, r = int(num_classes), half_pixel_radius(radius_px)
    check_args(C, r, by_class)
    p, lab, dev, p_d, lab_d, bounds = cellpoints.resident(points, labels, 'proximity', device)
    n = len(p)
    out, m, (m_rng,), calls = cellpoints.grow_to_fit(
        lambda cap, out: call(p_d, lab_d, C, r, int(by_class), cap, *out, bounds=bounds, device=device),
        lambda cap: outputs(n, cap, dev), first_edge_cap(n), 'nuhtc_cell_proximity', 'proximity')
    got = (out[0][:m].cpu().numpy(), out[1][:m].cpu().numpy(), out[2][:m].cpu().numpy(), out[3][:n].cpu().numpy(), m, m_rng)
    return got + (calls,) if with_calls else got


def derive(edges, edge_d2, edge_rng, degree, labels, num_classes):
    """The float64 side of the integers -> dict:
      edge_len_px               float64 (m,)    sqrt(edge_d2) / 2
      gabriel_class_count       int64 (C, C)    the Gabriel edges by [min label, max label] of their ends (upper triangle); an edge touching a
      rng_class_count           int64 (C, C)    label outside 0..C-1 is counted nowhere.  The same over the RNG edges
      mean_len_px               float64 (n, 2)  the mean length of the Gabriel and of the RNG edges at every nucleus, 0 where it has none
      other_class_share         float64 (n,)    the share of a nucleus's Gabriel neighbours with another label (plain inequality), 0 where it
                                                has none
      gabriel_class_enrichment  float64 (C, C)  gabriel_class_count over its expectation E under shuffled labels on the fixed graph (upper
                                                triangle): with n nuclei, n_a of them of class a, and all m Gabriel edges,
                                                E[a][b] = m * 2 n_a n_b / (n (n - 1)) for a < b and E[a][a] = m * n_a (n_a - 1) / (n (n - 1)).
                                                0 where E is 0; never NaN
      n_edges, n_rng            int64 0-d       m, m_rng"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    d2 = np.asarray(edge_d2, np.int64).reshape(-1)
    rng = np.asarray(edge_rng).reshape(-1).astype(bool)
    deg = np.asarray(degree, np.int64).reshape(-1, 2)
    lab = np.asarray(labels, np.int64).reshape(-1)
    C, n, m = int(num_classes), len(lab), len(d2)
    if len(e) != m or len(rng) != m or len(deg) != n or (m and (e.min() < 0 or e.max() >= n)) or (d2 < 0).any():
        raise ValueError('derive: one d2 and one rng flag per edge, one label and one degree row per nucleus, edges between rows')
    if not (np.array_equal(deg[:, 0], np.bincount(e.reshape(-1), minlength=n)) and np.array_equal(deg[:, 1], np.bincount(e[rng].reshape(-1), minlength=n))):
        raise ValueError('derive: degree is not the number of edges at every row')
    length = np.sqrt(d2.astype(np.float64)) / 2
    la, lb = lab[e[:, 0]], lab[e[:, 1]]
    gabriel, rng_count = cellpoints.class_pair_census(la, lb, C), cellpoints.class_pair_census(la[rng], lb[rng], C)
    mean_len = np.zeros((n, 2), np.float64)
    for col, keep in ((0, np.ones(m, bool)), (1, rng)):
        total = np.bincount(e[keep].reshape(-1), weights=np.repeat(length[keep], 2), minlength=n) if keep.any() else np.zeros(n)
        has = deg[:, col] > 0
        mean_len[has, col] = total[has] / deg[has, col]
    other = np.bincount(e[la != lb].reshape(-1), minlength=n).astype(np.float64)
    share = np.zeros(n, np.float64)
    has = deg[:, 0] > 0
    share[has] = other[has] / deg[has, 0]
    size = np.bincount(lab[(lab >= 0) & (lab < C)], minlength=C).astype(np.float64)
    expected = np.zeros((C, C), np.float64)
    if n > 1:
        expected = np.triu(2 * np.outer(size, size), 1) + np.diag(size * (size - 1))
        expected *= m / (n * (n - 1.0))
    enrichment = np.zeros((C, C), np.float64)
    np.divide(gabriel, expected, out=enrichment, where=expected > 0)
    return dict(edge_len_px=length, gabriel_class_count=gabriel, rng_class_count=rng_count, mean_len_px=mean_len, other_class_share=share,
                gabriel_class_enrichment=enrichment, n_edges=np.asarray(m, np.int64), n_rng=np.asarray(int(rng.sum()), np.int64))


def write_npz(path, nuclei_id, xy, label, edges, edge_d2, edge_rng, degree, num_classes, radius_px, by_class):
    """<id>_nuclei_proximity.npz, row i for the i-th row of <id>_nuclei_graph.npz / <id>_nuclei_feat.npz:
      nuclei_id int64 (n,), xy float64 (n, 2) (the unquantised centre in slide px), label int64 (n,)
      edges int32 (m, 2) (rows of this file), edge_d2 int32 (m,), edge_rng uint8 (m,), degree int32 (n, 2): the integers of the definition
      the arrays of `derive` (DERIVED_KEYS), and radius_px float64, by_class int64 as 0-d arrays."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    n = len(head['label'])
    edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
    edge_d2 = np.ascontiguousarray(edge_d2, np.int32).reshape(-1)
    edge_rng = np.ascontiguousarray(edge_rng, np.uint8).reshape(-1)
    degree = np.ascontiguousarray(degree, np.int32).reshape(-1, 2)
    if len(degree) != n or not len(edges) == len(edge_d2) == len(edge_rng):
        raise ValueError('write_npz: one degree row per nucleus, one d2 and one rng flag per edge')
    cellpoints.check_edge_rows(edges, n)
    check_args(num_classes, half_pixel_radius(radius_px), by_class)
    d = derive(edges, edge_d2, edge_rng, degree, head['label'], num_classes)
    with open(path, 'wb') as f:
        np.savez(f, **head, edges=edges, edge_d2=edge_d2, edge_rng=edge_rng, degree=degree, radius_px=np.asarray(float(radius_px), np.float64),
                 by_class=np.asarray(int(by_class), np.int64), **d)
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)
