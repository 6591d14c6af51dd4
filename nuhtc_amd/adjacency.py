"""Territory adjacency of a slide: the discrete Delaunay graph of the nucleus centres -- two nuclei are neighbours when their territories
(territory.py: the nearest-nucleus raster) touch on the lattice.  It is the Voronoi / Delaunay neighbourhood of the nucleus-architecture
literature, and the default graph of squidpy's `spatial_neighbors` on generic coordinates, in the form this project can state exactly: the
other graphs here either take a parameter that decides who is a neighbour (cellgraph.py: k nearest within a radius) or are not the standard
neighbourhood (proximity.py: Gabriel and RNG, both subgraphs of it; mst.py: the forest).  It gives each nucleus its number of neighbours,
their classes and the length of every common border.  The exact Delaunay triangulation stays out (circumcentres need more than
64 bits, cocircular half-pixel centres need a tie rule); on the lattice adjacency is a statement about integers: unique, bitwise
repeatable, and checkable by brute force from the owner map territory.py already defines.  Computed on the GPU (csrc/celladjacency.hip,
`nuhtc_territory_adjacency`, on the owner map `nuhtc_cell_territory` left on the device); tools/infer_wsi.py --nuclei-adjacency writes it as
<id>_nuclei_adjacency.npz.  Not in the reference.

Definition.

Inputs.  Those of the territories: n points in HALF pixels, one label each, C classes, the reach R and the pitch s in half pixels, and a
window gx0, gy0, W, H in lattice units; every limit is territory.py's (n <= 2**24, W * H <= 2**28).  The owner map is exactly territory's
`owner`, int32 (H, W) with entries in -1 .. n - 1: nothing about ownership is redefined here.

Site pair.  An unordered pair of 4-adjacent sites, both inside the window.  Each is counted once.

Edge.  {i, j} with i < j exists when some site pair has the owners i and j, both >= 0.  A site nobody owns makes no edge.  A row that owns
nothing has none: a row that does not compete, a coincident row behind a smaller one, a row the pitch steps over.

Adjacency is 4-ADJACENCY, the same as territory's `contact`: two territories that meet only diagonally (their sites share a corner and no
side) are NOT adjacent.

Outputs, integers only.
  edges   int32 (m, 2)  the rows (i, j) with i < j, in ascending lexicographic order: a pure function of the input
  shared  int32 (m,)    the site pairs with owners {i, j}: the length of the common border in lattice steps, at most 2 * 2**28.  Summed in
                        both directions by the classes of the two ends it IS territory's `contact` table (`contact_of`): the cross-check
                        against the tally kernel
  degree  int32 (n,)    the distinct neighbours of each row
  m       the number of edges

Like the territory tallies the result is OVER THE WINDOW: a sub-window gives the edges visible in it.

`adjacency_reference` is the numpy restatement in int64 (every horizontal and vertical site pair of the map, np.unique over the pair
keys): the oracle the device result must EQUAL.  `derive` makes the float64 side on the host.

Out of scope: 8-adjacency; the exact Delaunay triangulation and its triangles; the edges a window cuts off."""
import numpy as np

from . import cellpoints, density, territory
from .cellpoints import COORD_LIMIT, MAX_CLASSES, MAX_POINTS, MAX_R, centres, half_pixel_radius, quantize_centres  # noqa: F401 (re-exported)
from .territory import MAX_PITCH, MAX_SITES, window  # noqa: F401 (the lattice, the cap and the default window are territory's)

MAX_EDGE_CAP = (1 << 31) - 1
INT_NAMES = ('edges', 'shared', 'degree')
DERIVED_KEYS = ('edge_d2', 'edge_px', 'border_px', 'class_edge_count', 'class_border', 'neighbour_class', 'n_closed', 'closed_degree_mean', 'n_edges')
NPZ_KEYS = ('nuclei_id', 'xy', 'label') + INT_NAMES + territory.INT_NAMES + DERIVED_KEYS + ('reach_px', 'pitch_px', 'window')


def check_args(num_classes, r, s, win=None):
    """territory.check_args (density.check_lattice with territory's name and cap): ValueError otherwise."""
    territory.check_args(num_classes, r, s, win)


def first_edge_cap(n):
    """The rows of capacity of `build`'s first call.  A planar graph on n points has at most 3 n - 6 edges, and the Delaunay graph is
    planar -- but this is only a first guess on a LATTICE: four territories that meet near one point may all touch one another's sites
    pairwise along the two axes (the graph of the lattice need not be planar), and territories cut by the reach need not be convex.  The
    device says how many there are, and `build` calls once more."""
    return cellpoints.first_edge_cap(n, 3)


def adjacency_reference(owner, n):
    """The definition in int64: owner int (H, W) with entries in -1 .. n - 1 -> (edges int32 (m, 2), shared int32 (m,), degree int32 (n,), m).
    Every horizontal and every vertical site pair of the map, np.unique with counts over the keys lo * n + hi."""
    own = np.asarray(owner, np.int64)
    n = int(n)
    if own.ndim != 2 or own.size == 0 or own.min() < -1 or own.max() >= n:
        raise ValueError('adjacency_reference: the owner map is (H, W) with H, W >= 1 and entries in -1 .. n - 1')
    keys = []
    for a, b in ((own[:, :-1], own[:, 1:]), (own[:-1, :], own[1:, :])):
        pair = (a != b) & (a >= 0) & (b >= 0)
        keys.append(np.minimum(a, b)[pair] * n + np.maximum(a, b)[pair])
    key, count = np.unique(np.concatenate(keys), return_counts=True)
    edges = np.stack([key // max(n, 1), key % max(n, 1)], 1).astype(np.int32).reshape(-1, 2)
    return edges, count.astype(np.int32), np.bincount(edges.reshape(-1), minlength=n).astype(np.int32), len(key)


def contact_of(edges, shared, labels, num_classes):
    """territory's `contact` int64 (C, C) from the graph: every edge adds its shared at [label_i][label_j] and at [label_j][label_i]."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    lab = np.asarray(labels, np.int64).reshape(-1)
    contact = np.zeros((int(num_classes),) * 2, np.int64)
    w = np.asarray(shared, np.int64).reshape(-1)
    np.add.at(contact, (lab[e[:, 0]], lab[e[:, 1]]), w)
    np.add.at(contact, (lab[e[:, 1]], lab[e[:, 0]]), w)
    return contact


def call(owner, n, edge_cap, edges, shared, degree, device=0):
    """nuhtc_territory_adjacency on torch tensors of cuda:`device` (contiguous; owner int32 (H, W) as nuhtc_cell_territory wrote it, edges
    int32 (edge_cap, 2), shared int32 (edge_cap,), degree int32 (n,)) -> (the library's return code, m), nothing raised: the code is 0 or
    hip.E_INVALID / hip.E_HIP; m is None unless the code is 0.  With m > edge_cap edges and shared are untouched (degree is written): call
    again with edge_cap >= m."""
    import ctypes
    import torch
    from . import hip
    fn = hip.load().nuhtc_territory_adjacency
    m = ctypes.c_int64(-1)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    dev = torch.device('cuda', device)
    with torch.cuda.device(dev):
        rc = fn(int(device), vp(owner), int(owner.shape[1]), int(owner.shape[0]), int(n), int(edge_cap), vp(edges), vp(shared), vp(degree), ctypes.byref(m),
                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return rc, (int(m.value) if rc == 0 else None)


def outputs(n, edge_cap, device, fill=0):
    """The three output tensors of `call` for n rows and edge_cap rows of capacity on `device` (one row at least each), every entry `fill`."""
    import torch
    cap, n = max(int(edge_cap), 1), max(int(n), 1)
    return [torch.full(s, fill, dtype=torch.int32, device=device) for s in ((cap, 2), (cap,), (n,))]


def build(points, labels, num_classes, reach_px, pitch_px, win=None, device=0, with_calls=False):
    """The graph of `points` (int (n, 2) half pixels, see cellpoints.quantize_centres) with `labels` (n,) on cuda:`device`: numpy in,
    ((edges, shared, degree), the six territory tallies of territory.INT_NAMES, win) out, and the number of adjacency calls it took behind
    them when `with_calls`.  The territories are built first (territory.call into territory.outputs; the owner map stays on the device and
    is never copied off it), then the graph from the map: the first call has room for `first_edge_cap(n)` edges, and when there are more the
    device says how many and ONE second call has room for exactly that many.  Without `win` the window is territory's default one;
    ValueError when it exceeds 2**28 sites.  There is no host route: without the library or a GPU this raises."""
    n, C, r, s, win, dev, p_d, lab_d, bounds = density.lattice_points('adjacency', check_args, points, labels, num_classes, reach_px, pitch_px, win, device)
    terr = territory.outputs(n, C, win, dev)
    cellpoints.raise_for(territory.call(p_d, lab_d, C, r, s, win, *terr, bounds=bounds, device=device), 'nuhtc_cell_territory')
    owner = terr[0]
    del terr[1]                                                               # nearest_d2: not needed, and as large as the map
    out, m, _, calls = cellpoints.grow_to_fit(lambda cap, out: call(owner, n, cap, *out, device=device), lambda cap: outputs(n, cap, dev),
                                              first_edge_cap(n), 'nuhtc_territory_adjacency', 'adjacency', limit=None)      # m <= 2**29 by the window's cap
    area, border, is_open, contact, class_sites, free_sites = (t.cpu().numpy() for t in terr[1:])
    tallies = (area, border, is_open.astype(np.uint8), contact, class_sites, free_sites.reshape(()))
    got = ((out[0][:m].cpu().numpy(), out[1][:m].cpu().numpy(), out[2][:n].cpu().numpy()), tallies, win)
    return got + (calls,) if with_calls else got


def derive(edges, shared, degree, points, labels, num_classes, s, area=None, is_open=None):
    """The host side of the integers, in int64 / float64 (points int (n, 2) half pixels, s the pitch in HALF pixels; area and is_open the
    territory tallies, without them no territory counts as closed) -> dict, never a NaN:
      edge_d2             int64 (m,)     the squared distance of the two centres in half pixels^2: 64 bits, as two owners may lie two
                                         reaches and a pitch apart and |p| < 2**27 alone allows 2**57
      edge_px             float64 (m,)   sqrt(edge_d2) / 2
      border_px           float64 (m,)   shared * s / 2: the common border in px, as lattice steps of one pitch each
      class_edge_count    int64 (C, C)   the edges by [min label, max label] of their ends (cellpoints.class_pair_census: upper triangle)
      class_border        int64 (C, C)   the same census weighted by shared
      neighbour_class     int32 (n, C)   the neighbours of each nucleus by class; its row sums to degree
      n_closed            int64 (C,)     the closed territories of each class (territory.derive's `closed`: open == 0 and area > 0)
      closed_degree_mean  float64 (C,)   the mean degree over them, 0 where there are none: the number of Voronoi neighbours, which the
                                         rim of the window and the reach do not cut short
      n_edges             int64 0-d      m"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    w = np.asarray(shared, np.int64).reshape(-1)
    deg = np.asarray(degree, np.int64).reshape(-1)
    p = np.asarray(points, np.int64).reshape(-1, 2)
    lab = np.asarray(labels, np.int64).reshape(-1)
    C, n, m = int(num_classes), len(lab), len(w)
    if len(e) != m or len(deg) != n or len(p) != n or (m and (e.min() < 0 or e.max() >= n or (w < 1).any())) or not 1 <= int(s) <= MAX_PITCH or not 1 <= C <= MAX_CLASSES:
        raise ValueError('derive: one shared >= 1 per edge, one point, one label and one degree per nucleus, edges between rows, s 1..2**20, C 1..14')
    if not np.array_equal(deg, np.bincount(e.reshape(-1), minlength=n)):
        raise ValueError('derive: degree is not the number of edges at every row')
    la, lb = lab[e[:, 0]], lab[e[:, 1]]
    if m and (min(la.min(), lb.min()) < 0 or max(la.max(), lb.max()) >= C):
        raise ValueError('derive: a row with a label outside 0..C-1 owns nothing and has no edge')
    d2 = ((p[e[:, 0]] - p[e[:, 1]]) ** 2).sum(1).astype(np.int64)
    lo, hi = np.minimum(la, lb), np.maximum(la, lb)
    class_border = np.zeros((C, C), np.int64)
    np.add.at(class_border, (lo, hi), w)
    neighbour = np.zeros((n, C), np.int64)
    np.add.at(neighbour, (e[:, 0], lb), 1)
    np.add.at(neighbour, (e[:, 1], la), 1)
    n_closed, mean = np.zeros(C, np.int64), np.zeros(C, np.float64)
    if area is not None and is_open is not None:
        area, is_open = np.asarray(area, np.int64).reshape(-1), np.asarray(is_open, np.int64).reshape(-1)
        if not len(area) == len(is_open) == n:
            raise ValueError('derive: area and open have one entry per nucleus')
        closed = (is_open == 0) & (area > 0)
        for c in range(C):
            d = deg[closed & (lab == c)]
            n_closed[c] = len(d)
            if len(d):
                mean[c] = d.mean()
    return dict(edge_d2=d2, edge_px=np.sqrt(d2.astype(np.float64)) / 2, border_px=w.astype(np.float64) * (int(s) / 2.0),
                class_edge_count=cellpoints.class_pair_census(la, lb, C), class_border=class_border, neighbour_class=neighbour.astype(np.int32),
                n_closed=n_closed, closed_degree_mean=mean, n_edges=np.asarray(m, np.int64))


def write_npz(path, nuclei_id, xy, label, graph, tallies, win, reach_px, pitch_px):
    """<id>_nuclei_adjacency.npz, the header row i for the i-th row of <id>_nuclei_graph.npz / <id>_nuclei_feat.npz:
      nuclei_id int64 (n,), xy float64 (n, 2) (the unquantised centre in slide px), label int64 (n,)
      edges int32 (m, 2) (rows of this file), shared int32 (m,), degree int32 (n,): graph = the integers of the definition
      area, border int32 (n,), open uint8 (n,), contact int64 (C, C), class_sites int64 (C,), free_sites int64 0-d: the territory tallies
      the graph was read off, over the same window; contact must equal `contact_of` the graph
      the arrays of `derive` (DERIVED_KEYS; the centres are rint(2 xy), the points the graph was built on)
      reach_px, pitch_px float64 0-d; window int64 (4,) gx0, gy0, W, H."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    n = len(head['label'])
    edges, shared, degree = graph
    edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
    shared, degree = np.ascontiguousarray(shared, np.int32).reshape(-1), np.ascontiguousarray(degree, np.int32).reshape(-1)
    area, border, is_open, contact, class_sites, free_sites = tallies
    area, border = np.ascontiguousarray(area, np.int32).reshape(-1), np.ascontiguousarray(border, np.int32).reshape(-1)
    is_open = np.ascontiguousarray(is_open, np.uint8).reshape(-1)
    contact, class_sites = np.ascontiguousarray(contact, np.int64), np.ascontiguousarray(class_sites, np.int64).reshape(-1)
    free_sites = np.asarray(free_sites, np.int64).reshape(())
    r, s = half_pixel_radius(reach_px), half_pixel_radius(pitch_px)
    win = tuple(int(v) for v in win)
    C = len(class_sites)
    check_args(C, r, s, win)
    if len(degree) != n or len(edges) != len(shared) or not (len(area) == len(border) == len(is_open) == n) or contact.shape != (C, C):
        raise ValueError('write_npz: one degree, area, border and open per nucleus, one shared per edge, contact is (C, C)')
    cellpoints.check_edge_rows(edges, n)
    if int(class_sites.sum()) + int(free_sites) != win[2] * win[3]:
        raise ValueError('write_npz: class_sites and free_sites do not sum to the window\'s W * H')
    pts = np.rint(2 * head['xy']).astype(np.int64)
    d = derive(edges, shared, degree, pts, head['label'], C, s, area, is_open)
    if not np.array_equal(contact_of(edges, shared, head['label'], C), contact):
        raise ValueError('write_npz: the graph\'s shared borders do not sum to the territories\' contact table')
    with open(path, 'wb') as f:
        np.savez(f, **head, edges=edges, shared=shared, degree=degree, area=area, border=border, open=is_open, contact=contact,
                 class_sites=class_sites, free_sites=free_sites, **d, reach_px=np.asarray(float(reach_px), np.float64),
                 pitch_px=np.asarray(float(pitch_px), np.float64), window=np.asarray(win, np.int64))
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)
