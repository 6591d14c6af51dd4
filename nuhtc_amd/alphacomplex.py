"""The alpha complex of a slide's nuclei: the exact Delaunay edges, and through their apexes the Delaunay triangles, within a radius -- the
answer to "which nuclei are Delaunay neighbours" that the other graphs of the slide path do not give.  The Gabriel graph and the RNG of
proximity.py are exact but strict subgraphs of the Delaunay graph (they drop most of the long sides of the triangles); adjacency.py gives
the Delaunay graph in discrete form, read off a lattice, so its edges depend on the pitch.  This is the continuous statement of what
adjacency.py discretises: two territories at reach rho touch when some point of the plane is equally near to both nuclei, within rho of
them, and nearer to no third nucleus -- a disc of radius at most rho with both nuclei on its boundary and nobody strictly inside, which is
the definition of an edge of the alpha complex at radius rho.  forest in RNG in Gabriel in alpha complex in Delaunay, at matching radii.
Computed on the GPU (csrc/cellalpha.hip, `nuhtc_cell_alpha`); tools/infer_wsi.py --nuclei-alpha writes it as <id>_nuclei_alpha.npz.  Not
in the reference.

Definition.

Inputs.  n points in HALF pixels, int32 (n, 2), from `cellpoints.quantize_centres`, with |p| < 2**27 and n <= 2**24; labels, int32, one per
point; C classes, 1 <= C <= 14; a radius r in half pixels, an integer with 1 <= r <= 512, and D = 2 r the diameter; by_class in {0, 1} with
the meaning it has in proximity.py: candidates and witnesses all carry one label, by plain equality (also for labels outside 0..C-1).

Candidates.  A CANDIDATE is a pair i < j with d2(i, j) <= D * D, inclusive.  Put q = p_j - p_i and d2 = |q|**2.  The circles through both
ends have the centres (q + t q_perp) / 2 with q_perp = (-q_y, q_x) and t real, and the squared radius d2 (1 + t**2) / 4.  Such a circle has
radius <= r exactly when t**2 <= (D**2 - d2) / d2 = T**2.

Witnesses.  A WITNESS k != i, j at rho = p_k - p_i has s = q x rho = q_x rho_y - q_y rho_x and m = rho . (rho - q).  k lies strictly inside
circle t exactly when t s > m:
  * s > 0: k allows t <= m / s.
  * s < 0: k allows t >= m / s.
  * s = 0 and m < 0: k lies strictly between the ends and BLOCKS the pair outright.
  * s = 0 and m >= 0: k does not bind.  A witness coincident with an end is such a witness.

Bounds and edges.  hi is the smallest bound of the first kind, or open; lo is the largest bound of the second kind, or open.  The pair is an
EDGE exactly when it is not blocked, hi >= -T, lo <= T and lo <= hi -- all three inclusive, so four cocircular points keep both diagonals,
each with lo = hi, and no tie rule is needed ("no point strictly inside", as in proximity.py).
  * apex[e, 0] is the smallest row k that attains hi, when hi <= T; otherwise -1.  apex[e, 1] is the same for lo, when lo >= -T.  An apex is
    the third corner of a triangle with an empty circumcircle of radius <= r on that side of the edge.
  * An edge is GABRIEL when no witness has m < 0: m < 0 is d2(i, k) + d2(j, k) < d2(i, j), proximity.py's rule verbatim.
  * A coincident pair (d2 = 0) is an edge with both sides open and the Gabriel flag set; no witness is consulted.  m coincident points are a
    clique, so the edge count is not bounded by a multiple of n.

Why a grid suffices on the device.  A witness that binds within [-T, T], or kills the pair, lies on or inside a circle of radius <= r
through both ends, so it lies within D of i AND of j: a grid of side >= D and the 3 x 3 cells around i hold it.  A witness farther than D
from either end changes neither the verdict nor an apex (its bound lies beyond T on its own side); device and restatement both pass it
over, and tests/test_alpha_host.py holds the restatement against a loop over EVERY row in Python fractions.  Unlike the Gabriel test, a
binding witness may lie farther from i than j does.

Why int64 suffices.  For every witness that is not passed over |rho| <= D and |rho - q| <= D, so |s| <= D**2 and |m| <= D**2 with
D**2 <= 2**20.  Comparing m1 / s1 with m2 / s2 cross-multiplies to below 2**40.  Comparing m / s with +-T is a sign test followed by
m**2 d2 <= s**2 (D**2 - d2), both sides below 2**60.  csrc/cellgrid_host.h has the same argument beside the predicates.

Outputs, integers only.
  edges         int32 (m, 2)  the edges (i, j) with i < j, in ascending (i, j) order
  edge_d2       int32 (m,)    the squared length of each edge, half pixels squared
  apex          int32 (m, 2)  the rows above, or -1
  edge_gabriel  uint8 (m,)    1 for a Gabriel edge
  degree        int32 (n, 2)  the alpha and the Gabriel edges at every row
  m, m_gabriel

The result is a pure function of the rows in their order.  `alpha_reference` is the brute-force int64 restatement (every candidate against
every row, no grid): the oracle the device result must EQUAL.  `derive` makes the float64 side on the host."""
import numpy as np

from . import cellpoints
from .cellpoints import COORD_LIMIT, MAX_CLASSES, MAX_POINTS, centres, half_pixel_radius, quantize_centres  # noqa: F401 (re-exported)

MAX_R = 512                           # half pixels: D = 2 r <= 1024 keeps every compare in int64
INT_NAMES = ('edges', 'edge_d2', 'apex', 'edge_gabriel', 'degree')
DERIVED_KEYS = ('edge_len_px', 'voronoi_px', 'edge_kind', 'triangles', 'triangle_area_px2', 'triangle_circumradius_px', 'class_edge_count',
                'outline_class_count', 'on_outline', 'n_edges', 'n_gabriel', 'n_triangles', 'n_degenerate', 'alpha_area_px2')
NPZ_KEYS = ('nuclei_id', 'xy', 'label') + INT_NAMES + DERIVED_KEYS + ('radius_px', 'by_class')
BY = {'any': 0, 'class': 1}


def check_args(num_classes, r, by_class):
    """num_classes 1..14, r 1..512 half pixels, by_class 0 or 1: ValueError otherwise."""
    whole = all(float(v) == int(v) for v in (num_classes, r, by_class))
    if not (whole and 1 <= int(num_classes) <= MAX_CLASSES and 1 <= int(r) <= MAX_R and int(by_class) in (0, 1)):
        raise ValueError(f'alpha: num_classes 1..{MAX_CLASSES}, r 1..{MAX_R} half pixels (at most {MAX_R // 2} px), by_class 0 or 1 '
                         f'(got num_classes={num_classes}, r={r}, by_class={by_class})')


def first_edge_cap(n):
    """The rows of capacity of `build`'s first call: a triangulation has fewer than 3 n edges, a lattice that keeps both diagonals of every
    cell fewer than 4 n; coincident and many cocircular points add to that."""
    return cellpoints.first_edge_cap(n, 4)


def _smallest(num, den, valid, rows):
    """Per line of the (e, w) tables: the smallest fraction num / den (den > 0) among the `valid` entries, and the smallest of `rows` (w,)
    that attains it -> (num, den, row), each (e,), with den = 0 and row = -1 where a line has no valid entry.  Exact: a tournament over
    the columns that compares by cross-multiplication (|num|, den <= 2**20 where valid)."""
    e, w = num.shape
    width = 1
    while width < max(w, 1):
        width *= 2
    none = np.iinfo(np.int64).max
    a = np.ones((e, width), np.int64); b = np.zeros((e, width), np.int64); k = np.full((e, width), none, np.int64)
    a[:, :w] = np.where(valid, num, 1); b[:, :w] = np.where(valid, den, 0); k[:, :w] = np.where(valid, rows[None, :], none)
    while width > 1:
        width //= 2
        a0, b0, k0, a1, b1, k1 = a[:, :width], b[:, :width], k[:, :width], a[:, width:2 * width], b[:, width:2 * width], k[:, width:2 * width]
        left, right = a0 * b1, a1 * b0
        second = (right < left) | ((right == left) & (k1 < k0))
        a, b, k = np.where(second, a1, a0), np.where(second, b1, b0), np.where(second, k1, k0)
    a, b, k = a[:, 0], b[:, 0], k[:, 0]
    return np.where(b > 0, a, 0), b, np.where(b > 0, k, -1)


def _within(a, b, d2, D2):
    """|a / b| <= T for b > 0, elementwise in int64: a**2 d2 <= b**2 (D**2 - d2)."""
    return a * a * d2 <= b * b * (D2 - d2)


def alpha_reference(points, labels, num_classes, r, by_class):
    """The definition in int64: points int (n, 2) half pixels, labels int (n,), r in HALF pixels ->
    (edges int32 (m, 2), edge_d2 int32 (m,), apex int32 (m, 2), edge_gabriel uint8 (m,), degree int32 (n, 2), m, m_gabriel).  Every
    candidate against EVERY row as a witness, no grid: rows in blocks of 256 and the candidates of a block 1024 at a time; a row farther
    than D from every row of the block is farther than D from an end of each of its candidates and is dropped from the block's tables
    before they are built.  Meant for a few thousand points (more when they are spread out)."""
    check_args(num_classes, r, by_class)
    p, lab = cellpoints.reference_points(points, labels, 'alpha_reference')
    n, D2, by_class = len(p), (2 * int(r)) ** 2, int(by_class)
    idx = np.arange(n, dtype=np.int64)
    ii, jj, dd, aa, gg = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros((0, 2), np.int64)], [np.zeros(0, bool)]
    for rows, d2 in cellpoints.pair_blocks(p, 64):
        cand = d2 <= D2
        cols = np.flatnonzero(cand.any(0))                                    # the rows within D of some row of the block
        if by_class:
            cand &= lab[rows, None] == lab[None, :]
        cand &= rows[:, None] < idx[None, :]
        a, j = np.nonzero(cand)                                               # row-major: ascending (i, j)
        for c0 in range(0, len(a), 1024):
            ac, jc = a[c0:c0 + 1024], j[c0:c0 + 1024]
            i = rows[ac]
            dij = d2[ac, jc]
            q = p[jc] - p[i]
            rho = p[None, cols, :] - p[i, None, :]                            # (e, w, 2): from i to every row kept
            u = rho - q[:, None, :]                                           # from j
            valid = ((rho ** 2).sum(2) <= D2) & ((u ** 2).sum(2) <= D2) & (cols[None, :] != i[:, None]) & (cols[None, :] != jc[:, None])
            valid &= dij[:, None] > 0                                         # a coincident pair consults no witness
            if by_class:
                valid &= lab[None, cols] == lab[i, None]
            s = np.where(valid, q[:, None, 0] * rho[:, :, 1] - q[:, None, 1] * rho[:, :, 0], 0)      # |s|, |m| <= D**2 where valid
            m = np.where(valid, (rho * u).sum(2), 0)
            blocked = (valid & (s == 0) & (m < 0)).any(1)
            gabriel = ~(valid & (m < 0)).any(1)
            hn, hd, hk = _smallest(m, s, valid & (s > 0), cols)               # hi = hn / hd
            ln, ld, lk = _smallest(m, -s, valid & (s < 0), cols)              # the smallest m / (-s) is minus the largest m / s
            ln = -ln                                                          # lo = ln / ld
            hi_ge = (hd == 0) | (hn >= 0) | _within(hn, hd, dij, D2)          # hi >= -T
            hi_le = (hd > 0) & ((hn <= 0) | _within(hn, hd, dij, D2))         # hi <= T, and not open
            lo_le = (ld == 0) | (ln <= 0) | _within(ln, ld, dij, D2)          # lo <= T
            lo_ge = (ld > 0) & ((ln >= 0) | _within(ln, ld, dij, D2))         # lo >= -T, and not open
            edge = ~blocked & hi_ge & lo_le & ((hd == 0) | (ld == 0) | (ln * hd <= hn * ld))
            apex = np.stack([np.where(hi_le, hk, -1), np.where(lo_ge, lk, -1)], 1)
            ii.append(i[edge]); jj.append(jc[edge]); dd.append(dij[edge]); aa.append(apex[edge]); gg.append(gabriel[edge])
    ii, jj, dd, aa, gg = np.concatenate(ii), np.concatenate(jj), np.concatenate(dd), np.concatenate(aa), np.concatenate(gg)
    edges = np.stack([ii, jj], 1).astype(np.int32).reshape(-1, 2)
    degree = np.stack([np.bincount(edges.reshape(-1), minlength=n), np.bincount(edges[gg].reshape(-1), minlength=n)], 1).astype(np.int32).reshape(n, 2)
    return edges, dd.astype(np.int32), aa.astype(np.int32).reshape(-1, 2), gg.astype(np.uint8), degree, len(ii), int(gg.sum())


def call(points, labels, num_classes, r, by_class, edge_cap, edges, edge_d2, apex, edge_gabriel, degree, bounds=None, device=0):
    """nuhtc_cell_alpha on torch tensors of cuda:`device` (contiguous; edges and apex int32 (edge_cap, 2), edge_d2 int32 and edge_gabriel
    uint8 (edge_cap,), degree int32 (n, 2); r in HALF pixels) -> (the library's return code, m, m_gabriel), nothing raised: the code is 0
    or hip.E_INVALID / hip.E_HIP; m and m_gabriel are None unless the code is 0.  With m > edge_cap the four edge arrays are untouched
    (degree is written): call again with edge_cap >= m.  bounds = (x_min, y_min, x_max, y_max) of the points, computed on the host when
    not given."""
    import ctypes
    m, m_gab = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = cellpoints.launch('nuhtc_cell_alpha', device, points, labels, (int(num_classes), int(r), int(by_class), int(edge_cap)),
                           (edges, edge_d2, apex, edge_gabriel, degree), bounds, extra=(ctypes.byref(m), ctypes.byref(m_gab)))
    return (rc,) + ((int(m.value), int(m_gab.value)) if rc == 0 else (None, None))


def outputs(n, edge_cap, device, fill=0):
    """The five output tensors of `call` for n points and edge_cap rows of capacity on `device` (one row at least each), every entry `fill`."""
    import torch
    cap, n = max(int(edge_cap), 1), max(int(n), 1)
    return [torch.full(s, fill, dtype=t, device=device) for s, t in (((cap, 2), torch.int32), ((cap,), torch.int32), ((cap, 2), torch.int32),
                                                                     ((cap,), torch.uint8), ((n, 2), torch.int32))]


def build(points, labels, num_classes, radius_px, by_class=0, device=0, with_calls=False):
    """The alpha complex of `points` (int (n, 2) half pixels, see cellpoints.quantize_centres) with `labels` (n,) at `radius_px` on
    cuda:`device`: numpy in, the seven results of `alpha_reference` out, and the number of device calls it took behind them when
    `with_calls`.  The first call has room for `first_edge_cap(n)` edges; when there are more (many coincident or cocircular points) the
    device says how many and writes no edge, and ONE second call has room for exactly that many.  There is no host route: without the
    library or a GPU this raises."""
    C, r = int(num_classes), half_pixel_radius(radius_px)
    check_args(C, r, by_class)
    p, lab, dev, p_d, lab_d, bounds = cellpoints.resident(points, labels, 'alpha', device)
    n = len(p)
    out, m, (m_gab,), calls = cellpoints.grow_to_fit(
        lambda cap, out: call(p_d, lab_d, C, r, int(by_class), cap, *out, bounds=bounds, device=device),
        lambda cap: outputs(n, cap, dev), first_edge_cap(n), 'nuhtc_cell_alpha', 'alpha')
    got = tuple(t[:m].cpu().numpy() for t in out[:4]) + (out[4][:n].cpu().numpy(), m, m_gab)
    return got + (calls,) if with_calls else got


def _bounds_of_apexes(p, e, apex):
    """-> (s, m) int64 (len(e), 2) of the two apexes of every edge (0 where there is none): the bound of side c is m[:, c] / s[:, c]."""
    q = p[e[:, 1]] - p[e[:, 0]]
    s, m = np.zeros((len(e), 2), np.int64), np.zeros((len(e), 2), np.int64)
    for c in (0, 1):
        has = apex[:, c] >= 0
        rho = p[apex[has, c]] - p[e[has, 0]]
        s[has, c] = q[has, 0] * rho[:, 1] - q[has, 1] * rho[:, 0]
        m[has, c] = (rho * (rho - q[has])).sum(1)
    return s, m


def derive(edges, edge_d2, apex, edge_gabriel, degree, points, labels, num_classes, r):
    """The float64 side of the integers (points int (n, 2) half pixels, r in HALF pixels) -> dict:
      edge_len_px               float64 (m,)    sqrt(edge_d2) / 2
      voronoi_px                float64 (m,)    the length of the pair's Voronoi edge inside the radius, |q| (min(hi, T) - max(lo, -T)) / 4 px
                                                with hi and lo recomputed from the apexes (a side without an apex ends at +-T): the continuous
                                                counterpart of adjacency.py's `shared`.  0 for a coincident pair
      edge_kind                 uint8 (m,)      the apexes an edge has: 0 a singular edge (no triangle), 1 an edge on the outline of the alpha
                                                shape, 2 an interior edge
      triangles                 int32 (t, 3)    the distinct sorted triples (i, j, apex), in ascending order
      triangle_area_px2         float64 (t,)
      triangle_circumradius_px  float64 (t,)    at most r / 2 px, up to rounding
      class_edge_count          int64 (C, C)    the edges by [min label, max label] of their ends (upper triangle); an edge touching a label
      outline_class_count       int64 (C, C)    outside 0..C-1 is counted nowhere.  The same over the edges of kind 1
      on_outline                uint8 (n,)      1 for a row at an end of an edge of kind 1
      n_edges, n_gabriel, n_triangles           int64 0-d
      n_degenerate              int64 0-d       the edges with two apexes and lo = hi (decided in integers): the diagonals of cocircular points
      alpha_area_px2            float64 0-d     the sum of triangle_area_px2
    Without cocircular quadruples `triangles` are exactly the Delaunay triangles of circumradius <= r.  With cocircular points BOTH
    diagonals of a cocircular quadruple are edges, so triangles overlap and alpha_area_px2 counts the overlap more than once:
    n_degenerate tells which case a slide is (0: a triangulation; otherwise the number of such diagonals)."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    d2 = np.asarray(edge_d2, np.int64).reshape(-1)
    ap = np.asarray(apex, np.int64).reshape(-1, 2)
    gab = np.asarray(edge_gabriel).reshape(-1).astype(bool)
    deg = np.asarray(degree, np.int64).reshape(-1, 2)
    p = np.asarray(points, np.int64).reshape(-1, 2)
    lab = np.asarray(labels, np.int64).reshape(-1)
    C, n, m, D2 = int(num_classes), len(lab), len(d2), (2 * int(r)) ** 2
    if len(e) != m or len(gab) != m or len(ap) != m or len(deg) != n or len(p) != n or (m and (e.min() < 0 or e.max() >= n or ap.min() < -1 or ap.max() >= n)):
        raise ValueError('derive: one d2, one apex row and one Gabriel flag per edge, one point, one label and one degree row per nucleus, edges between rows')
    if not (np.array_equal(deg[:, 0], np.bincount(e.reshape(-1), minlength=n)) and np.array_equal(deg[:, 1], np.bincount(e[gab].reshape(-1), minlength=n))):
        raise ValueError('derive: degree is not the number of edges at every row')
    if not np.array_equal(d2, ((p[e[:, 1]] - p[e[:, 0]]) ** 2).sum(1)) or (d2 > D2).any():
        raise ValueError('derive: edge_d2 is not the squared distance of the points, or an edge is longer than 2 r')
    length = np.sqrt(d2.astype(np.float64)) / 2
    s, mm = _bounds_of_apexes(p, e, ap)
    if (s[:, 0] < 0).any() or (s[:, 1] > 0).any() or ((ap >= 0) & (s == 0)).any():
        raise ValueError('derive: apex[:, 0] lies on the left of i -> j, apex[:, 1] on the right')
    has = ap >= 0
    both = has.all(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        T = np.where(d2 > 0, np.sqrt((D2 - d2) / np.maximum(d2, 1).astype(np.float64)), 0.0)
        hi = np.where(has[:, 0], mm[:, 0] / np.where(has[:, 0], s[:, 0], 1).astype(np.float64), T)
        lo = np.where(has[:, 1], mm[:, 1] / np.where(has[:, 1], s[:, 1], 1).astype(np.float64), -T)
        span = hi - lo
        num = mm[:, 0] * s[:, 1] - mm[:, 1] * s[:, 0]                         # hi - lo = num / (s0 s1) when both sides have an apex: one rounding
        span[both] = num[both] / (s[both, 0] * s[both, 1]).astype(np.float64)
    voronoi = np.where(d2 > 0, np.sqrt(d2.astype(np.float64)) * np.maximum(span, 0.0) / 4, 0.0)
    kind = has.sum(1).astype(np.uint8)
    tri = np.concatenate([np.column_stack([e[has[:, c]], ap[has[:, c], c]]) for c in (0, 1)]) if m else np.zeros((0, 3), np.int64)
    tri = np.unique(np.sort(tri, 1), axis=0).reshape(-1, 3)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    cross = np.abs((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]))      # twice the area, half pixels squared
    area = cross / 8.0
    sides = [((x - y) ** 2).sum(1).astype(np.float64) for x, y in ((a, b), (b, c), (a, c))]
    radius = np.sqrt(sides[0]) * np.sqrt(sides[1]) * np.sqrt(sides[2]) / (2.0 * np.maximum(cross, 1)) / 2
    la, lb = lab[e[:, 0]], lab[e[:, 1]]
    outline = kind == 1
    on = np.zeros(n, np.uint8)
    on[e[outline].reshape(-1)] = 1
    return dict(edge_len_px=length, voronoi_px=voronoi, edge_kind=kind, triangles=tri.astype(np.int32), triangle_area_px2=area,
                triangle_circumradius_px=radius, class_edge_count=cellpoints.class_pair_census(la, lb, C),
                outline_class_count=cellpoints.class_pair_census(la[outline], lb[outline], C), on_outline=on,
                n_edges=np.asarray(m, np.int64), n_gabriel=np.asarray(int(gab.sum()), np.int64), n_triangles=np.asarray(len(tri), np.int64),
                n_degenerate=np.asarray(int((both & (num == 0)).sum()), np.int64), alpha_area_px2=np.asarray(float(area.sum()), np.float64))


def write_npz(path, nuclei_id, xy, label, edges, edge_d2, apex, edge_gabriel, degree, num_classes, radius_px, by_class):
    """<id>_nuclei_alpha.npz, row i for the i-th row of <id>_nuclei_graph.npz / <id>_nuclei_feat.npz:
      nuclei_id int64 (n,), xy float64 (n, 2) (the unquantised centre in slide px), label int64 (n,)
      edges int32 (m, 2) (rows of this file), edge_d2 int32 (m,), apex int32 (m, 2), edge_gabriel uint8 (m,), degree int32 (n, 2): the
      integers of the definition, on the half-pixel points rint(2 xy)
      the arrays of `derive` (DERIVED_KEYS), and radius_px float64, by_class int64 as 0-d arrays."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    n = len(head['label'])
    edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
    edge_d2 = np.ascontiguousarray(edge_d2, np.int32).reshape(-1)
    apex = np.ascontiguousarray(apex, np.int32).reshape(-1, 2)
    edge_gabriel = np.ascontiguousarray(edge_gabriel, np.uint8).reshape(-1)
    degree = np.ascontiguousarray(degree, np.int32).reshape(-1, 2)
    if len(degree) != n or not len(edges) == len(edge_d2) == len(apex) == len(edge_gabriel):
        raise ValueError('write_npz: one degree row per nucleus, one d2, one apex row and one Gabriel flag per edge')
    cellpoints.check_edge_rows(edges, n)
    r = half_pixel_radius(radius_px)
    check_args(num_classes, r, by_class)
    d = derive(edges, edge_d2, apex, edge_gabriel, degree, np.rint(2 * head['xy']).astype(np.int64), head['label'], num_classes, r)
    with open(path, 'wb') as f:
        np.savez(f, **head, edges=edges, edge_d2=edge_d2, apex=apex, edge_gabriel=edge_gabriel, degree=degree,
                 radius_px=np.asarray(float(radius_px), np.float64), by_class=np.asarray(int(by_class), np.int64), **d)
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)
