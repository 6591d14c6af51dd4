"""The alpha shape of a slide's nuclei as POLYGONS: the rings that bound the triangles of the alpha complex, and the components they
bound -- the step alphacomplex.py stops short of.  `alphacomplex.derive` flags the edges on the outline and sums the area; this module
links those edges into closed rings, tells outer rings from holes, says which rings belong to one piece of material, and writes the
pieces as a GeoJSON of regions that regions.py and margin.py read: "the tumour bed is the alpha shape of the tumour nuclei", handed to
the project's own census and margin analyses in a later run.  Computed on the GPU (csrc/celloutline.hip, `nuhtc_alpha_outline`, on the
tensors `nuhtc_cell_alpha` left on the device); tools/infer_wsi.py --nuclei-outline writes <id>_nuclei_outline.npz and
<id>_nuclei_outline.geojson.  Not in the reference.

Definition.

Input.  The points (int32 (n, 2) half pixels, |p| < 2**27, n <= 2**24), the labels, and the integer outputs of the alpha complex at
(r, by_class): edges (m, 2) in ascending (i, j) order, edge_d2 (m,) and apex (m, 2) -- edge_gabriel and degree are not consulted --
with m <= 2**24 on the device (its scans over the edges).

Representatives.  A row is a REPRESENTATIVE unless it is the larger end of an edge with edge_d2 == 0, that is, unless a smaller row lies
on the same half-pixel position (with by_class: a smaller row of the same label; the alpha complex joins no others).  An edge with an
end that is no representative is SET ASIDE: it repeats the geometry of the representatives' edge, and the apexes already name smallest
rows.  The KEPT edges are the alpha complex of the distinct positions (tests/test_outline_host.py holds them against `alpha_reference`
of the representatives alone).

Half-edges.  A kept edge with exactly one apex is an OUTLINE edge.  It gives one half-edge, directed with the apex -- the material --
on its left: i -> j when apex[e, 0] >= 0, otherwise j -> i.  Its id is the edge's index e.  ("Left" is the side where (head - tail) x
(k - tail) > 0 with x to the right and y as stored.)

Successor.  The successor of u -> v is the outline half-edge v -> w met first when turning CLOCKWISE from the direction a = u - v; that
turns through the material.  With b = w - v the clockwise angle from a to b is classed by the signs of a x b and a . b -- strictly
between 0 and pi (a x b < 0), pi (a x b == 0, a . b < 0), beyond pi (a x b > 0) -- and within one open half-turn b1 comes before b2
exactly when b1 x b2 < 0.  The vectors are no longer than D = 2 r <= 1024, every product is below 2**21: int64-exact (for any points
with |p| < 2**27 the products stay below 2**57).  No two out-half-edges at a vertex share a direction: the farther end would be blocked
by the nearer.  Under this rule a ring bounds ONE wedge of triangles at a pinch vertex, never the union of two.  The map is a
bijection (the mirror rule, counter-clockwise from v -> w among the in-half-edges, gives the predecessor); `outline_reference` asserts it.

Rings.  The RINGS are the cycles of the successor map.  A ring's leader is its smallest half-edge id; the ring is written from the tail
of the leader onward; rings are ordered by leader.  ring_area2 is the shoelace sum (v_t - o) x (v_t+1 - o) in half pixels squared with
o the leader's tail: positive for an outer ring (counter-clockwise, y as stored), negative for a hole.  |2 A| < 2**58; the device adds
the terms in wrap-around unsigned 64-bit arithmetic, where the total fits and the order of the adds does not matter.

Components.  Two kept edges with at least one apex are JOINED when they are sides of one triangle (i, j, apex): the edge (i, j) with
(i, k) and (j, k) for each of its apexes k.  This connects triangles across interior edges and never through a vertex alone.  A
COMPONENT is numbered by the rank of its smallest edge index.  component_of_ring is the component of the ring's edges.  `component`
(n,) is the SMALLEST component among the apexed kept edges at a representative (a pinch vertex lies in more than one), -1 for a row in
no triangle; a row that is no representative takes its representative's value.  Every component has exactly one ring of positive
area (its outer boundary; the others are its holes); `outline_reference` checks it.

Outputs, all integers.
  ring_vertex        int32 (h,)      the rows in ring order, rings concatenated
  ring_start         int32 (R + 1,)  where each ring begins in ring_vertex
  ring_area2         int64 (R,)      signed twice-area of each ring, half pixels squared
  component_of_ring  int32 (R,)      the component of each ring
  component          int32 (n,)      the component of each row, or -1
  component_label    int32 (K,)      with by_class the label the rows of the component share, else -1
  h, R, K

The result is a pure function of the rows in their order.  `outline_reference` is the brute-force restatement, a plain walk in Python
integers: the oracle the device result must EQUAL.  `derive` makes the float64 side on the host.  A ring that touches itself at a pinch
vertex is written as it is: it is legal for the even-odd rule of regions.py, and is not repaired."""
import json

import numpy as np

from . import alphacomplex, cellpoints
from .alphacomplex import BY, MAX_R  # noqa: F401 (re-exported)
from .cellpoints import COORD_LIMIT, MAX_CLASSES, MAX_POINTS, centres, half_pixel_radius, quantize_centres  # noqa: F401 (re-exported)

MAX_EDGES = 1 << 24                   # of one device call (csrc/cellgrid_host.h OUTLINE_MAX_EDGES)
INT_NAMES = ('ring_vertex', 'ring_start', 'ring_area2', 'component_of_ring', 'component', 'component_label')
INT_TYPES = (np.int32, np.int32, np.int64, np.int32, np.int32, np.int32)
DERIVED_KEYS = ('area_px2', 'hole_area_px2', 'perimeter_px', 'n_holes', 'n_nuclei', 'class_count', 'n_components', 'n_rings', 'largest_component',
                'area_share_by_label')
NPZ_KEYS = ('nuclei_id', 'xy', 'label') + INT_NAMES + DERIVED_KEYS + ('radius_px', 'by_class')
GEOJSON_SUFFIX = '.geojson'           # write_npz writes <path without .npz>.geojson beside the .npz


def check_args(num_classes, r, by_class, min_nuclei=0):
    """The arguments of the alpha complex (alphacomplex.check_args) and min_nuclei, a whole number >= 0: ValueError otherwise."""
    alphacomplex.check_args(num_classes, r, by_class)
    if float(min_nuclei) != int(min_nuclei) or int(min_nuclei) < 0:
        raise ValueError(f'outline: min_nuclei is a whole number >= 0 (got {min_nuclei})')


def turn_class(a, b):
    """The class of the clockwise angle from a to b (pairs of Python integers): 0 the same direction, 1 below pi, 2 pi, 3 beyond pi."""
    cr = a[0] * b[1] - a[1] * b[0]
    if cr:
        return 1 if cr < 0 else 3
    return 2 if a[0] * b[0] + a[1] * b[1] < 0 else 0


def turn_before(a, b1, b2):
    """Is b1 met strictly before b2 when turning clockwise from a?"""
    c1, c2 = turn_class(a, b1), turn_class(a, b2)
    if c1 != c2:
        return c1 < c2
    return bool(c1 & 1) and b1[0] * b2[1] - b1[1] * b2[0] < 0


def _as_complex(points, labels, edges, edge_d2, apex, what):
    p, lab = cellpoints.reference_points(points, labels, what)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    d2 = np.asarray(edge_d2, np.int64).reshape(-1)
    ap = np.asarray(apex, np.int64).reshape(-1, 2)
    n, m = len(p), len(e)
    if len(d2) != m or len(ap) != m:
        raise ValueError(f'{what}: one d2 and one apex row per edge')
    if m and (e.min() < 0 or e.max() >= n or (e[:, 0] >= e[:, 1]).any() or ap.min() < -1 or ap.max() >= n):
        raise ValueError(f'{what}: an edge is (i, j) with i < j, both rows; an apex is a row or -1')
    if m > 1 and not ((e[1:, 0] > e[:-1, 0]) | ((e[1:, 0] == e[:-1, 0]) & (e[1:, 1] > e[:-1, 1]))).all():
        raise ValueError(f'{what}: the edges are in ascending (i, j) order')
    s, _ = alphacomplex._bounds_of_apexes(p, e, ap)
    if ((ap[:, 0] >= 0) & (s[:, 0] <= 0)).any() or ((ap[:, 1] >= 0) & (s[:, 1] >= 0)).any():
        raise ValueError(f'{what}: apex[:, 0] lies on the left of i -> j, apex[:, 1] on the right')
    return p, lab, e, d2, ap


def representatives(n, edges, edge_d2):
    """-> int64 (n,): the smallest row on the same place, from the edges with d2 == 0 (a row's own index for a representative)."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    zero = np.asarray(edge_d2).reshape(-1) == 0
    rep = np.arange(int(n), dtype=np.int64)
    np.minimum.at(rep, e[zero, 1], e[zero, 0])
    return rep


def half_edges(edges, edge_d2, apex, n):
    """-> (ids int64 (h,) the outline edges in ascending order, tail int64 (h,), head int64 (h,), kept bool (m,), rep int64 (n,))."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    ap = np.asarray(apex, np.int64).reshape(-1, 2)
    rep = representatives(n, e, edge_d2)
    kept = (rep[e[:, 0]] == e[:, 0]) & (rep[e[:, 1]] == e[:, 1]) if len(e) else np.zeros(0, bool)
    has = ap >= 0
    ids = np.flatnonzero(kept & (has.sum(1) == 1))
    left = has[ids, 0]
    return ids, np.where(left, e[ids, 0], e[ids, 1]), np.where(left, e[ids, 1], e[ids, 0]), kept, rep


def outline_reference(points, labels, edges, edge_d2, apex, by_class=0):
    """The definition as a plain walk: points int (n, 2) half pixels, labels int (n,), the edges, edge_d2 and apex of the alpha complex ->
    (ring_vertex int32 (h,), ring_start int32 (R + 1,), ring_area2 int64 (R,), component_of_ring int32 (R,), component int32 (n,),
    component_label int32 (K,), h, R, K).  Every decision in Python integers.  AssertionError when the successor map is no bijection or
    a component has not exactly one ring of positive area: the input is no alpha complex then.  Meant for up to some 10**5 edges."""
    if int(by_class) not in (0, 1):
        raise ValueError(f'outline_reference: by_class 0 or 1 (got {by_class})')
    p, lab, e, d2, ap = _as_complex(points, labels, edges, edge_d2, apex, 'outline_reference')
    n, m = len(p), len(e)
    ids, tail, head, kept, rep = half_edges(e, d2, ap, n)
    P = [tuple(v) for v in p.tolist()]
    ids_l, tail_l, head_l = ids.tolist(), tail.tolist(), head.tolist()
    out_at = {}
    for x, t in zip(ids_l, tail_l):
        out_at.setdefault(t, []).append(x)
    tail_of, head_of = dict(zip(ids_l, tail_l)), dict(zip(ids_l, head_l))
    succ = {}
    for x in ids_l:
        u, v = tail_of[x], head_of[x]
        a = (P[u][0] - P[v][0], P[u][1] - P[v][1])
        best, bb = None, None
        for y in out_at.get(v, ()):
            w = head_of[y]
            b = (P[w][0] - P[v][0], P[w][1] - P[v][1])
            assert turn_class(a, b) != 0, f'half-edge {y} leaves {v} in the direction of {u}'
            if best is None or turn_before(a, b, bb):
                best, bb = y, b
            else:
                assert turn_before(a, bb, b), f'half-edges {y} and {best} leave {v} in one direction'
        assert best is not None, f'no half-edge leaves {v}, the head of half-edge {x}'
        succ[x] = best
    assert len(set(succ.values())) == len(ids_l), 'the successor map is no bijection'
    rings, area2, leaders, seen = [], [], [], set()
    for x in ids_l:                                       # ascending: x is the smallest id of its cycle
        if x in seen:
            continue
        ring, y = [], x
        while y not in seen:
            seen.add(y)
            ring.append(y)
            y = succ[y]
        o, s = P[tail_of[x]], 0
        for y in ring:
            a, b = P[tail_of[y]], P[head_of[y]]
            s += (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
        rings.append([tail_of[y] for y in ring]); area2.append(s); leaders.append(x)
    # the components: union-find over the edge indices
    napex = (ap >= 0).sum(1)
    live = kept & (napex > 0)
    index = {tuple(ij): k for k, ij in enumerate(e.tolist())}
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    live_l, e_l, ap_l = live.tolist(), e.tolist(), ap.tolist()
    for k in range(m):
        if not live_l[k]:
            continue
        for apx in ap_l[k]:
            if apx < 0:
                continue
            for end in e_l[k]:
                f = index.get((min(end, apx), max(end, apx)))
                if f is not None and live_l[f]:
                    a, b = find(k), find(f)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    root = np.asarray([find(k) if live_l[k] else -1 for k in range(m)], np.int64).reshape(-1)
    roots = np.unique(root[root >= 0])                    # ascending: the rank of the smallest edge index
    comp_of_edge = np.where(root >= 0, np.searchsorted(roots, np.maximum(root, 0)), -1)
    K = len(roots)
    big = np.iinfo(np.int64).max
    comp = np.full(n, big, np.int64)
    for c in (0, 1):
        np.minimum.at(comp, e[live, c], comp_of_edge[live])
    comp = np.where(comp == big, -1, comp)[rep]
    comp_label = lab[e[roots, 0]] if int(by_class) else np.full(K, -1, np.int64)
    comp_of_ring = comp_of_edge[np.asarray(leaders, np.int64)] if leaders else np.zeros(0, np.int64)
    positive = np.bincount(comp_of_ring[np.asarray([s > 0 for s in area2], bool)], minlength=K) if leaders else np.zeros(K, np.int64)
    assert (positive == 1).all() and (comp_of_ring >= 0).all(), 'a component has not exactly one ring of positive area'
    start = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
    vertex = np.asarray([v for r in rings for v in r], np.int32).reshape(-1)
    return (vertex, start, np.asarray(area2, np.int64).reshape(-1), comp_of_ring.astype(np.int32), comp.astype(np.int32), comp_label.astype(np.int32),
            len(vertex), len(rings), K)


# ---- the device
def outputs(n, m, device, fill=0):
    """The six output tensors of `call` for n points and m edges on `device` (one row at least each), every entry `fill`."""
    import torch
    m, n = max(int(m), 1), max(int(n), 1)
    shapes = ((m,), torch.int32), ((m + 1,), torch.int32), ((m,), torch.int64), ((m,), torch.int32), ((n,), torch.int32), ((m,), torch.int32)
    return [torch.full(s, fill, dtype=t, device=device) for s, t in shapes]


def call(points, labels, by_class, edges, edge_d2, apex, m, ring_vertex, ring_start, ring_area2, component_of_ring, component, component_label, device=0):
    """nuhtc_alpha_outline on torch tensors of cuda:`device` (contiguous; points, labels and the first m rows of edges, edge_d2 and apex as
    nuhtc_cell_alpha took and left them; the outputs as `outputs` makes them) -> (the library's return code, h, R, K), nothing raised: the
    code is 0 or hip.E_INVALID / hip.E_HIP; h, R and K are None unless the code is 0."""
    import ctypes
    import torch
    from . import hip
    fn = hip.load().nuhtc_alpha_outline
    counts = (ctypes.c_int64 * 3)(-1, -1, -1)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    dev = torch.device('cuda', device)
    with torch.cuda.device(dev):
        rc = fn(int(device), vp(points), vp(labels), int(points.shape[0]), int(by_class), vp(edges), vp(edge_d2), vp(apex), int(m), vp(ring_vertex),
                vp(ring_start), vp(ring_area2), vp(component_of_ring), vp(component), vp(component_label), counts,
                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return (rc,) + (tuple(int(c) for c in counts) if rc == 0 else (None, None, None))


def build(points, labels, num_classes, radius_px, by_class=0, min_nuclei=0, device=0, with_alpha=False):
    """The outline of the alpha complex of `points` (int (n, 2) half pixels) with `labels` (n,) at `radius_px` on cuda:`device`: numpy in,
    the nine results of `outline_reference` out, and behind them with `with_alpha` the seven results of `alphacomplex.build`.  The
    alpha complex is computed by `alphacomplex.call` with its capacity protocol (one call, or two when there are more edges than
    `first_edge_cap`); its tensors stay on the device and go to nuhtc_alpha_outline as they are.  The outline needs no capacity of its
    own: h, R, K <= m.  `min_nuclei` is checked and otherwise left to `write_npz` (it thins the GeoJSON only).  There is no host route:
    without the library or a GPU this raises."""
    C, r = int(num_classes), half_pixel_radius(radius_px)
    check_args(C, r, by_class, min_nuclei)
    p, lab, dev, p_d, lab_d, bounds = cellpoints.resident(points, labels, 'outline', device)
    n = len(p)
    cap = alphacomplex.first_edge_cap(n)
    for attempt in (0, 1):
        alpha = alphacomplex.outputs(n, cap, dev)
        rc, m, m_gab = alphacomplex.call(p_d, lab_d, C, r, int(by_class), cap, *alpha, bounds=bounds, device=device)
        cellpoints.raise_for(rc, 'nuhtc_cell_alpha')
        if m <= cap:
            break
        if attempt or m > MAX_EDGES:
            raise ValueError(f'outline: {m} edges, more than 2**24 (many coincident points)' if m > MAX_EDGES else f'nuhtc_cell_alpha: {m} edges on the second call')
        cap = m
    if m > MAX_EDGES:
        raise ValueError(f'outline: {m} edges, more than 2**24')
    out = outputs(n, m, dev)
    rc, h, R, K = call(p_d, lab_d, int(by_class), alpha[0], alpha[1], alpha[2], m, *out, device=device)
    cellpoints.raise_for(rc, 'nuhtc_alpha_outline')
    sizes = (h, R + 1, R, R, n, K)
    got = tuple(t[:k].cpu().numpy() for t, k in zip(out, sizes)) + (h, R, K)
    if with_alpha:
        got += tuple(t[:m].cpu().numpy() for t in alpha[:4]) + (alpha[4][:n].cpu().numpy(), m, m_gab)
    return got


# ---- the host side
def _as_outputs(ring_vertex, ring_start, ring_area2, component_of_ring, component, component_label):
    arrays = [np.ascontiguousarray(np.asarray(a).reshape(-1), t) for a, t in
              zip((ring_vertex, ring_start, ring_area2, component_of_ring, component, component_label), INT_TYPES)]
    rv, rs, ra, cr, comp, cl = arrays
    R, K, n = len(ra), len(cl), len(comp)
    if len(rs) != R + 1 or len(cr) != R or rs[0] != 0 or rs[-1] != len(rv) or (np.diff(rs) < 3).any():
        raise ValueError('outline: ring_start has one entry per ring and one more, from 0 to len(ring_vertex), and a ring has three vertices at least')
    if (len(rv) and (rv.min() < 0 or rv.max() >= n)) or (R and (cr.min() < 0 or cr.max() >= K)) or (n and (comp.min() < -1 or comp.max() >= K)):
        raise ValueError('outline: ring vertices are rows, components are 0..K-1 (or -1 for a row)')
    return arrays


def derive(ring_vertex, ring_start, ring_area2, component_of_ring, component, component_label, points, labels, num_classes):
    """The float64 side of the integers (points int (n, 2) half pixels) -> dict:
      area_px2             float64 (K,)    the area of the material of each component: the signed ring areas summed, / 8
      hole_area_px2        float64 (K,)    the area of its holes
      perimeter_px         float64 (K,)    the length of all its rings
      n_holes              int64 (K,)      its rings of negative area
      n_nuclei             int64 (K,)      the rows with `component` == k: every row, representative or not
      class_count          int64 (K, C)    the same by label; a label outside 0..C-1 is counted nowhere
      n_components, n_rings                int64 0-d
      largest_component    int64 0-d       the component of the largest area_px2 (the first of equals), -1 without any
      area_share_by_label  float64 (C,)    the share of the whole area that the components of each component_label hold (zeros when the
                                           alpha complex was not by class, or without any area)"""
    rv, rs, ra, cr, comp, cl = _as_outputs(ring_vertex, ring_start, ring_area2, component_of_ring, component, component_label)
    p = np.asarray(points, np.int64).reshape(-1, 2)
    lab = np.asarray(labels, np.int64).reshape(-1)
    C, K, R, n = int(num_classes), len(cl), len(ra), len(comp)
    if len(p) != n or len(lab) != n:
        raise ValueError('derive: one point and one label per row of `component`')
    signed, holes = np.zeros(K, np.int64), np.zeros(K, np.int64)
    np.add.at(signed, cr, ra)
    np.add.at(holes, cr[ra < 0], -ra[ra < 0])
    ring_of = np.repeat(np.arange(R), np.diff(rs))
    nxt = np.arange(len(rv)) + 1
    nxt[rs[1:] - 1] = rs[:-1]                              # the last place of a ring is followed by its first
    step = np.sqrt(((p[rv[nxt]] - p[rv]) ** 2).sum(1).astype(np.float64)) / 2 if len(rv) else np.zeros(0)
    perimeter = np.bincount(cr[ring_of], weights=step, minlength=K).astype(np.float64) if len(rv) else np.zeros(K)
    inside = comp >= 0
    known = inside & (lab >= 0) & (lab < C)
    counts = np.zeros((K, C), np.int64)
    np.add.at(counts, (comp[known], lab[known]), 1)
    area = signed / 8.0
    share = np.zeros(C, np.float64)
    if K and area.sum() > 0:
        named = (cl >= 0) & (cl < C)
        np.add.at(share, cl[named], area[named])
        share /= area.sum()
    return dict(area_px2=area, hole_area_px2=holes / 8.0, perimeter_px=perimeter, n_holes=np.bincount(cr[ra < 0], minlength=K).astype(np.int64),
                n_nuclei=np.bincount(comp[inside], minlength=K).astype(np.int64), class_count=counts, n_components=np.asarray(K, np.int64),
                n_rings=np.asarray(R, np.int64), largest_component=np.asarray(int(area.argmax()) if K else -1, np.int64), area_share_by_label=share)


def features(ring_vertex, ring_start, ring_area2, component_of_ring, component, component_label, points, min_nuclei=0):
    """The components as GeoJSON features (dicts), in component order: one Polygon each -- the outer ring first, then its holes in ring
    order; rings closed; slide pixels = half pixels / 2 -- with the properties name 'alpha-<k>', label, n_nuclei and area_px2.  A component
    with fewer than `min_nuclei` rows is left out."""
    rv, rs, ra, cr, comp, cl = _as_outputs(ring_vertex, ring_start, ring_area2, component_of_ring, component, component_label)
    p = np.asarray(points, np.int64).reshape(-1, 2)
    K = len(cl)
    nuclei = np.bincount(comp[comp >= 0], minlength=K)
    signed = np.zeros(K, np.int64)
    np.add.at(signed, cr, ra)
    feats = []
    for k in range(K):
        if nuclei[k] < int(min_nuclei):
            continue
        mine = np.flatnonzero(cr == k)
        mine = sorted(mine.tolist(), key=lambda ring: (ra[ring] <= 0, ring))     # the one ring of positive area first
        coords = []
        for ring in mine:
            v = p[rv[rs[ring]:rs[ring + 1]]]
            v = np.concatenate([v, v[:1]]) / 2.0
            coords.append(v.tolist())
        feats.append(dict(type='Feature', geometry=dict(type='Polygon', coordinates=coords),
                          properties=dict(name=f'alpha-{k}', label=int(cl[k]), n_nuclei=int(nuclei[k]), area_px2=float(signed[k] / 8.0))))
    return feats


def geojson_path(npz_path):
    path = str(npz_path)
    return (path[:-4] if path.endswith('.npz') else path) + GEOJSON_SUFFIX


def write_npz(path, nuclei_id, xy, label, ring_vertex, ring_start, ring_area2, component_of_ring, component, component_label, num_classes, radius_px,
              by_class, min_nuclei=0):
    """<id>_nuclei_outline.npz, row i for the i-th row of <id>_nuclei_graph.npz / <id>_nuclei_feat.npz:
      nuclei_id int64 (n,), xy float64 (n, 2) (the unquantised centre in slide px), label int64 (n,)
      the six integer arrays of the definition (INT_NAMES), on the half-pixel points rint(2 xy)
      the arrays of `derive` (DERIVED_KEYS), and radius_px float64, by_class int64 as 0-d arrays
    and beside it <id>_nuclei_outline.geojson, a FeatureCollection of `features` in the form regions.read_geojson reads; components with
    fewer than `min_nuclei` rows are left out of the GeoJSON only.  -> path."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    arrays = _as_outputs(ring_vertex, ring_start, ring_area2, component_of_ring, component, component_label)
    if len(arrays[4]) != len(head['label']):
        raise ValueError('write_npz: one component per nucleus')
    check_args(num_classes, half_pixel_radius(radius_px), by_class, min_nuclei)
    pts = np.rint(2 * head['xy']).astype(np.int64)
    d = derive(*arrays, pts, head['label'], num_classes)
    with open(path, 'wb') as f:
        np.savez(f, **head, **dict(zip(INT_NAMES, arrays)), radius_px=np.asarray(float(radius_px), np.float64),
                 by_class=np.asarray(int(by_class), np.int64), **d)
    with open(geojson_path(path), 'w') as f:
        json.dump(dict(type='FeatureCollection', features=features(*arrays, pts, min_nuclei)), f)
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)
