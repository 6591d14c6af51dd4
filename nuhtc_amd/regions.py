"""Nuclei by region: an exact point-in-polygon census of a slide's nucleus centres against annotated regions -- the tumour and stroma
annotations drawn in QuPath, or the tissue outline.  The other per-slide analyses (cellgraph.py, spatial.py, clusters.py, mst.py,
proximity.py, density.py) ask how the nuclei relate to each other; this one asks the first question put to a slide: how many nuclei of
each class lie in THIS region, and at what density.  It is the region with a known area and an exact "is this nucleus inside it" that
spatial.py (`tiles_area_px`) and density.py (no tissue-area normalisation) name as missing.  Computed on the GPU (csrc/cellregion.hip,
`nuhtc_cell_regions`); tools/infer_wsi.py --nuclei-regions writes it as <id>_nuclei_regions.npz.  Not in the reference.

Definition.

Inputs.  n points in HALF pixels, int32 (n, 2), from `cellpoints.quantize_centres`, with |p| < 2**27 and 0 <= n <= 2**24; labels, int32, one
per point; C classes, 1 <= C <= 14; G regions, 0 <= G <= 2**16.  A region is a set of closed rings: the exterior rings and the holes of a
GeoJSON Polygon or MultiPolygon, with no distinction between them.  Ring vertices are quantised like the centres: rint(2 x), half to even,
|v| < 2**27.  The regions are a flat edge table `edges` int32 (E, 4) = (ax, ay, bx, by), E <= 2**22, with `edge_region` int32 (E,)
non-decreasing, so an edge index orders the edges by region.  A ring's closing edge is included; a zero-length edge is legal.

Inside (even-odd, half-open).
  * An edge with ay != by STRADDLES p when (ay <= py) != (by <= py).
  * Orient a straddling edge upward: lo is its end with the smaller y, hi the other; u = hi - lo, w = p - lo.  The edge is CROSSED when
    u.x * w.y - u.y * w.x > 0: p lies strictly on the edge's -x side, the ray from p towards +x meets the edge beyond p.
  * p is inside region g when an odd number of g's edges are crossed.
  * Bit budget: differences are below 2**28 and products below 2**56, so int64 is exact (csrc/cellgrid_host.h has the argument); float64
    decides the side of a long thin edge wrongly.
  * Ring orientation does not matter; holes and multipolygons need no special case; two regions that share an edge TILE: every point on
    the shared edge is inside exactly one of them.  For an axis-aligned rectangle the min-x and min-y sides belong to it, the max-x and
    max-y sides do not.

On the boundary.  p is ON an edge when the cross product (b - a) x (p - a) is 0 (horizontal edges included) and p lies in the closed
bounding box of the edge; for a zero-length edge that is p == a.

Outputs, integers only, always fully written on success.
  region       int32 (n,)    the LARGEST region index that contains the point, -1 for none: later features lie on top, a viewer's z-order
                             (`read_geojson(order='area')` sorts so that "on top" means "innermost")
  depth        int32 (n,)    how many regions contain the point
  on_boundary  uint8 (n,)    1 when the point is on an edge of any region
  census       int64 (G, C)  the points of label c inside region g; a point is counted in EVERY region that contains it, a label outside
                             0..C-1 nowhere
With n == 0 or G == 0, region is all -1 and the others are zeros.

`regions_reference` is the brute-force int64 restatement (every point against every edge, no grid): the oracle the device result must EQUAL.
`derive` makes the float64 side on the host from the area the file states.

Beside it.  The distance from a nucleus to the region boundary as BANDS (the invasive-margin profile) is margin.py: "is the distance at
most e" is cross**2 <= e**2 * len**2, which fits 128 bits for e <= 16384 half pixels, so bands are exact.  Still out of scope: a
per-nucleus distance VALUE (the squared distance to a segment is the rational cross**2 / len**2, and comparing two such values takes more
than 128 bits at these coordinate ranges) and the area of a band (the area of an offset polygon is no integer statement).
Self-intersecting or improperly nested rings are not detected: even-odd is still well defined on them, but `area2` is then not the area
of what is inside."""
import json
import os
from collections import namedtuple

import numpy as np

from . import cellpoints
from .cellpoints import COORD_LIMIT, MAX_CLASSES, MAX_POINTS, MAX_R, centres, quantize_centres  # noqa: F401 (re-exported)

MAX_EDGES = 1 << 22
MAX_REGIONS = 1 << 16
MAX_SLOTS = 1 << 28                   # (edge, slab) records of one device call
MAX_CELLS = 1 << 22                   # of the device's grid (csrc/cellgrid_host.h REGION_MAX_CELLS)
SLAB_ROWS = 2048                      # `choose_slab` aims at this many slabs: a square box then fills the 2**22 cells
ORDERS = ('file', 'area')
INT_NAMES = ('region', 'depth', 'on_boundary', 'census')
DERIVED_KEYS = ('area_px2', 'density_per_px2', 'class_fraction', 'n_inside', 'n_outside', 'class_share_inside')
NPZ_KEYS = ('nuclei_id', 'xy', 'label') + INT_NAMES + DERIVED_KEYS + ('names', 'ring_start', 'edges', 'edge_region', 'area2', 'order')


class RegionTable(namedtuple('RegionTable', 'edges edge_region ring_start names area2')):
    """What `read_geojson` and `from_contours` return: edges int32 (E, 4), edge_region int32 (E,), ring_start int64 (R + 1,) (ring r is
    edges[ring_start[r]:ring_start[r + 1]]), names (G,) str, area2 int64 (G,).  `skipped` counts the geometries left out."""
    skipped = 0


# ---- the regions on the host
def _ring_vertices(ring):
    """One ring as written -> int64 (k, 2) quantised vertices without the closing repeat (k may be 0)."""
    v = np.asarray(ring, np.float64)
    if v.ndim != 2 or v.shape[1] < 2 or len(v) == 0:
        return np.zeros((0, 2), np.int64)
    v = v[:, :2]
    if not np.isfinite(v).all():
        raise ValueError('regions: a ring vertex is not finite')
    if len(v) > 1 and (v[0] == v[-1]).all():
        v = v[:-1]
    q = np.rint(2 * v)
    if np.abs(q).max() >= COORD_LIMIT:
        raise ValueError('regions: a ring vertex lies outside |v| < 2**27 half pixels')
    return q.astype(np.int64)


def _shoelace2(v):
    """|twice the shoelace area| of the ring v int64 (k, 2), in Python integers."""
    x, y = v[:, 0].tolist(), v[:, 1].tolist()
    return abs(sum(x[i] * y[i - 1] - x[i - 1] * y[i] for i in range(len(x))))


def _table(polygons, names, skipped=0):
    """polygons: per region a list of polygons, each a list of rings (the exterior first, then its holes) as int64 (k, 2) vertices -> RegionTable."""
    if len(polygons) > MAX_REGIONS:
        raise ValueError(f'regions: at most 2**16 regions (got {len(polygons)})')
    edges, region, ring_start, area2 = [], [], [0], []
    for g, polys in enumerate(polygons):
        a2 = 0
        for rings in polys:
            for k, v in enumerate(rings):
                if len(v) == 0:
                    continue
                edges.append(np.concatenate([v, np.roll(v, -1, 0)], 1))           # v[i] -> v[i + 1], the closing edge last
                region.append(np.full(len(v), g, np.int64))
                ring_start.append(ring_start[-1] + len(v))
                a2 += _shoelace2(v) if k == 0 else -_shoelace2(v)
        area2.append(a2)
    e = np.concatenate(edges, 0) if edges else np.zeros((0, 4), np.int64)
    if len(e) > MAX_EDGES:
        raise ValueError(f'regions: at most 2**22 edges (got {len(e)})')
    t = RegionTable(np.ascontiguousarray(e, np.int32).reshape(-1, 4), np.ascontiguousarray(np.concatenate(region) if region else np.zeros(0), np.int32),
                    np.asarray(ring_start, np.int64), np.asarray([str(s) for s in names], dtype=np.str_).reshape(-1), np.asarray(area2, np.int64).reshape(-1))
    t.skipped = int(skipped)
    return t


def features_table(features, order='file'):
    """GeoJSON features (dicts) -> RegionTable; see `read_geojson`."""
    if order not in ORDERS:
        raise ValueError(f"regions: order is 'file' or 'area' (got {order!r})")
    polygons, names, skipped = [], [], 0
    for f in features:
        geom = (f.get('geometry') if isinstance(f, dict) else None) or {}
        kind, coords = geom.get('type'), geom.get('coordinates') or []
        if kind not in ('Polygon', 'MultiPolygon'):
            skipped += 1
            continue
        polys = [coords] if kind == 'Polygon' else coords
        polygons.append([[_ring_vertices(r) for r in rings] for rings in polys])
        props = f.get('properties') or {}
        names.append((props.get('classification') or {}).get('name') or props.get('name') or '')
    if order == 'area':
        area = _table(polygons, names).area2.tolist()
        pick = sorted(range(len(polygons)), key=lambda g: (-area[g], g))           # the largest first: `region` is then the innermost
        polygons, names = [polygons[g] for g in pick], [names[g] for g in pick]
    return _table(polygons, names, skipped)


def read_geojson(path, order='file'):
    """A FeatureCollection, or a bare list of features (the layout of this project's own <id>.geojson), -> RegionTable
    (edges, edge_region, ring_start, names, area2), one region per Polygon or MultiPolygon feature; any other geometry is skipped and
    counted (`.skipped`).  names: properties.classification.name, else properties.name, else ''.  area2 int64 (G,): the sum over the
    feature's polygons of |twice the shoelace area| of the exterior ring minus that of its holes, in Python integers on the quantised
    vertices: area_px2 = area2 / 8.  It is the area the file STATES: valid for simple, properly nested rings, and not verified.
    order='area' sorts the features by descending area2, ties by file position, so that `region` is the innermost."""
    with open(path) as f:
        doc = json.load(f)
    if isinstance(doc, dict):
        doc = doc.get('features') if doc.get('type') == 'FeatureCollection' else [doc]
    if not isinstance(doc, list):
        raise ValueError(f'regions: {path} holds no list of features')
    return features_table(doc, order)


def from_contours(contours, holes):
    """The (contours_tissue, holes_tissue) lists of `tissue.segment_tissue`, level-0 pixels: contour g with its holes is region g."""
    ring = lambda c: _ring_vertices(np.asarray(c).reshape(-1, 2))
    if len(holes) != len(contours):
        raise ValueError('regions: one list of holes per contour')
    return _table([[[ring(c)] + [ring(h) for h in hs]] for c, hs in zip(contours, holes)], [''] * len(contours))


def source_check(path):
    """The argument of --nuclei-regions: a GeoJSON file for every slide, or a directory of <slide_id>.geojson: ValueError otherwise."""
    if not path or not (os.path.isfile(path) or os.path.isdir(path)):
        raise ValueError(f'{path!r} is neither a GeoJSON file nor a directory of <slide_id>.geojson files')


def source_for(path, slide_id):
    """-> the GeoJSON of this slide, or None when the directory holds none for it."""
    if os.path.isdir(path):
        path = os.path.join(path, slide_id + '.geojson')
    return path if os.path.isfile(path) else None


# ---- the definition
def check_args(num_classes, G=0, E=0, slab=1):
    """num_classes 1..14, 0 <= G <= 2**16, 0 <= E <= 2**22, slab 1..16384 half pixels: ValueError otherwise."""
    whole = all(float(v) == int(v) for v in (num_classes, G, E, slab))
    if not (whole and 1 <= int(num_classes) <= MAX_CLASSES and 0 <= int(G) <= MAX_REGIONS and 0 <= int(E) <= MAX_EDGES and 1 <= int(slab) <= MAX_R):
        raise ValueError(f'regions: num_classes 1..{MAX_CLASSES}, at most 2**16 regions and 2**22 edges, slab 1..{MAX_R} half pixels '
                         f'(got num_classes={num_classes}, G={G}, E={E}, slab={slab})')


def as_edges(edges, edge_region, G, what='regions'):
    """-> (edges int32 (E, 4), edge_region int32 (E,)), contiguous; ValueError unless int32 half pixels with |v| < 2**27, one region in
    0..G-1 per edge, non-decreasing."""
    raw = np.asarray(edges).reshape(-1, 4)
    e = np.ascontiguousarray(raw, np.int32)
    if not np.array_equal(e, raw):
        raise ValueError(f'{what}: the edges are not int32 half pixels')
    er = np.ascontiguousarray(np.asarray(edge_region).reshape(-1), np.int32)
    if len(er) != len(e):
        raise ValueError(f'{what}: one region per edge')
    if len(e) and np.abs(e.astype(np.int64)).max() >= COORD_LIMIT:
        raise ValueError(f'{what}: a vertex lies outside |v| < 2**27')
    if len(e) and (er.min() < 0 or er.max() >= int(G) or (np.diff(er) < 0).any()):
        raise ValueError(f'{what}: edge_region is non-decreasing and within 0..G-1')
    return e, er


def inside_block(px, py, e, start):
    """The even-odd, half-open rule of the definition for a block of points against every region: px, py int64 (b, 1), e int64 (E, 4),
    start int (G + 1,) the run of every region's edges -> bool (b, G).  The ONE numpy statement of it (margin.py takes its sides here)."""
    ax, ay, bx, by = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
    up = ay < by
    lx, ly, hx, hy = np.where(up, ax, bx), np.where(up, ay, by), np.where(up, bx, ax), np.where(up, by, ay)
    crossed = ((ay[None] <= py) != (by[None] <= py)) & ((hx - lx)[None] * (py - ly[None]) - (hy - ly)[None] * (px - lx[None]) > 0)
    cs = np.zeros((len(px), len(e) + 1), np.int64)
    np.cumsum(crossed, 1, out=cs[:, 1:])
    return ((cs[:, start[1:]] - cs[:, start[:-1]]) & 1).astype(bool)        # odd crossings of the region's run of edges


def regions_reference(points, labels, num_classes, edges, edge_region, G, block=1024):
    """The definition in int64: points int (n, 2) half pixels, labels int (n,), edges int (E, 4), edge_region int (E,) ->
    (region int32 (n,), depth int32 (n,), on_boundary uint8 (n,), census int64 (G, C)).  Every point against EVERY edge, no grid, `block`
    points at a time (a few (block, E) int64 temporaries, as cellpoints.pair_blocks keeps them).  Meant for a few thousand of each."""
    e, er = as_edges(edges, edge_region, G, 'regions_reference')
    check_args(num_classes, G, len(e))
    p, lab = cellpoints.reference_points(points, labels, 'regions_reference')
    n, C, G, E = len(p), int(num_classes), int(G), len(e)
    region, depth = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    on, census = np.zeros(n, np.uint8), np.zeros((G, C), np.int64)
    if n == 0 or G == 0 or E == 0:
        return region, depth, on, census
    e = e.astype(np.int64)
    ax, ay, bx, by = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
    x0, x1, y0, y1 = np.minimum(ax, bx), np.maximum(ax, bx), np.minimum(ay, by), np.maximum(ay, by)
    start = np.searchsorted(er, np.arange(G + 1))
    block = max(1, min(int(block), (1 << 21) // max(E, G)))                  # a temporary of at most 16 MiB
    known = (lab >= 0) & (lab < C)
    for i0 in range(0, n, block):
        px, py = p[i0:i0 + block, 0, None], p[i0:i0 + block, 1, None]
        inside = inside_block(px, py, e, start)
        depth[i0:i0 + block] = inside.sum(1)
        region[i0:i0 + block] = np.where(inside.any(1), G - 1 - np.argmax(inside[:, ::-1], 1), -1)
        touch = ((bx - ax)[None] * (py - ay[None]) - (by - ay)[None] * (px - ax[None]) == 0) & (px >= x0[None]) & (px <= x1[None]) & (py >= y0[None]) & (py <= y1[None])
        on[i0:i0 + block] = touch.any(1)
        row, g = np.nonzero(inside & known[i0:i0 + block, None])
        np.add.at(census, (g, lab[i0 + row]), 1)
    return region, depth, on, census


# ---- the device
def choose_slab(bounds):
    """The slab height `build` asks for, in half pixels: the box's height over SLAB_ROWS = 2048 slabs, rounded up, within 1..16384.  A
    point is tested against the edges of its slab only, and an edge is recorded once per slab it meets: more slabs mean fewer tests and
    more records; 2048 rows of square cells fill the device's 2**22 cells on a square box.  No output depends on it."""
    return int(min(max(-(-(int(bounds[3]) - int(bounds[1]) + 1) // SLAB_ROWS), 1), MAX_R))


def slots_needed(edges, bounds, slab, grow=0):
    """M, the (edge, slab) records the device call needs, stated exactly on the host: `cellpoints.cell_side` restates the grid, the rest
    restates edge_slab_range of csrc/cellgrid_host.h -- an edge has one record per slab of the box that its closed y-range, grown by
    `grow` (0 here, the largest threshold in margin.py), meets; none when the grown range lies above or below the box or the edge lies
    wholly left of x_min - grow."""
    e = np.asarray(edges, np.int64).reshape(-1, 4)
    if len(e) == 0 or bounds is None:
        return 0
    R = int(grow)
    x_min, y_min, x_max, y_max = (int(b) for b in bounds)
    side = cellpoints.cell_side(x_min, y_min, x_max, y_max, int(slab), MAX_CELLS)
    ylo, yhi = np.minimum(e[:, 1], e[:, 3]) - R, np.maximum(e[:, 1], e[:, 3]) + R
    keep = (yhi >= y_min) & (ylo <= y_max) & ~((e[:, 0] < x_min - R) & (e[:, 2] < x_min - R))
    s0, s1 = (np.maximum(ylo, y_min) - y_min) // side, (np.minimum(yhi, y_max) - y_min) // side
    return int((s1 - s0 + 1)[keep].sum())


def call_entry(name, points, labels, num_classes, edges, edge_region, G, more, slab, slot_cap, out, bounds, device):
    """What `call` here and in margin.py do alike: the entry point `name`, whose scalars are (num_classes, edges, edge_region, E, G, *more,
    slab, slot_cap), on the output tensors `out` -> (the library's return code, M or None)."""
    import ctypes
    m = ctypes.c_int64(-1)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = cellpoints.launch(name, device, points, labels,
                           (int(num_classes), vp(edges), vp(edge_region), int(edges.shape[0]), int(G), *more, int(slab), int(slot_cap)),
                           out, bounds, extra=(ctypes.byref(m),))
    return rc, (int(m.value) if rc == 0 else None)


def call(points, labels, num_classes, edges, edge_region, G, slab, slot_cap, region, depth, on_boundary, census, bounds=None, device=0):
    """nuhtc_cell_regions on torch tensors of cuda:`device` (contiguous; edges int32 (E, 4), edge_region int32 (E,); region and depth int32
    (n,), on_boundary uint8 (n,), census int64 (G, C); slab in HALF pixels) -> (the library's return code, M), nothing raised: the code is 0
    or hip.E_INVALID / hip.E_HIP; M, the (edge, slab) records the call needs, is None unless the code is 0.  With M > slot_cap the outputs
    are untouched: call again with slot_cap >= M.  bounds = (x_min, y_min, x_max, y_max) of the points, computed on the host when not given."""
    return call_entry('nuhtc_cell_regions', points, labels, num_classes, edges, edge_region, G, (), slab, slot_cap,
                      (region, depth, on_boundary, census), bounds, device)


def outputs(n, G, num_classes, device, fill=0):
    """The four output tensors of `call` on `device` (one row at least each), every entry `fill`."""
    import torch
    n, G = max(int(n), 1), max(int(G), 1)
    return [torch.full(s, fill, dtype=t, device=device) for s, t in (((n,), torch.int32), ((n,), torch.int32), ((n,), torch.uint8), ((G, int(num_classes)), torch.int64))]


def build_entry(what, entry, points, labels, C, e, er, G, device, slab, slot_cap, *, check, slab_rule, grow, call, make_outputs):
    """What `build` here and in margin.py do alike behind `as_edges` (e, er) and their own checks, in the name of `what` around the entry
    point `entry`.  The module passes, by keyword: check(C, G, E, slab), its check_args; slab_rule(bounds), its choose_slab; grow, by which
    `slots_needed` grows an edge's y-range; call(front, back, bounds) -> (rc, M), its `call` on front = (points, labels, C, edges,
    edge_region, G) and back = (slab, slot_cap, *outputs), its own scalars put between them; make_outputs(n, dev), its `outputs`.
    -> (the output tensors, n, the number of device calls).  The capacity loop is `cellpoints.grow_to_fit`; the outputs are made once."""
    import torch
    check(C, G, len(e), 1)
    p, lab, dev, p_d, lab_d, bounds = cellpoints.resident(points, labels, what, device)
    n = len(p)
    if n and np.abs(p).max() >= COORD_LIMIT:
        raise ValueError(f'{what}: a coordinate lies outside |p| < 2**27')
    slab = slab_rule(bounds) if slab is None and n else int(slab or 1)
    check(C, G, len(e), slab)
    refuse = lambda m: f'{what}: {m} (edge, slab) records, more than 2**28: a larger slab makes them fewer' if m > MAX_SLOTS else None
    cap = slots_needed(e, bounds, slab, grow) if slot_cap is None else int(slot_cap)
    if refuse(cap):                                          # the first cap too, before anything more is uploaded
        raise ValueError(refuse(cap))
    e_d, er_d = torch.from_numpy(e if len(e) else np.zeros((1, 4), np.int32)).to(dev), torch.from_numpy(er if len(e) else np.zeros(1, np.int32)).to(dev)
    front, out = (p_d, lab_d, C, e_d[:len(e)], er_d[:len(e)], G), make_outputs(n, dev)
    out, _, _, calls = cellpoints.grow_to_fit(lambda cap, out: call(front, (slab, cap, *out), bounds), lambda cap: out, cap, entry, what,
                                              refuse=refuse, unit='records')
    return out, n, calls


def build(points, labels, num_classes, edges, edge_region, G, device=0, slab=None, slot_cap=None, with_calls=False):
    """The census of `points` (int (n, 2) half pixels, see cellpoints.quantize_centres) with `labels` (n,) against the regions on
    cuda:`device`: numpy in, the four results of `regions_reference` out, and the number of device calls behind them when `with_calls`.
    The slab height is `choose_slab` of the points' box unless given; the first call has room for `slots_needed` records -- exactly what
    the device counts -- unless `slot_cap` says otherwise; when the device needs more it says how many and writes nothing, and ONE second
    call has room for exactly that many.  There is no host route: without the library or a GPU this raises."""
    C, G = int(num_classes), int(G)
    e, er = as_edges(edges, edge_region, G)
    out, n, calls = build_entry('regions', 'nuhtc_cell_regions', points, labels, C, e, er, G, device, slab, slot_cap,
                                check=check_args, slab_rule=choose_slab, grow=0, make_outputs=lambda n, dev: outputs(n, G, C, dev),
                                call=lambda front, back, bounds: call(*front, *back, bounds=bounds, device=device))
    got = (out[0][:n].cpu().numpy(), out[1][:n].cpu().numpy(), out[2][:n].cpu().numpy(), out[3][:G].cpu().numpy())
    return got + (calls,) if with_calls else got


# ---- the float64 side and the file
def derive(census, area2, depth, labels):
    """The float64 side of the integers -> dict:
      area_px2            float64 (G,)    area2 / 8: the area the file states, in px^2 (area2 is twice the area in half pixels squared)
      density_per_px2     float64 (G, C)  census / area_px2, nan where the area is 0
      class_fraction      float64 (G, C)  census[g] over its sum: each class's share of the nuclei of known class inside region g, 0 where
                                          the region holds none
      n_inside, n_outside int64 0-d       the nuclei inside at least one region (depth > 0), and the others
      class_share_inside  float64 (C,)    of the nuclei of class c, the share that lies inside at least one region, 0 where the class has none"""
    cen = np.asarray(census, np.int64)
    a2 = np.asarray(area2, np.int64).reshape(-1)
    dep = np.asarray(depth, np.int64).reshape(-1)
    lab = np.asarray(labels, np.int64).reshape(-1)
    if cen.ndim != 2 or len(a2) != len(cen) or len(dep) != len(lab) or (cen < 0).any() or (dep < 0).any():
        raise ValueError('derive: census is (G, C) with one area2 per region, not negative, and depth has one entry per label')
    G, C = cen.shape
    area = a2.astype(np.float64) / 8
    density = np.full((G, C), np.nan, np.float64)
    np.divide(cen, area[:, None], out=density, where=(area != 0)[:, None])
    total = cen.sum(1)
    fraction = np.zeros((G, C), np.float64)
    np.divide(cen, total[:, None], out=fraction, where=(total > 0)[:, None])
    known = (lab >= 0) & (lab < C)
    of_class = np.bincount(lab[known], minlength=C).astype(np.float64)
    inside = np.bincount(lab[known & (dep > 0)], minlength=C).astype(np.float64)
    share = np.zeros(C, np.float64)
    np.divide(inside, of_class, out=share, where=of_class > 0)
    n_in = int((dep > 0).sum())
    return dict(area_px2=area, density_per_px2=density, class_fraction=fraction, n_inside=np.asarray(n_in, np.int64),
                n_outside=np.asarray(len(dep) - n_in, np.int64), class_share_inside=share)


def write_npz(path, nuclei_id, xy, label, region, depth, on_boundary, census, table, order='file'):
    """<id>_nuclei_regions.npz, the header row i for the i-th row of <id>_nuclei_graph.npz / <id>_nuclei_feat.npz:
      nuclei_id int64 (n,), xy float64 (n, 2) (the unquantised centre in slide px), label int64 (n,)
      region int32 (n,), depth int32 (n,), on_boundary uint8 (n,), census int64 (G, C): the integers of the definition
      the arrays of `derive` (DERIVED_KEYS)
      names (G,) str, ring_start int64 (R + 1,), edges int32 (E, 4) and edge_region int32 (E,) in half pixels, area2 int64 (G,): the
      RegionTable the census was taken against; order: 'file' or 'area' as a 0-d str."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    n, G = len(head['label']), len(table.names)
    region = np.ascontiguousarray(region, np.int32).reshape(-1)
    depth = np.ascontiguousarray(depth, np.int32).reshape(-1)
    on_boundary = np.ascontiguousarray(on_boundary, np.uint8).reshape(-1)
    census = np.ascontiguousarray(census, np.int64)
    if not len(region) == len(depth) == len(on_boundary) == n or census.ndim != 2 or len(census) != G or len(table.area2) != G:
        raise ValueError('write_npz: one region, depth and on_boundary per nucleus, one census row and one area2 per region')
    if order not in ORDERS:
        raise ValueError(f"write_npz: order is 'file' or 'area' (got {order!r})")
    t = table_arrays(table, G)
    check_args(census.shape[1], G, len(t['edges']))
    d = derive(census, table.area2, depth, head['label'])
    with open(path, 'wb') as f:
        np.savez(f, **head, region=region, depth=depth, on_boundary=on_boundary, census=census, **d, **t, order=np.asarray(order))
    return path


def table_arrays(table, G):
    """The RegionTable behind a file, for a `write_npz` (here and in margin.py) -> dict in the order of the files' keys: names (G,) str,
    ring_start int64, edges int32 (E, 4) and edge_region int32 (E,) checked by `as_edges` against G, area2 int64."""
    e, er = as_edges(table.edges, table.edge_region, G, 'write_npz')
    return dict(names=np.asarray(table.names, dtype=np.str_).reshape(-1), ring_start=np.asarray(table.ring_start, np.int64), edges=e, edge_region=er,
                area2=np.asarray(table.area2, np.int64))


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)
