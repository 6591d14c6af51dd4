"""Margin bands: the nuclei of each class by distance to the boundary of an annotated region, inside it and outside it -- the
invasive-margin or infiltration profile ("how many lymphocytes lie within 0-50, 50-100, .. px of the tumour boundary"), what QuPath users
take from "distance to annotation".  A sibling of regions.py (how many nuclei of each class lie IN this region), with the same points,
regions and GeoJSON reader.  Computed on the GPU (csrc/cellmargin.hip, `nuhtc_cell_margin`); tools/infer_wsi.py --nuclei-margin writes it
as <id>_nuclei_margin.npz.  Not in the reference.

Definition.

Inputs.  As regions.py: n points in HALF pixels, int32 (n, 2), |p| < 2**27, 0 <= n <= 2**24; labels, one per point; C classes, 1..14; G
regions, 0 <= G <= 2**16, as the flat edge table `edges` int32 (E, 4) = (ax, ay, bx, by), E <= 2**22, with `edge_region` int32 (E,)
non-decreasing.  And `thresholds` int32 (B,), 1 <= B <= 32, in half pixels, strictly increasing, 1 <= e_0 and e_{B-1} <= 16384
(`thresholds_from_step` makes the row of the command line: step, 2 step, ..).

near(p, a -> b, e): "the distance from p to the segment a b is at most e", inclusive like every radius of the family.
  * d = b - a, w = p - a, L2 = d.d, s = w.d.
  * L2 == 0 or s <= 0 (a zero-length edge, or p at or behind a):  |w|**2 <= e**2.
  * s >= L2 (p at or beyond b):  |p - b|**2 <= e**2.
  * otherwise (p beside the edge):  (d x w)**2 <= e**2 * L2 -- the squared distance is the rational cross**2 / L2.
  * Bit budget: differences are below 2**28; s, L2, |w|**2 and d x w are below 2**57 and exact in int64; cross**2 < 2**114 and
    e**2 * L2 < 2**28 * 2**57 = 2**85, so the last compare is 128-bit unsigned (csrc/cellgrid_host.h has the argument).  Float64 -- project
    onto the segment, compare hypot with e -- decides about 1 % of designed exact-threshold pairs wrongly (tests/margin_cases.py).

band(p, g) = the smallest t for which some edge of g has near(p, edge, e_t); B when no edge does.
inside(p, g) is exactly regions.py's even-odd, half-open rule (`regions.inside_block`, region_crossed on the device): not restated here.

Outputs, integers only, always fully written on success.
  band_census  int64 (G, 2, B, C)  [g][side][t][c]: the points of label c with band(p, g) == t and inside(p, g) == side (0 outside, 1
                                   inside).  A point is counted for EVERY region it is near; a label outside 0..C-1 nowhere; a band of B
                                   (beyond the last threshold) is not counted here.
  census       int64 (G, C)        the points of label c inside g: the numbers of `regions_reference`'s census.  `derive` takes "inside,
                                   beyond the last band" from it.
  band         int32 (n,)          the minimum over g of band(p, g); B when none, or when G == 0
  band_region  int32 (n,)          the smallest g that attains `band`, -1 when band == B
  band_inside  uint8 (n,)          inside(p, band_region), 0 when there is none

`margin_reference` is the brute-force restatement (every point against every edge, no grid; the 128-bit compare in Python integers wherever
float64 cannot be trusted): the oracle the device result must EQUAL.  `derive` makes the float64 side on the host.

Out of scope.  A per-nucleus distance VALUE (comparing two rationals cross**2 / L2 takes more than 128 bits) and a density per band: a
band's area is the area of an offset polygon clipped by the region, which is no integer statement."""
import numpy as np

from . import cellpoints, regions
from .cellpoints import COORD_LIMIT, MAX_CLASSES, MAX_POINTS, MAX_R  # noqa: F401 (re-exported)
from .regions import MAX_CELLS, MAX_EDGES, MAX_REGIONS, MAX_SLOTS, as_edges, read_geojson, source_check, source_for  # noqa: F401 (re-exported)

MAX_BANDS = 32
INT_NAMES = ('band_census', 'census', 'band', 'band_region', 'band_inside')
DERIVED_KEYS = ('band_edges_px', 'inside_beyond', 'profile', 'class_fraction', 'n_near')
NPZ_KEYS = ('nuclei_id', 'xy', 'label') + INT_NAMES + ('thresholds',) + DERIVED_KEYS + ('names', 'ring_start', 'edges', 'edge_region', 'area2')


# ---- the definition
def as_thresholds(thresholds):
    """-> int32 (B,) contiguous; ValueError unless 1..32 whole half pixels, strictly increasing, within 1..16384."""
    raw = np.asarray(thresholds).reshape(-1)
    t = np.ascontiguousarray(raw, np.int32)
    if not np.array_equal(t, raw):
        raise ValueError('margin: the thresholds are not whole half pixels')
    if not (1 <= len(t) <= MAX_BANDS and t[0] >= 1 and t[-1] <= MAX_R and (np.diff(t.astype(np.int64)) > 0).all()):
        raise ValueError(f'margin: 1..{MAX_BANDS} thresholds, strictly increasing, within 1..{MAX_R} half pixels (got {raw.tolist()})')
    return t


def thresholds_from_step(step_px, bands):
    """The tool's row: e_t = 2 * step * (t + 1) half pixels, t = 0..bands-1 (`spatial.edges_from_step`); step a multiple of 0.5 px,
    1..32 bands, step * bands <= 8192 px: ValueError otherwise."""
    from . import spatial
    if not 1 <= int(bands) <= MAX_BANDS:
        raise ValueError(f'1..{MAX_BANDS} bands (got {bands})')
    return as_thresholds(spatial.edges_from_step(step_px, bands))


def check_args(num_classes, G=0, E=0, slab=1, thresholds=(1,)):
    """num_classes 1..14, 0 <= G <= 2**16, 0 <= E <= 2**22, slab 1..16384 half pixels, thresholds as `as_thresholds`: ValueError otherwise."""
    regions.check_args(num_classes, G, E, slab)
    as_thresholds(thresholds)


def near(ax, ay, bx, by, px, py, e):
    """near(p, a -> b, e) of the definition on Python integers."""
    ax, ay, bx, by, px, py, e = (int(v) for v in (ax, ay, bx, by, px, py, e))
    dx, dy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    L2, s = dx * dx + dy * dy, wx * dx + wy * dy
    if L2 == 0 or s <= 0:
        return wx * wx + wy * wy <= e * e
    if s >= L2:
        return (px - bx) ** 2 + (py - by) ** 2 <= e * e
    return (dx * wy - dy * wx) ** 2 <= e * e * L2


def _pair_bands(px, py, e, thr):
    """band of every (point, edge) pair: px, py int64 (b, 1), e int64 (E, 4), thr int64 (B,) -> int64 (b, E), B where not near at e_{B-1}.
    The measure of the pair is q (the squared distance to an end) or q**2 / L2 (beside the edge), exact in int64.  float64 places it among
    the squared thresholds wherever it is farther than 1e-9 (relative) from each of them -- its own error is a few 2**-53 -- and every
    other pair is decided by `near` in Python integers."""
    ax, ay, bx, by = e[None, :, 0], e[None, :, 1], e[None, :, 2], e[None, :, 3]
    dx, dy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    L2, s = dx * dx + dy * dy, wx * dx + wy * dy
    first, last = (L2 == 0) | (s <= 0), (L2 > 0) & (s >= L2)
    end2 = np.where(first, wx * wx + wy * wy, (px - bx) ** 2 + (py - by) ** 2)
    cross = np.abs(dx * wy - dy * wx).astype(np.float64)
    d2 = np.where(first | last, end2.astype(np.float64), cross * cross / np.maximum(L2, 1).astype(np.float64))
    e2 = (thr * thr).astype(np.float64)
    band = np.searchsorted(e2, d2.ravel(), side='left').reshape(d2.shape).astype(np.int64)
    above, below = e2[np.minimum(band, len(e2) - 1)], e2[np.maximum(band - 1, 0)]      # the squared thresholds on either side of d2
    rows, cols = np.nonzero((np.abs(d2 - above) <= 1e-9 * above) | (np.abs(d2 - below) <= 1e-9 * below))
    if len(rows):
        pxl, pyl, el, tl = px[:, 0].tolist(), py[:, 0].tolist(), e.tolist(), thr.tolist()
        for i, k in zip(rows.tolist(), cols.tolist()):
            band[i, k] = next((t for t, v in enumerate(tl) if near(*el[k], pxl[i], pyl[i], v)), len(tl))
    return band


def margin_reference(points, labels, num_classes, edges, edge_region, G, thresholds, block=1024):
    """The definition: points int (n, 2) half pixels, labels int (n,), edges int (E, 4), edge_region int (E,), thresholds int (B,) ->
    (band_census int64 (G, 2, B, C), census int64 (G, C), band int32 (n,), band_region int32 (n,), band_inside uint8 (n,)).  Every point
    against EVERY edge, no grid, `block` points at a time.  Meant for a few thousand of each."""
    e, er = as_edges(edges, edge_region, G, 'margin_reference')
    thr = as_thresholds(thresholds).astype(np.int64)
    check_args(num_classes, G, len(e))
    p, lab = cellpoints.reference_points(points, labels, 'margin_reference')
    n, C, G, E, B = len(p), int(num_classes), int(G), len(e), len(thr)
    band_census, census = np.zeros((G, 2, B, C), np.int64), np.zeros((G, C), np.int64)
    band, band_region, band_inside = np.full(n, B, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    if n == 0 or G == 0 or E == 0:
        return band_census, census, band, band_region, band_inside
    e = e.astype(np.int64)
    start = np.searchsorted(er, np.arange(G + 1))
    filled = np.flatnonzero(start[1:] > start[:-1])                          # the regions that have edges
    block = max(1, min(int(block), (1 << 19) // max(E, G)))
    known = (lab >= 0) & (lab < C)
    for i0 in range(0, n, block):
        px, py = p[i0:i0 + block, 0, None], p[i0:i0 + block, 1, None]
        inside = regions.inside_block(px, py, e, start)                      # (b, G)
        of_region = np.full((len(px), G), B, np.int64)
        of_region[:, filled] = np.minimum.reduceat(_pair_bands(px, py, e, thr), start[:-1][filled], axis=1)
        best = of_region.min(1)
        band[i0:i0 + block] = best
        first = np.argmax(of_region == best[:, None], 1)                     # the smallest g that attains it
        rows = np.arange(len(px))
        band_region[i0:i0 + block] = np.where(best < B, first, -1)
        band_inside[i0:i0 + block] = np.where(best < B, inside[rows, first], 0)
        k = known[i0:i0 + block, None]
        row, g = np.nonzero((of_region < B) & k)
        np.add.at(band_census, (g, inside[row, g].astype(np.int64), of_region[row, g], lab[i0 + row]), 1)
        row, g = np.nonzero(inside & k)
        np.add.at(census, (g, lab[i0 + row]), 1)
    return band_census, census, band, band_region, band_inside


# ---- the device
def choose_slab(bounds, thresholds):
    """The slab height `build` asks for, in half pixels: `regions.choose_slab` of the points' box, but at least R = e_{B-1}, within
    1..16384.  An edge has a record in every slab its y-range grown by R meets, so a slab of at least R keeps a short edge at about three
    records.  No output depends on it."""
    return int(min(max(regions.choose_slab(bounds), int(as_thresholds(thresholds)[-1])), MAX_R))


def slots_needed(edges, bounds, slab, thresholds):
    """M, the (edge, slab) records the device call needs, stated exactly on the host: `regions.slots_needed` with every edge's y-range
    grown by R = e_{B-1}.  Without edges or points it is 0 whatever the thresholds."""
    if np.size(edges) == 0 or bounds is None:
        return 0
    return regions.slots_needed(edges, bounds, slab, int(as_thresholds(thresholds)[-1]))


def call(points, labels, num_classes, edges, edge_region, G, thresholds, slab, slot_cap, band_census, census, band, band_region, band_inside,
         bounds=None, device=0):
    """nuhtc_cell_margin on torch tensors of cuda:`device` (contiguous; edges int32 (E, 4), edge_region int32 (E,); band_census int64
    (G, 2, B, C), census int64 (G, C), band and band_region int32 (n,), band_inside uint8 (n,); slab in HALF pixels) and the thresholds as
    a sequence of ints on the host, passed as they are -> (the library's return code, M), nothing raised: the code is 0 or hip.E_INVALID /
    hip.E_HIP; M, the (edge, slab) records the call needs, is None unless the code is 0.  With M > slot_cap the outputs are untouched:
    call again with slot_cap >= M.  bounds = (x_min, y_min, x_max, y_max) of the points, computed on the host when not given."""
    import ctypes
    row = [int(v) for v in np.asarray(thresholds).reshape(-1).tolist()]
    thr = (ctypes.c_int32 * max(len(row), 1))(*row)
    return regions.call_entry('nuhtc_cell_margin', points, labels, num_classes, edges, edge_region, G, (thr, len(row)), slab, slot_cap,
                              (band_census, census, band, band_region, band_inside), bounds, device)


def outputs(n, G, num_classes, B, device, fill=0):
    """The five output tensors of `call` on `device` (one row at least each), every entry `fill`."""
    import torch
    n, G, C, B = max(int(n), 1), max(int(G), 1), int(num_classes), max(int(B), 1)
    shapes = (((G, 2, B, C), torch.int64), ((G, C), torch.int64), ((n,), torch.int32), ((n,), torch.int32), ((n,), torch.uint8))
    return [torch.full(s, fill, dtype=t, device=device) for s, t in shapes]


def build(points, labels, num_classes, edges, edge_region, G, thresholds, device=0, slab=None, slot_cap=None, with_calls=False):
    """The margin bands of `points` (int (n, 2) half pixels, see cellpoints.quantize_centres) with `labels` (n,) against the regions on
    cuda:`device`: numpy in, the five results of `margin_reference` out, and the number of device calls behind them when `with_calls`.
    The slab height is `choose_slab` unless given; the first call has room for `slots_needed` records -- exactly what the device counts --
    unless `slot_cap` says otherwise; when the device needs more it says how many and writes nothing, and ONE second call has room for
    exactly that many.  There is no host route: without the library or a GPU this raises."""
    C, G = int(num_classes), int(G)
    e, er = as_edges(edges, edge_region, G, 'margin')
    thr = as_thresholds(thresholds)
    out, n, calls = regions.build_entry('margin', 'nuhtc_cell_margin', points, labels, C, e, er, G, device, slab, slot_cap,
                                        check=lambda *a: check_args(*a, thr), slab_rule=lambda bounds: choose_slab(bounds, thr), grow=int(thr[-1]),
                                        make_outputs=lambda n, dev: outputs(n, G, C, len(thr), dev),
                                        call=lambda front, back, bounds: call(*front, thr, *back, bounds=bounds, device=device))
    got = (out[0][:G].cpu().numpy(), out[1][:G].cpu().numpy(), out[2][:n].cpu().numpy(), out[3][:n].cpu().numpy(), out[4][:n].cpu().numpy())
    return got + (calls,) if with_calls else got


# ---- the float64 side and the file
def derive(band_census, census, thresholds):
    """The host side of the integers -> dict, float64 without NaN and int64:
      band_edges_px   float64 (B + 1,)      0, e_0 / 2, .., e_{B-1} / 2: band t lies between entries t and t + 1, in px
      inside_beyond   int64 (G, C)          census - sum_t band_census[g][1]: the nuclei inside g farther than e_{B-1} from its boundary
      profile         int64 (G, 2 B, C)     the bands from the innermost inside band to the outermost outside band: inside B-1, .., inside
                                            0, outside 0, .., outside B-1.  sum_k profile[g][k] over the inside half, plus inside_beyond,
                                            is the census
      class_fraction  float64 (G, 2, B, C)  band_census over its sum along the classes: each class's share of the nuclei of known class in
                                            that (region, side, band); 0 where the band is empty
      n_near          int64 (G,)            the nuclei of known class within e_{B-1} of the region's boundary
    No density per band: a band's area is the area of an offset polygon clipped by the region, which is no integer statement."""
    bc = np.asarray(band_census, np.int64)
    cen = np.asarray(census, np.int64)
    thr = as_thresholds(thresholds)
    if bc.ndim != 4 or bc.shape[1] != 2 or bc.shape[2] != len(thr) or cen.shape != (bc.shape[0], bc.shape[3]) or (bc < 0).any() or (cen < 0).any():
        raise ValueError('derive: band_census is (G, 2, B, C) with one threshold per band, census (G, C), neither negative')
    beyond = cen - bc[:, 1].sum(1)
    if (beyond < 0).any():
        raise ValueError('derive: more nuclei in the inside bands of a region than inside it')
    total = bc.sum(3, keepdims=True)
    fraction = np.zeros(bc.shape, np.float64)
    np.divide(bc, total, out=fraction, where=total > 0)
    return dict(band_edges_px=np.concatenate([[0.0], thr.astype(np.float64) / 2]), inside_beyond=beyond,
                profile=np.ascontiguousarray(np.concatenate([bc[:, 1, ::-1], bc[:, 0]], 1)), class_fraction=fraction, n_near=bc.sum((1, 2, 3)))


def write_npz(path, nuclei_id, xy, label, band_census, census, band, band_region, band_inside, thresholds, table):
    """<id>_nuclei_margin.npz, the header row i for the i-th row of <id>_nuclei_graph.npz / <id>_nuclei_feat.npz:
      nuclei_id int64 (n,), xy float64 (n, 2) (the unquantised centre in slide px), label int64 (n,)
      band_census int64 (G, 2, B, C), census int64 (G, C), band int32 (n,), band_region int32 (n,), band_inside uint8 (n,): the integers
      of the definition; thresholds int32 (B,) in half pixels
      the arrays of `derive` (DERIVED_KEYS)
      names (G,) str, ring_start int64 (R + 1,), edges int32 (E, 4) and edge_region int32 (E,) in half pixels, area2 int64 (G,): the
      RegionTable (regions.read_geojson, file order) the bands were taken against."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    n, G = len(head['label']), len(table.names)
    thr = as_thresholds(thresholds)
    band_census, census = np.ascontiguousarray(band_census, np.int64), np.ascontiguousarray(census, np.int64)
    band, band_region = np.ascontiguousarray(band, np.int32).reshape(-1), np.ascontiguousarray(band_region, np.int32).reshape(-1)
    band_inside = np.ascontiguousarray(band_inside, np.uint8).reshape(-1)
    if not len(band) == len(band_region) == len(band_inside) == n or census.ndim != 2 or len(census) != G or len(band_census) != G:
        raise ValueError('write_npz: one band, band_region and band_inside per nucleus, one row of census and band_census per region')
    t = regions.table_arrays(table, G)
    check_args(census.shape[1], G, len(t['edges']), 1, thr)
    d = derive(band_census, census, thr)
    with open(path, 'wb') as f:
        np.savez(f, **head, band_census=band_census, census=census, band=band, band_region=band_region, band_inside=band_inside, thresholds=thr, **d, **t)
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)
