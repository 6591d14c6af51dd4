"""Spatial statistics of a slide: how many nuclei of class b lie within r of a nucleus of class a, for every pair of classes and a whole
range of r, and how far every nucleus is from the nearest nucleus of each class -- the pair counts behind Ripley's K / L and the cross-type
nearest-neighbour function G.  Counted on the GPU (csrc/cellspatial.hip, `nuhtc_cell_spatial`); tools/infer_wsi.py --nuclei-spatial writes
them as <id>_nuclei_spatial.npz.  Not in the reference.

Definition.

Inputs.  n points in HALF pixels, int32 (n, 2), from `cellgraph.quantize_centres` (px = rint(x0 + x1), py = rint(y0 + y1) of the record's
box), with |p| < 2**27 and n <= 2**28; labels, int32, one per point; C classes, 1 <= C <= 14; B bin edges e_1 < e_2 < .. < e_B in half
pixels, int32, strictly increasing, 1 <= B <= 32, e_1 >= 1 and e_B <= 16384.  All geometry is integer arithmetic, so every squared distance
is exact and the result is a pure function of the input.

Bins.  The bin of an ordered pair (i, j), i != j, with d2 = dx * dx + dy * dy is the smallest t (0-based) with d2 <= e_t ** 2.
  * Edges are inclusive, like the graph's radius.
  * A pair with d2 > e_B ** 2 has no bin.
  * Coincident points have d2 = 0 and fall in bin 0.

Outputs, integers only.
  pair_hist int64 (C, C, B): entry [a][b][t] is the number of ordered pairs (i, j) with label_i = a, label_j = b and bin t.  NOT cumulative.
                             A point whose label lies outside 0..C-1 is counted in no row and no column.
  nn_d2     int32 (n, C):    entry [i][c] is the least d2 from i to a point j != i of class c with d2 <= e_B ** 2, or -1 when there is
                             none.  Written for every i, whatever its own label.
  class_n   int64 (C,):      the number of points of each class.

`spatial_reference` is the brute-force int64 restatement (every pair, no grid): the oracle the device result must EQUAL.  The device bins
the points into a uniform grid whose cell side is the smallest multiple of e_B with at most 2**18 cells over the points' bounding box
(`cell_side`), so the 3 x 3 cells around a point hold every disc; the bounding box is computed here on the host and passed in, as for the
cell graph.

`derive` turns the integers into the statistics on the host, in float64: the cumulative counts, `mean_within[a][b][t]` = cumulative /
class_n[a] (the mean number of b-nuclei within e_t of an a-nucleus; needs no area), `G[a][b][t]` (the share of a-nuclei whose nearest
b-nucleus lies within e_t, from nn_d2 by integer compares against e_t ** 2) and, only when an area is given, K[a][b][t] = area x cumulative
/ (class_n[a] x class_n[b]) and L = sqrt(K / pi), both in px.  There is NO edge correction: a nucleus near the border of the tissue sees
fewer neighbours than one inside, and nothing here compensates for that.  K carries Ripley's name and meaning only under a STATED area:
the intensity class_n[b] / area is what the counts are compared with, and this module does not estimate the tissue area.  The tool states
one -- the inferred tiles' area, the number of tiles x step_size ** 2 -- and labels K and L as resting on it."""
import numpy as np

from . import cellpoints
from .cellpoints import COORD_LIMIT, MAX_CLASSES, distances_px  # noqa: F401 (re-exported)

MAX_BINS, MAX_EDGE = 32, cellpoints.MAX_R
MAX_CELLS = 1 << 18

NPZ_KEYS = ('nuclei_id', 'xy', 'label', 'edges_px', 'pair_hist', 'nn_dist', 'class_n', 'nn_d2', 'mean_within', 'G', 'tiles_area_px',
            'K_tiles_area', 'L_tiles_area')


def check_args(num_classes, edges):
    """num_classes 1..14; edges: 1..32 strictly increasing integers of half pixels, the first >= 1, the last <= 16384.  -> int32 edges."""
    raw = np.asarray(edges).reshape(-1)
    e = raw.astype(np.int64) if raw.size else np.zeros(0, np.int64)
    if not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f'spatial statistics: num_classes 1..{MAX_CLASSES} (got {num_classes})')
    if not 1 <= len(e) <= MAX_BINS:
        raise ValueError(f'spatial statistics: 1..{MAX_BINS} bin edges (got {len(e)})')
    if not np.array_equal(e, raw):
        raise ValueError('spatial statistics: the bin edges are not whole numbers of half pixels')
    if e[0] < 1 or e[-1] > MAX_EDGE or (np.diff(e) <= 0).any():
        raise ValueError(f'spatial statistics: bin edges strictly increasing within 1..{MAX_EDGE} half pixels (got {e.tolist()})')
    return e.astype(np.int32)


def edges_from_step(step_px, bins):
    """The tool's edges: e_b = 2 * step * b half pixels, b = 1..bins; the step must be a whole number of half pixels."""
    s = int(round(2 * float(step_px)))
    if s != 2 * float(step_px) or s < 1:
        raise ValueError(f'bin step {step_px} px is not a whole, positive number of half pixels')
    if not 1 <= int(bins) <= MAX_BINS:
        raise ValueError(f'1..{MAX_BINS} bins (got {bins})')
    if s * int(bins) > MAX_EDGE:
        raise ValueError(f'bin step {step_px} px x {bins} bins reaches beyond {MAX_EDGE // 2} px')
    return (s * np.arange(1, int(bins) + 1)).astype(np.int32)


def cell_side(x_min, y_min, x_max, y_max, reach):
    """The grid cell side the device uses over the inclusive bounding box: the smallest multiple of e_B with at most 2**18 cells."""
    return cellpoints.cell_side(x_min, y_min, x_max, y_max, reach, MAX_CELLS)


def spatial_reference(points, labels, num_classes, edges):
    """The definition, pair by pair in int64: points int (n, 2) half pixels, labels int (n,), edges in HALF pixels ->
    (pair_hist int64 (C, C, B), nn_d2 int32 (n, C), class_n int64 (C,)).  O(n^2) time, rows in blocks of 512: for n of a few thousand."""
    e = check_args(num_classes, edges).astype(np.int64)
    p, lab = cellpoints.reference_points(points, labels, 'spatial_reference')
    n, C, B = len(p), int(num_classes), len(e)
    e2 = e * e
    known = (lab >= 0) & (lab < C)
    cls = np.where(known, lab, 0)
    pair_hist = np.zeros(C * C * B, np.int64)
    nn_d2 = np.full((n, C), -1, np.int32)
    class_n = np.bincount(lab[known], minlength=C).astype(np.int64)
    none = np.iinfo(np.int64).max
    for rows, d2 in cellpoints.pair_blocks(p, 512):
        within = d2 <= e2[-1]
        within[rows - rows[0], rows] = False                                 # j != i (a coincident OTHER point stays)
        t = np.searchsorted(e2, d2, side='left')                             # the smallest t with d2 <= e2[t]
        counted = within & known[rows, None] & known[None, :]
        flat = (cls[rows, None] * C + cls[None, :]) * B + t
        pair_hist += np.bincount(flat[counted], minlength=C * C * B)
        for c in range(C):
            best = np.where(within & (lab[None, :] == c), d2, none).min(axis=1) if n else np.zeros(0, np.int64)
            nn_d2[rows, c] = np.where(best == none, -1, best)
    return pair_hist.reshape(C, C, B), nn_d2, class_n


def call(points, labels, num_classes, edges, pair_hist, nn_d2, class_n, bounds=None, device=0):
    """nuhtc_cell_spatial on torch tensors of cuda:`device` (points, labels, nn_d2 int32; pair_hist, class_n int64; contiguous) -> the
    library's return code, nothing raised: 0 or hip.E_INVALID / hip.E_HIP.  `edges` are HALF pixels and are read on the host (a sequence, an
    array or a tensor).  bounds = (x_min, y_min, x_max, y_max) of the points, computed on the host when not given."""
    import ctypes
    if hasattr(edges, 'cpu'):
        edges = edges.cpu().numpy()
    e = np.ascontiguousarray(np.asarray(edges).reshape(-1), np.int32)
    e_host = (ctypes.c_int32 * max(len(e), 1))(*e.tolist())
    return cellpoints.launch('nuhtc_cell_spatial', device, points, labels, (int(num_classes), e_host, len(e)), (pair_hist, nn_d2, class_n), bounds)


def build(points, labels, num_classes, edges, device=0):
    """The statistics of `points` (int (n, 2) half pixels, see cellpoints.quantize_centres) with `labels` (n,) on cuda:`device`: numpy in,
    (pair_hist int64 (C, C, B), nn_d2 int32 (n, C), class_n int64 (C,)) out.  There is no host route: without the library or a GPU this
    raises."""
    import torch
    C = int(num_classes)
    e = check_args(C, edges)
    p, lab, dev, p_d, lab_d, bounds = cellpoints.resident(points, labels, 'spatial statistics', device, bounded=False)
    n = len(p)
    out = [torch.zeros((C, C, len(e)), dtype=torch.int64, device=dev), torch.full((n, C), -1, dtype=torch.int32, device=dev),
           torch.zeros((C,), dtype=torch.int64, device=dev)]
    cellpoints.raise_for(call(p_d, lab_d, C, e, *out, bounds=bounds, device=device), 'nuhtc_cell_spatial')
    return tuple(t.cpu().numpy() for t in out)


def derive(pair_hist, nn_d2, labels, class_n, edges, area_px=None):
    """The statistics of the integers, in float64 -> dict:
      cumulative  int64 (C, C, B)    pairs with d <= e_t
      mean_within float64 (C, C, B)  cumulative / class_n[a]
      G           float64 (C, C, B)  the share of the points of class a whose nearest point of class b lies within e_t
      K, L        float64 (C, C, B)  only with area_px (px^2): K = area x cumulative / (class_n[a] x class_n[b]) in px^2 with the edges
                                     taken in px (the counts do not depend on the unit), L = sqrt(K / pi) in px.
    A class with no point gives zeros, never NaN.  No edge correction (see the module's docstring)."""
    ph = np.asarray(pair_hist, np.int64)
    C, B = ph.shape[0], ph.shape[2]
    e = np.asarray(edges, np.int64).reshape(-1)
    cn = np.asarray(class_n, np.int64).reshape(-1)
    nn = np.asarray(nn_d2, np.int64).reshape(-1, C)
    lab = np.asarray(labels, np.int64).reshape(-1)
    if ph.shape != (C, C, B) or len(e) != B or len(cn) != C or len(lab) != len(nn):
        raise ValueError('derive: pair_hist (C, C, B), nn_d2 (n, C), labels (n,), class_n (C,), edges (B,)')
    cum = np.cumsum(ph, axis=2)
    na = cn.astype(np.float64)
    inv_a = np.divide(1.0, na, out=np.zeros(C), where=na > 0)
    out = dict(cumulative=cum, mean_within=cum * inv_a[:, None, None])
    G = np.zeros((C, C, B), np.float64)
    reached = (nn[:, :, None] >= 0) & (nn[:, :, None] <= (e * e)[None, None, :])           # (n, C, B), integer compares
    for a in range(C):
        rows = lab == a
        if rows.any():
            G[a] = reached[rows].sum(axis=0) / float(rows.sum())
    out['G'] = G
    if area_px is not None:
        K = float(area_px) * cum * inv_a[:, None, None] * inv_a[None, :, None]
        out['K'] = K
        out['L'] = np.sqrt(K / np.pi)
    return out


def write_npz(path, nuclei_id, xy, label, edges, pair_hist, nn_d2, class_n, tiles_area_px):
    """<id>_nuclei_spatial.npz, row i for the i-th row of <id>_nuclei_feat.npz:
      nuclei_id   int64 (n,)      the nucleus's position in <id>.geojson
      xy          float64 (n, 2)  the unquantised centre in slide px (the coordinates of <id>_point.geojson)
      label       int64 (n,)
      edges_px    float64 (B,)    the bin edges in px (edges / 2)
      pair_hist   int64 (C, C, B), class_n int64 (C,), nn_d2 int32 (n, C): the integers of the definition
      nn_dist     float32 (n, C)  sqrt(nn_d2) / 2 in px; inf where nn_d2 is -1
      mean_within, G float64 (C, C, B): `derive`
      tiles_area_px float64 0-d: the area K and L rest on (the inferred tiles: tiles x step_size^2), and
      K_tiles_area, L_tiles_area float64 (C, C, B): `derive` with that area -- Ripley's K and L only as far as that area is the tissue's."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    pair_hist = np.ascontiguousarray(pair_hist, np.int64)
    class_n = np.ascontiguousarray(class_n, np.int64).reshape(-1)
    C = len(class_n)
    nn_d2 = np.ascontiguousarray(nn_d2, np.int32).reshape(-1, C)
    e = check_args(C, edges)
    if len(nn_d2) != len(head['label']) or pair_hist.shape != (C, C, len(e)):
        raise ValueError('write_npz: one row per nucleus, pair_hist (C, C, B)')
    d = derive(pair_hist, nn_d2, head['label'], class_n, e, area_px=tiles_area_px)
    with open(path, 'wb') as f:
        np.savez(f, **head, edges_px=e.astype(np.float64) / 2, pair_hist=pair_hist, nn_dist=distances_px(nn_d2),
                 class_n=class_n, nn_d2=nn_d2, mean_within=d['mean_within'], G=d['G'], tiles_area_px=np.asarray(float(tiles_area_px), np.float64),
                 K_tiles_area=d['K'], L_tiles_area=d['L'])
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)
