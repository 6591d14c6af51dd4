"""Nucleus density maps of a slide: class-wise kernel rasters of the nucleus centres -- "where on the slide", the question the other
per-slide analyses (who relates to whom: cellgraph.py, spatial.py, clusters.py, mst.py, proximity.py) do not answer.  A lymphocyte density
map (a TIL map), a tumour-cellularity map, a heat map to lay over the slide in a viewer.  With the integer kernel h * h - d2 (the
Epanechnikov kernel, un-normalised) a density map is exact integer arithmetic: a pure function of its input, bitwise repeatable.  Computed
on the GPU (csrc/celldensity.hip, `nuhtc_cell_density`); tools/infer_wsi.py --nuclei-density writes it as <id>_nuclei_density.npz.  Not
in the reference.

Definition.

Inputs.  n points in HALF pixels, int32 (n, 2), from `cellpoints.quantize_centres`, with |p| < 2**27 and 0 <= n <= 2**24; labels, int32, one
per point; C classes, 1 <= C <= 14; the bandwidth h in half pixels, an integer with 1 <= h <= 16384; the pitch s in half pixels, an integer
with 1 <= s <= 2**20; the window in lattice units, integers gx0, gy0, W, H with W, H >= 1, W * H <= 2**24 and every site coordinate
|g * s| < 2**28 (checked on the host in 64 bits); and the points' bounding box, computed by the caller as for the siblings.

Sites.  Site (u, v) of the window lies at q = ((gx0 + u) * s, (gy0 + v) * s).  The lattice is anchored at the slide's origin, not at the
points: maps from different runs and different radii align.

Values.  For every class c in 0..C-1 and every site:
  * count[c][v][u] is the number of points i with labels[i] == c and d2(q, p_i) <= h * h.  The radius is inclusive, as everywhere else.
  * weight[c][v][u] is the sum over those points of h * h - d2(q, p_i).
  * A point with a label outside 0..C-1 is counted nowhere.
  * A point exactly at distance h adds 1 to count and 0 to weight.

Bit budget.  |q - p| < 2**28 + 2**27, so the differences are exact int32; the box test against h comes before the products; each term is
at most 2**28, and with n <= 2**24 a weight stays below 2**52: weight is int64, count int32 (csrc/cellgrid_host.h has the argument).

Outputs, integers only.
  count   int32 (C, H, W)
  weight  int64 (C, H, W)
Both are always fully written on success, zeros included where nothing is in reach; with n == 0 both are all zeros.

Default window.  `window(bounds, h, s)` covers every site that can be non-zero: gx0 = ceil((x_min - h) / s), the last column is
floor((x_max + h) / s), the same in y.  The entry point itself accepts any window: a sub-window, one partly off the points, or one
nowhere near them (all zeros).

`density_reference` is the brute-force int64 restatement (every site against every row, no grid): the oracle the device result must EQUAL.
`derive` makes the float64 side on the host: the density per px^2, each class's share of the counts, the class totals, the Morisita-Horn
co-localisation of every class pair and each class's peak site.  Not done: no tissue-area normalisation and no edge correction -- a site
near the tissue border sees fewer nuclei, and nothing compensates for that."""
import numpy as np

from . import cellpoints
from .cellpoints import COORD_LIMIT, MAX_CLASSES, MAX_POINTS, MAX_R, centres, half_pixel_radius, quantize_centres  # noqa: F401 (re-exported)

MAX_SITES = 1 << 24
MAX_PITCH = 1 << 20
SITE_LIMIT = 1 << 28                  # |g * s| < 2**28 half pixels
INT_NAMES = ('count', 'weight')
DERIVED_KEYS = ('density_per_px2', 'share', 'class_total', 'colocalisation', 'peak_site')
NPZ_KEYS = ('nuclei_id', 'xy', 'label') + INT_NAMES + DERIVED_KEYS + ('bandwidth_px', 'pitch_px', 'origin_px', 'window')


def check_lattice(name, reach_word, reach_letter, max_sites, num_classes, r, s, win=None):
    """The argument check of every raster on this lattice (`name`: the module, for the messages; `reach_word`, `reach_letter`: what it calls r in
    words and in its signature; max_sites: its cap, a power of two): num_classes 1..14, r 1..16384 and s 1..2**20 half pixels, and, when given, the window (gx0, gy0, W, H):
    W, H >= 1, W * H <= max_sites and every site coordinate |g * s| < 2**28: ValueError otherwise."""
    whole = all(float(v) == int(v) for v in (num_classes, r, s))
    if not (whole and 1 <= int(num_classes) <= MAX_CLASSES and 1 <= int(r) <= MAX_R and 1 <= int(s) <= MAX_PITCH):
        raise ValueError(f'{name}: num_classes 1..{MAX_CLASSES}, {reach_word} 1..{MAX_R} and pitch 1..{MAX_PITCH} half pixels '
                         f'(got num_classes={num_classes}, {reach_letter}={r}, s={s})')
    if win is None:
        return
    if len(win) != 4 or not all(float(v) == int(v) for v in win):
        raise ValueError(f'{name}: the window is four integers gx0, gy0, W, H (got {win})')
    gx0, gy0, W, H = (int(v) for v in win)
    if W < 1 or H < 1 or W * H > max_sites:
        raise ValueError(f'{name}: a window of {W} x {H} sites; W, H >= 1 and at most 2**{max_sites.bit_length() - 1} sites: coarsen the pitch')
    if max(abs(gx0), abs(gx0 + W - 1), abs(gy0), abs(gy0 + H - 1)) * int(s) >= SITE_LIMIT:
        raise ValueError(f'{name}: a site lies outside |q| < 2**28 half pixels')


def check_args(num_classes, h, s, win=None):
    """`check_lattice` with this module's cap of 2**24 sites."""
    check_lattice('density', 'bandwidth', 'h', MAX_SITES, num_classes, h, s, win)


def window(bounds, h, s):
    """The default window (gx0, gy0, W, H) for points with bounds = (x_min, y_min, x_max, y_max): every site that can be non-zero, those
    with x_min - h <= g * s <= x_max + h and the same in y.  Floor and ceiling division on Python integers: negative coordinates come out
    right.  W or H is 0 when no site lies in the interval (a pitch above 2 h between two sites)."""
    x_min, y_min, x_max, y_max = (int(b) for b in bounds)
    h, s = int(h), int(s)
    gx0, gy0 = -((h - x_min) // s), -((h - y_min) // s)                      # ceil(a / s) = -floor(-a / s)
    return gx0, gy0, max((x_max + h) // s - gx0 + 1, 0), max((y_max + h) // s - gy0 + 1, 0)


def density_reference(points, labels, num_classes, h, s, win, block=4096):
    """The definition in int64: points int (n, 2) half pixels, labels int (n,), h and s in HALF pixels, win = (gx0, gy0, W, H) ->
    (count int32 (C, H, W), weight int64 (C, H, W)).  Every site against EVERY row, no grid, `block` sites at a time (a few (block, n)
    int64 temporaries).  Meant for about 1e4 sites by a few thousand points."""
    check_args(num_classes, h, s, win)
    p, lab = cellpoints.reference_points(points, labels, 'density_reference')
    C, h, s = int(num_classes), int(h), int(s)
    gx0, gy0, W, H = (int(v) for v in win)
    count, weight = np.zeros((C, H * W), np.int64), np.zeros((C, H * W), np.int64)
    v, u = np.divmod(np.arange(H * W, dtype=np.int64), W)
    qx, qy = (gx0 + u) * s, (gy0 + v) * s
    known = (lab >= 0) & (lab < C)
    order = np.argsort(lab[known], kind='stable')                            # the rows by class: a class is one run of columns below
    p, lab = p[known][order], lab[known][order]
    run = np.searchsorted(lab, np.arange(C + 1))
    block = max(1, min(int(block), (1 << 22) // max(len(p), 1)))              # a temporary of at most 32 MiB
    for k0 in range(0, H * W if len(p) else 0, block):
        sl = slice(k0, k0 + block)
        d2 = (qx[sl, None] - p[None, :, 0]) ** 2 + (qy[sl, None] - p[None, :, 1]) ** 2
        near = d2 <= h * h
        term = np.where(near, h * h - d2, 0)
        for c in range(C):
            count[c, sl] = near[:, run[c]:run[c + 1]].sum(1)
            weight[c, sl] = term[:, run[c]:run[c + 1]].sum(1)
    return count.astype(np.int32).reshape(C, H, W), weight.reshape(C, H, W)


def call(points, labels, num_classes, h, s, win, count, weight, bounds=None, device=0):
    """nuhtc_cell_density on torch tensors of cuda:`device` (contiguous; count int32 and weight int64 (C, H, W); h and s in HALF pixels,
    win = (gx0, gy0, W, H)) -> the library's return code, nothing raised: 0 or hip.E_INVALID / hip.E_HIP.
    bounds = (x_min, y_min, x_max, y_max) of the points, computed on the host when not given."""
    return cellpoints.launch('nuhtc_cell_density', device, points, labels, (int(num_classes), int(h), int(s)) + tuple(int(v) for v in win),
                             (count, weight), bounds)


def lattice_points(name, check, points, labels, num_classes, reach_px, pitch_px, win, device):
    """The opening of a `build` on this lattice (`name`: the module, for the messages; `check`: its check_args): the points and labels as
    cellpoints.as_points takes them, the caps on n and on the coordinates, r and s in half pixels, the window -- `win`, or the default one
    of the points' bounding box with at least one site each way ((0, 0, 1, 1) for no points) -- checked, and the upload
    -> (n, C, r, s, win, dev, points and labels on cuda:`device`, bounds)."""
    p, lab = cellpoints.as_points(points, labels, name)
    n, C, r, s = len(p), int(num_classes), half_pixel_radius(reach_px), half_pixel_radius(pitch_px)
    if n > MAX_POINTS:
        raise ValueError(f'{name}: at most 2**24 points (got {n})')
    check(C, r, s)
    if n and np.abs(p).max() >= COORD_LIMIT:
        raise ValueError(f'{name}: a coordinate lies outside |p| < 2**27')
    if win is None:
        win = window(cellpoints.bounds_of(p), r, s) if n else (0, 0, 1, 1)
        win = (win[0], win[1], max(win[2], 1), max(win[3], 1))
    win = tuple(int(v) for v in win)
    check(C, r, s, win)
    return (n, C, r, s, win) + tuple(cellpoints.upload(p, lab, device))


def lattice_npz(win, s, pitch_px):
    """What a writer says of the lattice (s the pitch in HALF pixels): pitch_px float64 0-d; origin_px float64 (2,), the px position of site
    (0, 0); window int64 (4,) gx0, gy0, W, H."""
    return dict(pitch_px=np.asarray(float(pitch_px), np.float64), origin_px=np.array([win[0] * s / 2, win[1] * s / 2], np.float64),
                window=np.asarray(win, np.int64))


def outputs(num_classes, win, device, fill=0):
    """The two output tensors of `call` for a window on `device`, every entry `fill`."""
    import torch
    shape = (int(num_classes), int(win[3]), int(win[2]))
    return [torch.full(shape, fill, dtype=t, device=device) for t in (torch.int32, torch.int64)]


def build(points, labels, num_classes, bandwidth_px, pitch_px, win=None, device=0):
    """The density rasters of `points` (int (n, 2) half pixels, see cellpoints.quantize_centres) with `labels` (n,) on cuda:`device`: numpy
    in, (count, weight, window) out.  Without `win` the window is the default one of the points' bounding box (one site at the origin for
    no points, or where the pitch steps over every site in reach); ValueError when it exceeds 2**24 sites.  There is no host route:
    without the library or a GPU this raises."""
    _, C, h, s, win, dev, p_d, lab_d, bounds = lattice_points('density', check_args, points, labels, num_classes, bandwidth_px, pitch_px, win, device)
    out = outputs(C, win, dev)
    cellpoints.raise_for(call(p_d, lab_d, C, h, s, win, *out, bounds=bounds, device=device), 'nuhtc_cell_density')
    return out[0].cpu().numpy(), out[1].cpu().numpy(), win


def derive(count, weight, h):
    """The float64 side of the integers (h in HALF pixels) -> dict, never a NaN:
      density_per_px2  float64 (C, H, W)  weight * 8 / (pi * h**4): the 2-D Epanechnikov normalisation is pi h^4 / 2 per half pixel squared,
                                          times 4 half pixels squared per px^2 -- nuclei per px^2
      share            float64 (C, H, W)  count[c] / the sum of count over the classes, 0 where that sum is 0 (class c's plane is the
                                          TIL-map style fraction)
      class_total      int64 (C,)         the sum of count over the sites
      colocalisation   float64 (C, C)     the Morisita-Horn index of every class pair over the sites: p_a = weight_a / sum(weight_a),
                                          MH[a][b] = 2 sum(p_a p_b) / (sum(p_a^2) + sum(p_b^2)), 0 where the denominator is 0
      peak_site        int64 (C, 2)       (u, v) of the first row-major maximum of weight[c], (-1, -1) where the plane is all zero"""
    cnt, wt = np.asarray(count, np.int64), np.asarray(weight, np.int64)
    if cnt.ndim != 3 or cnt.shape != wt.shape or (cnt < 0).any() or (wt < 0).any() or not 1 <= int(h) <= MAX_R:
        raise ValueError('derive: count and weight are (C, H, W), not negative, and h is 1..16384 half pixels')
    C, H, W = cnt.shape
    density = wt.astype(np.float64) * (8.0 / (np.pi * float(int(h)) ** 4))
    total = cnt.sum(0)
    share = np.zeros(cnt.shape, np.float64)
    np.divide(cnt, total[None], out=share, where=(total > 0)[None])
    mass = wt.reshape(C, -1).sum(1)
    prob = np.zeros((C, H * W), np.float64)
    np.divide(wt.reshape(C, -1), mass[:, None], out=prob, where=(mass > 0)[:, None])
    cross, square = prob @ prob.T, (prob * prob).sum(1)
    denom = square[:, None] + square[None, :]
    coloc = np.zeros((C, C), np.float64)
    np.divide(2 * cross, denom, out=coloc, where=denom > 0)
    peak = np.full((C, 2), -1, np.int64)
    for c in range(C):
        if mass[c] > 0:
            v, u = divmod(int(wt[c].argmax()), W)
            peak[c] = (u, v)
    return dict(density_per_px2=density, share=share, class_total=cnt.reshape(C, -1).sum(1), colocalisation=coloc, peak_site=peak)


def write_npz(path, nuclei_id, xy, label, count, weight, win, bandwidth_px, pitch_px):
    """<id>_nuclei_density.npz, the header row i for the i-th row of <id>_nuclei_graph.npz / <id>_nuclei_feat.npz:
      nuclei_id int64 (n,), xy float64 (n, 2) (the unquantised centre in slide px), label int64 (n,)
      count int32 (C, H, W), weight int64 (C, H, W): the integers of the definition
      the arrays of `derive` (DERIVED_KEYS)
      bandwidth_px float64 0-d, and pitch_px, origin_px and window of `lattice_npz`."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    count = np.ascontiguousarray(count, np.int32)
    weight = np.ascontiguousarray(weight, np.int64)
    h, s = half_pixel_radius(bandwidth_px), half_pixel_radius(pitch_px)
    win = tuple(int(v) for v in win)
    if count.ndim != 3 or count.shape != weight.shape:
        raise ValueError('write_npz: count and weight are (C, H, W)')
    check_args(count.shape[0], h, s, win)
    if count.shape[1:] != (win[3], win[2]):
        raise ValueError('write_npz: the rasters are not the window\'s H x W')
    d = derive(count, weight, h)
    with open(path, 'wb') as f:
        np.savez(f, **head, count=count, weight=weight, **d, bandwidth_px=np.asarray(float(bandwidth_px), np.float64), **lattice_npz(win, s, pitch_px))
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)
