"""Cell graph of a slide: for every nucleus its k nearest nuclei within a radius, how far away they are, and how many nuclei of each class
lie around it -- the edges to the nodes the slide path already writes (<id>.geojson, <id>_nuclei_feat.npz).  Built on the GPU
(csrc/cellgraph.hip, `nuhtc_cell_graph`); tools/infer_wsi.py --nuclei-graph writes it as <id>_nuclei_graph.npz.  Not in the reference.

Definition.

Node position.  The centre <id>_point.geojson writes, ((x0 + x1) / 2, (y0 + y1) / 2) of the record's box (head columns 0..3), quantised to
HALF pixels: px = rint(x0 + x1), py = rint(y0 + y1), both int32, the sums taken in float64 and rounded half to even as np.rint does
(`quantize_centres`).  All geometry from there on is integer arithmetic in half-pixel units, so every squared distance is exact and the
result is a pure function of the input.  Coordinates must satisfy |p| < 2**27; anything else is NUHTC_E_INVALID.

Neighbour list.  n points, a radius R in pixels, i.e. r = 2 R half pixels, an integer with 1 <= r <= 16384, and 1 <= k <= 32.
  * The neighbours of i are the points j != i with d2(i, j) = dx * dx + dy * dy <= r * r.  The radius is inclusive.
  * They are ordered by (d2, j) ascending and cut to the first k.
  * Coincident points (d2 == 0) are neighbours of each other.

Outputs.
  neighbors   int32 (n, k): the row index of each neighbour, -1 past the end of the list
  d2          int32 (n, k): the squared distance in half pixels^2, -1 past the end of the list
  class_count int32 (n, C): how many points of each label 0..C-1 lie within the radius of i -- all of them, not only the first k, and not
                            i itself.  A label outside 0..C-1 is a neighbour like any other and is counted in no class.

`graph_reference` is the brute-force int64 restatement (every pair, no grid): the oracle the device result must EQUAL.  The device bins the
points into a uniform grid whose cell side is the smallest multiple of r with at most 2**22 cells over the points' bounding box
(`cell_side`), so the 3 x 3 cells around a point hold its whole disc; the bounding box is computed here on the host (numpy min / max, O(n))
and passed in, the way the cross-tile merge passes its extent."""
import numpy as np

from . import cellpoints
from .cellpoints import COORD_LIMIT, MAX_CLASSES, MAX_R, centres, distances_px, half_pixel_radius, quantize_centres  # noqa: F401 (re-exported)

MAX_K = 32
MAX_CELLS = 1 << 22

NPZ_KEYS = ('nuclei_id', 'xy', 'neighbors', 'dist', 'class_count', 'label', 'radius_px', 'k')


def cell_side(x_min, y_min, x_max, y_max, r):
    """The grid cell side the device uses over the inclusive bounding box: the smallest multiple of r with at most 2**22 cells."""
    return cellpoints.cell_side(x_min, y_min, x_max, y_max, r, MAX_CELLS)


def check_args(num_classes, r, k):
    if not (1 <= int(k) <= MAX_K and 1 <= int(r) <= MAX_R and 1 <= int(num_classes) <= MAX_CLASSES):
        raise ValueError(f'cell graph: k 1..{MAX_K}, r 1..{MAX_R} half pixels, num_classes 1..{MAX_CLASSES} (got k={k}, r={r}, num_classes={num_classes})')


def graph_reference(points, labels, num_classes, r, k):
    """The definition, pair by pair in int64: points int (n, 2) half pixels, labels int (n,), r in HALF pixels -> (neighbors, d2, class_count).
    O(n^2) time, rows in blocks of 512: meant for n of a few thousand or less."""
    check_args(num_classes, r, k)
    p, lab = cellpoints.reference_points(points, labels, 'graph_reference')
    n, C, k, r = len(p), int(num_classes), int(k), int(r)
    neighbors = np.full((n, k), -1, np.int32)
    d2_out = np.full((n, k), -1, np.int32)
    class_count = np.zeros((n, C), np.int32)
    onehot = (lab[:, None] == np.arange(C)[None, :]).astype(np.int64)
    idx = np.arange(n, dtype=np.int64)
    none = np.iinfo(np.int64).max
    for rows, d2 in cellpoints.pair_blocks(p, 512):
        within = d2 <= r * r
        within[rows - rows[0], rows] = False                                 # j != i (a coincident OTHER point stays)
        class_count[rows] = within.astype(np.int64) @ onehot
        key = np.sort(np.where(within, (d2 << 32) | idx[None, :], none), axis=1)[:, :k]      # the total order (d2, j)
        got = key != none
        kk = key.shape[1]
        neighbors[rows, :kk] = np.where(got, key & 0xffffffff, -1)
        d2_out[rows, :kk] = np.where(got, key >> 32, -1)
    return neighbors, d2_out, class_count


def call(points, labels, num_classes, r, k, neighbors, d2, class_count, bounds=None, device=0):
    """nuhtc_cell_graph on torch tensors of cuda:`device` (int32, contiguous; r in HALF pixels) -> the library's return code, nothing
    raised: 0 or hip.E_INVALID / hip.E_HIP.  bounds = (x_min, y_min, x_max, y_max) of the points, computed on the host when not given."""
    return cellpoints.launch('nuhtc_cell_graph', device, points, labels, (int(num_classes), int(r), int(k)), (neighbors, d2, class_count), bounds)


def build(points, labels, num_classes, radius_px, k, device=0):
    """The graph of `points` (int (n, 2) half pixels, see quantize_centres) with `labels` (n,) on cuda:`device`: numpy in,
    (neighbors int32 (n, k), d2 int32 (n, k), class_count int32 (n, num_classes)) out.  There is no host route: without the library or a
    GPU this raises."""
    import torch
    C, k, r = int(num_classes), int(k), half_pixel_radius(radius_px)
    check_args(C, r, k)
    p, lab, dev, p_d, lab_d, bounds = cellpoints.resident(points, labels, 'cell graph', device, bounded=False)
    n = len(p)
    out = [torch.full((n, w), fill, dtype=torch.int32, device=dev) for w, fill in ((k, -1), (k, -1), (C, 0))]
    cellpoints.raise_for(call(p_d, lab_d, C, r, k, *out, bounds=bounds, device=device), 'nuhtc_cell_graph')
    return tuple(t.cpu().numpy() for t in out)


def write_npz(path, nuclei_id, xy, neighbors, d2, class_count, label, radius_px, k):
    """<id>_nuclei_graph.npz, row i for the i-th row of <id>_nuclei_feat.npz:
      nuclei_id   int64 (n,)     the nucleus's position in <id>.geojson (the numbering of <id>_nuclei_feat.npz)
      xy          float64 (n, 2) the unquantised centre in slide px (the coordinates of <id>_point.geojson)
      neighbors   int32 (n, k)   positions into THIS file's rows, -1 for none
      dist        float32 (n, k) sqrt(d2) / 2 in px; inf where neighbors == -1
      class_count int32 (n, C), label int64 (n,), radius_px and k as 0-d arrays."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    n, k = len(head['nuclei_id']), int(k)
    neighbors = np.ascontiguousarray(neighbors, np.int32).reshape(-1, k)
    d2 = np.asarray(d2).reshape(-1, k)
    class_count = np.ascontiguousarray(class_count, np.int32)
    if not (len(neighbors) == len(d2) == len(class_count) == n) or class_count.ndim != 2:
        raise ValueError('write_npz: one row per nucleus in every field')
    if not np.array_equal(neighbors < 0, d2 < 0):
        raise ValueError('write_npz: neighbors and d2 disagree about where the lists end')
    with open(path, 'wb') as f:
        np.savez(f, **head, neighbors=neighbors, dist=distances_px(d2), class_count=class_count,
                 radius_px=np.asarray(float(radius_px), np.float64), k=np.asarray(k, np.int64))
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)
