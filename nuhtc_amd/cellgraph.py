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

MAX_K, MAX_R, MAX_CLASSES = 32, 16384, 14
COORD_LIMIT = 1 << 27                 # |p| < 2**27 half pixels
MAX_CELLS = 1 << 22

NPZ_KEYS = ('nuclei_id', 'xy', 'neighbors', 'dist', 'class_count', 'label', 'radius_px', 'k')


def centres(boxes):
    """boxes (n, 4) x0, y0, x1, y1 -> float64 (n, 2): the centres <id>_point.geojson writes."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    return np.ascontiguousarray(np.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2], 1))


def quantize_centres(boxes):
    """boxes (n, 4) x0, y0, x1, y1 -> int32 (n, 2) half-pixel node positions: rint(x0 + x1), rint(y0 + y1), half to even."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    p = np.rint(np.stack([b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1))
    if p.size and np.abs(p).max() >= COORD_LIMIT:
        raise ValueError('quantize_centres: a centre lies outside |p| < 2**27 half pixels')
    return np.ascontiguousarray(p.astype(np.int32))


def half_pixel_radius(radius_px):
    """The radius in half pixels: 2 R, which must be an integer."""
    r = int(round(2 * float(radius_px)))
    if r != 2 * float(radius_px):
        raise ValueError(f'radius {radius_px} px is not a whole number of half pixels')
    return r


def cell_side(x_min, y_min, x_max, y_max, r):
    """The grid cell side the device uses over the inclusive bounding box: the smallest multiple of r with at most 2**22 cells."""
    m = 1
    while ((int(x_max) - int(x_min)) // (m * r) + 1) * ((int(y_max) - int(y_min)) // (m * r) + 1) > MAX_CELLS:
        m += 1
    return m * r


def check_args(num_classes, r, k):
    if not (1 <= int(k) <= MAX_K and 1 <= int(r) <= MAX_R and 1 <= int(num_classes) <= MAX_CLASSES):
        raise ValueError(f'cell graph: k 1..{MAX_K}, r 1..{MAX_R} half pixels, num_classes 1..{MAX_CLASSES} (got k={k}, r={r}, num_classes={num_classes})')


def graph_reference(points, labels, num_classes, r, k):
    """The definition, pair by pair in int64: points int (n, 2) half pixels, labels int (n,), r in HALF pixels -> (neighbors, d2, class_count).
    O(n^2) time, rows in blocks of 512: meant for n of a few thousand or less."""
    check_args(num_classes, r, k)
    p = np.asarray(points, np.int64).reshape(-1, 2)
    lab = np.asarray(labels, np.int64).reshape(-1)
    n, C, k, r = len(p), int(num_classes), int(k), int(r)
    if len(lab) != n:
        raise ValueError('graph_reference: one label per point')
    if n and np.abs(p).max() >= COORD_LIMIT:
        raise ValueError('graph_reference: a coordinate lies outside |p| < 2**27')
    neighbors = np.full((n, k), -1, np.int32)
    d2_out = np.full((n, k), -1, np.int32)
    class_count = np.zeros((n, C), np.int32)
    onehot = (lab[:, None] == np.arange(C)[None, :]).astype(np.int64)
    idx = np.arange(n, dtype=np.int64)
    none = np.iinfo(np.int64).max
    for i0 in range(0, n, 512):
        rows = idx[i0:i0 + 512]
        dx = p[rows, None, 0] - p[None, :, 0]
        dy = p[rows, None, 1] - p[None, :, 1]
        d2 = dx * dx + dy * dy
        within = d2 <= r * r
        within[rows - i0, rows] = False                                      # j != i (a coincident OTHER point stays)
        class_count[rows] = within.astype(np.int64) @ onehot
        key = np.sort(np.where(within, (d2 << 32) | idx[None, :], none), axis=1)[:, :k]      # the total order (d2, j)
        got = key != none
        kk = key.shape[1]
        neighbors[rows, :kk] = np.where(got, key & 0xffffffff, -1)
        d2_out[rows, :kk] = np.where(got, key >> 32, -1)
    return neighbors, d2_out, class_count


def call(points, labels, num_classes, r, k, neighbors, d2, class_count, bounds=None, device=0):
    """nuhtc_cell_graph on torch tensors of cuda:`device` (int32, contiguous; r in HALF pixels) -> the library's return code, nothing
    raised: 0 or hip.E_INVALID / hip.E_HIP.  bounds = (x_min, y_min, x_max, y_max) of the points, computed here on the host when not given."""
    import ctypes
    import torch
    from . import hip
    lib = hip.load()
    n = int(points.shape[0])
    if bounds is None:
        if n:
            ph = points.cpu().numpy()
            bounds = (int(ph[:, 0].min()), int(ph[:, 1].min()), int(ph[:, 0].max()), int(ph[:, 1].max()))
        else:
            bounds = (0, 0, 0, 0)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    dev = torch.device('cuda', device)
    with torch.cuda.device(dev):
        return lib.nuhtc_cell_graph(int(device), vp(points), vp(labels), n, int(num_classes), int(r), int(k), *(int(b) for b in bounds),
                                    vp(neighbors), vp(d2), vp(class_count), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))


def build(points, labels, num_classes, radius_px, k, device=0):
    """The graph of `points` (int (n, 2) half pixels, see quantize_centres) with `labels` (n,) on cuda:`device`: numpy in,
    (neighbors int32 (n, k), d2 int32 (n, k), class_count int32 (n, num_classes)) out.  There is no host route: without the library or a
    GPU this raises."""
    import torch
    from . import hip
    p = np.ascontiguousarray(np.asarray(points).reshape(-1, 2), np.int32)
    if not np.array_equal(p, np.asarray(points).reshape(-1, 2)):
        raise ValueError('cell graph: the points are not int32 half pixels')
    lab = np.ascontiguousarray(np.asarray(labels).reshape(-1), np.int32)
    n, C, k, r = len(p), int(num_classes), int(k), half_pixel_radius(radius_px)
    if len(lab) != n:
        raise ValueError('cell graph: one label per point')
    check_args(C, r, k)
    dev = torch.device('cuda', device)
    bounds = (int(p[:, 0].min()), int(p[:, 1].min()), int(p[:, 0].max()), int(p[:, 1].max())) if n else None
    out = [torch.full((n, w), fill, dtype=torch.int32, device=dev) for w, fill in ((k, -1), (k, -1), (C, 0))]
    rc = call(torch.from_numpy(p).to(dev), torch.from_numpy(lab).to(dev), C, r, k, *out, bounds=bounds, device=device)
    if rc == hip.E_INVALID:
        raise ValueError('nuhtc_cell_graph: invalid arguments (a coordinate outside |p| < 2**27?)')
    if rc:
        raise RuntimeError(f'nuhtc_cell_graph failed ({rc})')
    return tuple(t.cpu().numpy() for t in out)


def distances_px(d2):
    """d2 int (n, k) half pixels^2 -> float32 (n, k): sqrt(d2) / 2 in pixels, computed in float64 and then cast; inf where d2 < 0 (no neighbour)."""
    d2 = np.asarray(d2, np.int64)
    return np.where(d2 >= 0, np.sqrt(np.maximum(d2, 0).astype(np.float64)) / 2, np.inf).astype(np.float32)


def write_npz(path, nuclei_id, xy, neighbors, d2, class_count, label, radius_px, k):
    """<id>_nuclei_graph.npz, row i for the i-th row of <id>_nuclei_feat.npz:
      nuclei_id   int64 (n,)     the nucleus's position in <id>.geojson (the numbering of <id>_nuclei_feat.npz)
      xy          float64 (n, 2) the unquantised centre in slide px (the coordinates of <id>_point.geojson)
      neighbors   int32 (n, k)   positions into THIS file's rows, -1 for none
      dist        float32 (n, k) sqrt(d2) / 2 in px; inf where neighbors == -1
      class_count int32 (n, C), label int64 (n,), radius_px and k as 0-d arrays."""
    nuclei_id = np.ascontiguousarray(nuclei_id, np.int64).reshape(-1)
    n, k = len(nuclei_id), int(k)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    neighbors = np.ascontiguousarray(neighbors, np.int32).reshape(-1, k)
    d2 = np.asarray(d2).reshape(-1, k)
    class_count = np.ascontiguousarray(class_count, np.int32)
    label = np.ascontiguousarray(label, np.int64).reshape(-1)
    if not (len(xy) == len(neighbors) == len(d2) == len(label) == len(class_count) == n) or class_count.ndim != 2:
        raise ValueError('write_npz: one row per nucleus in every field')
    if not np.array_equal(neighbors < 0, d2 < 0):
        raise ValueError('write_npz: neighbors and d2 disagree about where the lists end')
    with open(path, 'wb') as f:
        np.savez(f, nuclei_id=nuclei_id, xy=xy, neighbors=neighbors, dist=distances_px(d2), class_count=class_count, label=label,
                 radius_px=np.asarray(float(radius_px), np.float64), k=np.asarray(k, np.int64))
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    with np.load(path) as z:
        return {key: z[key] for key in NPZ_KEYS}
