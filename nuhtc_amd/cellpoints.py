"""What the per-slide point analyses -- cellgraph.py, spatial.py, clusters.py, mst.py, proximity.py, alphacomplex.py, outline.py, density.py, territory.py, enrichment.py, and regions.py and margin.py with their second input, which hold the definitions -- do in the same way: half-pixel
nucleus centres with one label each, the grid over the host-computed bounding box, the pair loop of the brute-force references, the one
call into the library, the opening of a `build`, the capacity loop of a `build` whose device call may need more room than it was given
(`grow_to_fit`: proximity.py, alphacomplex.py, adjacency.py, regions.py, margin.py), the header of the .npz files, and the checks and the
census more than one of them holds
(slidepoints.py is the table that runs them for the slide path).  |p| < 2**27 and a reach of at most 16384 half pixels keep every squared distance
within reach an exact int32 on the device (csrc/cellgrid_host.h has the argument); the references restate it in int64."""
import numpy as np

MAX_R, MAX_CLASSES = 16384, 14
COORD_LIMIT = 1 << 27                 # |p| < 2**27 half pixels
MAX_POINTS = 1 << 24                  # of clusters, mst, proximity, density, territory and enrichment


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


def cell_side(x_min, y_min, x_max, y_max, reach, max_cells):
    """The grid cell side the device uses over the inclusive bounding box: the smallest multiple of the reach with at most max_cells cells."""
    m = 1
    while ((int(x_max) - int(x_min)) // (m * reach) + 1) * ((int(y_max) - int(y_min)) // (m * reach) + 1) > max_cells:
        m += 1
    return m * reach


def bounds_of(points):
    """points int (n, 2), n >= 1 -> (x_min, y_min, x_max, y_max) as Python integers."""
    return int(points[:, 0].min()), int(points[:, 1].min()), int(points[:, 0].max()), int(points[:, 1].max())


def as_points(points, labels, what):
    """-> (points int32 (n, 2), labels int32 (n,)), contiguous; ValueError, in the name of `what`, unless int32 half pixels, one label each."""
    raw = np.asarray(points).reshape(-1, 2)
    p = np.ascontiguousarray(raw, np.int32)
    if not np.array_equal(p, raw):
        raise ValueError(f'{what}: the points are not int32 half pixels')
    lab = np.ascontiguousarray(np.asarray(labels).reshape(-1), np.int32)
    if len(lab) != len(p):
        raise ValueError(f'{what}: one label per point')
    return p, lab


def check_radius_args(what, num_classes, r, by_class):
    """num_classes 1..14, r 1..16384 half pixels, by_class 0 or 1: ValueError, in the name of `what`, otherwise."""
    whole = all(float(v) == int(v) for v in (num_classes, r, by_class))
    if not (whole and 1 <= int(num_classes) <= MAX_CLASSES and 1 <= int(r) <= MAX_R and int(by_class) in (0, 1)):
        raise ValueError(f'{what}: num_classes 1..{MAX_CLASSES}, r 1..{MAX_R} half pixels, by_class 0 or 1 '
                         f'(got num_classes={num_classes}, r={r}, by_class={by_class})')


def class_pair_census(la, lb, C):
    """The labels int64 (m,) at the two ends of m edges -> int64 (C, C): the edges by [min label, max label] (upper triangle); an edge
    touching a label outside 0..C-1 is counted nowhere."""
    known = (la >= 0) & (la < C) & (lb >= 0) & (lb < C)
    census = np.zeros((C, C), np.int64)
    np.add.at(census, (np.minimum(la, lb)[known], np.maximum(la, lb)[known]), 1)
    return census


def check_edge_rows(edges, n):
    """edges int (m, 2) of a write_npz: ValueError unless every edge is (i, j) with i < j, both among the n rows of the file."""
    if len(edges) and not ((edges[:, 0] < edges[:, 1]).all() and edges.min() >= 0 and edges.max() < n):
        raise ValueError('write_npz: an edge is (i, j) with i < j, both rows of the file')


def reference_points(points, labels, what):
    """-> (points int64 (n, 2), labels int64 (n,)) for a brute-force reference; ValueError unless one label each and |p| < 2**27."""
    p = np.asarray(points, np.int64).reshape(-1, 2)
    lab = np.asarray(labels, np.int64).reshape(-1)
    if len(lab) != len(p):
        raise ValueError(f'{what}: one label per point')
    if len(p) and np.abs(p).max() >= COORD_LIMIT:
        raise ValueError(f'{what}: a coordinate lies outside |p| < 2**27')
    return p, lab


def pair_blocks(p, block):
    """Every ordered pair of p int64 (n, 2), `block` rows at a time: yields (rows int64 (b,), d2 int64 (b, n)), d2[a][j] from point rows[a]
    to point j (the point itself included).  In-place arithmetic: one (b, n) temporary beside d2, which the caller may keep."""
    idx = np.arange(len(p), dtype=np.int64)
    for i0 in range(0, len(p), block):
        rows = idx[i0:i0 + block]
        d2 = p[rows, None, 0] - p[None, :, 0]
        d2 *= d2
        dy = p[rows, None, 1] - p[None, :, 1]
        dy *= dy
        d2 += dy
        yield rows, d2


def launch(name, device, points, labels, scalars, outputs, bounds=None, extra=()):
    """The library's entry point `name` on torch tensors of cuda:`device` -> its return code, nothing raised.  Every entry point takes
    (device, points, labels, n, *scalars, *bounds, *outputs, *extra, stream): `outputs` are tensors, the stream is the device's current one,
    bounds = (x_min, y_min, x_max, y_max) of the points, computed here on the host when not given."""
    import ctypes
    import torch
    from . import hip
    fn = getattr(hip.load(), name)
    n = int(points.shape[0])
    if bounds is None:
        bounds = bounds_of(points.cpu().numpy()) if n else (0, 0, 0, 0)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    dev = torch.device('cuda', device)
    with torch.cuda.device(dev):
        return fn(int(device), vp(points), vp(labels), n, *scalars, *(int(b) for b in bounds), *(vp(t) for t in outputs), *extra,
                  ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))


def upload(p, lab, device):
    """as_points' arrays -> (the torch device, points and labels on it, the bounds for `launch`)."""
    import torch
    dev = torch.device('cuda', device)
    return dev, torch.from_numpy(p).to(dev), torch.from_numpy(lab).to(dev), (bounds_of(p) if len(p) else None)


def resident(points, labels, what, device, bounded=True):
    """How a `build` opens once its arguments are checked: as_points, at most MAX_POINTS of them when `bounded`, upload ->
    (p, lab) + upload's four."""
    p, lab = as_points(points, labels, what)
    if bounded and len(p) > MAX_POINTS:
        raise ValueError(f'{what}: at most 2**24 points (got {len(p)})')
    return (p, lab) + upload(p, lab, device)


def raise_for(rc, name):
    """The return code of `launch` as an exception: ValueError for hip.E_INVALID, RuntimeError for anything else but 0."""
    from . import hip
    if rc == hip.E_INVALID:
        raise ValueError(f'{name}: invalid arguments (a coordinate outside |p| < 2**27?)')
    if rc:
        raise RuntimeError(f'{name} failed ({rc})')


def first_edge_cap(n, per_point=4):
    """The rows of capacity of the first call of an analysis that returns an edge list: per_point * n + 64.  A planar graph has fewer than
    3 n edges; proximity.py and alphacomplex.py take 4 n (coincident and cocircular points add to a triangulation's count), adjacency.py
    3 n (a first guess on a lattice).  The device says how many there are when this is too few."""
    return int(per_point) * int(n) + 64


def grow_to_fit(call, make_outputs, first_cap, entry_name, what, limit=1 << 31, refuse=None, unit='edges'):
    """The capacity protocol of the project, once -- the edge lists of proximity.py, alphacomplex.py and adjacency.py, and the (edge, slab)
    records of regions.py and margin.py: the first call has room for first_cap of them; with m > cap the device has written nothing
    and says how many there are, and ONE second call has room for exactly that many.  call(cap, out) -> (rc, m, *more) never raises;
    make_outputs(cap) -> out (the same tensors again where they do not depend on cap).  -> (out, m, more, calls).  raise_for after each
    call; ValueError in the name of `what` for m >= limit (None: no such limit, where the device bounds m itself) -- or, for a caller
    with another bound and wording, with the message refuse(m) returns (None: m is fine); RuntimeError when the second call counts
    another m of `unit`."""
    cap, calls = int(first_cap), 1
    out = make_outputs(cap)
    rc, m, *more = call(cap, out)
    raise_for(rc, entry_name)
    if m > cap:
        if refuse and refuse(m):
            raise ValueError(refuse(m))
        if not refuse and limit is not None and m >= limit:
            raise ValueError(f'{what}: {m} edges, more than 2**31 - 1 (many coincident points)')
        cap, calls = m, 2
        out = make_outputs(cap)
        rc, m, *more = call(cap, out)
        raise_for(rc, entry_name)
        if m != cap:
            raise RuntimeError(f'{entry_name}: {m} {unit} on the second call, {cap} on the first')
    return out, m, tuple(more), calls


def distances_px(d2):
    """d2 int, any shape, half pixels^2 -> float32: sqrt(d2) / 2 in pixels, computed in float64 and then cast; inf where d2 < 0 (none)."""
    d2 = np.asarray(d2, np.int64)
    return np.where(d2 >= 0, np.sqrt(np.maximum(d2, 0).astype(np.float64)) / 2, np.inf).astype(np.float32)


def npz_header(nuclei_id, xy, label):
    """-> dict(nuclei_id int64 (n,), xy float64 (n, 2), label int64 (n,)) of every <id>_nuclei_*.npz; ValueError unless one row each."""
    nuclei_id = np.ascontiguousarray(nuclei_id, np.int64).reshape(-1)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    label = np.ascontiguousarray(label, np.int64).reshape(-1)
    if not len(xy) == len(label) == len(nuclei_id):
        raise ValueError('write_npz: one row per nucleus in nuclei_id, xy and label')
    return dict(nuclei_id=nuclei_id, xy=xy, label=label)


def read_npz(path, keys):
    """-> dict of the arrays `keys` of a file one of the write_npz functions wrote."""
    with np.load(path) as z:
        return {key: z[key] for key in keys}
