"""Tissue segmentation and tissue-restricted tile coordinates for the WSI path (host side, numpy/scipy).

Reference: tools/wsi_core/WholeSlideImage.py:105-199 `segmentTissue` (HSV saturation -> median blur -> threshold ->
morphological close -> contours with holes -> area filter), :407-493 `process_contour` (grid over the contour's bounding box,
kept where the contour check passes and the patch centre is not inside a hole), tools/wsi_core/util_classes.py:48-111 (the
`basic` / `center` / `four_pt` / `four_pt_hard` checks), parameters of tools/infer_wsi.py:385-389
(sthresh 8, mthresh 7, close 4, a_t 100, a_h 16, max_n_holes 8, use_padding, four_pt).

The reference does all of this with OpenCV on an OpenSlide pyramid level; neither library is available here, so the OpenCV
steps are restated (8-bit RGB->HSV saturation in OpenCV's fixed point, medianBlur with replicated borders, rectangular
close anchored at size//2, border following for outer contours and holes, shoelace contourArea, boundingRect,
pointPolygonTest) -- PARITY UNPINNED against cv2 itself; checked against the independent scalar restatements of the same OpenCV
routines in oracle/cv_ops.py and the Suzuki-Abe oracle (tests/test_oracle_cv.py), plus behaviour on synthetic slides.  Slides are arrays: the
segmentation level is a strided view of the level-0 image (`scale` = its downsample factor).
"""
import numpy as np
from scipy import ndimage

from .contours import trace_outer_contour

SEG_PARAMS = dict(sthresh=8, sthresh_up=255, mthresh=7, close=4, use_otsu=False)      # tools/infer_wsi.py:385-386
FILTER_PARAMS = dict(a_t=100, a_h=16, max_n_holes=8)                                  # :387


# ----------------------------------------------------------------------------- OpenCV restatements
def saturation_u8(rgb):
    """S channel of cv2.cvtColor(img, COLOR_RGB2HSV) for uint8 input: (v - min) * sdiv_table[v] in 12-bit fixed point,
    sdiv_table[v] = round((255 << 12) / v)."""
    a = np.asarray(rgb)[..., :3].astype(np.int64)
    v = a.max(-1)
    diff = v - a.min(-1)
    sdiv = np.zeros(256, np.int64)
    sdiv[1:] = np.rint((255 << 12) / np.arange(1, 256)).astype(np.int64)
    return ((diff * sdiv[v] + (1 << 11)) >> 12).astype(np.uint8)


def median_blur(img, k):
    """cv2.medianBlur(img, k): k x k median, replicated borders."""
    return ndimage.median_filter(img, size=k, mode='nearest')


def otsu_threshold(img):
    """Threshold value of cv2.threshold(..., THRESH_OTSU) on uint8: maximises the between-class variance."""
    hist = np.bincount(img.reshape(-1), minlength=256).astype(np.float64)
    total = hist.sum()
    mu = (hist * np.arange(256)).sum() / total
    best, best_t, q1, mu1 = 0.0, 0, 0.0, 0.0
    for t in range(256):
        p = hist[t] / total
        mu1 = (q1 * mu1 + t * p) / (q1 + p) if q1 + p > 0 else 0.0
        q1 += p
        q2 = 1.0 - q1
        if min(q1, q2) < 1e-12 or max(q1, q2) > 1.0 - 1e-12:
            continue
        mu2 = (mu - q1 * mu1) / q2
        s = q1 * q2 * (mu1 - mu2) ** 2
        if s > best:
            best, best_t = s, t
    return best_t


def otsu_threshold_hist(hist):
    """`otsu_threshold` on a given 256-bin histogram (the device route counts the median plane on the GPU and runs this loop on the host)."""
    hist = np.asarray(hist).reshape(-1).astype(np.float64)
    total = hist.sum()
    mu = (hist * np.arange(256)).sum() / total
    best, best_t, q1, mu1 = 0.0, 0, 0.0, 0.0
    for t in range(256):
        p = hist[t] / total
        mu1 = (q1 * mu1 + t * p) / (q1 + p) if q1 + p > 0 else 0.0
        q1 += p
        q2 = 1.0 - q1
        if min(q1, q2) < 1e-12 or max(q1, q2) > 1.0 - 1e-12:
            continue
        mu2 = (mu - q1 * mu1) / q2
        s = q1 * q2 * (mu1 - mu2) ** 2
        if s > best:
            best, best_t = s, t
    return best_t


def morph_close(binary, k):
    """cv2.morphologyEx(img, MORPH_CLOSE, ones((k, k))): dilate then erode with the anchor at k//2.  The erosion window
    covers offsets -k//2 .. k-k//2-1; OpenCV's dilation reflects kernel and anchor (offsets -(k-k//2-1) .. k//2), which keeps
    an even-sized close from shifting the image -- the same convention as scipy's grey_dilation / grey_erosion pair.  Borders
    never win (0 for the dilation, 255 for the erosion)."""
    d = ndimage.grey_dilation(binary, size=(k, k), mode='constant', cval=0)
    return ndimage.grey_erosion(d, size=(k, k), mode='constant', cval=255)


def contour_area(contour):
    """cv2.contourArea: |shoelace| over the vertex list."""
    c = np.asarray(contour, np.float64).reshape(-1, 2)
    if len(c) < 3:
        return 0.0
    x, y = c[:, 0], c[:, 1]
    return float(abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))) * 0.5)


def bounding_rect(contour):
    c = np.asarray(contour).reshape(-1, 2)
    x0, y0 = c.min(0)
    x1, y1 = c.max(0)
    return int(x0), int(y0), int(x1 - x0 + 1), int(y1 - y0 + 1)


def points_polygon_test(contour, pts, chunk=512):
    """cv2.pointPolygonTest(contour, pt, False) for many points: +1 inside, 0 on an edge or vertex, -1 outside."""
    c = np.asarray(contour, np.float64).reshape(-1, 2)
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    out = np.full(len(pts), -1, np.int64)
    if len(c) == 0:
        return out
    x1, y1 = c[:, 0][None, :], c[:, 1][None, :]
    x2, y2 = np.roll(x1, -1, 1), np.roll(y1, -1, 1)
    for i in range(0, len(pts), chunk):
        px, py = pts[i:i + chunk, 0][:, None], pts[i:i + chunk, 1][:, None]
        cross = (x2 - x1) * (py - y1) - (y2 - y1) * (px - x1)
        on = (cross == 0) & (np.minimum(x1, x2) <= px) & (px <= np.maximum(x1, x2)) & (np.minimum(y1, y2) <= py) & (py <= np.maximum(y1, y2))
        straddle = (y1 <= py) != (y2 <= py)
        with np.errstate(divide='ignore', invalid='ignore'):
            xi = x1 + (py - y1) * (x2 - x1) / (y2 - y1)
        inside = (np.count_nonzero(straddle & (px < xi), axis=1) & 1).astype(bool)
        out[i:i + chunk] = np.where(on.any(1), 0, np.where(inside, 1, -1))
    return out


def point_polygon_test(contour, pt):
    return int(points_polygon_test(contour, [pt])[0])


def points_polygon_test_int(contour, pts, chunk=512):
    """`points_polygon_test` for integer input in exact int64 arithmetic -- the arithmetic of the device kernel (csrc/tissue.hip), restated in
    numpy.  One cross product per edge decides both questions: zero inside the edge's box is "on the edge"; for an edge with exactly one end
    at y <= py, the float test px < x1 + (py - y1) * (x2 - x1) / dy is (px - x1) * dy < (py - y1) * (x2 - x1) for dy > 0 and > for dy < 0, i.e.
    the sign of the cross product against the sign of dy.  The two sides are integers: equal means on the edge (where `on` decides), otherwise the
    float sides differ by at least 1 / |dy|, far beyond float64 rounding -- so this returns what `points_polygon_test` returns."""
    c = np.asarray(contour, np.int64).reshape(-1, 2)
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    out = np.full(len(pts), -1, np.int64)
    if len(c) == 0:
        return out
    x1, y1 = c[:, 0][None, :], c[:, 1][None, :]
    x2, y2 = np.roll(x1, -1, 1), np.roll(y1, -1, 1)
    dx, dy = x2 - x1, y2 - y1
    for i in range(0, len(pts), chunk):
        px, py = pts[i:i + chunk, 0][:, None], pts[i:i + chunk, 1][:, None]
        cross = dx * (py - y1) - dy * (px - x1)
        on = (cross == 0) & (np.minimum(x1, x2) <= px) & (px <= np.maximum(x1, x2)) & (np.minimum(y1, y2) <= py) & (py <= np.maximum(y1, y2))
        straddle = (y1 <= py) != (y2 <= py)
        left = np.where(dy > 0, cross > 0, cross < 0)
        inside = (np.count_nonzero(straddle & left, axis=1) & 1).astype(bool)
        out[i:i + chunk] = np.where(on.any(1), 0, np.where(inside, 1, -1))
    return out


# ----------------------------------------------------------------------------- device route (csrc/tissue.hip)
_COORD_LIMIT = 1 << 30          # the kernels are exact while differences fit 32 bits


def _device_index(device):
    """`device` (int, 'cuda:N' or torch.device) -> its index.  There is no fallback: without a GPU the device route is an error."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('the device route of tissue segmentation needs a GPU (none is visible); device=None is the host route')
    if isinstance(device, (int, np.integer)):
        return int(device)
    return torch.device(device).index or 0


def _int32_coords(a, what):
    a = np.asarray(a)
    if a.dtype.kind not in 'iu':
        raise TypeError(f'{what}: integer coordinates expected, got {a.dtype}')
    a = a.astype(np.int64).reshape(-1, 2)
    if len(a) and np.abs(a).max() > _COORD_LIMIT:
        raise ValueError(f'{what}: coordinates beyond +-2^30')
    return np.ascontiguousarray(a, np.int32)


def _dev_call(device, fn):
    """Runs fn(torch device, upload, stream pointer) with `device` current; upload(ndarray) -> tensor on it."""
    import ctypes
    import torch
    dev = torch.device('cuda', _device_index(device))
    with torch.cuda.device(dev):
        return fn(dev, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))


def tissue_mask_device(img, sthresh=8, sthresh_up=255, mthresh=7, close=4, use_otsu=False, device=0, planes=False):
    """`segment_tissue` up to the binary image its contours are found on, on the GPU (nuhtc_tissue_mask): saturation_u8 -> median_blur ->
    threshold -> morph_close, each byte for byte the host function.  img: (H, W, C >= 3) uint8, channels past the third ignored.  With
    Otsu the device counts the median plane, the host runs `otsu_threshold_hist`, and a second launch thresholds and closes.
    Returns the (H, W) uint8 binary image; with `planes` a dict(binary, sat, med, hist, thr) for the tests."""
    import ctypes
    import torch
    from . import hip
    img = np.asarray(img)
    if img.ndim != 3 or img.shape[2] < 3 or img.dtype != np.uint8:
        raise ValueError(f'an (H, W, C >= 3) uint8 image expected, got {img.shape} {img.dtype}')
    H, W, C = img.shape
    lib = hip.load()

    def run(dev, up, stream):
        vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        d_img = up(img)
        new = lambda: torch.empty((H, W), dtype=torch.uint8, device=dev)
        d_bin, d_med, d_sat = new(), new() if planes or use_otsu else None, new() if planes else None
        d_hist = torch.empty(256, dtype=torch.int64, device=dev)
        call = lambda stage, thr: lib.nuhtc_tissue_mask(dev.index, vp(d_img), H, W, W * C, C, stage, int(mthresh), int(thr), int(sthresh_up), int(close),
                                                        vp(d_bin), vp(d_sat), vp(d_med), vp(d_hist), stream)
        thr = sthresh
        if use_otsu:
            rc = call(hip.TISSUE_MEDIAN, 0)
            if rc == 0:
                thr = otsu_threshold_hist(d_hist.cpu().numpy())
                rc = call(hip.TISSUE_THRESHOLD, thr)
        else:
            rc = call(hip.TISSUE_ALL, thr)
        if rc:
            raise RuntimeError(f'nuhtc_tissue_mask failed ({rc})')
        binary = d_bin.cpu().numpy()
        if not planes:
            return binary
        return dict(binary=binary, sat=d_sat.cpu().numpy(), med=d_med.cpu().numpy(), hist=d_hist.cpu().numpy(), thr=thr)
    return _dev_call(device, run)


def points_polygon_test_device(contour, pts, device=0):
    """`points_polygon_test` of integer points against an integer contour on the GPU (nuhtc_points_polygon_test) -> int64 +1 / 0 / -1."""
    import ctypes
    import torch
    from . import hip
    c, p = _int32_coords(contour, 'contour'), _int32_coords(pts, 'pts')
    if len(c) == 0:
        return np.full(len(p), -1, np.int64)
    if len(p) == 0:
        return np.zeros(0, np.int64)
    lib = hip.load()

    def run(dev, up, stream):
        d_c, d_p = up(c), up(p)
        out = torch.empty(len(p), dtype=torch.int8, device=dev)
        rc = lib.nuhtc_points_polygon_test(dev.index, ctypes.c_void_p(d_c.data_ptr()), len(c), ctypes.c_void_p(d_p.data_ptr()), len(p),
                                           ctypes.c_void_p(out.data_ptr()), stream)
        if rc:
            raise RuntimeError(f'nuhtc_points_polygon_test failed ({rc})')
        return out.cpu().numpy().astype(np.int64)
    return _dev_call(device, run)


def grid_in_contour_device(contour, holes, start_xy, n_xy, step_size, patch_size, contour_fn='four_pt', device=0):
    """`in_contour(...) & ~in_holes(...)` over the grid start + (ix, iy) * step of one contour, on the GPU (nuhtc_grid_in_contour): bool
    (nx * ny,) in the meshgrid(indexing='ij') order of `contour_coords`.  No candidate list is uploaded.  An odd patch size makes the hole
    test's patch_size / 2 a half-integer: every coordinate is then doubled, which keeps the arithmetic integer and the answers the same."""
    import ctypes
    import torch
    from . import hip
    nx, ny = int(n_xy[0]), int(n_xy[1])
    if nx * ny == 0:
        return np.zeros(0, bool)
    m = 2 if patch_size % 2 else 1
    c = None if contour is None else _int32_coords(np.asarray(contour).astype(np.int64) * m, 'contour')
    hs = [_int32_coords(np.asarray(h).astype(np.int64) * m, 'hole') for h in (holes or [])]
    hs = [h for h in hs if len(h)]                       # (an empty hole contains no point)
    offs = np.asarray(_check_offsets(patch_size, contour_fn), np.int32).reshape(-1, 2) * m
    hole_off = np.zeros(len(hs) + 1, np.int64)
    hole_off[1:] = np.cumsum([len(h) for h in hs])
    lib = hip.load()

    def run(dev, up, stream):
        vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        if c is not None and len(c) == 0:                # an empty contour contains no point (points_polygon_test: all -1)
            return np.zeros(nx * ny, bool)
        d_c = up(c) if c is not None else None
        d_h = up(np.concatenate(hs, 0)) if hs else None
        keep = torch.empty(nx * ny, dtype=torch.uint8, device=dev)
        centre = int(patch_size) * m // 2                # patch_size / 2 in the (doubled) coordinates
        rc = lib.nuhtc_grid_in_contour(dev.index, int(start_xy[0]) * m, int(start_xy[1]) * m, nx, ny, int(step_size) * m,
                                       offs.ctypes.data_as(ctypes.c_void_p), len(offs), 1 if contour_fn == 'four_pt_hard' else 0,
                                       vp(d_c), 0 if c is None else len(c), vp(d_h), int(hole_off[-1]), hole_off.ctypes.data_as(ctypes.c_void_p), len(hs),
                                       centre, centre, vp(keep), stream)
        if rc:
            raise RuntimeError(f'nuhtc_grid_in_contour failed ({rc})')
        return keep.cpu().numpy().astype(bool)
    return _dev_call(device, run)


def find_contours_ccomp(binary):
    """cv2.findContours(img, RETR_CCOMP, CHAIN_APPROX_NONE) reduced to what `segmentTissue` uses: for every 8-connected
    foreground component its outer border (all border pixels, (n,2) x,y) and the borders of the holes inside it (4-connected
    background components that do not reach the image edge; a hole's border runs over the foreground pixels around it)."""
    fg = np.asarray(binary) > 0
    lab, n = ndimage.label(fg, structure=np.ones((3, 3), int))
    bg_lab, nb = ndimage.label(~fg)                                   # 4-connectivity
    edge = np.unique(np.concatenate([bg_lab[0], bg_lab[-1], bg_lab[:, 0], bg_lab[:, -1]]))
    hole_ids = [i for i in range(1, nb + 1) if i not in set(edge.tolist())]
    holes_of = {i: [] for i in range(1, n + 1)}
    slices = ndimage.find_objects(bg_lab)
    for h in hole_ids:
        sl = slices[h - 1]
        ys, xs = sl[0], sl[1]
        y0, y1 = max(ys.start - 1, 0), min(ys.stop + 1, fg.shape[0])
        x0, x1 = max(xs.start - 1, 0), min(xs.stop + 1, fg.shape[1])
        hm = bg_lab[y0:y1, x0:x1] == h
        yy, xx = np.nonzero(hm)
        owner = 0
        for dy, dx in ((0, -1), (-1, 0), (0, 1), (1, 0)):              # a 4-neighbour of the hole is foreground of its parent
            py, px = yy[0] + dy + y0, xx[0] + dx + x0
            if 0 <= py < fg.shape[0] and 0 <= px < fg.shape[1] and lab[py, px]:
                owner = lab[py, px]
                break
        if owner == 0:
            continue
        # the hole border runs over the foreground pixels around the hole, followed from the hole's side (Suzuki-Abe: start at the
        # foreground pixel left of the hole's first raster pixel, whose east neighbour is the hole)
        c = _follow_hole_border(fg, int(yy[0]) + y0, int(xx[0]) + x0 - 1)
        holes_of[owner].append(c)
    out = []
    obj = ndimage.find_objects(lab)
    for i in range(1, n + 1):
        sl = obj[i - 1]
        comp = lab[sl] == i
        c = _trace_all(comp) + np.array([sl[1].start, sl[0].start])
        out.append((c, holes_of[i][::-1]))
    # cv2's list order: every new border is linked at the head of its parent's list, so the outer borders come in the REVERSE of
    # the order the raster scan finds them (scipy labels components and background regions in scan order of their first pixel),
    # and so do the holes of one component
    return out[::-1]


_DXY = ((1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1))     # chain codes counter-clockwise from east (dx, dy), y down


def _follow_hole_border(fg, y0, x0):
    """Suzuki-Abe border following (CHAIN_APPROX_NONE) of the hole border that starts at foreground pixel (y0, x0) whose east
    neighbour belongs to the hole: every foreground pixel 4-adjacent to the hole, in following order, as (n, 2) (x, y).  Unlike
    the outer trace of the dilated hole, it keeps the foreground pixel inside a concave corner of the hole."""
    H, W = fg.shape

    def on(y, x):
        return 0 <= y < H and 0 <= x < W and fg[y, x]
    s = 0                                      # the east neighbour is the hole: search clockwise from it
    k = 0
    while True:
        s = (s - 1) & 7
        k += 1
        if on(y0 + _DXY[s][1], x0 + _DXY[s][0]):
            break
        if k == 8:
            return np.array([[x0, y0]], np.int64)
    y1, x1 = y0 + _DXY[s][1], x0 + _DXY[s][0]
    pts = []
    cy, cx = y0, x0
    while True:
        while True:                            # counter-clockwise from the code after the one pointing back
            s = (s + 1) & 7
            ny, nx = cy + _DXY[s][1], cx + _DXY[s][0]
            if on(ny, nx):
                break
        pts.append((cx, cy))
        if (ny, nx) == (y0, x0) and (cy, cx) == (y1, x1):
            break
        cy, cx = ny, nx
        s = (s + 4) & 7
    return np.array(pts, np.int64)


def _trace_all(mask):
    """Outer border with every border pixel (CHAIN_APPROX_NONE): the Moore trace of contours.py without its compression."""
    m = np.asarray(mask, bool)
    # trace_outer_contour compresses collinear runs; re-expand the runs between consecutive vertices (unit 8-steps)
    v = trace_outer_contour(m)
    if len(v) <= 1:
        return v
    pts = []
    for a, b in zip(v, np.roll(v, -1, 0)):
        d = b - a
        steps = int(max(abs(d[0]), abs(d[1])))
        if steps == 0:
            continue
        s = d // steps
        for t in range(steps):
            pts.append(a + s * t)
    return np.array(pts, np.int64)


# ----------------------------------------------------------------------------- segmentTissue
def segment_tissue(image, scale=64, sthresh=8, sthresh_up=255, mthresh=7, close=4, use_otsu=False, filter_params=None,
                   ref_patch_size=512, exclude_ids=(), keep_ids=(), level_image=None, device=None):
    """`WholeSlideImage.segmentTissue` on an RGB array.  `scale`: downsample factor of the segmentation level (the reference
    picks the pyramid level closest to 64x).  Returns (contours_tissue, holes_tissue) in level-0 pixels: lists of (n,2) int32
    contours and, per contour, a list of hole contours.
    `level_image`: the segmentation level of a pyramid slide as the reference reads it (`read_region((0, 0), seg_level, level_dim)`, :159);
    `scale` is then that level's (x, y) downsample pair (`_assertLevelDownsamples`, :378-386): the area thresholds use scale[0] (:176) and
    the contours go back to level 0 by `cont * scale` truncated to int32 (`scaleContourDim`, :371).
    `device`: a GPU (index, 'cuda:N' or torch.device) computes the binary image (`tissue_mask_device`, byte-equal); None = the host code."""
    fp = dict(FILTER_PARAMS if filter_params is None else filter_params)
    if level_image is not None:
        scale = np.asarray(scale, np.float64).reshape(-1)
        scale = np.array([scale[0], scale[-1]])
        img = np.asarray(level_image)[:, :, :3]
        ref_scale = float(scale[0])
    else:
        scale = int(scale)
        img = np.asarray(image[::scale, ::scale])          # (sliced first: a TIFF slide serves this from its pyramid, nuhtc_amd.tiffslide)
        ref_scale = scale
    if device is not None:
        binary = tissue_mask_device(img, sthresh, sthresh_up, mthresh, close, use_otsu, device)
    else:
        sat = saturation_u8(img)
        med = median_blur(sat, mthresh)
        thr = otsu_threshold(med) if use_otsu else sthresh
        binary = np.where(med > thr, np.uint8(min(sthresh_up, 255)), np.uint8(0))
        if close > 0:
            binary = morph_close(binary, close)
    scaled_ref = round(ref_patch_size / ref_scale)
    a_t, a_h = fp['a_t'] * scaled_ref, fp['a_h'] * scaled_ref
    fore, holes = [], []
    for cont, hs in find_contours_ccomp(binary):
        a = contour_area(cont) - sum(contour_area(h) for h in hs)
        if a == 0 or not a > a_t:
            continue
        hs = sorted(hs, key=contour_area, reverse=True)[:fp['max_n_holes']]
        fore.append(cont)
        holes.append([h for h in hs if contour_area(h) > a_h])
    fore = [np.array(c * scale, dtype='int32') for c in fore]
    holes = [[np.array(h * scale, dtype='int32') for h in hs] for hs in holes]
    ids = (set(keep_ids) if len(keep_ids) else set(range(len(fore)))) - set(exclude_ids)
    ids = sorted(ids)
    return [fore[i] for i in ids], [holes[i] for i in ids]


# ----------------------------------------------------------------------------- tile coordinates
def _check_offsets(patch_size, fn, center_shift=0.5):
    """Offsets from a tile origin of the points util_classes.py:53-111 test: 'basic' (corner), 'center', 'four_pt*'."""
    if fn == 'basic':
        return [(0, 0)]
    h = patch_size // 2
    if fn == 'center':
        return [(h, h)]
    s = int(patch_size // 2 * center_shift)
    return [(h - s, h - s), (h + s, h + s), (h + s, h - s), (h - s, h + s)] if s > 0 else [(h, h)]


def in_contour(contour, pts, patch_size, contour_fn='four_pt'):
    """For tile origins `pts` (n,2): 'four_pt' passes when any of the 4 points is inside or on the contour, 'four_pt_hard'
    when all are; 'basic' / 'center' test one point."""
    pts = np.asarray(pts).reshape(-1, 2)
    tests = np.stack([points_polygon_test(contour, pts + np.array(o)) >= 0 for o in _check_offsets(patch_size, contour_fn)], 1)
    return tests.all(1) if contour_fn == 'four_pt_hard' else tests.any(1)


def in_holes(holes, pts, patch_size):
    """WholeSlideImage.isInHoles (:353-358): patch centre strictly inside a hole."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    hit = np.zeros(len(pts), bool)
    for h in holes:
        hit |= points_polygon_test(h, pts + patch_size / 2) > 0
    return hit


def contour_coords(contour, holes, image_wh, patch_size=256, step_size=256, contour_fn='four_pt', use_padding=True,
                   top_left=None, bot_right=None, device=None):
    """`process_contour` (:407-493) at patch_level 0: (n,2) int64 level-0 (x, y) tile origins of one tissue contour.
    `device`: a GPU evaluates the grid's contour and hole tests (`grid_in_contour_device`, the same answers); None = the host code."""
    if contour_fn not in ('basic', 'center', 'four_pt', 'four_pt_hard'):
        raise NotImplementedError(contour_fn)
    img_w, img_h = image_wh
    start_x, start_y, w, h = bounding_rect(contour) if contour is not None else (0, 0, img_w, img_h)
    if use_padding:
        stop_y, stop_x = start_y + h, start_x + w
    else:
        stop_y, stop_x = min(start_y + h, img_h - patch_size + 1), min(start_x + w, img_w - patch_size + 1)
    if bot_right is not None:
        stop_y, stop_x = min(bot_right[1], stop_y), min(bot_right[0], stop_x)
    if top_left is not None:
        start_y, start_x = max(top_left[1], start_y), max(top_left[0], start_x)
    if (bot_right is not None or top_left is not None) and (stop_x - start_x <= 0 or stop_y - start_y <= 0):
        return np.zeros((0, 2), np.int64)
    xs = np.arange(start_x, stop_x, step=step_size)
    ys = np.arange(start_y, stop_y, step=step_size)
    gx, gy = np.meshgrid(xs, ys, indexing='ij')
    cand = np.stack([gx.reshape(-1), gy.reshape(-1)], 1)
    if device is not None:
        ok = grid_in_contour_device(contour, holes, (start_x, start_y), (len(xs), len(ys)), step_size, patch_size, contour_fn, device)
    else:
        ok = np.ones(len(cand), bool) if contour is None else in_contour(contour, cand, patch_size, contour_fn)
        ok &= ~in_holes(holes or [], cand, patch_size)
    keep = cand[ok].astype(np.int64)
    # the reference stores a contour's coordinates only when it yields more than one (`if len(results) > 1`, :476)
    return keep if len(keep) > 1 else np.zeros((0, 2), np.int64)


def tissue_tile_coords(image, patch_size=256, step_size=256, scale=64, seg_params=None, filter_params=None,
                       contour_fn='four_pt', use_padding=True, device=None):
    """segmentTissue + process_contours: tile origins over all tissue contours, in contour order (the .h5 `coords`).
    `device`: passed to `segment_tissue` and `contour_coords` (None = the host code)."""
    sp = dict(SEG_PARAMS if seg_params is None else seg_params)
    conts, holes = segment_tissue(image, scale=scale, filter_params=filter_params, device=device, **sp)
    H, W = image.shape[:2]
    parts = [contour_coords(c, h, (W, H), patch_size, step_size, contour_fn, use_padding, device=device) for c, h in zip(conts, holes)]
    coords = np.concatenate(parts, 0) if parts else np.zeros((0, 2), np.int64)
    return coords, conts, holes


def read_tiles(image, coords, patch_size=256):
    """`Whole_Slide_Bag_FP.__getitem__` (:886-898) on an array slide: RGB tiles at `coords`, zero padded past the edge."""
    H, W = image.shape[:2]
    out = np.zeros((len(coords), patch_size, patch_size, 3), np.uint8)
    for i, (x, y) in enumerate(coords):
        sub = image[max(y, 0):min(y + patch_size, H), max(x, 0):min(x + patch_size, W), :3]
        out[i, :sub.shape[0], :sub.shape[1]] = sub
    return out
