"""Per-nucleus morphometry and haematoxylin intensity: the hand-crafted table of the reference's tools/wsi_feat_extract.py /
tools/nuclei_feat_extract.py (histomicstk over one crop per nucleus on the host), from integers the GPU computes under the final mask of
every kept detection (csrc/nucmorph.hip).  THE DEVICE PRODUCES INTEGERS ONLY -- exact counts, sums and a histogram -- and every named
floating-point feature is derived here, on the host, in float64, by one function (`derive`) for the device route and the reference
route alike.  `morph_reference` is the plain-numpy restatement of the integers; the device must equal it bit for bit.

The integers of a binary mask M in an H x W frame (a pixel outside the frame is 0), raw int64[16]:

    0      A        set pixels
    1..4   x0 y0 x1 y1   bounding rectangle, x1 / y1 exclusive (all 0 when A == 0)
    5..9   Sx Sy Sxx Syy Sxy   sums over the set pixels of x, y, x^2, y^2, x y (tile pixels)
    10     E        pixel edges between a set pixel and an unset or out-of-frame 4-neighbour (the crack length)
    11..13 n1 n2 n3 the perimeter classes of skimage.measure.perimeter(neighbourhood=4): B = M & ~erode4(M) (the erosion sees 0 outside
                    the frame), code(p) = sum over the 3 x 3 neighbourhood of B with weights [[10, 2, 10], [2, 1, 2], [10, 2, 10]] for p in
                    B; n1 counts codes in {5, 7, 15, 17, 25, 27}, n2 in {21, 33}, n3 in {13, 23}
    14     hull2    twice the area of the convex hull of the corner lattice points of all set pixels: per lattice row Y the leftmost
                    and rightmost corner (of the pixel rows Y - 1 and Y), one monotone chain per side with integer cross products,
                    hull2 = sum over the right chain of (X_i + X_i+1)(Y_i+1 - Y_i) minus the same over the left chain
    15     0        (reserved)

and hist int[256]: the histogram under M of the haematoxylin value h(p) of the tile pixel.

h is THE PROJECT'S OWN linear optical-density scale: a fixed-point Ruifrok-Johnston colour deconvolution with no transcendental on the
device.  The host builds once, in float64, then rounds: LUT[v] = rint(-ln(max(v, 1) / 255) * 2^16) (int32, v = 0..255) and K_c =
rint(q_c * 255 / ln(255) * 2^12) for c in R, G, B, q the haematoxylin row of the inverse of the stain matrix whose columns are
haematoxylin (0.65, 0.70, 0.29), eosin (0.07, 0.99, 0.11), both normalised, and their normalised cross product.  Then, in int64 with a
floor shift, h = clamp((K_r LUT[R] + K_g LUT[G] + K_b LUT[B] + 2^27) >> 28, 0, 255): 255 is the optical density ln(255) of pure
haematoxylin.  (|K_c| < 2^19 and LUT < 2^19: the sum stays below 2^40.)  It is NOT bit-equal to histomicstk's `255 - stains[..., 0]`
(an 8-bit image of exp(-density)); histomicstk is not a dependency and cannot be pinned.  Table and coefficients are parameters of the
kernel, and the same constants serve both routes.

Named features (`COLUMNS`; histomicstk's names where the meaning coincides).  Degenerate cases: A == 0 gives a row of zeros; a
perimeter of 0 (a single pixel) gives Circularity 0; lambda1 == 0 (A == 1, no extent) gives Eccentricity 0, axis lengths 0 and
MinorMajorAxisRatio 1; lambda1 == lambda2 gives Orientation 0; an intensity variance of 0 gives Skewness 0 and Kurtosis 0.  No value
is ever NaN or infinite."""
import math

import numpy as np

RAW = 16
BINS = 256
(I_A, I_X0, I_Y0, I_X1, I_Y1, I_SX, I_SY, I_SXX, I_SYY, I_SXY, I_E, I_N1, I_N2, I_N3, I_HULL2) = range(15)
LUT_SHIFT, K_SHIFT = 16, 12
CODES_1, CODES_2, CODES_3 = (5, 7, 15, 17, 25, 27), (21, 33), (13, 23)
CODE_WEIGHTS = np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]], np.int64)

COLUMNS = ('Size.Area', 'Size.Perimeter', 'Size.MajorAxisLength', 'Size.MinorAxisLength',
           'Shape.Eccentricity', 'Shape.Circularity', 'Shape.EquivalentDiameter', 'Shape.Extent', 'Shape.MinorMajorAxisRatio', 'Shape.Solidity',
           'Orientation.Orientation',
           'Identifier.CentroidX', 'Identifier.CentroidY', 'Identifier.Xmin', 'Identifier.Ymin', 'Identifier.Xmax', 'Identifier.Ymax',
           'Nucleus.Intensity.Min', 'Nucleus.Intensity.Max', 'Nucleus.Intensity.Mean', 'Nucleus.Intensity.Median',
           'Nucleus.Intensity.MeanMedianDiff', 'Nucleus.Intensity.Std', 'Nucleus.Intensity.IQR', 'Nucleus.Intensity.MAD',
           'Nucleus.Intensity.Skewness', 'Nucleus.Intensity.Kurtosis', 'Nucleus.Intensity.HistEnergy', 'Nucleus.Intensity.HistEntropy')


def stain_constants():
    """-> (lut int32 (256,), k int64 (3,)): the table and the R, G, B coefficients of the haematoxylin value (module docstring)."""
    hem, eos = np.array([0.65, 0.70, 0.29]), np.array([0.07, 0.99, 0.11])
    hem, eos = hem / np.linalg.norm(hem), eos / np.linalg.norm(eos)
    res = np.cross(hem, eos)
    q = np.linalg.inv(np.stack([hem, eos, res / np.linalg.norm(res)], 1))[0]
    v = np.maximum(np.arange(256, dtype=np.float64), 1.0)
    lut = np.rint(-np.log(v / 255.0) * 2.0 ** LUT_SHIFT).astype(np.int32)
    k = np.rint(q * (255.0 / math.log(255.0)) * 2.0 ** K_SHIFT).astype(np.int64)
    return lut, k


def haematoxylin(tile_rgb):
    """(..., 3) uint8 RGB -> int64 (...): the integer haematoxylin value of every pixel."""
    lut, k = stain_constants()
    l = lut.astype(np.int64)[np.asarray(tile_rgb, np.uint8)]
    acc = l[..., 0] * k[0] + l[..., 1] * k[1] + l[..., 2] * k[2] + (1 << (LUT_SHIFT + K_SHIFT - 1))
    return np.clip(acc >> (LUT_SHIFT + K_SHIFT), 0, 255)


def _chain2(ys, xs, upper):
    """Twice the integral over Y of the convex (upper=False: lower) / concave (upper=True) envelope of the points (xs[i], ys[i]), ys
    strictly increasing: one monotone chain with integer cross products."""
    st = []
    for y, x in zip(ys, xs):
        while len(st) >= 2:
            (ay, ax), (by, bx) = st[-2], st[-1]
            lhs, rhs = (bx - ax) * (y - by), (x - bx) * (by - ay)
            if (lhs <= rhs) if upper else (lhs >= rhs):
                st.pop()
            else:
                break
        st.append((y, x))
    return sum((st[i][1] + st[i + 1][1]) * (st[i + 1][0] - st[i][0]) for i in range(len(st) - 1))


def hull2_of(mask_bool):
    """Twice the area of the convex hull of the pixel corners of a mask (an integer; 0 for an empty mask)."""
    m = np.asarray(mask_bool, bool)
    rows = np.nonzero(m.any(1))[0]
    if len(rows) == 0:
        return 0
    left = {int(y): int(np.argmax(m[y])) for y in rows}
    right = {int(y): int(m.shape[1] - np.argmax(m[y, ::-1])) for y in rows}         # exclusive: the right corners of the last pixel
    ys, lo, hi = [], [], []
    for Y in range(int(rows[0]), int(rows[-1]) + 2):                                # lattice rows: the corners of pixel rows Y - 1 and Y
        near = [y for y in (Y - 1, Y) if y in left]
        if near:
            ys.append(Y); lo.append(min(left[y] for y in near)); hi.append(max(right[y] for y in near))
    return _chain2(ys, hi, True) - _chain2(ys, lo, False)


def morph_reference(tile_rgb, mask_bool):
    """tile_rgb (H, W, 3) uint8 in R, G, B order, mask_bool (H, W) -> (raw int64 (16,), hist int64 (256,)): the integers of the module
    docstring in plain numpy (scipy.ndimage only for the exact binary erosion and the integer correlation)."""
    from scipy import ndimage
    m = np.asarray(mask_bool, bool)
    raw, hist = np.zeros(RAW, np.int64), np.zeros(BINS, np.int64)
    ys, xs = np.nonzero(m)
    if len(ys) == 0:
        return raw, hist
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    raw[I_A] = len(ys)
    raw[I_X0:I_Y1 + 1] = xs.min(), ys.min(), xs.max() + 1, ys.max() + 1
    raw[I_SX:I_SXY + 1] = xs.sum(), ys.sum(), (xs * xs).sum(), (ys * ys).sum(), (xs * ys).sum()
    p = np.pad(m, 1)
    raw[I_E] = sum(int((p[1:-1, 1:-1] & ~nb).sum()) for nb in (p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]))
    cross = ndimage.generate_binary_structure(2, 1)
    border = m & ~ndimage.binary_erosion(m, cross, border_value=0)
    code = ndimage.correlate(border.astype(np.int64), CODE_WEIGHTS, mode='constant', cval=0)[border]
    raw[I_N1], raw[I_N2], raw[I_N3] = (int(np.isin(code, c).sum()) for c in (CODES_1, CODES_2, CODES_3))
    raw[I_HULL2] = hull2_of(m)
    hist[:] = np.bincount(haematoxylin(np.asarray(tile_rgb, np.uint8)[m]), minlength=BINS)
    return raw, hist


def _order_stat(cum, k):
    """Value at sorted position k (per row) of the integer samples whose cumulative histogram is `cum` (n, 256)."""
    return (cum <= np.asarray(k, np.int64)[:, None]).sum(1)


def _quantile(cum, n, q):
    """numpy's default (linear) quantile q of the samples, from the cumulative histogram; exact for q = 0.25, 0.5, 0.75 (the fraction is
    a multiple of 1/4 and the samples are integers)."""
    pos = (n - 1).astype(np.float64) * q
    lo = np.floor(pos).astype(np.int64)
    a, b = _order_stat(cum, lo), _order_stat(cum, np.minimum(lo + 1, n - 1))
    return a + (b - a) * (pos - lo)


def derive(raw, hist, origin=None):
    """raw int (n, 16) or (16,), hist int (n, 256) or (256,), origin (n, 2) or (2,) = slide (x, y) of the tile's pixel (0, 0) (default 0)
    -> (COLUMNS, float64 (n, len(COLUMNS))).  Host float64 only; the degenerate cases are those of the module docstring."""
    raw = np.asarray(raw, np.int64).reshape(-1, RAW)
    hist = np.asarray(hist, np.int64).reshape(-1, BINS)
    n = len(raw)
    org = np.zeros((n, 2), np.float64) if origin is None else np.broadcast_to(np.asarray(origin, np.float64).reshape(-1, 2), (n, 2))
    out = np.zeros((n, len(COLUMNS)), np.float64)
    if len(hist) != n:
        raise ValueError('derive: one histogram per row of raw')
    if (hist.sum(1) != raw[:, I_A]).any():
        raise ValueError('derive: a histogram does not hold A samples')
    ok = raw[:, I_A] > 0
    if not ok.any():
        return COLUMNS, out
    r, hh, og = raw[ok], hist[ok], org[ok]
    Ai = r[:, I_A]
    A = Ai.astype(np.float64)
    col = {c: i for i, c in enumerate(COLUMNS)}
    v = np.zeros((len(r), len(COLUMNS)), np.float64)

    def put(name, val):
        v[:, col[name]] = val

    P = r[:, I_N1] + r[:, I_N2] * math.sqrt(2.0) + r[:, I_N3] * ((1.0 + math.sqrt(2.0)) / 2.0)
    put('Size.Area', A)
    put('Size.Perimeter', P)
    # central moments times A^2, as exact integers before the first division (below 2^57 for a full 1024 x 1024 frame)
    n20 = Ai * r[:, I_SXX] - r[:, I_SX] ** 2              # x
    n02 = Ai * r[:, I_SYY] - r[:, I_SY] ** 2              # y
    n11 = Ai * r[:, I_SXY] - r[:, I_SX] * r[:, I_SY]
    iso = (n11 == 0) & (n20 == n02)                        # lambda1 == lambda2, decided on the integers
    tr, root = (n20 + n02).astype(np.float64), np.hypot(2.0 * n11.astype(np.float64), (n20 - n02).astype(np.float64))
    l1 = (tr + root) / (2.0 * A * A)
    l2 = np.maximum(tr - root, 0.0) / (2.0 * A * A)
    l2 = np.where(iso, l1, l2)
    flat = l1 <= 0.0
    major, minor = 4.0 * np.sqrt(l1), 4.0 * np.sqrt(l2)
    put('Size.MajorAxisLength', major)
    put('Size.MinorAxisLength', minor)
    safe1 = np.where(flat, 1.0, l1)
    put('Shape.Eccentricity', np.where(flat, 0.0, np.sqrt(np.maximum(1.0 - l2 / safe1, 0.0))))
    put('Shape.Circularity', np.where(P > 0, 4.0 * math.pi * A / np.where(P > 0, P, 1.0) ** 2, 0.0))
    put('Shape.EquivalentDiameter', np.sqrt(4.0 * A / math.pi))
    put('Shape.Extent', A / ((r[:, I_X1] - r[:, I_X0]) * (r[:, I_Y1] - r[:, I_Y0])).astype(np.float64))
    put('Shape.MinorMajorAxisRatio', np.where(flat, 1.0, minor / np.where(flat, 1.0, major)))
    put('Shape.Solidity', 2.0 * A / r[:, I_HULL2].astype(np.float64))
    # skimage 0.18 regionprops.orientation on the inertia tensor [[a, b], [b, c]] = [[mu_xx, -mu_xy], [-mu_xy, mu_yy]] / A
    ori = 0.5 * np.arctan2(2.0 * n11.astype(np.float64), (n02 - n20).astype(np.float64))
    ori = np.where(n20 == n02, np.where(n11 > 0, -math.pi / 4.0, math.pi / 4.0), ori)
    put('Orientation.Orientation', np.where(iso, 0.0, ori))
    put('Identifier.CentroidX', og[:, 0] + r[:, I_SX] / A)
    put('Identifier.CentroidY', og[:, 1] + r[:, I_SY] / A)
    put('Identifier.Xmin', og[:, 0] + r[:, I_X0])
    put('Identifier.Ymin', og[:, 1] + r[:, I_Y0])
    put('Identifier.Xmax', og[:, 0] + r[:, I_X1])
    put('Identifier.Ymax', og[:, 1] + r[:, I_Y1])
    # ---- intensity, from the histogram alone
    k = np.arange(BINS, dtype=np.float64)
    cum = np.cumsum(hh, 1)
    put('Nucleus.Intensity.Min', (hh > 0).argmax(1))
    put('Nucleus.Intensity.Max', BINS - 1 - (hh[:, ::-1] > 0).argmax(1))
    mean = (hh * np.arange(BINS, dtype=np.int64)).sum(1) / A
    med = (_order_stat(cum, (Ai - 1) // 2) + _order_stat(cum, Ai // 2)) / 2.0
    put('Nucleus.Intensity.Mean', mean)
    put('Nucleus.Intensity.Median', med)
    put('Nucleus.Intensity.MeanMedianDiff', mean - med)
    d = k[None, :] - mean[:, None]
    m2, m3, m4 = ((hh * d ** p).sum(1) / A for p in (2, 3, 4))
    put('Nucleus.Intensity.Std', np.sqrt(m2))
    put('Nucleus.Intensity.IQR', _quantile(cum, Ai, 0.75) - _quantile(cum, Ai, 0.25))
    dev = np.abs(k[None, :] - med[:, None])                 # median of |x - median|: the histogram reordered by deviation
    order = np.argsort(dev, 1, kind='stable')
    dcum, dsort = np.cumsum(np.take_along_axis(hh, order, 1), 1), np.take_along_axis(dev, order, 1)
    pick = lambda pos: np.take_along_axis(dsort, _order_stat(dcum, pos)[:, None], 1)[:, 0]
    put('Nucleus.Intensity.MAD', (pick((Ai - 1) // 2) + pick(Ai // 2)) / 2.0)
    var = m2 > 0
    s2 = np.where(var, m2, 1.0)
    put('Nucleus.Intensity.Skewness', np.where(var, m3 / s2 ** 1.5, 0.0))
    put('Nucleus.Intensity.Kurtosis', np.where(var, m4 / (s2 * s2) - 3.0, 0.0))
    p = hh / A[:, None]
    put('Nucleus.Intensity.HistEnergy', (p * p).sum(1))
    put('Nucleus.Intensity.HistEntropy', -(p * np.log(np.where(p > 0, p, 1.0))).sum(1))
    out[ok] = v
    return COLUMNS, out


ROW = RAW + 2 + BINS // 2        # one record's integers as int64 words: raw | tile origin (x, y) | the int32 histogram, two bins a word


def pack_rows(raw, hist, origin):
    """raw (n, 16) int64, hist (n, 256) int32, origin (n, 2) or (2,) -> int64 (n, ROW): the form the rows travel in (nuhtc_amd.wsi)."""
    raw = np.asarray(raw, np.int64).reshape(-1, RAW)
    rows = np.zeros((len(raw), ROW), np.int64)
    rows[:, :RAW] = raw
    rows[:, RAW:RAW + 2] = np.asarray(origin, np.int64).reshape(-1, 2)
    rows[:, RAW + 2:] = np.ascontiguousarray(hist, np.int32).reshape(-1, BINS).view(np.int64)
    return rows


def unpack_rows(rows):
    """int64 (n, ROW) -> (raw int64 (n, 16), hist int32 (n, 256), origin int64 (n, 2))."""
    rows = np.ascontiguousarray(rows, np.int64).reshape(-1, ROW)
    return rows[:, :RAW].copy(), np.ascontiguousarray(rows[:, RAW + 2:]).view(np.int32).reshape(-1, BINS), rows[:, RAW:RAW + 2].copy()


def write_npz(path, nuclei_id, raw, hist, label, score, origin=None):
    """The morphometry table of a slide: columns (F,) str, values float64 (n, F) = derive(raw, hist, origin), raw int64 (n, 16), hist
    int32 (n, 256), origin int64 (n, 2), nuclei_id int64 (n,), label int64 (n,), score float64 (n,).  origin is the slide position of
    the tile the integers were measured in: raw is in that tile's pixels, and derive needs it for the position columns.  Row k belongs to
    the k-th feature of the GeoJSON written beside the file; nuclei_id is that nucleus's position in <id>.geojson (as in
    <id>_nuclei_feat.npz)."""
    raw = np.ascontiguousarray(raw, np.int64).reshape(-1, RAW)
    hist = np.ascontiguousarray(hist, np.int32).reshape(-1, BINS)
    nuclei_id = np.ascontiguousarray(nuclei_id, np.int64)
    if not (len(nuclei_id) == len(raw) == len(hist) == len(label) == len(score)):
        raise ValueError('write_npz: one row per nucleus in every field')
    columns, values = derive(raw, hist, origin)
    with open(path, 'wb') as f:
        np.savez(f, columns=np.array(columns), values=values, raw=raw, hist=hist, nuclei_id=nuclei_id,
                 origin=np.zeros((len(raw), 2), np.int64) if origin is None else np.ascontiguousarray(np.broadcast_to(np.asarray(origin, np.int64).reshape(-1, 2), (len(raw), 2))),
                 label=np.ascontiguousarray(label, np.int64), score=np.ascontiguousarray(score, np.float64))
    return path


def read_npz(path):
    """-> dict(columns, values, raw, hist, origin, nuclei_id, label, score) of a file write_npz wrote."""
    with np.load(path) as z:
        return {k: z[k] for k in ('columns', 'values', 'raw', 'hist', 'origin', 'nuclei_id', 'label', 'score')}
