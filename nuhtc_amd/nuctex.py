"""Per-nucleus Haralick texture: the 26 `Haralick.*` columns that follow `Nucleus.Intensity.*` in the reference's hand-crafted table
(tools/wsi_feat_extract.py / tools/nuclei_feat_extract.py: histomicstk over one crop per nucleus on the host), from grey-level
co-occurrence COUNTS the GPU takes under the final mask of every kept detection (csrc/nuctex.hip).  THE DEVICE PRODUCES INTEGERS ONLY,
and every named floating-point feature is derived here, on the host, in float64, by one function (`derive`) for the device route and the
reference route alike.  `glcm_reference` is the plain-numpy restatement of the integers; the device must equal it bit for bit.

Grey level.  q(p) = h(p) >> 4, h the project's haematoxylin value of the tile pixel (nucmorph.haematoxylin, 0..255, the same table and
coefficients): L = 16 levels over the FIXED range.  This is THE PROJECT'S OWN scale: histomicstk quantises an 8-bit stain image to 32
levels between grey limits that depend on the crop; it is not a dependency, and that cannot be reproduced or pinned.  (16 levels keep a
record at 1088 bytes, about the size of a morphometry record.)

Offsets.  (dy, dx) = (0, 1) and (1, 0): distance 1 along the row and along the column, histomicstk's default.

Counts.  For offset o, T[o][t(a, b)] is the number of unordered pixel pairs {p, p + o} with both pixels set in the mask M and inside the
H x W frame whose levels are {a, b}, a <= b; t(a, b) = a L - a (a - 1) / 2 + (b - a) numbers the upper triangle in row-major order, 136
cells per offset: T is int32 [2][136] per nucleus.  A pair with one pixel outside the mask is not counted (what `exclude_boundary` and
the ROI mask do in histomicstk).  The symmetric matrix of Haralick, of histomicstk (symmetric=True) and of skimage is G[a][b] = G[b][a]
= T[t(a, b)] for a < b and G[a][a] = 2 T[t(a, a)] (`full_matrix`); its sum is twice the number of pairs.  An empty mask, a single
pixel, a mask without 4-neighbour pairs (a checkerboard) and an entry outside the batch give a zero row.

Features (`derive`).  Per offset p = G / sum(G), level indices i, j = 0 .. L - 1 (0-based, as in skimage), px = py the marginal (G is
symmetric), mu and var its mean and variance, p_sum(k) = sum over i + j = k of p (k = 0 .. 2L - 2), p_diff(k) = sum over |i - j| = k
of p (k = 0 .. L - 1); natural logarithms and 0 log 0 = 0.  The 13 features of Haralick, Shanmugam and Dinstein 1973 under histomicstk's
names:

    ASM                 sum p^2
    Contrast            sum (i - j)^2 p
    Correlation         sum (i - mu)(j - mu) p / var
    SumOfSquares        sum (i - mu)^2 p                     (= var)
    IDM                 sum p / (1 + (i - j)^2)
    SumAverage          sum k p_sum(k)
    SumVariance         sum (k - SumAverage)^2 p_sum(k)
    SumEntropy          - sum p_sum log p_sum
    Entropy             - sum p log p                        (= HXY)
    DifferenceVariance  sum (k - m)^2 p_diff(k), m = sum k p_diff(k)
    DifferenceEntropy   - sum p_diff log p_diff
    IMC1                (HXY - HXY1) / max(HX, HY), HX = HY = - sum px log px, HXY1 = - sum p log(px(i) py(j))
    IMC2                sqrt(max(0, 1 - exp(-2 (HXY2 - HXY)))), HXY2 = - sum px(i) py(j) log(px(i) py(j))

`COLUMNS` are Haralick.<name>.Mean and Haralick.<name>.Range, the mean and the absolute difference over the two offsets.  Degenerate
cases, so that no value is ever NaN or infinite: an offset without pairs gives 13 zeros and still enters Mean and Range; a marginal
with one level only (zero variance, decided on the integers) gives Correlation 1 (skimage's rule); max(HX, HY) == 0 gives IMC1 0; the
argument of IMC2's root is clamped at 0."""
import numpy as np

from . import nucmorph

SHIFT = 4
L = 256 >> SHIFT                      # 16 grey levels
OFFSETS = ((0, 1), (1, 0))            # (dy, dx)
CELLS = L * (L + 1) // 2              # 136: the upper triangle
ROW = len(OFFSETS) * CELLS // 2       # one record as int64 words: the 272 int32, two to a word

NAMES = ('ASM', 'Contrast', 'Correlation', 'SumOfSquares', 'IDM', 'SumAverage', 'SumVariance', 'SumEntropy', 'Entropy',
         'DifferenceVariance', 'DifferenceEntropy', 'IMC1', 'IMC2')
COLUMNS = tuple(f'Haralick.{n}.{s}' for n in NAMES for s in ('Mean', 'Range'))


def tri(a, b):
    """Cell of the levels a <= b in the upper triangle (scalars or arrays)."""
    return a * L - a * (a - 1) // 2 + (b - a)


_IA, _IB = np.triu_indices(L)         # row-major upper triangle: cell t holds the levels (_IA[t], _IB[t])


def levels(tile_rgb):
    """(..., 3) uint8 RGB -> int64 (...): the grey level 0 .. 15 of every pixel."""
    return nucmorph.haematoxylin(tile_rgb) >> SHIFT


def glcm_reference(tile_rgb, mask_bool):
    """tile_rgb (H, W, 3) uint8 in R, G, B order, mask_bool (H, W) -> int64 (2, 136): the counts of the module docstring in plain numpy
    (the mask and the level image shifted against themselves, one np.add.at per offset)."""
    m = np.asarray(mask_bool, bool)
    q = levels(np.asarray(tile_rgb, np.uint8))
    H, W = m.shape
    T = np.zeros((len(OFFSETS), CELLS), np.int64)
    for o, (dy, dx) in enumerate(OFFSETS):
        both = m[:H - dy, :W - dx] & m[dy:, dx:]
        a, b = q[:H - dy, :W - dx][both], q[dy:, dx:][both]
        np.add.at(T[o], tri(np.minimum(a, b), np.maximum(a, b)), 1)
    return T


def full_matrix(T):
    """int (..., 136) -> int64 (..., 16, 16): the symmetric co-occurrence matrix G of the counts (its sum is twice the pairs)."""
    T = np.asarray(T, np.int64)
    G = np.zeros(T.shape[:-1] + (L, L), np.int64)
    G[..., _IA, _IB] += T
    G[..., _IB, _IA] += T
    return G


def _xlogx(p):
    return p * np.log(np.where(p > 0, p, 1.0))


def derive(T):
    """T int (n, 2, 136) or (2, 136) -> (COLUMNS, float64 (n, 26)).  Host float64 only; the formulas and the degenerate cases are those
    of the module docstring."""
    T = np.asarray(T, np.int64).reshape(-1, len(OFFSETS), CELLS)
    G = full_matrix(T)                                                     # (n, 2, L, L)
    tot = G.sum((-1, -2))
    some = tot > 0
    p = G / np.where(some, tot, 1)[..., None, None].astype(np.float64)
    i, j = np.arange(L, dtype=np.float64)[:, None], np.arange(L, dtype=np.float64)[None, :]
    d2 = (i - j) ** 2
    px = p.sum(-1)                                                         # = py: G is symmetric
    mu = (px * i[:, 0]).sum(-1)[..., None, None]
    var = (p * (i - mu) ** 2).sum((-1, -2))
    one_level = (G.sum(-1) > 0).sum(-1) == 1
    cov = (p * (i - mu) * (j - mu)).sum((-1, -2))
    f = np.zeros(T.shape[:2] + (len(NAMES),), np.float64)
    f[..., 0] = (p * p).sum((-1, -2))
    f[..., 1] = (p * d2).sum((-1, -2))
    f[..., 2] = np.where(one_level, 1.0, cov / np.where(one_level | ~some, 1.0, var))
    f[..., 3] = var
    f[..., 4] = (p / (1.0 + d2)).sum((-1, -2))
    ks, kd = (np.arange(L)[:, None] + np.arange(L)[None, :]).ravel(), np.abs(np.arange(L)[:, None] - np.arange(L)[None, :]).ravel()
    flat = p.reshape(p.shape[:2] + (L * L,))
    psum, pdiff = np.zeros(p.shape[:2] + (2 * L - 1,)), np.zeros(p.shape[:2] + (L,))
    for k in range(2 * L - 1):
        psum[..., k] = flat[..., ks == k].sum(-1)
    for k in range(L):
        pdiff[..., k] = flat[..., kd == k].sum(-1)
    k2, k1 = np.arange(2 * L - 1, dtype=np.float64), np.arange(L, dtype=np.float64)
    f[..., 5] = (psum * k2).sum(-1)
    f[..., 6] = (psum * (k2 - f[..., 5:6]) ** 2).sum(-1)
    f[..., 7] = -_xlogx(psum).sum(-1)
    hxy = -_xlogx(p).sum((-1, -2))
    f[..., 8] = hxy
    md = (pdiff * k1).sum(-1)[..., None]
    f[..., 9] = (pdiff * (k1 - md) ** 2).sum(-1)
    f[..., 10] = -_xlogx(pdiff).sum(-1)
    hx = -_xlogx(px).sum(-1)                                               # = HY
    pxy = px[..., :, None] * px[..., None, :]
    lpxy = np.log(np.where(pxy > 0, pxy, 1.0))
    hxy1, hxy2 = -(p * lpxy).sum((-1, -2)), -(pxy * lpxy).sum((-1, -2))
    f[..., 11] = np.where(hx > 0, (hxy - hxy1) / np.where(hx > 0, hx, 1.0), 0.0)
    f[..., 12] = np.sqrt(np.maximum(0.0, 1.0 - np.exp(-2.0 * (hxy2 - hxy))))
    f[~some] = 0.0                                                         # an offset without pairs: 13 zeros
    out = np.zeros((len(T), len(COLUMNS)), np.float64)
    out[:, 0::2] = (f[:, 0] + f[:, 1]) / 2.0
    out[:, 1::2] = np.abs(f[:, 0] - f[:, 1])
    return COLUMNS, out


def pack_rows(glcm):
    """glcm (n, 2, 136) int32 -> int64 (n, ROW = 136): the form the rows travel in (nuhtc_amd.wsi), two counts to a word."""
    return np.ascontiguousarray(glcm, np.int32).reshape(-1, len(OFFSETS) * CELLS).view(np.int64)


def unpack_rows(rows):
    """int64 (n, ROW) -> glcm int32 (n, 2, 136)."""
    return np.ascontiguousarray(rows, np.int64).reshape(-1, ROW).view(np.int32).reshape(-1, len(OFFSETS), CELLS)


def write_npz(path, nuclei_id, glcm, label, score):
    """The texture table of a slide: columns (26,) str, values float64 (n, 26) = derive(glcm), glcm int32 (n, 2, 136), nuclei_id int64
    (n,), label int64 (n,), score float64 (n,).  Row k belongs to the k-th feature of the GeoJSON written beside the file; nuclei_id is
    that nucleus's position in <id>.geojson (as in <id>_nuclei_feat.npz)."""
    glcm = np.ascontiguousarray(glcm, np.int32).reshape(-1, len(OFFSETS), CELLS)
    nuclei_id = np.ascontiguousarray(nuclei_id, np.int64)
    if not (len(nuclei_id) == len(glcm) == len(label) == len(score)):
        raise ValueError('write_npz: one row per nucleus in every field')
    columns, values = derive(glcm)
    with open(path, 'wb') as f:
        np.savez(f, columns=np.array(columns), values=values, glcm=glcm, nuclei_id=nuclei_id,
                 label=np.ascontiguousarray(label, np.int64), score=np.ascontiguousarray(score, np.float64))
    return path


def read_npz(path):
    """-> dict(columns, values, glcm, nuclei_id, label, score) of a file write_npz wrote."""
    with np.load(path) as z:
        return {k: z[k] for k in ('columns', 'values', 'glcm', 'nuclei_id', 'label', 'score')}
