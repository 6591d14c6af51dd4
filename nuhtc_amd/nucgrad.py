"""Per-nucleus gradient features: the eight `Nucleus.Gradient.*` columns that stand between `Nucleus.Intensity.*` and `Haralick.*` in the
reference's hand-crafted table (tools/wsi_feat_extract.py / tools/nuclei_feat_extract.py: histomicstk's compute_nuclei_features with its
defaults, over one crop per nucleus on the host), from integers the GPU takes under the mask of a nucleus (csrc/nucgrad.hip).  THE DEVICE
PRODUCES INTEGERS ONLY, and every named floating-point feature is derived here, on the host, in float64, by one function (`derive`).
`grad_reference` is the numpy restatement of the integers (np.gradient, math.isqrt, np.histogram); the device must equal it bit for bit.
The integers of one nucleus are a pure function of its mask, its H x W frame of tile pixels, the stain table and coefficients
(nucmorph.stain_constants), the channel mode and the threshold T.

Haematoxylin value.  h(x, y) is the project's fixed-point haematoxylin value of the frame pixel, 0..255 (nucmorph.haematoxylin,
csrc/haematoxylin.h): the value the morphometry and the texture use.

Doubled gradient.  numpy's np.gradient (edge order 1) times two, so that it is an integer: inside the frame gx2 = h(x + 1, y) -
h(x - 1, y); at x = 0 gx2 = 2 (h(1, y) - h(0, y)); at x = W - 1 gx2 = 2 (h(W - 1, y) - h(W - 2, y)); a frame of width 1 gives gx2 = 0
(np.gradient refuses that case; it is defined here).  gy2 is the same along y.  A neighbour outside the mask but inside the frame counts
with its real pixel, as in histomicstk, which differentiates the whole crop: the frame should hold a margin round the mask (the document
route gives it 2 pixels).

Magnitude.  q = gx2^2 + gy2^2, 0 <= q <= 520 200, and m = isqrt(4 q) = floor(4 |grad h|): the gradient magnitude in QUARTER grey levels
per pixel, 0..1442, the exact integer floor.

Per nucleus, over the pixels of the mask: A, their number; S1..S4, the sums of m, m^2, m^3, m^4 (int64: a full 1024 x 1024 frame at m =
1442 gives S4 = 4.53e18 < 2^63); mn, mx, the least and the greatest m; hist[10], numpy's np.histogram(m, bins=10) on the nucleus's own
range in integers -- bin = min((m - mn) * 10 // (mx - mn), 9) when mx > mn, every pixel in bin 5 when mx == mn; and n_edge.

Edge count.  n_edge stands for histomicstk's Canny.Sum.  It is THE PROJECT'S OWN definition, like the grey scales of the morphometry and
the texture: scikit-image's Canny, with its Gaussian smoothing and hysteresis, is not a dependency and is NOT reproduced.  A mask pixel p
is an edge pixel when m(p) >= T and q(p) is a local maximum along its quantised gradient direction.  The sector rule is OpenCV's integer
rule, with ax = |gx2| and ay = |gy2|:

    horizontal   ay << 15 < ax * 13573                        neighbours (x - 1, y) and (x + 1, y)
    vertical     ay << 15 > ax * 13573 + (ax << 16)           neighbours (x, y - 1) and (x, y + 1)
    diagonal     neither, gx2 * gy2 > 0                       neighbours (x - 1, y - 1) and (x + 1, y + 1)
    diagonal     neither, otherwise                           neighbours (x + 1, y - 1) and (x - 1, y + 1)

p is an edge when q(p) > q(first neighbour) and q(p) >= q(second neighbour), in the order listed: a plateau two pixels wide counts once.
A neighbour outside the frame has q = 0; one outside the mask but inside the frame has its real q.  T is in quarter levels, 1..1442;
the default 1 counts every local maximum of a non-zero gradient.

Row.  int64 [18]: A, S1, S2, S3, S4, mn, mx, n_edge, hist[0..9].  An empty mask, or a list entry outside the batch, gives a zero row.

Features (`derive`; `COLUMNS` are histomicstk's names).  Mag.Mean = S1 / (4 A).  The central-moment numerators are exact Python integers
before the first division: n2 = A S2 - S1^2, n3 = A^2 S3 - 3 A S1 S2 + 2 S1^3, n4 = A^3 S4 - 4 A^2 S1 S3 + 6 A S1^2 S2 - 3 S1^4 (they
outgrow int64).  Mag.Std = sqrt(n2) / (4 A), the population one; Mag.Skewness = n3 / n2^1.5 and Mag.Kurtosis = n4 / n2^2 - 3 (the
conventions of nucmorph.derive and of scipy.stats.skew / kurtosis; both are free of the unit).  With p = hist / A, Mag.HistEnergy = sum
p^2 and Mag.HistEntropy = - sum p ln p, 0 ln 0 = 0.  Canny.Sum = n_edge, Canny.Mean = n_edge / A.  Degenerate cases, so that no value is
ever NaN or infinite: A == 0 gives a row of zeros; a variance of zero (decided on the integer n2) gives Skewness = Kurtosis = 0."""
import math

import numpy as np

from . import nucmorph

ROW = 18
BINS = 10
(I_A, I_S1, I_S2, I_S3, I_S4, I_MN, I_MX, I_EDGE, I_HIST) = range(9)
T_MIN, T_MAX, T_DEFAULT = 1, 1442, 1
TAN_22 = 13573                        # tan(22.5 degrees) * 2^15, OpenCV's constant

COLUMNS = ('Nucleus.Gradient.Mag.Mean', 'Nucleus.Gradient.Mag.Std', 'Nucleus.Gradient.Mag.Skewness', 'Nucleus.Gradient.Mag.Kurtosis',
           'Nucleus.Gradient.Mag.HistEntropy', 'Nucleus.Gradient.Mag.HistEnergy', 'Nucleus.Gradient.Canny.Sum', 'Nucleus.Gradient.Canny.Mean')


def threshold(levels):
    """Grey levels per pixel -> T in quarter levels (round(4 x levels)); ValueError outside 1..1442."""
    T = int(round(4.0 * float(levels)))
    if not T_MIN <= T <= T_MAX:
        raise ValueError(f'edge threshold {levels}: {T_MIN / 4:g} .. {T_MAX / 4:g} grey levels per pixel')
    return T


def gradient2(h):
    """h int (H, W) -> (gx2, gy2) int64 (H, W): twice np.gradient along x and y; 0 along an axis of length 1."""
    h = np.asarray(h, np.float64)
    g = [np.zeros(h.shape, np.int64) if h.shape[ax] < 2 else np.rint(2.0 * np.gradient(h, axis=ax)).astype(np.int64) for ax in (1, 0)]
    return g[0], g[1]


def magnitude(tile_rgb):
    """(H, W, 3) uint8 RGB -> (m, q, gx2, gy2) int64 (H, W) of every frame pixel."""
    gx2, gy2 = gradient2(nucmorph.haematoxylin(np.asarray(tile_rgb, np.uint8)))
    q = gx2 * gx2 + gy2 * gy2
    vals, inv = np.unique(q, return_inverse=True)
    m = np.array([math.isqrt(4 * int(v)) for v in vals], np.int64)[inv].reshape(q.shape)
    return m, q, gx2, gy2


def edges(m, q, gx2, gy2, T=T_DEFAULT):
    """bool (H, W): the edge pixels of the whole frame (module docstring)."""
    H, W = q.shape
    ax, ay = np.abs(gx2), np.abs(gy2)
    hor = (ay << 15) < ax * TAN_22
    ver = ~hor & ((ay << 15) > ax * TAN_22 + (ax << 16))
    dia = ~hor & ~ver
    same = dia & (gx2 * gy2 > 0)
    other = dia & ~same
    p = np.pad(q, 1)
    at = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    out = np.zeros((H, W), bool)
    for sel, (d1, d2) in ((hor, ((0, -1), (0, 1))), (ver, ((-1, 0), (1, 0))), (same, ((-1, -1), (1, 1))), (other, ((-1, 1), (1, -1)))):
        out |= sel & (q > at(*d1)) & (q >= at(*d2))
    return out & (m >= T)


def grad_reference(tile_rgb, mask, T=T_DEFAULT):
    """tile_rgb (H, W, 3) uint8 in R, G, B order, mask bool (H, W), T 1..1442 -> int64 (18,): the row of the module docstring in numpy."""
    if not T_MIN <= int(T) <= T_MAX:
        raise ValueError(f'T {T}: {T_MIN} .. {T_MAX} quarter levels')
    mask = np.asarray(mask, bool)
    row = np.zeros(ROW, np.int64)
    if not mask.any():
        return row
    m, q, gx2, gy2 = magnitude(tile_rgb)
    v = m[mask]
    row[I_A] = len(v)
    row[I_S1:I_S4 + 1] = v.sum(), (v ** 2).sum(), (v ** 3).sum(), (v ** 4).sum()
    row[I_MN], row[I_MX] = v.min(), v.max()
    row[I_EDGE] = int((edges(m, q, gx2, gy2, int(T)) & mask).sum())
    row[I_HIST:] = np.histogram(v, bins=BINS)[0]
    return row


def derive(rows):
    """rows int (n, 18) or (18,) -> (COLUMNS, float64 (n, 8)).  Host float64 on exact Python integers; the formulas and the degenerate
    cases are those of the module docstring."""
    rows = np.asarray(rows, np.int64).reshape(-1, ROW)
    out = np.zeros((len(rows), len(COLUMNS)), np.float64)
    for i, r in enumerate(rows.tolist()):
        A, S1, S2, S3, S4 = r[I_A:I_S4 + 1]
        if A <= 0:
            continue
        if sum(r[I_HIST:]) != A:
            raise ValueError('derive: a histogram does not hold A samples')
        n2 = A * S2 - S1 * S1
        n3 = A * A * S3 - 3 * A * S1 * S2 + 2 * S1 ** 3
        n4 = A ** 3 * S4 - 4 * A * A * S1 * S3 + 6 * A * S1 * S1 * S2 - 3 * S1 ** 4
        out[i, 0] = S1 / (4.0 * A)
        out[i, 1] = math.sqrt(n2) / (4.0 * A)
        if n2 > 0:
            out[i, 2] = n3 / float(n2) ** 1.5
            out[i, 3] = n4 / (float(n2) * float(n2)) - 3.0
        p = [c / A for c in r[I_HIST:]]
        out[i, 4] = -sum(v * math.log(v) for v in p if v > 0)
        out[i, 5] = sum(v * v for v in p)
        out[i, 6] = float(r[I_EDGE])
        out[i, 7] = r[I_EDGE] / A
    return COLUMNS, out
