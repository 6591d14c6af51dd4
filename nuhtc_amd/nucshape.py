"""Per-nucleus shape features: the seven `Shape.HuMoments*` columns and `Shape.FractalDimension` of the reference's hand-crafted table
(tools/wsi_feat_extract.py / tools/nuclei_feat_extract.py: histomicstk's compute_nuclei_features over one crop per nucleus on the host),
from integers the GPU takes from the mask of a nucleus (csrc/nucshape.hip).  THE DEVICE PRODUCES INTEGERS ONLY, and every named
floating-point feature is derived here, on the host, in float64, by one function (`derive`).  `shape_reference` is the numpy restatement
of the integers (np.add.reduceat on the rectangle's crop); the device must equal it bit for bit.  The integers of one nucleus are a pure
function of its mask: no tile, no stain table.  histomicstk's names and meaning; the box counts are the project's own definition --
written from the numpy-100 #87 box-counting recipe that histomicstk uses for Shape.FractalDimension, and not compared with histomicstk
itself, which is not a dependency.  The Hu moments are scikit-image's (regionprops(...).moments_hu of 0.18.3, which histomicstk calls;
tests/golden/nucshape_skimage.npz).  histomicstk's third shape family, Shape.FSD1..6, is a function of the ring, not of the mask: nucfsd.py.

Mask.  A binary mask M in an H x W frame; x is the column, y the row, both frame pixels.

Row.  int64 [24]:

    0        A, the number of set pixels
    1 .. 4   x0 y0 x1 y1, the bounding rectangle of the set pixels, x1 and y1 exclusive; all 0 when A == 0
    5 .. 9   Sx Sy Sxx Sxy Syy, the sums over the set pixels of x, y, x^2, x y, y^2
    10 .. 13 Sxxx Sxxy Sxyy Syyy, the sums of x^3, x^2 y, x y^2, y^3 (a full 1024 x 1024 frame gives 2.8e14: int64 with room)
    14 .. 23 N_1 .. N_10, the box counts

Box counts.  With s = 2^j, the boxes are the s x s squares anchored at the RECTANGLE's corner (x0, y0), not at the frame's: box (i, k)
covers x0 + i s <= x < x0 + (i + 1) s and y0 + k s <= y < y0 + (k + 1) s.  A position outside the rectangle is unset, whether or not it
lies inside the frame.  N_j counts the boxes that hold at least one set pixel and at least one unset position among their s^2 positions;
a box truncated by the rectangle's right or bottom edge therefore counts whenever it holds a set pixel.  This is numpy-100's
`0 < S < k * k` on the region image with np.add.reduceat.  All ten are written, sizes larger than the rectangle included (one box, which
counts unless the rectangle is a solid square of exactly that side).  An empty mask, or a list entry outside the batch, gives a zero row.

Features (`derive`; `COLUMNS` are histomicstk's names).

Hu moments.  The central-moment numerators are exact Python integers before the first division: c20 = A Sxx - Sx^2, c11 = A Sxy - Sx Sy,
c02 = A Syy - Sy^2, c30 = A^2 Sxxx - 3 A Sx Sxx + 2 Sx^3, c21 = A^2 Sxxy - 2 A Sx Sxy - A Sy Sxx + 2 Sx^2 Sy, c12 = A^2 Sxyy - 2 A Sy Sxy -
A Sx Syy + 2 Sy^2 Sx, c03 = A^2 Syyy - 3 A Sy Syy + 2 Sy^3 (first index the power of x).  The normalised moments are c_pq / A^3 for the
second order and c_pq / A^4.5 for the third, and the seven standard Hu invariants follow.  scikit-image indexes moments (row, column):
its nu[p, q] carries y^p x^q.  The first six invariants do not notice; the seventh changes sign.  SCIKIT-IMAGE'S CONVENTION IS USED: the
invariants are formed with n20 = c02 / A^3, n02 = c20 / A^3, n30 = c03 / A^4.5, n21 = c12 / A^4.5, n12 = c21 / A^4.5, n03 = c30 / A^4.5,
which reproduces regionprops(...).moments_hu; fed as (x, y), Hu7 would have the opposite sign.

Fractal dimension.  With w = x1 - x0, h = y1 - y0 and n = floor(log2(min(w, h))), the sizes 2^j for j = 2 .. n are used (the recipe
leaves size 2 out); the dimension is minus the least-squares slope of ln N_j on ln 2^j, in closed form in float64 (no np.polyfit, whose
RankWarning the reference has to silence).  It is 0.0 when fewer than two sizes exist (min(w, h) < 8) or when any used N_j is 0, decided
on the integers.  A == 0 gives a row of zeros; no value is ever NaN or infinite."""
import math

import numpy as np

ROW = 24
LEVELS = 10
(I_A, I_X0, I_Y0, I_X1, I_Y1, I_SX, I_SY, I_SXX, I_SXY, I_SYY, I_SXXX, I_SXXY, I_SXYY, I_SYYY, I_BOX) = range(15)

COLUMNS = tuple(f'Shape.HuMoments{k}' for k in range(1, 8)) + ('Shape.FractalDimension',)


def box_counts(crop):
    """crop bool (h, w), the rectangle's crop -> list of the ten counts N_1 .. N_10: numpy-100's rule with np.add.reduceat."""
    z = np.asarray(crop).astype(np.int64)
    out = []
    for j in range(1, LEVELS + 1):
        s = 1 << j
        S = np.add.reduceat(np.add.reduceat(z, np.arange(0, z.shape[0], s), axis=0), np.arange(0, z.shape[1], s), axis=1)
        out.append(int(((S > 0) & (S < s * s)).sum()))
    return out


def shape_reference(mask):
    """mask bool (H, W) -> int64 (24,): the row of the module docstring in numpy."""
    mask = np.asarray(mask, bool)
    row = np.zeros(ROW, np.int64)
    ys, xs = np.nonzero(mask)
    if len(xs) == 0:
        return row
    x, y = xs.astype(np.int64), ys.astype(np.int64)
    x0, y0, x1, y1 = int(x.min()), int(y.min()), int(x.max()) + 1, int(y.max()) + 1
    row[I_A] = len(x)
    row[I_X0:I_Y1 + 1] = x0, y0, x1, y1
    row[I_SX:I_SYY + 1] = x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum()
    row[I_SXXX:I_SYYY + 1] = (x * x * x).sum(), (x * x * y).sum(), (x * y * y).sum(), (y * y * y).sum()
    row[I_BOX:] = box_counts(mask[y0:y1, x0:x1])
    return row


def hu_invariants(n20, n11, n02, n30, n21, n12, n03):
    """The seven Hu invariants of normalised central moments, the first index the power of the FIRST coordinate."""
    t0, t1 = n30 + n12, n21 + n03
    q0, q1 = t0 * t0, t1 * t1
    s, d = n20 + n02, n20 - n02
    a, b = n30 - 3.0 * n12, 3.0 * n21 - n03
    return (s, d * d + 4.0 * n11 * n11, a * a + b * b, q0 + q1, a * t0 * (q0 - 3.0 * q1) + b * t1 * (3.0 * q0 - q1),
            d * (q0 - q1) + 4.0 * n11 * t0 * t1, b * t0 * (q0 - 3.0 * q1) - a * t1 * (3.0 * q0 - q1))


def fractal_sizes(w, h):
    """The exponents j of the box sizes the dimension uses: 2 .. floor(log2(min(w, h))) (empty or one entry: no dimension)."""
    side = min(int(w), int(h))
    return list(range(2, side.bit_length())) if side > 0 else []


def slope(xs, ys):
    """The least-squares slope of ys on xs in closed form; len >= 2 and the xs not all equal."""
    n = len(xs)
    mx, my = math.fsum(xs) / n, math.fsum(ys) / n
    return math.fsum((x - mx) * (y - my) for x, y in zip(xs, ys)) / math.fsum((x - mx) * (x - mx) for x in xs)


def derive(rows):
    """rows int (n, 24) or (24,) -> (COLUMNS, float64 (n, 8)).  Host float64 on exact Python integers; the formulas and the degenerate
    cases are those of the module docstring."""
    rows = np.asarray(rows, np.int64).reshape(-1, ROW)
    out = np.zeros((len(rows), len(COLUMNS)), np.float64)
    for i, r in enumerate(rows.tolist()):
        A = r[I_A]
        if A <= 0:
            continue
        Sx, Sy, Sxx, Sxy, Syy, Sxxx, Sxxy, Sxyy, Syyy = r[I_SX:I_SYYY + 1]
        c20, c11, c02 = A * Sxx - Sx * Sx, A * Sxy - Sx * Sy, A * Syy - Sy * Sy
        c30 = A * A * Sxxx - 3 * A * Sx * Sxx + 2 * Sx ** 3
        c21 = A * A * Sxxy - 2 * A * Sx * Sxy - A * Sy * Sxx + 2 * Sx * Sx * Sy
        c12 = A * A * Sxyy - 2 * A * Sy * Sxy - A * Sx * Syy + 2 * Sy * Sy * Sx
        c03 = A * A * Syyy - 3 * A * Sy * Syy + 2 * Sy ** 3
        a3, a4, root = A ** 3, A ** 4, math.sqrt(A)
        # scikit-image's (row, column) order: the first index is the power of y
        out[i, :7] = hu_invariants(c02 / a3, c11 / a3, c20 / a3, c03 / a4 / root, c12 / a4 / root, c21 / a4 / root, c30 / a4 / root)
        js = fractal_sizes(r[I_X1] - r[I_X0], r[I_Y1] - r[I_Y0])
        counts = [r[I_BOX + j - 1] for j in js]
        if len(js) >= 2 and all(c > 0 for c in counts):
            out[i, 7] = 0.0 - slope([math.log(1 << j) for j in js], [math.log(c) for c in counts])
    return COLUMNS, out
