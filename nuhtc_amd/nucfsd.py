"""Per-nucleus Fourier shape descriptors: the six `Shape.FSD*` columns of the reference's hand-crafted table (tools/wsi_feat_extract.py /
tools/nuclei_feat_extract.py: histomicstk's compute_nuclei_features over one crop per nucleus on the host), from integers the GPU takes
from the ORDERED BOUNDARY of a nucleus (csrc/nucfsd.hip).  THE DEVICE PRODUCES INTEGERS ONLY, and every named floating-point feature is
derived here, on the host, in float64, by one function (`derive`).  `fsd_reference` is the numpy restatement of the integers (np.cumsum
and a vectorised exact comparison, no floats); the device must equal it bit for bit.  The integers of one nucleus are a pure function of
its ring: no mask, no frame, no tile, no tracing -- on the document route (nuhtc_amd/ringfeat.py) the ring is already on the device, as
the `verts` / `ring_off` that nuhtc_op_ring_fill receives.

histomicstk's names and meaning, THE PROJECT'S OWN DEFINITION: histomicstk and scikit-image are not dependencies, nothing here was
compared with histomicstk and no fixture is pinned to it.  Two differences are known.  histomicstk hands its `_FSDs` the boundary pixels
in RASTER order (np.argwhere of the boundary image); this module walks the ring in CONTOUR order, vertex after vertex, which is what
"tangent angle along the boundary" means.  And the resampling here is exact: a sample's edge is an integer decision (below), where
histomicstk interpolates in floats.

Ring.  Integer vertices v_0 .. v_{n-1}, the closing vertex not repeated; x right, y down.  Edge e runs from v_e to v_{(e+1) mod n}, with
(dx, dy) its difference.  An edge is ON THE CHAIN when dx == 0, dy == 0 or |dx| == |dy|: max(|dx|, |dy|) unit steps (dx == 0 or
dy == 0: axial steps of length 1) or diagonal steps (length sqrt 2).  A zero-length edge is on the chain and contributes nothing.  The
Freeman code d_e follows csrc/contour.hip: 0 = east, counter-clockwise on the screen, dx = {1,1,0,-1,-1,-1,0,1}, dy = {0,-1,-1,-1,0,1,1,1}
(DX, DY); a zero-length edge has the code 0.  a_e and b_e are the numbers of axial and of diagonal unit steps on the edges BEFORE e
(a_0 = b_0 = 0), A and B the totals over all n edges: the edge e starts at the length a_e + b_e sqrt 2 along the ring, and the perimeter
is L = A + B sqrt 2.

Row.  int32 [4 + 5 * 128] = [644], K = 128 samples:

    0 .. 3                status, A, B, n
    4 + 5 k .. 8 + 5 k    x_e, y_e, d_e, a_e, b_e of the edge e = e(k) that holds sample k = 0 .. 127: its start vertex, code and start length

e(k) is the LARGEST e in 0 .. n - 1 with a_e + b_e sqrt 2 <= (k / K) (A + B sqrt 2), decided EXACTLY: with the integers
p = K a_e - k A and q = K b_e - k B the condition is p + q sqrt 2 <= 0, and the sign of p + q sqrt 2 (`sign`) is
    that of p and q where neither contradicts the other (p >= 0 and q >= 0: +1 unless both are 0; p <= 0 and q <= 0: -1 unless both are 0),
    otherwise (p q < 0) the sign of p times the sign of p^2 - 2 q^2, in int64.
sqrt 2 is irrational, so the value is zero only when p = q = 0 and p^2 - 2 q^2 is never zero for non-zero integers.  A tie therefore
selects the later vertex: a sample that falls on a vertex belongs to the edge that LEAVES it (and, past zero-length edges, to the last
edge that starts there).  The start lengths do not decrease with e, so the condition holds for e = 0 .. e(k) and fails beyond.

The bound.  A ring is measured when A + B <= 2^24 (MAX_STEPS).  Then 0 <= a_e <= A, 0 <= b_e <= B and 0 <= k < K give |p| <= K A and
|q| <= K B.  The squares are formed only when p q < 0, which needs A >= 1 and B >= 1, so |p| <= 2^7 (2^24 - 1) and |q| <= 2^7 (2^24 - 1):
p^2 < 2^62 and 2 q^2 < 2^63, both inside int64.  One step more and 2 q^2 could reach 2^63.  Every cumulative count fits an int32.

Status.  0 = measured.  1 = degenerate: no vertex (an empty ring) or A + B == 0 (every vertex the same point).  2 = not a traced ring: an
edge off the chain, or -- in a batch -- ring offsets that leave [0, nv] or decrease (nuhtc_op_ring_fill's 2).  3 = A + B > 2^24 steps.
With any status other than 0 the other 643 entries are zero.

Features (`derive`; COLUMNS are histomicstk's names).  Sample k lies s_k = (k / K) L - (a_e + b_e sqrt 2) = -(p + q sqrt 2) / K >= 0
along its edge: P_k = v_e + (DX, DY)[d_e] s_k / (1 or sqrt 2).  The K chords P_{k+1} - P_k (P_K = P_0) have the angles theta_k = atan2
of the chord; the turning steps theta_k - theta_{k-1}, k = 1 .. K - 1, are wrapped into (-pi, pi]; the unwrapped tangent angle relative
to the first chord is c_0 = 0, c_k = the running sum of the wrapped steps.  E_m = |FFT(c)_m|^2 for m = 0 .. 64, and
Shape.FSD i = sum of E_m over band i / sum of E_m over m = 0 .. 64 with the bands [0, 2) [2, 4) [4, 8) [8, 16) [16, 32) [32, 65) (BANDS):
the six columns sum to 1.  The ramp 2 pi k / K of a closed curve is NOT removed (what is left of a round nucleus would be normalised
discretisation noise), and the spectrum is that of the angle, not of the turning steps (chain turns are impulses: a disc would put most
of its energy into the two highest bands).  A row with a status other than 0, or a zero denominator, gives six zeros; no value is ever
NaN or infinite."""
import numpy as np

K = 128
HEAD = 4
PER = 5
ROW = HEAD + PER * K
MAX_STEPS = 1 << 24
(I_STATUS, I_A, I_B, I_N) = range(4)
(OK, DEGENERATE, NOT_TRACED, TOO_LONG) = range(4)
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, -1, -1, -1, 0, 1, 1, 1)
BANDS = ((0, 2), (2, 4), (4, 8), (8, 16), (16, 32), (32, 65))

COLUMNS = tuple(f'Shape.FSD{i}' for i in range(1, 7))

_CODE = np.zeros((3, 3), np.int64)                  # [sign dy + 1][sign dx + 1] -> Freeman code; the centre (no step) is 0
for _d in range(8):
    _CODE[DY[_d] + 1, DX[_d] + 1] = _d


def sign(p, q):
    """The sign (-1, 0, 1) of p + q sqrt 2 for int64 arrays within the module docstring's bound, exactly."""
    p, q = np.asarray(p, np.int64), np.asarray(q, np.int64)
    opposite = ((p > 0) & (q < 0)) | ((p < 0) & (q > 0))
    po, qo = np.where(opposite, p, 0), np.where(opposite, q, 0)         # the squares are formed where they are needed, and only there
    return np.where(opposite, np.sign(po) * np.sign(po * po - 2 * qo * qo), np.where((p > 0) | (q > 0), 1, np.where((p < 0) | (q < 0), -1, 0)))


def edges(ring):
    """ring int (n, 2) -> (on_chain bool (n,), steps int64 (n,), diagonal bool (n,), code int64 (n,)) of the n edges."""
    v = np.asarray(ring, np.int64).reshape(-1, 2)
    d = np.roll(v, -1, 0) - v
    ax, ay = np.abs(d[:, 0]), np.abs(d[:, 1])
    diagonal = (ax != 0) & (ay != 0)
    return ~diagonal | (ax == ay), np.maximum(ax, ay), diagonal, _CODE[np.sign(d[:, 1]) + 1, np.sign(d[:, 0]) + 1]


def fsd_reference(ring):
    """ring int (n, 2) without the closing vertex -> int32 (644,): the row of the module docstring in numpy, integers only."""
    v = np.asarray(ring, np.int64).reshape(-1, 2)
    row = np.zeros(ROW, np.int32)
    n = len(v)
    if n < 1:
        row[I_STATUS] = DEGENERATE
        return row
    on_chain, steps, diagonal, code = edges(v)
    if not on_chain.all():
        row[I_STATUS] = NOT_TRACED
        return row
    sa, sb = np.where(diagonal, 0, steps), np.where(diagonal, steps, 0)
    A, B = int(sa.sum()), int(sb.sum())                                  # |coordinate| < 2^30 and n < 2^31: inside int64
    if A + B == 0 or A + B > MAX_STEPS:
        row[I_STATUS] = DEGENERATE if A + B == 0 else TOO_LONG
        return row
    a, b = np.cumsum(sa) - sa, np.cumsum(sb) - sb                        # exclusive: the steps before the edge
    k = np.arange(K, dtype=np.int64)[:, None]
    e = (sign(K * a[None, :] - k * A, K * b[None, :] - k * B) <= 0).sum(1) - 1      # the condition holds for e = 0 .. e(k): count, minus one
    row[:HEAD] = OK, A, B, n
    row[HEAD:] = np.stack([v[e, 0], v[e, 1], code[e], a[e], b[e]], 1).reshape(-1)
    return row


def fsd_reference_batch(verts, ring_off):
    """verts int (nv, 2), ring_off int (n + 1,) -> int32 (n, 644): ring i = verts[ring_off[i]:ring_off[i + 1]], the status 2 for
    offsets that leave [0, nv] or decrease."""
    verts, off = np.asarray(verts, np.int64).reshape(-1, 2), np.asarray(ring_off, np.int64)
    out = np.zeros((len(off) - 1, ROW), np.int32)
    for i in range(len(off) - 1):
        lo, hi = int(off[i]), int(off[i + 1])
        if lo < 0 or hi < lo or hi > len(verts):
            out[i, I_STATUS] = NOT_TRACED
        else:
            out[i] = fsd_reference(verts[lo:hi])
    return out


def sample_points(rows):
    """rows int (n, 644) -> (P float64 (n, 128, 2), s float64 (n, 128)): the sample points and their distance along their edge; zeros for
    a row whose status is not 0."""
    rows = np.asarray(rows, np.int64).reshape(-1, ROW)
    ok = (rows[:, I_STATUS] == OK)[:, None]
    A, B = rows[:, I_A, None], rows[:, I_B, None]
    x, y, d, a, b = (rows[:, HEAD + j::PER] for j in range(PER))
    k = np.arange(K, dtype=np.int64)[None, :]
    root = np.sqrt(2.0)
    # -(p + q sqrt 2) / K with the exact integers p and q: the same number as (k / K) L - (a + b sqrt 2), without its rounding of L
    s = np.where(ok, np.maximum(((k * A - K * a) + (k * B - K * b) * root) / K, 0.0), 0.0)
    t = s / np.where(d & 1, root, 1.0)
    P = np.stack([x + np.asarray(DX, np.float64)[d & 7] * t, y + np.asarray(DY, np.float64)[d & 7] * t], -1)
    return np.where(ok[:, :, None], P, 0.0), s


def tangent_angle(rows):
    """rows int (n, 644) -> c float64 (n, 128): the unwrapped tangent angle relative to the first chord (module docstring)."""
    P, _ = sample_points(rows)
    chord = np.roll(P, -1, 1) - P
    theta = np.arctan2(chord[..., 1], chord[..., 0])
    w = np.diff(theta, axis=1)
    w = w - 2.0 * np.pi * np.ceil((w - np.pi) / (2.0 * np.pi))          # into (-pi, pi]
    return np.concatenate([np.zeros((len(P), 1)), np.cumsum(w, 1)], 1)


def derive(rows):
    """rows int (n, 644) or (644,) -> (COLUMNS, float64 (n, 6)).  Host float64, vectorised over the nuclei; the formulas and the
    degenerate cases are those of the module docstring."""
    rows = np.asarray(rows, np.int64).reshape(-1, ROW)
    E = np.abs(np.fft.rfft(tangent_angle(rows), axis=1)) ** 2           # m = 0 .. 64
    band = np.stack([E[:, lo:hi].sum(1) for lo, hi in BANDS], 1)
    total = E.sum(1)
    good = (rows[:, I_STATUS] == OK) & (total > 0.0) & np.isfinite(total)
    return COLUMNS, np.where(good[:, None], band / np.where(good, total, 1.0)[:, None], 0.0)
