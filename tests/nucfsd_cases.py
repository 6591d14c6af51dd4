"""Designed rings for the Fourier-descriptor integers (nuhtc_amd/nucfsd.py), shared by tests/test_nucfsd_host.py and
tests/test_hip_nucfsd.py: every ring is an int64 (n, 2) array of (x, y) without the closing vertex, a few to a few thousand vertices."""
import math

import numpy as np

from nuhtc_amd import nucfsd as nf

CHAIN = np.stack([np.asarray(nf.DX), np.asarray(nf.DY)], 1)


def from_moves(moves, start=(0, 0)):
    """[(code, length)] -> the ring that starts at `start` and makes the moves; the last move must lead back to the start and is the
    closing edge."""
    v = [np.asarray(start, np.int64)]
    for d, n in moves:
        v.append(v[-1] + CHAIN[d] * n)
    assert (v[-1] == v[0]).all(), 'the moves do not close'
    return np.stack(v[:-1])


def saw(n, seed=0):
    """A closed ring of exactly n >= 4 vertices: teeth of diagonal edges with axial runs between them along the top, then down, back
    along the bottom and up."""
    rng = np.random.default_rng(seed)
    pts, x, y = [(0, 0)], 0, 0
    while len(pts) < n - 2:
        kind = len(pts) % 3
        step = int(rng.integers(1, 4))
        if kind == 0:
            x += step                                  # east
        elif y == 0:
            x, y = x + step, -step                     # north-east
        else:
            x, y = x - y, 0                            # south-east, back to the base line
        pts.append((x, y))
    pts += [(x, 7), (0, 7)]
    return np.asarray(pts, np.int64)


def comb(teeth=520):
    """4 * teeth + 2 vertices (more than 2000: several chunks of the device's walk), axial edges only."""
    pts = []
    for i in range(teeth):
        pts += [(4 * i, 0), (4 * i, -9), (4 * i + 2, -9), (4 * i + 2, 0)]
    pts += [(4 * teeth - 2, 3), (0, 3)]
    return np.asarray(pts, np.int64)


# ---- the ring on which float64 picks the wrong edge.  (P, Q) = (318281039, 225058681) is a convergent of sqrt 2 (P^2 - 2 Q^2 = -1), so
# p = 2 Q, q = -P has p^2 - 2 q^2 = +2: p + q sqrt 2 = 2 / (p - q sqrt 2) = 2.2e-9 > 0, far below the 6e-8 spacing of float64 at q sqrt 2.
# (p is even because the axial steps of a closed chain ring are.)  With k = 71, A = 7896834 and B = 4482873 the vertex whose start length
# is (a, b) = (7896817, 23) has K a - k A = p and K b - k B = q exactly: it lies 1.7e-11 pixels BEYOND sample 71.
PELL = dict(k=71, p=450117362, q=-318281039, A=7896834, B=4482873, a=7896817, b=23, vertex=4)


def pell_ring():
    """Nine vertices near (2^29, 2^29): east / west spikes of a axial steps and south-east / north-west spikes of b diagonal steps, the
    vertex PELL['vertex'], then the remaining A - a and B - b steps the same way and one step north to close."""
    c = PELL
    a, b, ra, rb = c['a'], c['b'], c['A'] - c['a'] - 1, c['B'] - c['b']
    split = lambda total, net: ((total + net) // 2, (total - net) // 2)          # (forth, back) with forth + back = total, forth - back = net
    sx, sd = a % 2, b % 2
    (e1, w1), (d1, u1) = split(a, sx), split(b, sd)
    (e2, w2), (d2, u2) = split(ra, -1 - sx), split(rb, 1 - sd)
    ring = from_moves([(0, e1), (4, w1), (7, d1), (3, u1), (0, e2), (4, w2), (7, d2), (3, u2), (2, 1)], start=(1 << 29, 1 << 29))
    assert len(ring) == 9 and np.abs(ring).max() < 2 ** 30
    return ring


def float_sign(p, q):
    """The sign of p + q * sqrt(2.0) as float64 evaluates it."""
    v = float(p) + float(q) * math.sqrt(2.0)
    return (v > 0) - (v < 0)


def designed():
    """name -> ring, in a fixed order; the statuses are in STATUS."""
    out = {
        'one vertex': [(5, 7)],
        'two vertices, axial': [(0, 0), (9, 0)],
        'two vertices, diagonal': [(3, 3), (-6, 12)],
        'square of perimeter 128': [(10, 20), (42, 20), (42, 52), (10, 52)],
        'square of perimeter 256': [(0, 0), (0, 64), (64, 64), (64, 0)],
        'diamond, A = 0': [(0, 0), (7, 7), (14, 0), (7, -7)],
        'rectangle, B = 0': [(2, 3), (22, 3), (22, 9), (2, 9)],
        'zero-length edges': [(0, 0), (0, 0), (5, 0), (5, 0), (5, 0), (8, 3), (5, 6), (0, 6), (0, 6)],
        'closing vertex repeated': [(0, 0), (6, 0), (6, 6), (0, 6), (0, 0)],
        'one point three times': [(4, 4), (4, 4), (4, 4)],
        'off the chain': [(0, 0), (3, 1), (3, 3), (0, 3)],
        'more than 2^24 steps': [(0, 0), (3000000, 0), (6000000, 3000000), (6000000, 6000000), (3000000, 6000000), (0, 3000000)],
        'exactly 2^24 steps': [(0, 0), (8388607, 0), (8388607, 1), (0, 1)],
        'empty': np.zeros((0, 2), np.int64),
        'comb of 2082 vertices': comb(),
        'pell': pell_ring(),
    }
    for n in (63, 64, 65, 255, 256, 257, 1025):
        out[f'saw of {n} vertices'] = saw(n, seed=n)
    return {k: np.asarray(v, np.int64).reshape(-1, 2) for k, v in out.items()}


STATUS = {'one vertex': 1, 'one point three times': 1, 'empty': 1, 'off the chain': 2, 'more than 2^24 steps': 3}       # every other ring: 0


def disc(r):
    yy, xx = np.mgrid[-r - 1:r + 2, -r - 1:r + 2]
    return xx * xx + yy * yy <= r * r


def ellipse(rx, ry):
    yy, xx = np.mgrid[-ry - 1:ry + 2, -rx - 1:rx + 2]
    return (xx / float(rx)) ** 2 + (yy / float(ry)) ** 2 <= 1.0


def clover(r=12, lobe=5):
    yy, xx = np.mgrid[-r - lobe - 1:r + lobe + 2, -r - lobe - 1:r + lobe + 2]
    return np.hypot(xx, yy) <= r + lobe * np.cos(4 * np.arctan2(yy, xx))


def traced(mask, origin=(0, 0)):
    """The ring contours.mask_to_ring writes for the mask, without its closing vertex."""
    from nuhtc_amd import contours
    r = np.asarray(contours.mask_to_ring(mask, origin), np.int64).reshape(-1, 2)
    return r[:-1] if len(r) > 1 and (r[0] == r[-1]).all() else r
