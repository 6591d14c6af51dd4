"""Designed crops, offsets and exact pair references shared by tests/test_merge_cases.py (what the cases reach, CPU) and
tests/test_hip_merge.py (csrc/merge.hip against them, GPU).  Plain numpy and the oracle.

A pair is two detections: member A (a shape) at the pair's position and member B (the same shape, or another one) shifted by
an offset.  Pairs sit on a 512-px pitch, so boxes of different pairs never meet and every pair is decided on its own; a
jitter of (7k % 64, 13k % 64) varies where a pair lies relative to the 64-px grid cells of the merge.  Every pair appears
twice: with scores (0.9, 0.8) and with the scores swapped, so each crop is read once as `i` (the wave's own detection) and
once as `j` (the candidate) by merge_pairs_kernel.

References (integers; the ratio is one double division, the same one the kernel does):
  polygon   oracle.merge_poly.Poly of the oracle.contour.mask2inst rings: inter8 / uni8 (1/8 px^2), 0.0 when uni8 == 0
  mask      pixel sets on a canvas: inter / uni
Every shape is named after what it guards; column numbers are crop columns (bit x & 31 of word x >> 5 of a row)."""
import functools

import numpy as np

PITCH = 512
MARGIN = 64                       # the placed set starts here, so that the offsets to the left stay at positive coordinates
PER_ROW = 40                      # pairs per row of the placement
SCORES = (0.9, 0.8)
DXS = (-33, -32, -31, -1, 0, 1, 5, 30, 31, 32, 33, 62, 63, 64)
DYS = (0, 3)
OFFSETS = tuple((dx, dy) for dx in DXS for dy in DYS)
CROSS_TARGETS = ('rect9x33', 'frag24')        # every shape also meets these two
CROSS_OFFSETS = ((5, 3), (-31, 0))
PINCH_COLS = (32, 33, 64)         # first column of the right part: the touch point lies between columns c - 1 | c


def disc(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return (yy * yy + xx * xx) <= r * r


def pinch(c, mirror):
    """Two rectangles that touch only diagonally between columns c - 1 | c: a larger one (12 rows; 14 columns, or 40 where
    the crop has room for them, so that the part itself crosses a word boundary) and a smaller one (8 x 9).  The larger one is
    left of the touch point, or right of it in the mirror image.  buffer(0) splits the ring's region there and the larger part
    is kept."""
    bw = 40 if c >= 40 else 14
    m = np.zeros((20, c + bw), bool)
    if not mirror:
        m[0:12, c - bw:c] = True
        m[12:20, c:c + 9] = True
    else:
        m[0:12, c:c + bw] = True
        m[12:20, c - 9:c] = True
    return m


@functools.lru_cache(maxsize=None)
def shapes():
    """name -> bool crop, in a fixed order."""
    s = {}
    for w in (31, 32, 33, 63, 64, 65, 97):                       # last word full, one bit into the next, one short of it
        s[f'rect9x{w}'] = np.ones((9, w), bool)
    s['rect1x40'] = np.ones((1, 40), bool)                       # a line: no polygon area
    s['rect2x40'] = np.ones((2, 40), bool)                       # one row of cells: the minimal polygon
    rng = np.random.default_rng(2024)
    for r in (16, 24, 40):                                       # several components, holes; 2, 2 and 3 words per row
        s[f'frag{r}'] = disc(r) & (rng.uniform(size=(2 * r + 1, 2 * r + 1)) < 0.93)
    for c in PINCH_COLS:
        s[f'pinch{c - 1}|{c}'] = pinch(c, False)
        s[f'pinch{c - 1}|{c}_mirror'] = pinch(c, True)
    m = np.zeros((12, 50), bool); m[1:11, 20:28] = True; m[5, 28:37] = True; m[1:11, 37:48] = True      # lobes 10 x 8 and 10 x 11
    s['bridge_over_32'] = m
    m = np.zeros((9, 65), bool); m[1:8, 50:57] = True; m[4, 57:65] = True                                # its last pixel is bit 0 of word 2
    s['spur_to_64'] = m
    m = np.zeros((48, 100), bool); m[2:46, 2:98] = True; m[8:40, 8:92] = False; m[14:34, 32:70] = True; m[20:28, 40:64] = False
    s['ring_island_at_32'] = m                                   # the island's first pixel is bit 0 of word 1, west of it a hole
    m = np.zeros((14, 40), bool); m[0:6, 2:12] = True; m[8:14, 32:40] = True
    s['second_comp_at_32'] = m                                   # found last, first pixel bit 0 of word 1, west of it the frame's background
    m = np.zeros((14, 40), bool); m[0:6, 20:40] = True; m[8:14, 0:8] = True
    s['second_comp_at_0'] = m                                    # found last, first pixel bit 0 of the first word of its row
    m = np.ones((150, 150), bool); m[50:90, 60:100] = False
    s['big150_hole'] = m                                         # 3 x 3 grid cells or more wherever it lies
    return s


PINCH = tuple(k for k in shapes() if k.startswith('pinch'))
SEVERAL_RINGS = ('frag16', 'frag24', 'frag40', 'ring_island_at_32', 'second_comp_at_32', 'second_comp_at_0')

# offsets at which the boxes of a shape and its shifted copy intersect but the pixel sets do not
DISJOINT = {
    'frag16': ((29, 29),), 'frag24': ((45, 45),), 'frag40': ((77, 77),),          # the 4 x 4 box corners of a disc are empty
    'pinch31|32': ((0, -12), (-14, 8)), 'pinch32|33_mirror': ((0, -12), (14, 8)),   # a part over the empty quadrant of the copy
    'second_comp_at_32': ((0, 7), (10, 0)), 'second_comp_at_0': ((0, 7),),
}


@functools.lru_cache(maxsize=None)
def pairs():
    """[(name of A, name of B, dx, dy, swapped)]: B is shifted by (dx, dy) against A; swapped: B has the higher score."""
    out = []
    for a in shapes():
        for dx, dy in OFFSETS + DISJOINT.get(a, ()):
            out.append((a, a, dx, dy))
        for b in CROSS_TARGETS:
            if b != a:
                for dx, dy in CROSS_OFFSETS:
                    out.append((a, b, dx, dy))
    return tuple(p + (sw,) for p in out for sw in (False, True))


def position(k):
    return (MARGIN + PITCH * (k % PER_ROW) + (7 * k) % 64, MARGIN + PITCH * (k // PER_ROW) + (13 * k) % 64)


@functools.lru_cache(maxsize=None)
def placed():
    """-> (masks [(crop, x0, y0)], scores): pair k is detections 2k (member A) and 2k + 1 (member B)."""
    masks, scores = [], []
    sh = shapes()
    for k, (a, b, dx, dy, sw) in enumerate(pairs()):
        x, y = position(k)
        masks += [(sh[a], x, y), (sh[b], x + dx, y + dy)]
        scores += list(SCORES[::-1] if sw else SCORES)
    return masks, scores


def boxes_intersect(a, b, dx, dy):
    (ha, wa), (hb, wb) = shapes()[a].shape, shapes()[b].shape
    return min(wa, dx + wb) > max(0, dx) and min(ha, dy + hb) > max(0, dy)


def inter_width(a, b, dx, dy):
    """Columns of the intersection rectangle of the two boxes (0 if they do not intersect)."""
    (ha, wa), (hb, wb) = shapes()[a].shape, shapes()[b].shape
    return max(0, min(wa, dx + wb) - max(0, dx)) if boxes_intersect(a, b, dx, dy) else 0


@functools.lru_cache(maxsize=None)
def rings():
    from oracle import contour as OC
    return {k: OC.mask2inst(m) for k, m in shapes().items()}


@functools.lru_cache(maxsize=None)
def _poly_ref(a, b, dx, dy):
    from oracle.merge_poly import Poly
    pa, pb = Poly(rings()[a]), Poly(rings()[b] + np.array([dx, dy], np.int64))
    inter = pa.inter8(pb)
    return inter, pa.area8 + pb.area8 - inter


@functools.lru_cache(maxsize=None)
def _mask_ref(a, b, dx, dy):
    ma, mb = shapes()[a], shapes()[b]
    x0, y0 = min(0, dx), min(0, dy)
    x1, y1 = max(ma.shape[1], dx + mb.shape[1]), max(ma.shape[0], dy + mb.shape[0])
    ca, cb = np.zeros((y1 - y0, x1 - x0), bool), np.zeros((y1 - y0, x1 - x0), bool)
    ca[-y0:-y0 + ma.shape[0], -x0:-x0 + ma.shape[1]] = ma
    cb[dy - y0:dy - y0 + mb.shape[0], dx - x0:dx - x0 + mb.shape[1]] = mb
    return int((ca & cb).sum()), int((ca | cb).sum())


@functools.lru_cache(maxsize=None)
def reference(mode):
    """-> (inter [pairs], uni [pairs], r [pairs] float64) of one overlap measure ('polygon' in 1/8 px^2, 'mask' in pixels)."""
    f = dict(polygon=_poly_ref, mask=_mask_ref)[mode]
    iu = [f(a, b, dx, dy) for a, b, dx, dy, _ in pairs()]
    r = np.array([i / u if u > 0 else 0.0 for i, u in iu], np.float64)
    r.setflags(write=False)
    return tuple(i for i, _ in iu), tuple(u for _, u in iu), r


def describe(k, mode):
    a, b, dx, dy, sw = pairs()[k]
    inter, uni, r = reference(mode)
    return (f'pair {k}: {a} at {position(k)} vs {b} shifted by ({dx}, {dy}), {"B" if sw else "A"} scored higher; '
            f'{mode} inter {inter[k]} uni {uni[k]} r {float(r[k])!r}')
