"""Designed masks of the shape tests (tests/test_nucshape_host.py, tests/test_hip_nucshape.py) and of the skimage fixture
(tools/dev/make_shape_golden.py -> tests/golden/nucshape_skimage.npz), and the row of nuhtc_amd/nucshape.py in plain Python loops.
numpy only: the fixture script runs under another interpreter."""
import numpy as np

H_SMALL, W_SMALL = 64, 40            # W is no multiple of 32: the last word of a row has 8 pixels and 24 padding bits


def blob(h, w, rng):
    """bool (h, w): a random blob that touches all four sides of its h x w rectangle -- an ellipse with a noisy rim and, from 12 pixels a
    side, a hole."""
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    ang = np.arctan2(yy - cy, xx - cx)
    rim = 1.0 + 0.25 * np.sin(3 * ang + rng.uniform(0, 6.28)) * rng.uniform(0.3, 1.0) + 0.1 * np.sin(7 * ang + rng.uniform(0, 6.28))
    d = np.sqrt(((yy - cy) / (h / 2.0)) ** 2 + ((xx - cx) / (w / 2.0)) ** 2)
    m = d <= 0.8 * rim
    m &= rng.random((h, w)) < 0.97
    if min(h, w) >= 12:
        hy, hx = rng.integers(h // 3, 2 * h // 3), rng.integers(w // 3, 2 * w // 3)
        m &= (yy - hy) ** 2 + (xx - hx) ** 2 > (min(h, w) // 8) ** 2
    m[0, w // 2] = m[h - 1, w // 2] = m[h // 2, 0] = m[h // 2, w - 1] = True      # the rectangle is the whole h x w
    return m


def disc(h, w, cx, cy, r, r_in=-1):
    """bool (h, w): r_in^2 < (x - cx)^2 + (y - cy)^2 <= r^2, clipped by the frame."""
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (yy - cy) ** 2 + (xx - cx) ** 2
    return (d2 <= r * r) & (d2 > r_in * abs(r_in))


def checkerboard(h, w, x0, y0, n):
    """bool (h, w): an n x n checkerboard whose corner pixel (x0, y0) is set."""
    m = np.zeros((h, w), bool)
    yy, xx = np.mgrid[0:n, 0:n]
    m[y0:y0 + n, x0:x0 + n] = ((yy + xx) & 1) == 0
    return m


def small_masks():
    """name -> bool (64, 40): the designed masks of the device test, in the frame whose width is no multiple of 32."""
    H, W = H_SMALL, W_SMALL
    blank = lambda: np.zeros((H, W), bool)
    m = {'empty': blank()}
    m['pixel at (0, 0)'] = blank(); m['pixel at (0, 0)'][0, 0] = True
    m['pixel at (39, 63)'] = blank(); m['pixel at (39, 63)'][63, 39] = True
    m['solid 8x8 at x0=0'] = blank(); m['solid 8x8 at x0=0'][10:18, 0:8] = True
    m['solid 8x8 at x0=29'] = blank(); m['solid 8x8 at x0=29'][20:28, 29:37] = True                  # straddles the word boundary at 32
    m['solid 7x5 in the last corner'] = blank(); m['solid 7x5 in the last corner'][H - 5:, W - 7:] = True
    m['disc r=12 at x=32'] = disc(H, W, 32, 30, 12)                                                  # centred on the word boundary, cut by the frame's right edge
    m['disc r=12 at x=20'] = disc(H, W, 20, 40, 12)
    m['annulus'] = disc(H, W, 19, 32, 15, 7)
    m['checkerboard 16x16 at x0=3'] = checkerboard(H, W, 3, 5, 16)
    m['L'] = blank(); m['L'][8:50, 25:30] = True; m['L'][45:50, 25:39] = True
    m['full frame'] = np.ones((H, W), bool)
    rng = np.random.default_rng(31)
    for k, (h, w, x0, y0) in enumerate(((33, 21, 17, 2), (9, 37, 1, 50), (40, 40, 0, 24), (17, 12, 26, 11))):
        m[f'blob {k}'] = blank(); m[f'blob {k}'][y0:y0 + h, x0:x0 + w] = blob(h, w, rng)
    return m


def hand_masks():
    """name -> bool: the small cases whose rows are counted by hand (tests/test_nucshape_host.py)."""
    m = {'pixel': np.zeros((5, 7), bool), 'solid 8x8': np.zeros((12, 20), bool), 'solid 5x3': np.zeros((9, 9), bool)}
    m['pixel'][3, 4] = True
    m['solid 8x8'][2:10, 5:13] = True
    m['solid 5x3'][4:7, 2:7] = True                                                                  # 5 wide, 3 tall
    m['checkerboard 16x16'] = checkerboard(20, 24, 3, 2, 16)
    return m


def golden_blobs(n=40, seed=87):
    """list of n bool masks, random blobs of 3 .. 60 pixels a side each in a frame with a margin (the skimage fixture)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        h, w = (int(v) for v in rng.integers(3, 61, 2))
        m = np.zeros((h + 3, w + 5), bool)
        m[1:1 + h, 2:2 + w] = blob(h, w, rng)
        out.append(m)
    return out


def holed_ellipse(side, x0=33):
    """bool (side, side): an ellipse with an elliptic hole whose rectangle starts at x0 and spans the rest of the frame (all its rows)."""
    yy, xx = np.mgrid[0:side, 0:side]
    cx, cy, a, b = (x0 + side - 1) / 2.0, (side - 1) / 2.0, (side - x0) / 2.0, side / 2.0
    d = ((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2
    m = (d <= 1.0) & (d > 0.16)
    m[side // 2, x0] = m[side // 2, side - 1] = m[0, int(cx)] = m[side - 1, int(cx)] = True
    return m


def loops(mask):
    """The row of nuhtc_amd/nucshape.py in plain Python loops on a list-of-lists mask: the sums pixel by pixel, the boxes position by
    position.  -> list of 24 ints."""
    H, W = len(mask), len(mask[0])
    pts = [(x, y) for y in range(H) for x in range(W) if mask[y][x]]
    if not pts:
        return [0] * 24
    x0, y0 = min(x for x, _ in pts), min(y for _, y in pts)
    x1, y1 = max(x for x, _ in pts) + 1, max(y for _, y in pts) + 1
    row = [len(pts), x0, y0, x1, y1]
    for px, py in ((1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3)):
        row.append(sum(x ** px * y ** py for x, y in pts))
    for j in range(1, 11):
        s = 1 << j
        n = 0
        for k in range((y1 - y0 + s - 1) // s):
            for i in range((x1 - x0 + s - 1) // s):
                got = 0
                for y in range(y0 + k * s, min(y0 + (k + 1) * s, y1)):        # a position outside the rectangle is unset
                    for x in range(x0 + i * s, min(x0 + (i + 1) * s, x1)):
                        got += 1 if mask[y][x] else 0
                n += 1 if 0 < got < s * s else 0
        row.append(n)
    return row
