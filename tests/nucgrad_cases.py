"""Designed masks and tiles of the gradient tests (tests/test_nucgrad_host.py, tests/test_hip_nucgrad.py), on top of tests/nuctex_cases.py
and tests/nucmorph_cases.py.  numpy only."""
import numpy as np

import nuctex_cases as tex

H_SMALL, W_SMALL = tex.H_SMALL, tex.W_SMALL


def edge_masks():
    """name -> bool (64, 40): masks along each edge of the frame and in each corner (where a difference is one-sided and a neighbour of
    the edge test lies outside the frame), and single pixels on both sides of the word boundary."""
    blank = lambda: np.zeros((H_SMALL, W_SMALL), bool)
    m = {}
    m['top edge'] = blank(); m['top edge'][0:3, 4:37] = True
    m['bottom edge'] = blank(); m['bottom edge'][H_SMALL - 3:, 4:37] = True
    m['left edge'] = blank(); m['left edge'][7:50, 0:3] = True
    m['right edge'] = blank(); m['right edge'][7:50, W_SMALL - 3:] = True
    for name, (ys, xs) in {'block top left': (slice(0, 5), slice(0, 5)), 'block top right': (slice(0, 5), slice(W_SMALL - 5, W_SMALL)),
                           'block bottom left': (slice(H_SMALL - 5, H_SMALL), slice(0, 5)),
                           'block bottom right': (slice(H_SMALL - 5, H_SMALL), slice(W_SMALL - 5, W_SMALL))}.items():
        m[name] = blank(); m[name][ys, xs] = True
    m['pixel at x=31'] = blank(); m['pixel at x=31'][33, 31] = True
    m['pixel at x=32'] = blank(); m['pixel at x=32'][33, 32] = True
    return m


def small_masks():
    """name -> bool (64, 40): the texture's masks (the morphometry's among them), then the edge masks."""
    out = dict(tex.small_masks())
    out.update(edge_masks())
    return out


def step(h, w, vertical=True):
    """uint8 (h, w, 3): white left of x = w // 2 (above y = h // 2), black from there -- one step edge of 255 haematoxylin levels."""
    t = np.full((h, w, 3), 255, np.uint8)
    if vertical:
        t[:, w // 2:] = 0
    else:
        t[h // 2:] = 0
    return t


RIDGE_X = 12                         # the ridge's two plateau columns are RIDGE_X + 1 and RIDGE_X + 2 (needs w >= RIDGE_X + 5)


def ridge_greys():
    """-> (greys (4,), k): four grey values whose haematoxylin values are 0, k, 2k, 3k with the largest such k."""
    from nuhtc_amd import nucmorph
    g = np.arange(256, dtype=np.uint8)
    hg = nucmorph.haematoxylin(np.stack([g, g, g], -1))
    first = {}
    for v in range(255, -1, -1):
        first.setdefault(int(hg[v]), v)
    k = max(k for k in range(1, 86) if all(j * k in first for j in range(4)))
    return np.array([first[j * k] for j in range(4)], np.uint8), k


def ridge(h, w):
    """uint8 (h, w, 3): grey columns whose haematoxylin values rise 0, 0, k, 2k, 3k, 3k from x = RIDGE_X - 1 on: the doubled gradient is
    k, 2k, 2k, k over the columns RIDGE_X .. RIDGE_X + 3 -- a ridge of the magnitude with a plateau two pixels wide, of which the tie
    rule counts the first column only."""
    g, _ = ridge_greys()
    v = np.full(w, g[0], np.uint8)
    v[RIDGE_X + 1], v[RIDGE_X + 2] = g[1], g[2]
    v[RIDGE_X + 3:] = g[3]
    return np.repeat(np.repeat(v[None, :, None], h, 0), 3, 2)


def checker(h, w):
    """uint8 (h, w, 3): a black and white checkerboard -- the corner pixels hold the largest magnitude, m = 1442."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, 2)


def columns(h, w):
    """uint8 (h, w, 3): alternating black and white columns."""
    return np.repeat(np.repeat(((np.arange(w) & 1) * 255).astype(np.uint8)[None, :, None], h, 0), 3, 2)


def tiles(h, w, seed=0):
    """name -> uint8 (h, w, 3): random, zeros, full, planes, ramp (tests/nuctex_cases.py), a vertical and a horizontal step, the ridge and
    the checkerboard."""
    out = dict(tex.tiles(h, w, seed))
    out['vertical step'] = step(h, w, True)
    out['horizontal step'] = step(h, w, False)
    out['ridge'] = ridge(h, w)
    out['checker'] = checker(h, w)
    return out


GPU_TILES = ('random', 'planes', 'ramp', 'vertical step', 'ridge')      # the five tiles of the device test (the others: host only)


def loops(h, mask, T=1):
    """The row of nuhtc_amd/nucgrad.py in plain Python loops on a list-of-lists h (H x W ints) and mask: the doubled gradient case by
    case, math.isqrt, the sector rule and the bins written out.  -> list of 18 ints."""
    import math
    H, W = len(h), len(h[0])

    def g2(x, y):
        if W == 1:
            gx = 0
        elif x == 0:
            gx = 2 * (h[y][1] - h[y][0])
        elif x == W - 1:
            gx = 2 * (h[y][W - 1] - h[y][W - 2])
        else:
            gx = h[y][x + 1] - h[y][x - 1]
        if H == 1:
            gy = 0
        elif y == 0:
            gy = 2 * (h[1][x] - h[0][x])
        elif y == H - 1:
            gy = 2 * (h[H - 1][x] - h[H - 2][x])
        else:
            gy = h[y + 1][x] - h[y - 1][x]
        return gx, gy

    def q(x, y):
        if x < 0 or x >= W or y < 0 or y >= H:
            return 0
        gx, gy = g2(x, y)
        return gx * gx + gy * gy

    ms, edge = [], 0
    for y in range(H):
        for x in range(W):
            if not mask[y][x]:
                continue
            gx, gy = g2(x, y)
            qq = gx * gx + gy * gy
            m = math.isqrt(4 * qq)
            ms.append(m)
            if m < T:
                continue
            ax, ay = abs(gx), abs(gy)
            if ay * 32768 < ax * 13573:
                a, b = (x - 1, y), (x + 1, y)
            elif ay * 32768 > ax * 13573 + ax * 65536:
                a, b = (x, y - 1), (x, y + 1)
            elif gx * gy > 0:
                a, b = (x - 1, y - 1), (x + 1, y + 1)
            else:
                a, b = (x + 1, y - 1), (x - 1, y + 1)
            if qq > q(*a) and qq >= q(*b):
                edge += 1
    if not ms:
        return [0] * 18
    mn, mx = min(ms), max(ms)
    hist = [0] * 10
    for m in ms:
        hist[min((m - mn) * 10 // (mx - mn), 9) if mx > mn else 5] += 1
    return [len(ms), sum(ms), sum(m ** 2 for m in ms), sum(m ** 3 for m in ms), sum(m ** 4 for m in ms), mn, mx, edge] + hist
