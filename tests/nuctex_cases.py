"""Designed masks and tiles of the texture tests (tests/test_nuctex_host.py, tests/test_hip_nuctex.py) and of the skimage fixture
(tools/dev/make_texture_golden.py -> tests/golden/nuctex_skimage.npz), on top of tests/nucmorph_cases.py.  numpy only: the fixture script
runs under another interpreter."""
import numpy as np

import nucmorph_cases as base

H_SMALL, W_SMALL = base.H_SMALL, base.W_SMALL


def pair_masks():
    """name -> bool (64, 40): the smallest masks that hold a pair, where a pair can be lost, and the whole frame."""
    blank = lambda: np.zeros((H_SMALL, W_SMALL), bool)
    m = {}
    m['1x2 pair'] = blank(); m['1x2 pair'][12, 5:7] = True
    m['2x1 pair'] = blank(); m['2x1 pair'][12:14, 5] = True
    m['pair across x=31|32'] = blank(); m['pair across x=31|32'][40, 31:33] = True
    m['pair in the last row'] = blank(); m['pair in the last row'][H_SMALL - 1, 17:19] = True
    m['pair in the last column'] = blank(); m['pair in the last column'][30:32, W_SMALL - 1] = True
    m['2x2 in the last corner'] = blank(); m['2x2 in the last corner'][H_SMALL - 2:, W_SMALL - 2:] = True
    m['full frame'] = np.ones((H_SMALL, W_SMALL), bool)
    return m


def small_masks():
    """name -> bool (64, 40): the morphometry's designed masks, then the pair masks."""
    out = dict(base.small_masks())
    out.update(pair_masks())
    return out


def ramp(h, w):
    """uint8 (h, w, 3): R = 255 - 3y - x, G = 255 - 2y - 3x, B = 255 - y - 2x, clipped -- a smooth tile whose neighbouring pixels lie
    in the same or in adjacent grey levels."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(np.stack([255 - 3 * yy - xx, 255 - 2 * yy - 3 * xx, 255 - yy - 2 * xx], -1), 0, 255).astype(np.uint8)


def tiles(h, w, seed=0):
    """name -> uint8 (h, w, 3): random, zeros, full, planes (tests/nucmorph_cases.py) and the ramp."""
    out = dict(base.tiles(h, w, seed))
    out['ramp'] = ramp(h, w)
    return out


GOLDEN_TILES = ('random', 'ramp')     # the tiles of the skimage fixture (the constant ones hold one cell)
