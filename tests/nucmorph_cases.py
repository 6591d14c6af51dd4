"""Designed masks and tiles of the morphometry tests (tests/test_nucmorph_host.py, tests/test_hip_nucmorph.py) and of the skimage fixture
(tools/dev/make_morph_golden.py -> tests/golden/nucmorph_skimage.npz).  numpy only: the fixture script runs under another interpreter."""
import numpy as np

H_SMALL, W_SMALL = 64, 40            # 40: the width is no multiple of 32
SIDE_BIG = 256


def small_masks():
    """name -> bool (64, 40)."""
    blank = lambda: np.zeros((H_SMALL, W_SMALL), bool)
    yy, xx = np.mgrid[0:H_SMALL, 0:W_SMALL]
    m = {}
    m['empty'] = blank()
    m['pixel'] = blank(); m['pixel'][17, 9] = True
    for name, (y, x) in {'corner top left': (0, 0), 'corner top right': (0, W_SMALL - 1), 'corner bottom left': (H_SMALL - 1, 0),
                         'corner bottom right': (H_SMALL - 1, W_SMALL - 1)}.items():
        m[name] = blank(); m[name][y, x] = True
    m['horizontal line'] = blank(); m['horizontal line'][20, 3:38] = True           # crosses the word boundary
    m['vertical line'] = blank(); m['vertical line'][5:50, 33] = True
    m['diagonal line'] = (yy - 10 == xx - 4) & (xx >= 4) & (xx < 36)                # 45 degrees, through x = 31 | 32
    m['disc r=7'] = (yy - 30) ** 2 + (xx - 29) ** 2 <= 7 ** 2                       # x 22 .. 36: both words
    ring = (yy - 32) ** 2 + (xx - 20) ** 2
    m['annulus'] = (ring <= 15 ** 2) & (ring > 8 ** 2)
    two = blank(); two[3:9, 2:7] = True; two[40:52, 21:38] = True; two[45, 30] = False
    m['two blobs'] = two                                                             # empty rows between them, a hole in the second
    m['checkerboard'] = (yy >= 8) & (yy < 16) & (xx >= 28) & (xx < 36) & ((yy + xx) % 2 == 0)
    ell = blank(); ell[10:40, 29:33] = True; ell[36:40, 29:39] = True
    m['L across x=31|32'] = ell
    frame = blank(); frame[0, :] = frame[-1, :] = True; frame[:, 0] = frame[:, -1] = True; frame[20:30, 10:30] = True
    m['touches four edges'] = frame
    return m


def big_masks():
    """name -> bool (256, 256)."""
    yy, xx = np.mgrid[0:SIDE_BIG, 0:SIDE_BIG]
    ring = (yy - 120) ** 2 + (xx - 131) ** 2
    return {'full frame': np.ones((SIDE_BIG, SIDE_BIG), bool), 'big annulus': (ring <= 100 ** 2) & (ring > 61 ** 2)}


def tiles(h, w, seed=0):
    """name -> uint8 (h, w, 3): uniform random, constant 0, constant 255, three distinct constant planes."""
    rng = np.random.default_rng(seed)
    planes = np.zeros((h, w, 3), np.uint8)
    planes[..., 0], planes[..., 1], planes[..., 2] = 40, 120, 210
    return {'random': rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 'zeros': np.zeros((h, w, 3), np.uint8),
            'full': np.full((h, w, 3), 255, np.uint8), 'planes': planes}


def all_masks():
    """name -> bool mask, the small ones then the big ones (the order of the fixture)."""
    out = dict(small_masks())
    out.update(big_masks())
    return out
