"""Designed masks shared by tests/test_rle_cases.py (host encoder, nuhtc_amd/cocomask.py) and tests/test_hip_rle.py (device encoder,
csrc/rle.hip).  Frames are H x W = 64 x 96, deliberately not square so that a transposition slip cannot cancel; the cases that need a
frame of 2^14 pixels (counts of 16 383 / 16 384, the checkerboard that exceeds the device's run capacity) are 128 x 128.  Every case is
named after what it guards."""
import functools

import numpy as np

H, W = 64, 96
BIG = 128                         # side of the second frame
RUN_CAP = 1024                    # default run_cap of nuhtc_rle_encode
FIRST_RUNS = (15, 16, 511, 512)   # leading zero runs at the 1 / 2 and 2 / 3 character boundaries (64 x 96 frame)
DELTAS = (-16, -17, 15, 16)       # fourth count minus second count: the sign-aware stop rule's boundaries
N_BLOBS = 200


def from_counts(counts, h, w):
    """Run lengths in column-major order (first run zeros; the last run is extended to the end of the frame) -> (h, w) uint8 mask."""
    flat = np.zeros(h * w, np.uint8)
    pos, v = 0, 0
    for k, c in enumerate(counts):
        end = h * w if k == len(counts) - 1 else pos + c
        flat[pos:end] = v
        pos, v = end, v ^ 1
    assert pos == h * w
    return flat.reshape(w, h).T.copy()


def blob(rng, h=H, w=W):
    """One wobbly ellipse of 5 to 40 px diameter inside the frame."""
    dy, dx = rng.uniform(5, 40, 2)
    cy, cx = rng.uniform(dy / 2 + 1, h - dy / 2 - 1), rng.uniform(dx / 2 + 1, w - dx / 2 - 1)
    rot, lobes, phase, amp = rng.uniform(0, np.pi), rng.integers(2, 7), rng.uniform(0, 2 * np.pi), rng.uniform(0, 0.25)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    u = (xx - cx) * np.cos(rot) + (yy - cy) * np.sin(rot)
    v = -(xx - cx) * np.sin(rot) + (yy - cy) * np.cos(rot)
    th = np.arctan2(v, u)
    r = np.sqrt((2 * u / dx) ** 2 + (2 * v / dy) ** 2)
    m = r <= 1 + amp * np.sin(lobes * th + phase)
    m[int(round(cy)), int(round(cx))] = True          # never empty
    return m.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (H, W) uint8 mask, in a fixed order."""
    z = lambda h=H, w=W: np.zeros((h, w), np.uint8)
    c = {}
    c['empty'] = z()
    c['full'] = z() + 1
    for name, (y, x) in dict(pixel_first=(0, 0), pixel_last=(H - 1, W - 1), pixel_mid=(H // 2 + 3, W // 2 - 5)).items():
        c[name] = z()
        c[name][y, x] = 1
    c['bar_crossing'] = z()                  # bottom of column 40 into the top of column 41: ONE run (the rleToBbox quirk)
    c['bar_crossing'][H - 4:, 40] = 1
    c['bar_crossing'][:4, 41] = 1
    c['bar_gap'] = z()                       # the same with the last row clear: two runs
    c['bar_gap'][H - 5:H - 1, 40] = 1
    c['bar_gap'][:4, 41] = 1
    c['word_seam_pixels'] = z()
    for y, x in ((10, 31), (11, 32), (12, 63), (13, 64)):
        c['word_seam_pixels'][y, x] = 1
    c['word_seam_row'] = z()
    c['word_seam_row'][5, 30:66] = 1
    yy, xx = np.mgrid[0:H, 0:W]
    c['wider_than_a_wave'] = (((yy - 30) / 22.0) ** 2 + ((xx - 47) / 43.0) ** 2 <= 1).astype(np.uint8)          # columns 4 .. 90
    c['bottom_row_to_last_column'] = z()     # set pixels in the last row and the last column: the frame's end closes a run
    c['bottom_row_to_last_column'][H - 1, 70:] = 1
    c['bottom_row_to_last_column'][H - 9:, W - 1] = 1
    for L in FIRST_RUNS:
        c[f'first_run_{L}'] = from_counts([L, 3, 0], H, W)
    for d in DELTAS:
        c[f'delta_{d:+d}'] = from_counts([7, 40, 9, 40 + d, 11, 5, 0], H, W)
    rng = np.random.default_rng(0)
    for k in range(N_BLOBS):
        c[f'blob_{k:03d}'] = blob(rng)
    # ---- 128 x 128
    c['big_empty_16384'] = z(BIG, BIG)                           # the single count 16 384: 4 characters
    c['big_pixel_last_16383'] = z(BIG, BIG)                      # counts [16 383, 1]: 3 characters + 1
    c['big_pixel_last_16383'][BIG - 1, BIG - 1] = 1
    c['big_checkerboard'] = z(BIG, BIG)                          # a 64 x 64 checkerboard: 4096 runs, over the device's run capacity
    by, bx = np.mgrid[0:64, 0:64]
    c['big_checkerboard'][32:96, 32:96] = (by + bx) & 1
    return c


def pack(masks):
    """[(H, W) masks of one frame size] -> uint32 (n, H * W // 32): rows of W // 32 words, pixel x in bit x & 31 of word x >> 5."""
    m = np.stack([np.asarray(a, np.uint8) for a in masks])
    n, h, w = m.shape
    return np.packbits(m.reshape(n, h, w // 8, 8), axis=-1, bitorder='little').reshape(n, h * w // 32, 4).view(np.uint32).reshape(n, h * w // 32)


def frames():
    """(H, W) -> [names] of the cases of that frame size, in case order."""
    out = {}
    for name, m in cases().items():
        out.setdefault(m.shape, []).append(name)
    return out


@functools.lru_cache(maxsize=None)
def expected():
    """name -> (counts string as bytes, [x, y, w, h] ints, number of counts) by the host encoder; computed once, shared."""
    from nuhtc_amd import cocomask
    out = {}
    for name, m in cases().items():
        r = cocomask.encode(m)
        out[name] = (r['counts'].encode('ascii'), [int(v) for v in cocomask.to_bbox(r)], len(cocomask.string_to_counts(r['counts'])))
    return out
