"""Designed inputs shared by tests/test_tissue_int.py (host) and tests/test_hip_tissue.py (device): contours and the points that probe the
edge rules of pointPolygonTest, and level images for the tissue mask."""
import numpy as np

from nuhtc_amd import tissue as T

CHUNK = 1024                      # PIP_CHUNK of csrc/tissue.hip: vertices staged through LDS at a time
BIG = 1 << 18
FILTER = dict(a_t=20, a_h=4, max_n_holes=8)          # area filters that the blobs and the hole of blob_slide pass and its speck fails


def chain(n, seed=0):
    """A closed ring of exactly n integer vertices: a wobbling circle, radius ~3000."""
    th = 2 * np.pi * np.arange(n) / n
    r = 3000 * (1 + 0.3 * np.sin(7 * th + seed) + 0.05 * np.sin(41 * th))
    return np.stack([np.rint(r * np.cos(th)) + 5000, np.rint(r * np.sin(th)) + 4000], 1).astype(np.int64)


def pixel_chain():
    """Unit-step border of a blob with long horizontal runs (what find_contours_ccomp hands to the grid)."""
    m = np.zeros((40, 120), bool)
    m[5:30, 10:100] = True
    m[30:36, 40:60] = True
    m[2:5, 20:25] = True
    m[12:20, 100:110] = True
    return T._trace_all(m)


def small_contours():
    """name -> (n, 2) int64; even coordinates, so every edge midpoint is a lattice point."""
    return {
        'one': np.array([[4, 6]]),
        'two': np.array([[2, 2], [10, 6]]),
        'three': np.array([[0, 0], [12, 2], [4, 10]]),
        'square': np.array([[0, 0], [8, 0], [8, 6], [0, 6]]),
        'concave_u': np.array([[0, 0], [4, 0], [4, 8], [8, 8], [8, 0], [12, 0], [12, 12], [0, 12]]),
        'repeated': np.array([[0, 0], [0, 0], [10, 0], [10, 0], [10, 0], [10, 8], [4, 8], [4, 8], [0, 8]]),
        'pixel_chain': pixel_chain() * 2,
    }


def large_contours():
    sizes = [63, 64, 65, 1023, 1024, 1025, CHUNK - 1, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, 4097, 10000]
    out = {f'chain{n}': chain(n, n % 5) for n in sorted(set(sizes))}
    out['big_triangle'] = np.array([[0, 0], [200000, 1], [3, 180000]]) + BIG          # products beyond 2^31
    return out


def probe_points(contour, max_vertices=200, n_random=300, seed=0):
    """Every vertex (a spread subset of a long chain, the ones at the LDS chunk seams always included), every edge midpoint, the point one edge
    length past each edge on its line, points sharing y with a vertex, the 8 neighbours of each vertex, and random points."""
    c = np.asarray(contour, np.int64).reshape(-1, 2)
    n = len(c)
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    if n > max_vertices:
        seams = np.concatenate([np.arange(s - 2, s + 3) for s in range(0, n + 1, CHUNK)] + [np.arange(n - 3, n)])
        idx = np.unique(np.concatenate([np.linspace(0, n - 1, max_vertices).astype(np.int64), seams[(seams >= 0) & (seams < n)]]))
    a, b = c[idx], c[(idx + 1) % n]
    span = int(np.ptp(c, 0).max()) + 4
    lo, hi = c.min(0) - 3, c.max(0) + 4
    nb = np.array([(dx, dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if dx or dy])
    pts = [a, (a + b) // 2, b + (b - a), a - (b - a),
           np.stack([a[:, 0] - span, a[:, 1]], 1), np.stack([a[:, 0] + span, a[:, 1]], 1), np.stack([a[:, 0] - 1 - (idx % 7), a[:, 1]], 1),
           np.stack([(a[:, 0] + c[(idx * 5 + 3) % n][:, 0]) // 2, a[:, 1]], 1),
           (a[:, None, :] + nb[None]).reshape(-1, 2), rng.integers(lo, hi, (n_random, 2))]
    return np.concatenate(pts, 0).astype(np.int64)


# ----------------------------------------------------------------------------- level images
def noisy_tissue(H, W, seed=0):
    """Greyish pixels whose saturation straddles the default threshold of 8 in patches: every stage of the mask has work to do."""
    rng = np.random.default_rng(seed)
    v = rng.integers(40, 256, (H, W, 1))
    amp = np.kron(rng.integers(0, 4, (-(-H // 6), -(-W // 6))), np.ones((6, 6), np.int64))[:H, :W, None] * 12
    return np.clip(v - rng.integers(0, 1 + amp, (H, W, 3)), 0, 255).astype(np.uint8)


def image_kinds(H, W, seed=0):
    """name -> (H, W, C) uint8."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    tissue, glass = np.array([200, 120, 180], np.uint8), np.array([235, 235, 235], np.uint8)
    pick = lambda m: np.where(m[..., None], tissue, glass)
    border = np.ones((H, W), bool)
    border[H // 4:H - H // 4, W // 4:W - W // 4] = False
    border[H // 2, :] = True                                # a bar joins the frame: gaps of every width against the four borders
    bright = np.full((H, W, 3), 128, np.uint8)
    bright[H // 2, W // 2] = (255, 0, 0)
    four = np.concatenate([noisy_tissue(H, W, seed + 1), rng.integers(0, 256, (H, W, 1), dtype=np.uint8)], 2)
    return {
        'random': rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
        'noisy': noisy_tissue(H, W, seed),
        'constant': np.broadcast_to(tissue, (H, W, 3)).copy(),
        'grey': np.repeat(rng.integers(0, 256, (H, W, 1), dtype=np.uint8), 3, 2),
        'black': np.zeros((H, W, 3), np.uint8),
        'checker': pick((yy + xx) % 2 == 0),
        'one_bright': bright,
        'borders': pick(border),
        'four_channel': four,
    }


def host_planes(img, sthresh=8, sthresh_up=255, mthresh=7, close=4, use_otsu=False):
    """The stages of `segment_tissue` from the host functions, as tissue_mask_device(planes=True) returns them."""
    sat = T.saturation_u8(img)
    med = T.median_blur(sat, mthresh)
    thr = T.otsu_threshold(med) if use_otsu else sthresh
    binary = np.where(med > thr, np.uint8(min(sthresh_up, 255)), np.uint8(0))
    if close > 0:
        binary = T.morph_close(binary, close)
    return dict(binary=binary, sat=sat, med=med, hist=np.bincount(med.reshape(-1), minlength=256).astype(np.int64), thr=thr)


def blob_slide(H=2048, W=3072):
    """Level-0 slide with two tissue blobs, one with a hole, and a speck below the area filter (at scale 16: 128 x 192 level pixels)."""
    rng = np.random.default_rng(3)
    img = np.full((H, W, 3), 235, np.uint8)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    ell = lambda cy, cx, ry, rx: ((yy - cy * H) / (ry * H)) ** 2 + ((xx - cx * W) / (rx * W)) ** 2 <= 1
    blob1, hole = ell(0.39, 0.29, 0.30, 0.23), ell(0.37, 0.287, 0.12, 0.10)
    blob2, speck = ell(0.68, 0.765, 0.245, 0.18), ell(0.07, 0.91, 0.024, 0.016)
    img[(blob1 & ~hole) | blob2 | speck] = (200, 120, 180)
    img -= rng.integers(0, 6, img.shape, dtype=np.uint8)
    return img
