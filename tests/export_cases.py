"""Designed inputs and plain numpy references shared by tests/test_export_cases.py (checked on the CPU) and tests/test_hip_export.py (the
device side: nuhtc_export_kept, nuhtc_export_crops and nuhtc_mask_contours of csrc/contour.hip).  numpy only: nothing here needs torch
or a GPU.  Frames are 64 x 96 (192 words per mask: the 16-byte copy of export_copy_kernel) and 65 x 96 (195 words: its dword copy), never
square, so that a transposition slip cannot cancel.  Every case is named after what it guards.

Output buffers start filled with one byte value, `mark`, whatever their element type: a reference returns the whole buffer, so a
comparison for equality also proves that nothing else was written."""
import functools

import numpy as np

FRAMES = ((64, 96), (65, 96))
MARK = 0xA5                        # the byte every output buffer is filled with before a call
CCAP = 70                          # contour capacity of the designed detection sets: more than one wave of vertices
# engine geometries of the device tests: frame, max_batch, max_per_img.  The scan kernels cut B * K rows into ceil(B * K / 1024) per
# thread: 800 rows is one per thread with idle threads, 1203 is two per thread, one for thread 601 and none for the 422 threads past the end.
GEOMETRY = {
    'small64': dict(frame=(64, 96), max_batch=4, K=200),
    'big65': dict(frame=(65, 96), max_batch=3, K=401),
    'big64': dict(frame=(64, 96), max_batch=3, K=401),
}
PATTERNS = ('none', 'all', 'alternating', 'last_only', 'beyond_counts', 'empty_tile_between', 'counts_full', 'past_B')
CONTOUR_N = (CCAP, 1, 0, -1, CCAP + 3, 5, 64, 65)      # cycled over the slots: full, one, none, overflow, past the capacity, the wave seam
X_RANGES = ((31, 33), (1, 33), (0, 33), (64, 96), (95, 96))
N_BLOBS = 12


# ----------------------------------------------------------------------------- layout
def marked(shape, dtype, mark=MARK):
    """A buffer of `shape` / `dtype` whose every byte is `mark`."""
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, mark, np.uint8).view(dtype).reshape(shape)


def pack(masks):
    """(n, H, W) masks (W % 32 == 0) -> uint32 (n, H * W // 32): rows of W // 32 words, pixel x in bit x & 31 of word x >> 5."""
    m = np.asarray(masks).astype(bool)
    n, h, w = m.shape
    assert w % 32 == 0
    out = np.zeros((n, h, w // 32), np.uint32)
    for x in range(w):
        out[:, :, x >> 5] |= m[:, :, x].astype(np.uint32) << np.uint32(x & 31)
    return out.reshape(n, h * w // 32)


def unpack(words, H, W):
    """uint32 (n, H * W // 32) -> bool (n, H, W); the inverse of pack."""
    w = np.asarray(words, np.uint32).reshape(-1, H, W // 32)
    x = np.arange(W)
    return ((w[:, :, x >> 5] >> (x & 31).astype(np.uint32)) & 1).astype(bool)


# ----------------------------------------------------------------------------- nuhtc_export_kept
def reference_export(boxes, labels, counts, keep, masks_words, contour_n, contour_xy, B, K, cap, ccap, mark=MARK):
    """What nuhtc_export_kept leaves in its seven output buffers, each `cap` rows that held `mark` bytes: the slots r < counts[b] with
    keep set of the tiles b < B, in (tile, slot) order, the first `cap` of them.  boxes: (., 5) of any 4-byte type, compared and returned
    as int32 bit patterns.  contour_n / contour_xy may be None: cn = 0 then, and xy is written only when contour_xy is given (ccap
    vertices per row without contour_n).  n = [true number of kept slots, 0 (the capacity flag of an inference that did not overflow)]."""
    bits = np.ascontiguousarray(boxes).view(np.int32).reshape(-1, 5)
    words = np.asarray(masks_words, np.uint32)
    out = dict(n=np.zeros(2, np.int32), idx=marked(cap, np.int64, mark), boxes=marked((cap, 5), np.int32, mark), labels=marked(cap, np.int32, mark),
               cn=marked(cap, np.int32, mark), xy=marked((cap, ccap, 2), np.int16, mark), words=marked((cap, words.shape[1]), np.uint32, mark))
    d = 0
    for b in range(B):
        for r in range(K):
            i = b * K + r
            if not (r < counts[b] and keep[i]):
                continue
            if d < cap:
                out['idx'][d], out['boxes'][d], out['labels'][d], out['words'][d] = i, bits[i], labels[i], words[i]
                out['cn'][d] = contour_n[i] if contour_n is not None else 0
                if contour_xy is not None:
                    nv = min(max(int(contour_n[i]), 0), ccap) if contour_n is not None else ccap
                    out['xy'][d, :nv] = contour_xy[i, :nv]
            d += 1
    out['n'][0] = d
    return out


def _special_boxes(n, rng):
    """float32 (n, 5) as int32 bit patterns: random finite values with -0.0, both infinities, a quiet and a signalling NaN payload and a
    denormal spread through them -- a copy that goes through arithmetic would change some of them."""
    a = rng.uniform(-300, 300, (n, 5)).astype(np.float32).view(np.int32)
    special = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0x7F812345, 0x00000001, 0xFFC00001], np.uint32).view(np.int32)
    flat = a.reshape(-1)
    flat[::11] = special[np.arange(len(flat[::11])) % len(special)]
    return a


@functools.lru_cache(maxsize=None)
def detection_set(geometry, pattern, masks='noise'):
    """One designed input of nuhtc_export_kept for an engine geometry: dict of boxes (int32 bit patterns of float32, (B_max * K, 5)), labels,
    counts (B_max), keep (uint8), masks_words (every slot different: `noise` = random words, `designed` = the crop masks of the frame in
    turn), contour_n, contour_xy (B_max * K, CCAP, 2), B (tiles the call names), K, frame.  Every slot of every tile is filled, also those
    past counts[b] and past B, so a row copied from a slot that should have been ignored differs from every expected row."""
    g = GEOMETRY[geometry]
    (H, W), Bm, K = g['frame'], g['max_batch'], g['K']
    rng = np.random.default_rng(sorted(GEOMETRY).index(geometry) * 100 + PATTERNS.index(pattern))
    total = Bm * K
    B = Bm
    counts = rng.integers(K // 3, K, Bm).astype(np.int32)           # partial tiles unless the pattern says otherwise
    keep = (rng.random(total) < 0.4).astype(np.uint8)
    if pattern == 'none':
        keep[:] = 0
    elif pattern == 'all':
        keep[:] = 1
    elif pattern == 'alternating':
        keep[:] = np.arange(total) & 1
    elif pattern == 'last_only':                                      # the scan's last row, written by the last thread that has rows
        counts[:] = K
        keep[:] = 0
        keep[total - 1] = 1
    elif pattern == 'beyond_counts':                                  # keep set in every slot: those at r >= counts[b] must not count
        keep[:] = 1
    elif pattern == 'empty_tile_between':
        counts[1] = 0
        keep[K:2 * K] = 1                                             # ... although its slots say keep
    elif pattern == 'counts_full':
        counts[:] = K
    elif pattern == 'past_B':                                         # the call names fewer tiles than the buffers hold
        B = Bm - 2
        keep[B * K:] = 1
        counts[B:] = K
    if masks == 'noise':
        words = rng.integers(0, 1 << 32, (total, H * W // 32), dtype=np.uint64).astype(np.uint32)
    else:
        base = pack(np.stack(list(crop_cases(H, W).values())))
        words = base[(np.arange(total) * 5 + 3) % len(base)]          # 5 is coprime to the number of cases: neighbours differ
    return dict(boxes=_special_boxes(total, rng), labels=rng.integers(0, 5, total).astype(np.int32), counts=counts, keep=keep, masks_words=words,
                contour_n=np.array(CONTOUR_N, np.int32)[(np.arange(total) + 3 * (np.arange(total) // K)) % len(CONTOUR_N)],
                contour_xy=rng.integers(-32768, 32768, (total, CCAP, 2)).astype(np.int16), B=B, K=K, frame=(H, W), max_batch=Bm)


def kept_slots(s):
    """Flat indices b * K + r the export of detection set `s` lists, in order."""
    K = s['K']
    i = np.arange(s['B'] * K)
    return i[(i % K < s['counts'][i // K]) & (s['keep'][:s['B'] * K] != 0)]


# ----------------------------------------------------------------------------- nuhtc_export_crops
def reference_crops(masks_bool, n, cap, pool_cap, pool_len, mark=MARK):
    """What nuhtc_export_crops leaves behind for the first `cap` masks of masks_bool (cap, H, W) with *n_dev = n: box (cap, 4) = x0, y0,
    x1, y1 (exclusive) of the set pixels, area (cap), off (cap + 1) = exclusive scan of the crop sizes in words with the total need in
    off[cap], pool (pool_len uint32 that held `mark` bytes) = each crop as rows of ceil(w / 32) words, column x - x0 in bit (x - x0) & 31.
    Rows >= min(n, cap) are zero in box and area and take no words; an empty mask likewise.  A crop with off + size > pool_cap is not
    written.  Also `written` (cap) bool: non-empty crops that went into the pool."""
    m = np.asarray(masks_bool).astype(bool)
    box, area, off = np.zeros((cap, 4), np.int32), np.zeros(cap, np.int32), np.zeros(cap + 1, np.int32)
    pool, written = marked(pool_len, np.uint32, mark), np.zeros(cap, bool)
    crops = [None] * cap
    for d in range(min(n, cap)):
        ys, xs = np.nonzero(m[d])
        if len(ys):
            x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1
            box[d], area[d] = (x0, y0, x1, y1), len(ys)
            c = m[d, y0:y1, x0:x1]
            cw = (x1 - x0 + 31) // 32
            padded = np.zeros((y1 - y0, cw * 32), bool)
            padded[:, :x1 - x0] = c
            crops[d] = pack(padded[None])[0]
    sizes = np.array([0 if c is None else len(c) for c in crops], np.int64)
    off[1:] = np.cumsum(sizes)
    for d, c in enumerate(crops):
        if c is not None and off[d] + len(c) <= pool_cap:
            pool[off[d]:off[d] + len(c)] = c
            written[d] = True
    return dict(box=box, area=area, off=off, pool=pool, written=written)


def _blob(rng, h, w):
    """One wobbly ellipse of 4 to 40 px diameter inside the frame."""
    dy, dx = rng.uniform(4, 40, 2)
    cy, cx = rng.uniform(dy / 2 + 1, h - dy / 2 - 1), rng.uniform(dx / 2 + 1, w - dx / 2 - 1)
    rot, lobes, phase, amp = rng.uniform(0, np.pi), rng.integers(2, 7), rng.uniform(0, 2 * np.pi), rng.uniform(0, 0.25)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    u = (xx - cx) * np.cos(rot) + (yy - cy) * np.sin(rot)
    v = -(xx - cx) * np.sin(rot) + (yy - cy) * np.cos(rot)
    m = np.sqrt((2 * u / dx) ** 2 + (2 * v / dy) ** 2) <= 1 + amp * np.sin(lobes * np.arctan2(v, u) + phase)
    m[int(round(cy)), int(round(cx))] = True          # never empty
    return m


@functools.lru_cache(maxsize=None)
def crop_cases(H, W):
    """name -> (H, W) bool mask, in a fixed order that matters: the masks lie one after the other in the words buffer, so the word after
    the last word of a mask's last row is the first word of the next mask.  `pixel_bottom_right` and `tail_bottom` (crops that end in the
    last word of the frame's last row, shifted) are each followed by a mask whose first word is set: a shift that reads one word too far
    picks up that mask's pixels."""
    z = lambda: np.zeros((H, W), bool)
    c = {}

    def put(name, ys, xs):
        c[name] = z()
        c[name][ys, xs] = True
    put('pixel_bottom_right', H - 1, W - 1)
    put('pixel_top_left', 0, 0)
    put('pixel_top_right', 0, W - 1)
    put('pixel_bottom_left', H - 1, 0)
    for x in (31, 32, 63, 64, 95):
        put(f'pixel_x{x}', 20 + x % 7, x)
    put('tail_bottom', slice(H - 6, H), slice(40, W))               # two words wide, shifted by 8, up to the frame's last word
    put('full_frame', slice(None), slice(None))
    put('full_row', 17, slice(None))
    put('full_column', slice(None), 45)
    for x0, x1 in X_RANGES:
        put(f'x{x0}_{x1}', slice(9, 20), slice(x0, x1))
        c[f'x{x0}_{x1}'][10:19:2, x0 + (x1 - x0) // 2] = False     # not a solid block: every row of the crop has its own pattern
    c['two_blobs'] = z()                                            # the box is the box of the union
    c['two_blobs'][3:8, 2:9] = True
    c['two_blobs'][H - 9:H - 2, 70:93] = True
    put('empty_first', [], [])
    put('one_row', 40, slice(33, 70))
    put('empty', [], [])                                            # strictly between two non-empty masks
    put('one_column', slice(5, 50), 64)
    rng = np.random.default_rng(11)
    for k in range(N_BLOBS):
        c[f'blob_{k:02d}'] = _blob(rng, H, W)
    put('last_row', H - 1, slice(30, 67))
    c['noise'] = rng.random((H, W)) < 0.5
    put('empty_last', [], [])
    return c


def crop_words_per_mask(m):
    """Words the crop of one mask takes."""
    ys, xs = np.nonzero(m)
    return 0 if not len(ys) else int(ys.max() + 1 - ys.min()) * ((int(xs.max() + 1 - xs.min()) + 31) // 32)


# ----------------------------------------------------------------------------- nuhtc_mask_contours at 65 x 96
def _box_blur(a, rounds):
    for _ in range(rounds):
        p = np.pad(a, 1, mode='edge')
        a = sum(p[dy:dy + a.shape[0], dx:dx + a.shape[1]] for dy in range(3) for dx in range(3)) / 9.0
    return a


@functools.lru_cache(maxsize=None)
def contour_shapes(H=65, W=96):
    """name -> (H, W) bool mask for the contour kernel at a frame with three words per row and H != W."""
    z = lambda: np.zeros((H, W), bool)
    c = {}
    c['seam_31_32'] = z(); c['seam_31_32'][10:30, 25:40] = True
    c['seam_63_64'] = z(); c['seam_63_64'][12:20, 60:70] = True; c['seam_63_64'][20:26, 63:65] = True
    c['touches_right_and_bottom'] = z(); c['touches_right_and_bottom'][H - 8:H, W - 12:W] = True
    c['right_edge_blob_and_bottom_edge_blob'] = z()
    c['right_edge_blob_and_bottom_edge_blob'][5:15, 90:W] = True
    c['right_edge_blob_and_bottom_edge_blob'][H - 4:H, 10:50] = True
    c['last_word_column_only'] = z(); c['last_word_column_only'][20:45, 66:94] = True; c['last_word_column_only'][30:35, 75:80] = False
    c['hole_across_seam'] = z(); c['hole_across_seam'][8:40, 20:50] = True; c['hole_across_seam'][15:30, 28:36] = False
    m = z(); m[5:45, 5:60] = True; m[10:40, 10:55] = False; m[20:30, 28:36] = True          # island in a hole, across the 31|32 seam
    c['island_in_hole'] = m
    m = m.copy(); m[50:60, 70:90] = True                                                    # ... plus a later top-level blob in the last word column
    c['island_in_hole_and_later_blob'] = m
    m = z()                                       # one pixel wide: every second row, joined at alternating ends
    m[0::2, :] = True
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = True
    c['serpentine'] = m
    rng = np.random.default_rng(23)
    for k in range(10):
        a = _box_blur(rng.standard_normal((H, W)), int(rng.integers(2, 6)))
        m = a > np.quantile(a, rng.uniform(0.6, 0.9))
        if k % 3 == 0:
            m &= ~(_box_blur(rng.standard_normal((H, W)), 1) > 0.25)
        c[f'fragments_{k}'] = m
    return c
