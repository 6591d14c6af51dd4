"""The detection tail of the path, op by op, against float64 references on designed inputs: everything behind the RoI features in
run_roi_path (csrc/roi_engine.hip) that turns numbers into decisions -- bbox_tail_kernel, det_candidates_kernel, the class-offset
multiclass NMS (launch_nms with ids, csrc/proposals.hip), det_finish_kernel, paste_kernel and tile_post_kernel (csrc/roi.hip).

Engine.op_bbox_tail / op_det_post / op_paste / op_tile_post (nuhtc_op_*) fill the parameter blocks nuhtc_infer fills and call the same
launch functions (test_ops_are_the_engines_path shows it bit for bit), so these tests reach what four small synthetic tiles never do: the
second greedy pass of tile_post_kernel (more than 512 filtered candidates), the chunk carry of the candidate scan (more than 1024 RoIs on a
tile), ties and the class-major position in the sort key, degenerate / off-canvas / oversized paste boxes, the per-tile class offset of the
NMS, and every strict comparison on its edge.

The references are written here in float64 numpy and are cross-checked on the CPU against oracle.model / oracle.ops_np (the restatements
tests/test_oracle_*.py pin).  Nothing below was measured: every tolerance is derived where it is defined, or is the 1e-5 threshold band
tests/test_hip_full.py uses for pasted masks.

u = 2^-24 is the unit roundoff of fp32 (round to nearest); bounds are first order in u (n u << 1 for every n below)."""
import ctypes

import numpy as np
import pytest
import torch

U = 2.0 ** -24
MAX_RATIO = 4.135166556742356          # |log(16 / 1000)|, the dw / dh clamp of delta2bbox
SENTINEL = 0x7fc0dead                  # a quiet NaN with a payload: outputs that must not be written keep it bit for bit
SENT_U8 = 0xA5

# ---- bbox tail: |got - ref| <= TOL_TAIL * mag, mag = sum |x_i w_i| + |b| in fp64.
# cls_n = sum_i xn_i wn_i + b_n with xn = 20 h / (|h| + 1e-6), wn = W_n / (|W_n| + 1e-6).  Relative error of each factor, counted in u:
#   |h|^2: 1 (square) + 255 (any order of the 256-term sum) = 256;  sqrt halves it and rounds: 129;  + 1e-6f (the constant is within 1 u of
#   1e-6) and the add: 131;  h / den: 132;  * 20: 133                                                             -> xn_i: 133
#   the same chain for the weight row, packed on the host (sequential sum), without the * 20                       -> wn_i: 132
#   the product x w: 1;  the 256-term sum in any order: 255;  + b: 1                                               -> 257
# in all (256 + 266) u.  reg_n = sum_i h_i W_ni + b_n needs 257 u and is held to the same TOL.
TAIL_C = 266
TOL_TAIL = (256 + TAIL_C) * U
# delta2bbox in fp32 on exact inputs: |o - ref| <= BOX_C u (|x0| + |x2| + |pw dx| + gw (1 + |dw|)) per axis, from
#   pxc: 1 u |pxc|;  pw: 1 u |pw|;  dx = d std: 1;  pw dx: 3 u |pw dx|;  gx: 1 u |gx|;  expf(dw) with dw = d std rounded: (|dw| + 2) u (expf itself
#   within 2 u);  gw = pw exp: (|dw| + 4) u gw;  gx -+ gw / 2: 1 u |o|;  the clip is 1-Lipschitz;  / scale: 1 u |o|
# with |pxc| <= (|x0| + |x2|) / 2, |pw| <= |x0| + |x2|, |gx| <= |pxc| + |pw dx|, |o| <= |gx| + gw / 2 this is at most
# u (3 (|x0| + |x2|) + 6 |pw dx| + (3 + |dw| / 2) gw) <= 8 u (...).
BOX_C = 8
# ---- Seesaw score s_c = softmax(l[:nc])_c * softmax(l[nc:])_0 with l = ((c0 + c1) + c2) / 3 and |c_k| <= L_MAX:
#   l: absolute error (2 L + 3 L) / 3 u + L u <= 3 L u;  l_c - max: both operands carry that, the subtraction 2 L u: <= 8 L u
#   expf: 2 u of its own + the argument's absolute error: e_c within (8 L + 2) u;  the nc-term sum adds nc - 1;  e_c / sum: + 1
#   -> class factor (16 L + 4 + nc) u;  objectness factor e0 / (e0 + e1): (16 L + 6) u;  their product: + 1
# relative error of a score <= (32 L + nc + 11) u; scores are <= 1, so that is also the absolute margin around score_thr inside which a
# decision of the kernel may differ from the float64 reference.
L_MAX = 8.0
SEESAW_NC = 5
SCORE_REL = (32 * L_MAX + SEESAW_NC + 11) * U
SCORE_MARGIN = SCORE_REL
# the placed case: nc equal class logits and two equal objectness logits give (1 / nc) * 0.5 with every fp32 step exact but the one
# division 1 / 5, so the kernel's score IS float32(0.2) * 0.5; with score_thr set to that number `score > score_thr` must say no
PLACED_THR = float(np.float32(0.2) * np.float32(0.5))
PASTE_BAND = 1e-5                      # tests/test_hip_full.py: a pasted pixel may differ only where the sampled value is this close to the threshold
PASTE_BAND_SHARE = 1e-3                # at most 0.1 % of the hull pixels of a designed case may lie in that band

STDS = [(0.1, 0.1, 0.2, 0.2), (0.05, 0.05, 0.1, 0.1), (0.033, 0.033, 0.067, 0.067)]
OBSERVED = {}


def _obs(key, v):
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), float(v))


# ================================================================================================================ references (float64)
def ref_delta2bbox(rois4, d, stds, img_w, img_h):
    """delta2bbox (means 0) in float64 -> (boxes (R, 4), terms dict for the error bounds)."""
    rois4, d = np.asarray(rois4, np.float64), np.asarray(d, np.float64)
    s = np.asarray(stds, np.float64)
    dx, dy = d[:, 0] * s[0], d[:, 1] * s[1]
    dw, dh = np.clip(d[:, 2] * s[2], -MAX_RATIO, MAX_RATIO), np.clip(d[:, 3] * s[3], -MAX_RATIO, MAX_RATIO)
    pxc, pyc = (rois4[:, 0] + rois4[:, 2]) * 0.5, (rois4[:, 1] + rois4[:, 3]) * 0.5
    pw, ph = rois4[:, 2] - rois4[:, 0], rois4[:, 3] - rois4[:, 1]
    gx, gy = pxc + pw * dx, pyc + ph * dy
    gw, gh = pw * np.exp(dw), ph * np.exp(dh)
    o = np.stack([np.clip(gx - gw * 0.5, 0, img_w), np.clip(gy - gh * 0.5, 0, img_h), np.clip(gx + gw * 0.5, 0, img_w), np.clip(gy + gh * 0.5, 0, img_h)], 1)
    geom_x = np.abs(rois4[:, 0]) + np.abs(rois4[:, 2]) + np.abs(pw * dx) + np.abs(gw) * (1 + np.abs(dw))
    geom_y = np.abs(rois4[:, 1]) + np.abs(rois4[:, 3]) + np.abs(ph * dy) + np.abs(gh) * (1 + np.abs(dh))
    return o, dict(pw=pw, ph=ph, gw=gw, gh=gh, dw=d[:, 2] * s[2], dh=d[:, 3] * s[3], gx=gx, gy=gy, geom=np.stack([geom_x, geom_y, geom_x, geom_y], 1))


def ref_bbox_tail(h, cls_w, cls_b, reg_w, reg_b):
    """NormedLinear classifier and the regression rows in float64 -> cls, reg and their magnitudes sum |x_i w_i| + |b|."""
    h, cw, cb, rw, rb = (np.asarray(a, np.float64) for a in (h, cls_w, cls_b, reg_w, reg_b))
    with np.errstate(all='ignore'):
        xn = h / (np.sqrt((h * h).sum(1, keepdims=True)) + 1e-6) * 20.0
        wn = cw / (np.sqrt((cw * cw).sum(1, keepdims=True)) + 1e-6)
        cls = xn @ wn.T + cb
        mag_cls = np.abs(xn) @ np.abs(wn).T + np.abs(cb)
        reg = h @ rw.T + rb
        mag_reg = np.abs(h) @ np.abs(rw).T + np.abs(rb)
    return cls, reg, mag_cls, mag_reg


def refine_bound(rois4, reg, mag_reg, stds, img_w, img_h):
    """Bound of the refined RoI: the regression rows' error TOL_TAIL * mag_reg propagated through delta2bbox (dx linearly, dw through the
    exponential: gw (e^eps - 1), valid for any eps) plus delta2bbox's own fp32 error on exact deltas."""
    o, t = ref_delta2bbox(rois4, reg, stds, img_w, img_h)
    s = np.asarray(stds, np.float64)
    ed = TOL_TAIL * mag_reg
    with np.errstate(all='ignore'):
        bx = np.abs(t['pw']) * s[0] * ed[:, 0] + 0.5 * np.abs(t['gw']) * np.expm1(s[2] * ed[:, 2])
        by = np.abs(t['ph']) * s[1] * ed[:, 1] + 0.5 * np.abs(t['gh']) * np.expm1(s[3] * ed[:, 3])
    bound = np.stack([bx, by, bx, by], 1) + BOX_C * U * t['geom']
    return o, np.where(np.isfinite(bound), bound, np.inf), t


def ref_seesaw(c0, c1, c2, nc):
    """Mean of the three stages' logits and the Seesaw activation in float64 -> scores (R, nc)."""
    l = (np.asarray(c0, np.float64) + np.asarray(c1, np.float64) + np.asarray(c2, np.float64))[:, :nc + 2] / 3.0
    a = l[:, :nc] - l[:, :nc].max(1, keepdims=True)
    sc = np.exp(a) / np.exp(a).sum(1, keepdims=True)
    o = l[:, nc:] - l[:, nc:].max(1, keepdims=True)
    pos = np.exp(o[:, 0]) / np.exp(o).sum(1)
    return sc * pos[:, None]


def ref_paste(prob, boxes, H, W, vH, vW, thr):
    """Float64 bilinear sampling with zero padding (grid_sample, align_corners=False) of prob (D, 28, 28) at the pixel centres of the boxes'
    frames, inside the integer hull [floor(x0) - 1, ceil(x1) + 1) x [floor(y0) - 1, ceil(y1) + 1) clamped to the valid canvas vH x vW.
    A non-finite grid coordinate from a zero-size box becomes 0 when infinite and stays NaN otherwise (0 / 0), as in paste_masks.
    -> (mask (D, H, W) bool, values (D, H, W) float64, hull (D, H, W) bool)."""
    prob, boxes = np.asarray(prob, np.float64), np.asarray(boxes, np.float64)
    D = len(boxes)
    mask, vals, hull = np.zeros((D, H, W), bool), np.zeros((D, H, W)), np.zeros((D, H, W), bool)

    def axis(n, lo, hi):
        with np.errstate(all='ignore'):
            g = (np.arange(n) + 0.5 - lo) / (hi - lo) * 2.0 - 1.0
            g[np.isinf(g)] = 0.0
            i = ((g + 1.0) * 28.0 - 1.0) / 2.0
            f = np.floor(i)
        i0 = np.where(np.isnan(f), -9, f).astype(np.int64)
        return i0, i0 + 1, (f + 1.0) - i, i - f

    for d in range(D):
        x0, y0, x1, y1 = boxes[d]
        hx0, hy0 = max(int(np.floor(x0)) - 1, 0), max(int(np.floor(y0)) - 1, 0)
        hx1, hy1 = min(int(np.ceil(x1)) + 1, vW), min(int(np.ceil(y1)) + 1, vH)
        if hx1 > hx0 and hy1 > hy0:
            hull[d, hy0:hy1, hx0:hx1] = True
        ix0, ix1, wx0, wx1 = axis(W, x0, x1)
        iy0, iy1, wy0, wy1 = axis(H, y0, y1)
        v = np.zeros((H, W))
        nan = np.isnan(wx0)[None, :] | np.isnan(wy0)[:, None]
        with np.errstate(all='ignore'):
            for iy, wy in ((iy0, wy0), (iy1, wy1)):
                for ix, wx in ((ix0, wx0), (ix1, wx1)):
                    ok = ((iy >= 0) & (iy < 28))[:, None] & ((ix >= 0) & (ix < 28))[None, :]
                    p = prob[d][np.clip(iy, 0, 27)[:, None], np.clip(ix, 0, 27)[None, :]]
                    v = v + np.where(ok, p * (wx[None, :] * wy[:, None]), 0.0)
        v[nan] = np.nan
        vals[d] = v
        with np.errstate(invalid='ignore'):
            mask[d] = (v >= thr) & hull[d]
    return mask, vals, hull


def ref_tile_post(dets, labels, masks, vH, vW, margin, min_area, thr):
    """tools/infer_wsi.py:486-531 in the kernel's documented convention: detections in class-major order (stable), the margin / area filter,
    the order np.argsort(score, kind='stable')[::-1] (ties: the LATER class-major position first), greedy suppression at integer mask
    IoU > thr.  dets (n, 5), labels (n,), masks (n, H, W) bool -> (keep (n,) uint8 in the input order, filtered count)."""
    n = len(dets)
    keep = np.zeros(n, np.uint8)
    if n == 0:
        return keep, 0
    cm = np.argsort(labels, kind='stable')
    d, m = dets[cm], masks[cm].reshape(n, -1)
    area = m.sum(1)
    ok = (d[:, 0] >= margin) & (d[:, 1] >= margin) & (d[:, 2] <= vW - margin) & (d[:, 3] <= vH - margin) & (area >= min_area)
    idx = np.nonzero(ok)[0]
    if len(idx) == 0:
        return keep, 0
    order = idx[np.argsort(d[idx, 4], kind='stable')[::-1]]
    f = m[order].astype(np.float32)               # counts <= 2^24: the float32 product is exact
    inter = (f @ f.T).astype(np.int64)
    a = area[order].astype(np.int64)
    union = a[:, None] + a[None, :] - inter
    with np.errstate(all='ignore'):
        over = (union > 0) & (inter.astype(np.float64) / union.astype(np.float64) > thr)
    sup = np.zeros(len(order), bool)
    for i in range(len(order)):
        if sup[i]:
            continue
        keep[cm[order[i]]] = 1
        sup[i + 1:] |= over[i, i + 1:]
    return keep, len(idx)


def pack_masks(m):
    """(…, H, W) bool -> (…, H, W // 32) int32 words, bit x & 31 of word x >> 5."""
    b = np.packbits(np.asarray(m, bool), axis=-1, bitorder='little')
    return np.ascontiguousarray(b).view(np.uint32).view(np.int32)


def unpack_masks(words, W):
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint32)
    return np.unpackbits(w.view(np.uint8), axis=-1, bitorder='little').astype(bool)[..., :W]


# ================================================================================================================ designed inputs
H_CLASSES = ('ordinary', 'zero', 'large', 'small', 'eps-sized', 'dominant', 'nonfinite')


def tail_case(R, nc, refine, shift, cap=12):
    """Operands of one bbox-tail case: `cap` rows of which the first R are live; row i is of class H_CLASSES[(i + shift) % 7]."""
    rng = np.random.default_rng(1000 + 97 * R + 13 * nc + refine + 7 * shift)
    h = np.abs(rng.standard_normal((cap, 256))).astype(np.float32)           # the FCs end in a ReLU; signs come from the weights
    kinds = [H_CLASSES[(i + shift) % len(H_CLASSES)] for i in range(cap)]
    for i, k in enumerate(kinds):
        if k == 'zero':
            h[i] = 0.0                                                       # denominator 1e-6, cls = bias
        elif k == 'large':
            h[i] *= 1e15                                                     # squares ~1e30, their sum stays finite
        elif k == 'small':
            h[i] *= 1e-12                                                    # |h| far below the 1e-6 of the denominator, squares still normal
        elif k == 'eps-sized':
            h[i] *= 6e-8                                                     # |h| ~ 1e-6: both terms of the denominator count
        elif k == 'dominant':
            h[i, rng.integers(256)] = 1e4
        elif k == 'nonfinite':
            h[i, rng.integers(256)] = [np.nan, np.inf, -np.inf][i % 3]
    cw = rng.standard_normal((nc + 2, 256)).astype(np.float32) * 0.05
    cb = rng.standard_normal(nc + 2).astype(np.float32)
    rw = (rng.standard_normal((4, 256)) * 1.6).astype(np.float32)            # reg ~ N(0, 20^2) on ordinary rows: dw = 0.2 reg leaves +-4.135 often
    rb = rng.standard_normal(4).astype(np.float32)
    xy = rng.uniform(-4, 120, (cap, 2))
    wh = rng.uniform(2, 60, (cap, 2))
    rois = np.concatenate([np.zeros((cap, 1)), xy, xy + wh], 1).astype(np.float32)
    return dict(h=h, kinds=kinds, cw=cw, cb=cb, rw=rw, rb=rb, rois=rois, stds=STDS[R % 2], img_hw=(128, 128))


def seesaw_case(counts, seed, no_cand_tile=None, placed_every=97):
    """Logits, deltas and RoIs of sum(counts) RoIs laid out tile after tile with a gap of 3 unused rows between tiles (roi_off is not the
    running sum).  Rows are re-drawn until no float64 score lies within SCORE_MARGIN of PLACED_THR; every placed_every-th row is the placed
    case (equal class logits, equal objectness logits: score exactly on the threshold, strictly not a candidate); the RoIs of
    `no_cand_tile` get objectness logits (-8, 8): every score below e^-16."""
    nc = SEESAW_NC
    rng = np.random.default_rng(seed)
    off, total = [], 0
    for n in counts:
        off.append(total)
        total += n + 3
    T = max(total, 1)
    draw = lambda n: np.clip(rng.standard_normal((3, n, 16)) * 2.5, -L_MAX, L_MAX).astype(np.float32)
    cls = draw(T)
    placed = np.zeros(T, bool)
    for b, n in enumerate(counts):
        rows = np.arange(off[b], off[b] + n)
        if no_cand_tile == b:
            cls[:, rows, nc], cls[:, rows, nc + 1] = -8.0, 8.0
        else:
            p = rows[5::placed_every]
            placed[p] = True
            cls[:, p, :] = np.float32(1.5)
    for _ in range(100):
        sc = ref_seesaw(cls[0], cls[1], cls[2], nc)
        bad = (np.abs(sc - PLACED_THR) < SCORE_MARGIN).any(1) & ~placed
        if not bad.any():
            break
        cls[:, bad] = draw(int(bad.sum()))
        if no_cand_tile is not None:
            rows = np.arange(off[no_cand_tile], off[no_cand_tile] + counts[no_cand_tile])
            cls[:, rows, nc], cls[:, rows, nc + 1] = -8.0, 8.0
    xy = rng.uniform(-4, 230, (T, 2))
    wh = rng.uniform(2, 60, (T, 2))
    rois = np.concatenate([np.zeros((T, 1)), xy, xy + wh], 1).astype(np.float32)
    reg2 = (rng.standard_normal((T, 4)) * 8).astype(np.float32)
    return dict(cls=cls, reg2=reg2, rois=rois, off=np.asarray(off, np.int32), cnt=np.asarray(counts, np.int32), placed=placed, nc=nc,
                stds=STDS[2], img_hw=(256, 256), scale=2.0)


def seesaw_expect(c, score_thr):
    """Float64 candidates of a seesaw_case per tile: (roi index within the tile, class, score, box) in roi-major, class-minor order."""
    nc = c['nc']
    sc = ref_seesaw(c['cls'][0], c['cls'][1], c['cls'][2], nc)
    boxes, t = ref_delta2bbox(c['rois'][:, 1:], c['reg2'], c['stds'], c['img_hw'][1], c['img_hw'][0])
    out = []
    for b, n in enumerate(c['cnt']):
        sl = slice(int(c['off'][b]), int(c['off'][b]) + int(n))
        r, k = np.nonzero(sc[sl] > score_thr)
        out.append(dict(roi=r, cls=k, score=sc[sl][r, k], box=boxes[sl][r] / c['scale'], geom=t['geom'][sl][r] / c['scale']))
    return out, sc


def _logits_for(scores, nc):
    """Class / objectness logits whose Seesaw scores are `scores` (nc,) (sum < 1): objectness = their sum, class softmax = their share."""
    s = np.asarray(scores, np.float64)
    P = s.sum()
    l = np.zeros(16, np.float32)
    l[:nc] = np.log(s / P)
    l[nc], l[nc + 1] = np.log(P / (1 - P)), 0.0
    return l


def nms_tiles():
    """Designed tiles for the multiclass NMS (nc = 5, score_thr 0.05, nms_iou 0.5, scale 2, network image 256 x 256): lists of
    (box in output pixels, {class: score}).  Coordinates are multiples of 2^-9 below 128 and the deltas are zero, so delta2bbox and the
    division by the scale are exact and the candidates ARE these boxes.
    tile 'small' (coordinates <= 31.337): identical boxes in two classes; identical boxes in one class with tied scores; IoU pairs at 0.45 /
      0.55 and exactly 0.5 in class 0; eight pairs of class 4 at IoU exactly 0.5 whose fp32 verdict depends on the class offset.
    tile 'wide' (coordinates up to 125.5, four times the other's): the same kinds spread out, and one box at the far corner.
    tile 'many': 40 disjoint boxes (more survivors than max_per_img = 16)."""
    q = lambda v: np.round(np.asarray(v, np.float64) * 512) / 512
    # the y coordinates of the class-4 pairs carry bits down to 2^-17 (still exact through delta2bbox: sums below 128 on a 2^-16 grid), so
    # adding a class offset of 129 (ulp 2^-16) or 506 (2^-15, 2^-14 above 512) rounds them, differently for the two
    q17 = lambda v: np.round(np.asarray(v, np.float64) * 2 ** 17) / 2 ** 17
    lo = 1e-4
    small = []
    small.append((q([1, 1, 7, 6]), {0: 0.30, 1: 0.29, 2: lo, 3: lo, 4: lo}))                    # one box, two classes: both survive
    small.append((q([9, 1, 15, 6]), {2: 0.28}))                                                  # identical box, one class, tied scores:
    small.append((q([9, 1, 15, 6]), {2: 0.28}))                                                  #   the first survives
    small.append((q([17, 1, 27, 11]), {0: 0.40}))                                                # IoU 0.55 with the next: suppressed
    small.append((q([17, 1, 27, 6.5]), {0: 0.39}))
    small.append((q([1, 8, 11, 18]), {0: 0.38}))                                                 # IoU 0.45: kept
    small.append((q([1, 8, 11, 12.5]), {0: 0.37}))
    small.append((q([1, 20, 11, 30]), {0: 0.36}))                                                # IoU exactly 0.5 at offset 0: kept (strict >)
    small.append((q([1, 20, 11, 25]), {0: 0.35}))
    rng = np.random.default_rng(77)
    for k in range(8):                                                                           # class 4, IoU exactly 0.5 in exact arithmetic
        x, y = 13 + (k % 4) * 4.5, 13 + (k // 4) * 9
        w, hh = q(rng.uniform(2.5, 4.0)), q17(rng.uniform(3.0, 4.0)) * 2
        x, y = q(x + rng.uniform(0, 0.4)), q17(y + rng.uniform(0, 0.4))
        small.append((np.array([x, y, x + w, y + hh]), {4: 0.60 - 0.01 * k}))
        small.append((np.array([x, y, x + w, y + hh / 2]), {4: 0.50 - 0.01 * k}))
    small.append((q([25.5, 28.25, 31.337, 31.0]), {3: 0.2}))                                     # the tile's largest coordinate
    wide = [(q(np.concatenate([b[:2] * 4, b[2:] * 4])), s) for b, s in small[:9]]
    wide.append((q([100.25, 110.5, 125.5, 124.0]), {1: 0.22}))
    many = [(q([2 + 12 * (i % 10), 3 + 14 * (i // 10), 10.5 + 12 * (i % 10), 12.25 + 14 * (i // 10)]), {i % 5: 0.9 - 0.02 * i}) for i in range(40)]
    return dict(small=small, wide=wide, many=many)


def nms_case(names):
    """The tiles `names` of nms_tiles() as one det_post input (rows tile after tile)."""
    nc, tiles = 5, nms_tiles()
    rois, cls, off, cnt = [], [], [], []
    for b, name in enumerate(names):
        off.append(len(rois))
        for box, sc in tiles[name]:
            s = np.full(nc, 1e-4)
            for k, v in sc.items():
                s[k] = v
            rois.append(np.concatenate([[b], box * 2.0]))
            cls.append(_logits_for(s, nc))
        cnt.append(len(tiles[name]))
    rois, cls = np.asarray(rois, np.float32), np.asarray(cls, np.float32)
    return dict(rois=rois, cls=np.stack([cls, cls, cls]), reg2=np.zeros((len(rois), 4), np.float32), off=np.asarray(off, np.int32),
                cnt=np.asarray(cnt, np.int32), nc=nc, stds=STDS[2], img_hw=(256, 256), scale=2.0, score_thr=0.05, nms_iou=0.5)


def offset_verdicts(boxes, scores, ids, max_coord):
    """Keep set of mmcv's batched_nms in float32 when the class offset is ids * (max_coord + 1)."""
    from oracle import ops_np
    f32 = np.float32
    off = np.asarray(ids).astype(f32) * (f32(max_coord) + f32(1))
    return ops_np.nms(np.asarray(boxes, f32) + off[:, None], np.asarray(scores, f32), 0.5)


PASTE_GEOMS = [(128, 128, 128, 128, 2.0), (72, 96, 72, 90, 2.0), (64, 64, 60, 50, 4.0)]          # H, W, vH, vW, scale


def paste_boxes(vH, vW):
    """The designed boxes of a paste case in output pixels (float32), with a tag each."""
    b = [('sub-pixel', [10.3, 20.7, 10.6, 20.9]), ('sub-pixel 2', [30.05, 8.4, 30.95, 9.2]), ('integer corners', [8, 8, 24, 24]),
         ('integer corners 28', [12, 20, 40, 48]), ('zero width on k + 0.5', [12.5, 10, 12.5, 22]), ('zero width off it', [14.3, 10, 14.3, 22]),
         ('zero height on k + 0.5', [20, 17.5, 33, 17.5]), ('zero height off it', [20, 19.2, 33, 19.2]), ('zero size', [25.5, 25.5, 25.5, 25.5]),
         ('zero size off', [27.25, 27.75, 27.25, 27.75]),
         ('over the left edge', [-5.2, 10, 6.3, 22]), ('over the top edge', [10, -7.7, 22.5, 5.1]), ('over the right edge', [vW - 6.5, 30, vW + 7.2, 44]),
         ('over the bottom edge', [30, vH - 5.5, 44, vH + 9.1]), ('over a corner', [vW - 4.2, vH - 3.3, vW + 3, vH + 2]),
         ('outside left / top', [-30, -30, -20, -20]), ('outside right', [vW + 5, 5, vW + 20, 20]), ('outside bottom', [5, vH + 2.5, 20, vH + 12]),
         ('whole canvas and more', [-3, -2, vW + 4, vH + 5]), ('wide', [3.2, 5.1, vW - 3.3, vH - 7.7])]
    rng = np.random.default_rng(5)
    for i in range(8):
        x, y = rng.uniform(0, vW - 12), rng.uniform(0, vH - 12)
        b.append((f'random {i}', [x, y, x + rng.uniform(3, 40), y + rng.uniform(3, 40)]))
    return [t for t, _ in b], np.asarray([v for _, v in b], np.float32)


def paste_case(geom, seed=11):
    """Two tiles of one geometry: tile 0 takes the first 17 designed boxes, tile 1 the rest; probabilities are random and away from 0.5
    (0.05 .. 0.4 or 0.6 .. 0.95 per cell), one map of tile 1 holds a NaN cell and one is NaN throughout."""
    H, W, vH, vW, scale = geom
    tags, boxes = paste_boxes(vH, vW)
    D = len(boxes)
    rng = np.random.default_rng(seed)
    hi = rng.random((D, 28, 28)) < 0.5
    prob = np.where(hi, rng.uniform(0.6, 0.95, (D, 28, 28)), rng.uniform(0.05, 0.4, (D, 28, 28))).astype(np.float32)
    prob[D - 2, 13, 14] = np.nan
    prob[D - 1] = np.nan
    counts = np.asarray([17, D - 17], np.int32)
    off = np.asarray([0, 17], np.int32)
    tile = np.repeat(np.arange(2), counts).astype(np.float32)
    mrois = np.concatenate([tile[:, None], boxes * np.float32(scale)], 1).astype(np.float32)
    return dict(tags=tags, prob=prob, mrois=mrois, off=off, counts=counts, H=H, W=W, vH=vH, vW=vW, scale=scale,
                boxes=mrois[:, 1:].astype(np.float64) / scale)


def const_boxes():
    """Boxes whose width and height are powers of two and whose corners are short dyadic numbers: (x + 0.5 - x0) / 2^k, * 2, - 1, + 1, * 28,
    - 1, / 2 are then all exact in fp32 and fp64, the bilinear weights are dyadic with a few bits, their products and sums exact: a sample
    whose four taps lie inside the 28 x 28 grid of a constant 0.5 map IS 0.5, and the comparison with thr = 0.5 is decided by `>=` alone."""
    return np.asarray([[8, 8, 40, 40], [4.5, 6.25, 20.5, 22.25], [1, 2, 65, 34], [-6, 30, 26, 62], [40, 40.5, 56, 56.5], [50.25, 3, 58.25, 11]], np.float32)


def blob_tile(n_pass, n_pad, seed, H=128, W=128, vH=128, vW=128, margin=2, min_area=4):
    """n_pass detections that pass the margin / area filter (small rectangular blobs with plenty of overlaps, each mask the interior of its
    box and so inside the box's hull -- what the kernel's hull test relies on) followed and interleaved by n_pad that do not (area
    min_area - 1, or a box edge outside the margin).  Scores are distinct.  -> dets (n, 5) float32, labels, masks (n, H, W) bool."""
    rng = np.random.default_rng(seed)
    n = n_pass + n_pad
    passing = np.zeros(n, bool)
    passing[rng.permutation(n)[:n_pass]] = True
    dets, masks = np.zeros((n, 5), np.float32), np.zeros((n, H, W), bool)
    for i in range(n):
        if passing[i]:
            lo = 2 if min_area <= 4 else 4                                   # area >= min_area
            w, h = rng.integers(lo, 7), rng.integers(lo, 7)
            x, y = rng.integers(margin, vW - margin - w + 1), rng.integers(margin, vH - margin - h + 1)
        elif i % 2:
            w, h = min_area - 1, 1                                           # too small
            x, y = rng.integers(margin, vW - margin - w + 1), rng.integers(margin, vH - margin - h + 1)
        else:
            w, h = 4, 4                                                      # touches the left margin
            x, y = margin - 1, rng.integers(margin, vH - margin - h + 1)
        dets[i, :4] = [x, y, x + w, y + h]
        masks[i, y:y + h, x:x + w] = True
    dets[:, 4] = rng.permutation(n).astype(np.float32) / np.float32(n + 1) * 0.9 + 0.05      # distinct
    labels = rng.integers(0, 5, n).astype(np.int32)
    return dets, labels, masks


_CACHE = {}


def blob_lists_and_refs():
    """nested_blob_lists() and the reference keep flags / filtered counts of its lists, computed once per process."""
    if 'blobs' not in _CACHE:
        lists, low = nested_blob_lists()
        refs = {k: ref_tile_post(d, l, m, 128, 128, 2, 4, 0.05) for k, (d, l, m) in lists.items()}
        _CACHE['blobs'] = (lists, low, refs)
    return _CACHE['blobs']


def nested_blob_lists(seed=31):
    """Lists with 511, 512, 513 and 1500 filtered candidates plus filtered-out padding; the first three are nested: the 512- and 513-lists
    add one candidate each whose score is below every other, so it can suppress nothing and the keep flags of the shared detections must
    agree between the bit-matrix pass (511, 512) and the barrier pass (513)."""
    d, l, m = blob_tile(513, 37, seed)
    area = m.reshape(len(m), -1).sum(1)
    ok = (d[:, 0] >= 2) & (area >= 4)
    low = np.nonzero(ok)[0][-2:]                                             # the last two passing detections get the two lowest scores
    d[low[0], 4], d[low[1], 4] = 0.02, 0.01
    l513 = (d, l, m)
    cut = lambda drop: tuple(np.delete(a, drop, 0) for a in (d, l, m))
    return {511: cut(low), 512: cut(low[1:]), 513: l513, 1500: blob_tile(1500, 101, seed + 1)}, low


def pinned_tile():
    """One 128 x 128 tile (valid 124 x 120, margin 2, min_area 10, thr 0.05) holding every strict comparison on its edge.  -> dets, labels,
    masks, expect {slot: keep flag}."""
    H, W, vH, vW, mg = 128, 128, 124, 120, 2
    rows, exp = [], {}

    def add(box, score, label, pix, keep):
        m = np.zeros((H, W), bool)
        for (y0, y1, x0, x1) in pix:
            m[y0:y1, x0:x1] = True
        rows.append((np.asarray(list(box) + [score], np.float32), label, m))
        exp[len(rows) - 1] = keep

    # intersection 1, union 20: IoU == 0.05 exactly, not > thr: both kept
    add((10, 10, 20, 11), 0.90, 0, [(10, 11, 10, 20)], 1)
    add((19, 10, 20, 21), 0.89, 0, [(10, 21, 19, 20)], 1)
    # intersection 2, union 39: 2 / 39 > 0.05: the lower score goes
    add((30, 10, 40, 12), 0.88, 0, [(10, 12, 30, 40)], 1)
    add((39, 10, 40, 31), 0.87, 0, [(10, 31, 39, 40)], 0)
    # areas min_area - 1 and min_area
    add((50, 10, 53, 13), 0.86, 1, [(10, 13, 50, 53)], 0)
    add((56, 10, 61, 12), 0.85, 1, [(10, 12, 56, 61)], 1)
    # box edges on the margin, just inside and just outside, each side (vW = 120 != W)
    f = np.float32
    up, dn = (lambda v: float(np.nextafter(f(v), f(1e9)))), (lambda v: float(np.nextafter(f(v), f(-1e9))))
    blob = lambda x, y: [(y, y + 4, x, x + 4)]
    add((mg, 40, 6, 44), 0.84, 2, blob(2, 40), 1)
    add((dn(mg), 46, 6, 50), 0.83, 2, blob(2, 46), 0)
    add((up(mg), 52, 6, 56), 0.82, 2, blob(2, 52), 1)
    add((10, mg, 14, 6), 0.81, 2, blob(10, 2), 1)
    add((16, dn(mg), 20, 6), 0.80, 2, blob(16, 2), 0)
    add((vW - mg - 4, 40, vW - mg, 44), 0.79, 2, blob(vW - mg - 4, 40), 1)
    add((vW - mg - 4, 46, up(vW - mg), 50), 0.78, 2, blob(vW - mg - 4, 46), 0)
    add((vW - mg - 4, 52, dn(vW - mg), 56), 0.77, 2, blob(vW - mg - 4, 52), 1)
    add((40, vH - mg - 4, 44, vH - mg), 0.76, 2, blob(40, vH - mg - 4), 1)
    add((46, vH - mg - 4, 50, up(vH - mg)), 0.75, 2, blob(46, vH - mg - 4), 0)
    add((vW - mg - 3, 60, vW - mg + 1, 64), 0.74, 2, blob(vW - mg - 3, 60), 0)                  # inside W - margin but outside vW - margin
    # a tie between two overlapping masks, labels out of order: slot A (label 3) sits behind slot B (label 1) in class-major order, so the
    # reversed stable sort visits A first: A kept, B suppressed (by index order it would be the other way round)
    add((60, 40, 66, 46), 0.5, 3, [(40, 46, 60, 66)], 1)
    add((61, 40, 67, 46), 0.5, 1, [(40, 46, 61, 67)], 0)
    # chain: A suppresses B; B would have suppressed C; A and C do not meet: C kept
    add((70, 60, 76, 64), 0.70, 4, [(60, 64, 70, 76)], 1)
    add((74, 60, 80, 64), 0.69, 0, [(60, 64, 74, 80)], 0)
    add((78, 60, 84, 64), 0.68, 4, [(60, 64, 78, 84)], 1)
    dets = np.stack([r[0] for r in rows])
    return dets, np.asarray([r[1] for r in rows], np.int32), np.stack([r[2] for r in rows]), exp, dict(H=H, W=W, vH=vH, vW=vW, margin=mg, min_area=10)


# ================================================================================================================ GPU fixtures / helpers
@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    return Engine(weights.seeded_state_dict(0), device=0, max_batch=1, tile=(64, 64))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)


def sentinel_i32(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device='cuda')


def _keeps_sentinel(t):
    return bool((_bits(t) == SENTINEL).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_tail(eng, c, R, refine):
    cap = len(c['h'])
    cls, reg = sentinel(cap, 16), sentinel(cap, 4)
    rois = dev(c['rois'])
    eng.op_bbox_tail(dev(c['h']), c['cw'], c['cb'], c['rw'], c['rb'], rois, R, c['stds'], c['img_hw'], refine, cls=cls, reg=reg)
    return cls, reg, rois


def _run_det_post(eng, c, score_thr=None, nms_iou=None, max_per_img=500, limit=None, cap=None):
    return eng.op_det_post(dev(c['rois']), [dev(c['cls'][k]) for k in range(3)], dev(c['reg2']), c['off'], c['cnt'], c['nc'], c['stds'], c['img_hw'],
                           c['scale'], c.get('score_thr', 0.05) if score_thr is None else score_thr, c.get('nms_iou', 0.5) if nms_iou is None else nms_iou,
                           max_per_img, limit=limit, cap=cap)


# ================================================================================================================ bbox tail
@pytest.mark.gpu
def test_bbox_tail_vs_fp64(eng):
    """R in {1, 3, 4, 5, 9} live rows of 12 (four RoIs share a workgroup), nc in {4, 5}, refinement on and off, every class of h row.
    cls / reg within TOL_TAIL * mag, the refined RoIs within the propagated bound; rows from R on and the unused cls columns keep the
    sentinel; a non-finite row stays in its own row."""
    seen, flags, combo = set(), set(), 0
    for R in (1, 3, 4, 5, 9):
        for nc in (4, 5):
            for refine in (0, 1):
                c = tail_case(R, nc, refine, combo)
                combo += 1
                cls, reg, rois = _run_tail(eng, c, R, refine)
                rcls, rreg, mcls, mreg = ref_bbox_tail(c['h'], c['cw'], c['cb'], c['rw'], c['rb'])
                live = np.arange(len(c['h'])) < R
                good = live & np.asarray([k != 'nonfinite' for k in c['kinds']])
                seen |= {k for k, l in zip(c['kinds'], live) if l}
                gcls, greg, grois = cls.cpu().numpy().astype(np.float64), reg.cpu().numpy().astype(np.float64), rois.cpu().numpy()
                assert _keeps_sentinel(cls[R:]) and _keeps_sentinel(reg[R:]) and _keeps_sentinel(cls[:R, nc + 2:]), (R, nc, refine)
                assert (grois[R:].view(np.int32) == c['rois'][R:].view(np.int32)).all(), 'RoIs past R were touched'
                assert np.isfinite(gcls[good, :nc + 2]).all() and np.isfinite(greg[good]).all(), (R, nc, refine)
                for tag, g, r, m in (('cls', gcls[good, :nc + 2], rcls[good], mcls[good]), ('reg', greg[good], rreg[good], mreg[good])):
                    rel = (np.abs(g - r) / np.maximum(m, 1e-300)).max() if g.size else 0.0
                    _obs(f'bbox tail {tag} err / mag', rel)
                    assert (np.abs(g - r) <= TOL_TAIL * m).all(), f'{tag} R={R} nc={nc} refine={refine}: max err/mag {rel:.3e} > {TOL_TAIL:.3e}'
                zero = good & np.asarray([k == 'zero' for k in c['kinds']])
                assert (gcls[zero, :nc + 2] == c['cb'].astype(np.float64)).all() and (greg[zero] == c['rb'].astype(np.float64)).all()
                if refine:
                    o, bound, t = refine_bound(c['rois'][:, 1:], rreg, mreg, c['stds'], 128, 128)
                    err = np.abs(grois[:, 1:].astype(np.float64) - o)
                    ok = good & np.isfinite(bound).all(1)
                    assert (grois[good, 0] == 0).all() and np.isfinite(grois[good]).all()
                    assert (err[ok] <= bound[ok]).all(), f'refined RoIs R={R} nc={nc}: {err[ok].max():.3e}'
                    fin = err[ok][bound[ok] > 0] / bound[ok][bound[ok] > 0]
                    _obs('bbox tail refined roi err / bound', fin.max() if fin.size else 0.0)
                    g = good & ok
                    flags |= {'dw > max'} if (t['dw'][g] > MAX_RATIO).any() or (t['dh'][g] > MAX_RATIO).any() else set()
                    flags |= {'dw < -max'} if (t['dw'][g] < -MAX_RATIO).any() or (t['dh'][g] < -MAX_RATIO).any() else set()
                    flags |= {'clip at 0'} if ((t['gx'] - t['gw'] / 2)[g] < 0).any() else set()
                    flags |= {'clip at size'} if ((t['gx'] + t['gw'] / 2)[g] > 128).any() else set()
                else:
                    assert (grois.view(np.int32) == c['rois'].view(np.int32)).all(), 'refine off must leave the RoIs alone'
    assert seen == set(H_CLASSES), seen
    assert flags == {'dw > max', 'dw < -max', 'clip at 0', 'clip at size'}, flags


# ================================================================================================================ Seesaw candidates
SEESAW_COUNTS = [(1023, 0, 2100), (1, 1024, 1025)]


def _check_candidates(r, c, exp, tag):
    n_got = r['cand_count'].cpu().numpy()
    ids, sc, bx = r['cand_ids'].cpu().numpy(), r['cand_scores'].cpu().numpy().astype(np.float64), r['cand_boxes'].cpu().numpy().astype(np.float64)
    for b, e in enumerate(exp):
        n = len(e['roi'])
        assert n_got[b] == n, f'{tag} tile {b}: {n_got[b]} candidates, reference {n}'
        assert (ids[b, :n] == e['cls']).all(), f'{tag} tile {b}: class ids / order differ'
        err = np.abs(sc[b, :n] - e['score'])
        if n:
            _obs('candidate score relative error', (err / e['score']).max())
            assert (err <= SCORE_REL * e['score']).all(), f'{tag} tile {b}: score error {(err / e["score"]).max():.3e} > {SCORE_REL:.3e}'
            berr = np.abs(bx[b, :n] - e['box'])
            _obs('candidate box err / (u geom)', (berr / (U * e['geom'])).max())
            assert (berr <= BOX_C * U * e['geom']).all(), f'{tag} tile {b}: box error'


@pytest.mark.gpu
@pytest.mark.parametrize('counts', SEESAW_COUNTS)
def test_seesaw_candidates_vs_fp64(eng, counts):
    """Per-tile RoI counts around the 1024-RoI chunk of det_candidates_kernel (2100: three chunks) with non-trivial roi_off: candidate count,
    class ids and (roi-major, class-minor) order exact, scores within SCORE_REL; a tile without any candidate; the placed rows (score exactly
    on the threshold) are not candidates; then score_thr = -1 (the fixed-load setting): every pair passes, in order."""
    no_cand = int(np.argmin(counts))                   # the tile with the fewest RoIs (0 or 1): no candidate at all
    c = seesaw_case(counts, seed=sum(counts), no_cand_tile=no_cand)
    exp, sc = seesaw_expect(c, PLACED_THR)
    assert not ((np.abs(sc - PLACED_THR) < SCORE_MARGIN).any(1) & ~c['placed']).any(), 'a reference score lies within the margin of score_thr'
    assert len(exp[no_cand]['roi']) == 0 and c['placed'].sum() >= 2
    assert max(counts) <= 1025 or max(counts) > 2048, 'three chunks wanted'
    r = _run_det_post(eng, c, score_thr=PLACED_THR, nms_iou=2.0, max_per_img=8)
    _check_candidates(r, c, exp, f'{counts}')
    # a later chunk contributes: the candidates of the longest tile come from RoIs beyond the first 1024 as well (the carry of `written`)
    if max(counts) > 1024:
        b = int(np.argmax(counts))
        assert (exp[b]['roi'] >= 1024).any() and (exp[b]['roi'] < 1024).any()
    print(f'seesaw {counts}: candidates per tile {[len(e["roi"]) for e in exp]}, placed rows {int(c["placed"].sum())}')
    exp_all, _ = seesaw_expect(c, -1.0)
    r = _run_det_post(eng, c, score_thr=-1.0, nms_iou=2.0, max_per_img=8)
    for b, e in enumerate(exp_all):
        assert len(e['roi']) == counts[b] * c['nc'] and (e['cls'] == np.tile(np.arange(c['nc']), counts[b])).all()
    _check_candidates(r, c, exp_all, f'{counts} score_thr -1')


# ================================================================================================================ multiclass NMS + finish
def _check_nms(r, c, max_per_img, limit, tag):
    """dets / labels / counts equal ops_np.batched_nms on the op's own candidates; mask_rois, det_off, det_total follow from the counts."""
    from oracle import ops_np
    ncand = r['cand_count'].cpu().numpy()
    cb, cs, ci = r['cand_boxes'].cpu().numpy(), r['cand_scores'].cpu().numpy(), r['cand_ids'].cpu().numpy()
    dets, labels, counts = r['dets'].cpu().numpy(), r['labels'].cpu().numpy(), r['counts'].cpu().numpy()
    mrois, det_off, det_total = r['mask_rois'].cpu().numpy(), r['det_off'].cpu().numpy(), int(r['det_total'].item())
    acc, out = 0, []
    for b in range(len(ncand)):
        n = int(ncand[b])
        d, keep = ops_np.batched_nms(cb[b, :n], cs[b, :n], ci[b, :n], c['nms_iou'])
        k = min(len(d), max_per_img, limit)
        assert counts[b] == k, f'{tag} tile {b}: {counts[b]} detections, reference {k} (of {len(d)} survivors)'
        assert (dets[b, :k].view(np.int32) == d[:k].view(np.int32)).all(), f'{tag} tile {b}: rows / order differ'
        assert (labels[b, :k] == ci[b, :n][keep[:k]]).all(), f'{tag} tile {b}: labels differ'
        assert det_off[b] == acc
        want = np.concatenate([np.full((k, 1), b, np.float32), dets[b, :k, :4] * np.float32(c['scale'])], 1)
        assert (mrois[acc:acc + k].view(np.int32) == want.view(np.int32)).all(), f'{tag} tile {b}: mask_rois'
        acc += k
        out.append((len(d), k))
    assert det_total == acc
    return out


@pytest.mark.gpu
def test_multiclass_nms_and_finish(eng):
    """The designed tiles of nms_tiles(): identical boxes across classes survive, tied identical boxes keep the first, IoU on both sides of
    and exactly on nms_iou, the per-tile class offset (tile 'small' beside a tile four times as wide), more survivors than max_per_img,
    limit < max_per_img, mask_rois / det_off / det_total, and batch independence bit for bit."""
    c = nms_case(['small', 'wide', 'many'])
    r = _run_det_post(eng, c, max_per_img=16)
    # the candidates are the designed boxes exactly (dyadic coordinates, zero deltas)
    tiles = nms_tiles()
    cb, ci, ncand = r['cand_boxes'].cpu().numpy(), r['cand_ids'].cpu().numpy(), r['cand_count'].cpu().numpy()
    for b, name in enumerate(['small', 'wide', 'many']):
        want = [(box, k) for box, sc in tiles[name] for k in sorted(sc) if sc[k] > 0.05]
        assert ncand[b] == len(want)
        assert (cb[b, :ncand[b]] == np.asarray([w[0] for w in want], np.float32)).all() and (ci[b, :ncand[b]] == [w[1] for w in want]).all()
    res = _check_nms(r, c, 16, 16, 'nms')
    assert res[2] == (40, 16), res
    # the per-tile offset decides: with the batch's largest coordinate as tile 0's offset base, some verdict of tile 0 would differ
    n0 = int(ncand[0])
    cs = r['cand_scores'].cpu().numpy()
    own = offset_verdicts(cb[0, :n0], cs[0, :n0], ci[0, :n0], cb[0, :n0].max())
    other = offset_verdicts(cb[0, :n0], cs[0, :n0], ci[0, :n0], max(cb[b, :ncand[b]].max() for b in range(3)))
    assert cb[1, :ncand[1]].max() >= 4 * cb[0, :n0].max() - 1e-3
    assert set(own.tolist()) != set(other.tolist()), 'the designed pairs do not tell the per-tile offset from a batch-wide one'
    d0 = r['dets'][0, :res[0][1]].cpu().numpy()
    assert (d0.view(np.int32) == np.concatenate([cb[0, own], cs[0, own, None]], 1)[:16].view(np.int32)).all()
    print(f'nms: survivors / kept per tile {res}; verdicts that depend on the offset base: {len(set(own.tolist()) ^ set(other.tolist()))}')
    # designed outcomes, read off the labels and boxes of tile 0 (max_per_img large enough to hold them all)
    r2 = _run_det_post(eng, c, max_per_img=64)
    res2 = _check_nms(r2, c, 64, 64, 'nms K=64')
    k0 = res2[0][1]
    d, l = r2['dets'][0, :k0].cpu().numpy(), r2['labels'][0, :k0].cpu().numpy()
    has = lambda box, lab: int(((d[:, :4] == np.asarray(box, np.float32)).all(1) & (l == lab)).sum())
    assert has([1, 1, 7, 6], 0) == 1 and has([1, 1, 7, 6], 1) == 1, 'identical boxes in two classes must both survive'
    assert has([9, 1, 15, 6], 2) == 1, 'tied identical boxes in one class: exactly one survives'
    assert has([17, 1, 27, 11], 0) == 1 and has([17, 1, 27, 6.5], 0) == 0, 'IoU 0.55 is suppressed'
    assert has([1, 8, 11, 18], 0) == 1 and has([1, 8, 11, 12.5], 0) == 1, 'IoU 0.45 is kept'
    assert has([1, 20, 11, 30], 0) == 1 and has([1, 20, 11, 25], 0) == 1, 'IoU exactly 0.5 at offset 0 is kept (strict >)'
    # limit < max_per_img
    r3 = _run_det_post(eng, c, max_per_img=16, limit=10)
    res3 = _check_nms(r3, c, 16, 10, 'nms limit 10')
    assert res3[2] == (40, 10)
    # batch independence: tile 'small' at position 0 beside ('wide', 'many') and at position 2 beside ('many', 'wide')
    c4 = nms_case(['many', 'wide', 'small'])
    r4 = _run_det_post(eng, c4, max_per_img=16)
    _check_nms(r4, c4, 16, 16, 'nms permuted')
    assert int(r4['counts'][2]) == int(r['counts'][0])
    for key in ('dets', 'labels'):
        assert _same_bits(r4[key][2], r[key][0]) and _same_bits(r4[key][0], r[key][2]), key


# ================================================================================================================ paste
def _run_paste(eng, c, prob=None, thr=0.5, max_keep=24):
    B = len(c['counts'])
    masks = sentinel_i32(B, max_keep, c['H'], c['W'] // 32)
    areas = sentinel_i32(B, max_keep)
    eng.op_paste(dev(c['prob'] if prob is None else prob), dev(c['mrois']), c['off'], c['counts'], max_keep, c['H'], c['W'], c['vH'], c['vW'], c['scale'], thr,
                 masks=masks, areas=areas)
    return masks, areas


def _paste_band(vals, hull, thr):
    with np.errstate(invalid='ignore'):
        return hull & (np.abs(vals - thr) <= PASTE_BAND)


@pytest.mark.gpu
@pytest.mark.parametrize('geom', PASTE_GEOMS)
def test_paste_vs_fp64_grid_sample(eng, geom):
    """Every designed box of paste_boxes() on random probabilities: a pixel may differ from the float64 reference only where the sampled
    value is within 1e-5 of the threshold; areas equal the popcounts of the op's own masks; nothing is set outside the valid canvas or the
    hull; NaN probabilities set no bit; slots from det_counts[b] on keep their sentinel."""
    c = paste_case(geom)
    H, W, vH, vW = c['H'], c['W'], c['vH'], c['vW']
    ref, vals, hull = ref_paste(c['prob'], c['boxes'], H, W, vH, vW, 0.5)
    band = _paste_band(vals, hull, 0.5)
    assert band.sum() <= PASTE_BAND_SHARE * hull.sum(), (int(band.sum()), int(hull.sum()))
    masks, areas = _run_paste(eng, c)
    ndiff = 0
    for b in range(2):
        n, o = int(c['counts'][b]), int(c['off'][b])
        got = unpack_masks(masks[b, :n].cpu().numpy(), W)
        assert _keeps_sentinel(masks[b, n:]) and _keeps_sentinel(areas[b, n:]), 'slots past det_counts were written'
        assert (areas[b, :n].cpu().numpy() == got.reshape(n, -1).sum(1)).all(), 'areas differ from the popcounts'
        assert not got[:, vH:].any() and not got[:, :, vW:].any(), 'a bit outside the valid canvas'
        assert not (got & ~hull[o:o + n]).any(), 'a bit outside the integer hull'
        diff = got != ref[o:o + n]
        ndiff += int(diff.sum())
        assert not (diff & ~band[o:o + n]).any(), [c['tags'][o + j] for j in np.nonzero((diff & ~band[o:o + n]).reshape(n, -1).any(1))[0]]
    D = len(c['boxes'])
    tag = dict(zip(c['tags'], range(D)))
    # the branches are taken: zero-size boxes sample (the isinf patch gives a stripe) or yield NaN (0 / 0: nothing), off-canvas boxes are empty
    for t in ('outside left / top', 'outside right', 'outside bottom'):
        assert not hull[tag[t]].any() and not ref[tag[t]].any()
    assert np.isnan(vals[tag['zero width on k + 0.5']][hull[tag['zero width on k + 0.5']]]).any()
    assert np.isfinite(vals[tag['zero width off it']][hull[tag['zero width off it']]]).all() and hull[tag['zero width off it']].any()
    if vW >= 120:
        assert c['boxes'][tag['wide'], 2] - c['boxes'][tag['wide'], 0] > 112
    assert not ref[D - 1].any() and np.isnan(vals[D - 2]).any()
    print(f'paste {geom}: {int(hull.sum())} hull pixels, {int(band.sum())} within {PASTE_BAND:g} of the threshold on the reference, {ndiff} differ, '
          f'{int(ref.sum())} set')


@pytest.mark.gpu
def test_paste_constant_half_pins_the_threshold(eng):
    """A constant 0.5 map under boxes of power-of-two size (const_boxes: every step exact in fp32 and fp64): the mask equals the float64
    reference exactly, with no band -- every sample whose four taps lie in the grid is 0.5 == thr and must be set (`>=`), every sample that
    lost a tap with non-zero weight is below."""
    boxes = const_boxes()
    D = len(boxes)
    for H, W, vH, vW, scale in [(128, 128, 128, 128, 2.0), (64, 64, 60, 50, 4.0)]:
        mrois = np.concatenate([np.zeros((D, 1), np.float32), boxes * np.float32(scale)], 1).astype(np.float32)
        c = dict(prob=np.full((D, 28, 28), 0.5, np.float32), mrois=mrois, off=np.asarray([0], np.int32), counts=np.asarray([D], np.int32), H=H, W=W,
                 vH=vH, vW=vW, scale=scale)
        ref, vals, hull = ref_paste(c['prob'], boxes, H, W, vH, vW, 0.5)
        assert ((vals == 0.5) & hull).sum() > 500 and ((vals < 0.5) & (vals > 0) & hull).any()
        masks, areas = _run_paste(eng, c, max_keep=D)
        got = unpack_masks(masks[0].cpu().numpy(), W)
        assert (got == ref).all(), int((got != ref).sum())
        assert (areas[0].cpu().numpy() == ref.reshape(D, -1).sum(1)).all()
        lower, _, _ = ref_paste(c['prob'], boxes, H, W, vH, vW, float(np.nextafter(np.float32(0.5), np.float32(1))))
        masks, _ = _run_paste(eng, c, thr=float(np.nextafter(np.float32(0.5), np.float32(1))), max_keep=D)
        assert not lower.any() and not unpack_masks(masks[0].cpu().numpy(), W).any()


# ================================================================================================================ tile filter + mask-NMS
def _run_tile_post(eng, tiles, K, geo, thr=0.05):
    """tiles: list of (dets, labels, masks bool) -> keep (B, K) on the host, with the slots past each count preset to SENT_U8."""
    B, H, W = len(tiles), geo['H'], geo['W']
    dets, labels = np.zeros((B, K, 5), np.float32), np.zeros((B, K), np.int32)
    areas, words = np.zeros((B, K), np.int32), np.zeros((B, K, H, W // 32), np.int32)
    counts = np.asarray([len(t[0]) for t in tiles], np.int32)
    for b, (d, l, m) in enumerate(tiles):
        n = len(d)
        if n:
            dets[b, :n], labels[b, :n], areas[b, :n], words[b, :n] = d, l, m.reshape(n, -1).sum(1), pack_masks(m)
    keep = torch.full((B, K), SENT_U8, dtype=torch.uint8, device='cuda')
    eng.op_tile_post(dev(dets), dev(labels), dev(areas), counts, dev(words), H, W, geo['vH'], geo['vW'], geo['margin'], geo['min_area'], thr, keep=keep)
    keep = keep.cpu().numpy()
    for b in range(B):
        assert (keep[b, counts[b]:] == SENT_U8).all(), 'keep beyond n was touched'
    return keep


@pytest.mark.gpu
def test_tile_post_small_counts_and_pinned_comparisons(eng):
    """Detection counts {0, 1, 2, 3, 64, 65, 500} and the pinned tile (IoU exactly 0.05 kept, 2 / 39 suppressed, areas min_area - 1 / min_area,
    box edges on / inside / outside the margin on each side with vW != W, a tie with labels out of order, a suppression chain), B = 8 in one
    launch; exact against ref_tile_post.  Masks are the interiors of their boxes, i.e. inside the box hulls: the precondition of the
    kernel's hull test.  The tie case pins the kernel's documented convention (the reverse of a STABLE ascending sort over the class-major
    list); numpy's default argsort promises no tie order, so tied scores between overlapping masks occur in that one designed case only."""
    geo = dict(H=128, W=128, vH=124, vW=120, margin=2, min_area=10)
    tiles = []
    for i, n in enumerate((0, 1, 2, 3, 64, 65, 500)):
        tiles.append(blob_tile(n - n // 4, n // 4, 50 + i, vH=124, vW=120, min_area=10))
    pd, pl, pm, exp, pgeo = pinned_tile()
    assert pgeo == geo
    tiles.append((pd, pl, pm))
    keep = _run_tile_post(eng, tiles, 512, geo)
    for b, (d, l, m) in enumerate(tiles):
        ref, nf = ref_tile_post(d, l, m, 124, 120, 2, 10, 0.05)
        assert (keep[b, :len(d)] == ref).all(), f'tile {b} (n = {len(d)}, {nf} filtered): {int((keep[b, :len(d)] != ref).sum())} keep flags differ'
        print(f'tile_post n = {len(d)}: {nf} pass the filter, {int(ref.sum())} kept (bit-matrix pass)')
        assert nf <= 512
    for slot, flag in exp.items():
        assert keep[7, slot] == flag, f'pinned slot {slot}: keep {keep[7, slot]}, designed {flag}'
    # batch independence, bit for bit: the same tiles at other batch positions with other neighbours
    perm = [7, 6, 0, 5, 4, 1, 3, 2]
    keep2 = _run_tile_post(eng, [tiles[p] for p in perm], 512, geo)
    for i, p in enumerate(perm):
        assert (keep2[i] == keep[p]).all(), (i, p)


@pytest.mark.gpu
def test_tile_post_both_greedy_passes(eng):
    """max_keep = 2048 on a 128 x 128 tile, min_area 4: 511 and 512 filtered candidates run the LDS bit-matrix pass, 513 and 1500 the
    per-candidate barrier pass (the switch is the FILTERED count; each list also holds filtered-out padding).  Exact against
    ref_tile_post; the nested lists must agree on their shared detections across the two passes."""
    geo = dict(H=128, W=128, vH=128, vW=128, margin=2, min_area=4)
    lists, low, refs_nf = blob_lists_and_refs()
    order = (511, 512, 513, 1500)
    refs = {}
    for k in order:
        d, l, m = lists[k]
        refs[k], nf = refs_nf[k]
        assert nf == k, (k, nf)
        print(f'tile_post {len(d)} detections, {nf} filtered -> {"bit-matrix" if nf <= 512 else "barrier"} pass, {int(refs[k].sum())} kept, '
              f'{nf - int(refs[k].sum())} suppressed')
        assert 0 < refs[k].sum() < nf, 'the list must have both kept and suppressed candidates'
    keep = _run_tile_post(eng, [lists[k] for k in order[:3]], 2048, geo)
    keep1500 = _run_tile_post(eng, [lists[1500]], 2048, geo)
    for b, k in enumerate(order[:3]):
        n = len(lists[k][0])
        assert (keep[b, :n] == refs[k]).all(), f'{k} filtered candidates: {int((keep[b, :n] != refs[k]).sum())} keep flags differ'
    n = len(lists[1500][0])
    assert (keep1500[0, :n] == refs[1500]).all(), f'1500 filtered candidates: {int((keep1500[0, :n] != refs[1500]).sum())} keep flags differ'
    k513 = keep[2, :len(lists[513][0])]
    assert (np.delete(k513, low) == keep[0, :len(lists[511][0])]).all(), 'bit-matrix pass (511) and barrier pass (513) disagree'
    assert (np.delete(k513, low[1:]) == keep[1, :len(lists[512][0])]).all(), 'bit-matrix pass (512) and barrier pass (513) disagree'
    # B = 3 with different counts, other positions: bitwise the same
    keep2 = _run_tile_post(eng, [lists[1500], lists[511], lists[513]], 2048, geo)
    assert (keep2[0] == keep1500[0]).all() and (keep2[1] == keep[0]).all() and (keep2[2] == keep[2]).all()


# ================================================================================================================ the ops are the engine's path
@pytest.mark.gpu
def test_ops_are_the_engines_path(hip_device):
    """One engine on the small_b2 golden with the token dump on; each op, fed the engine's own buffers (and the checkpoint's stage-2 head
    weights), reproduces the matching engine output bit for bit."""
    import golden_util as G
    from nuhtc_amd.engine import Engine
    g = G.load('small_b2')
    sd, tiles = G.seeded_sd(g), g['tiles']
    B = len(tiles)
    e = Engine(sd, device=0, max_batch=B, tile=tiles.shape[1:3])
    e.enable_token_dump()
    e.infer_async(e.to_device(tiles), int(g['channel_mode']))
    e.check()
    cfg = e.cfg
    nc, K, sf = cfg.num_classes, cfg.max_per_img, float(cfg.scale_factor)
    H, W = cfg.tile_h, cfg.tile_w
    img_hw = (int(tiles.shape[1] * sf + 0.5), int(tiles.shape[2] * sf + 0.5))
    stds = [[float(cfg.stage_stds[k][j]) for j in range(4)] for k in range(3)]
    R = int(e.buffer('roi_total').item())
    counts = e.counts[:B].clone()
    assert R > 0 and int(counts.sum()) > 0
    # bbox tail of stage 2 (no refinement): h2 -> cls2, reg2
    p = 'roi_head.bbox_head.2.'
    rois2 = e.buffer('rois_stage2')
    rois_in = rois2.clone()
    cls, reg = e.op_bbox_tail(e.buffer('h2'), sd[p + 'fc_cls.weight'], sd[p + 'fc_cls.bias'], sd[p + 'fc_reg.weight'], sd[p + 'fc_reg.bias'], rois_in,
                              e.buffer('roi_total'), stds[2], img_hw, refine=0, cls=sentinel(*e.buffer('cls2').shape), reg=sentinel(*e.buffer('reg2').shape))
    assert _same_bits(cls[:R, :nc + 2], e.buffer('cls2')[:R, :nc + 2]) and _same_bits(reg[:R], e.buffer('reg2')[:R])
    assert _same_bits(rois_in, rois2) and _same_bits(e.buffer('rois')[:R], rois2[:R])
    # candidates + NMS + finish
    r = e.op_det_post(rois2, [e.buffer(f'cls{k}') for k in range(3)], e.buffer('reg2'), e.buffer('roi_off')[:B], e.buffer('roi_counts')[:B], nc, stds[2],
                      img_hw, sf, float(cfg.score_thr), float(cfg.nms_iou), K)
    assert torch.equal(r['counts'], counts)
    D = int(e.buffer('det_total').item())
    assert int(r['det_total'].item()) == D and torch.equal(r['det_off'], e.buffer('det_off')[:B])
    assert _same_bits(r['mask_rois'][:D], e.buffer('mask_rois')[:D])
    for b in range(B):
        n = int(counts[b])
        assert _same_bits(r['dets'][b, :n], e.boxes[b, :n]) and torch.equal(r['labels'][b, :n], e.labels[b, :n]), b
    # paste
    masks, areas = e.op_paste(e.buffer('mask_prob'), e.buffer('mask_rois'), e.buffer('det_off')[:B], counts, K, H, W, cfg.valid_h, cfg.valid_w, sf,
                              float(cfg.mask_thr_binary))
    for b in range(B):
        n = int(counts[b])
        assert torch.equal(masks[b, :n], e.masks[b, :n]) and torch.equal(areas[b, :n], e.areas[b, :n]), b
    # tile filter + mask-NMS
    keep = e.op_tile_post(e.boxes[:B], e.labels[:B], e.areas[:B], counts, e.masks[:B], H, W, cfg.valid_h, cfg.valid_w, cfg.margin, cfg.min_area,
                          float(cfg.mask_nms_thr))
    for b in range(B):
        n = int(counts[b])
        assert torch.equal(keep[b, :n], e.keep[b, :n]), b
    print(f'engine path: {R} RoIs, detections per tile {counts.tolist()}, kept {[int(e.keep[b, :int(counts[b])].sum()) for b in range(B)]}')
    e.close()


# ================================================================================================================ refusals
@pytest.mark.gpu
def test_refusals_leave_the_engine_usable(eng):
    """Null pointers, nc + 6 > 64, nc + 2 > 16, max_keep > 2048, W % 32 != 0 and B > 256 are refused with an error and no launch; a good
    call afterwards gives the same bits as before."""
    from nuhtc_amd import hip
    from nuhtc_amd.engine import HipError
    # --- bbox tail
    c = tail_case(5, 5, 1, 0)
    good = [t.clone() for t in _run_tail(eng, c, 5, 1)]

    def tail_ok(label):
        for a, b in zip(_run_tail(eng, c, 5, 1), good):
            assert _same_bits(a, b), label
    for nc_bad in (15, 59):                                # nc + 2 > 16;  nc + 6 > 64 (and nc + 2 > 16)
        rng = np.random.default_rng(0)
        with pytest.raises(HipError):
            eng.op_bbox_tail(dev(c['h']), rng.standard_normal((nc_bad + 2, 256)), np.zeros(nc_bad + 2), c['rw'], c['rb'], dev(c['rois']), 5, c['stds'], (128, 128), 0)
        tail_ok(nc_bad)
    with pytest.raises(HipError):                          # more live rows than the buffers hold
        eng.op_bbox_tail(dev(c['h']), c['cw'], c['cb'], c['rw'], c['rb'], dev(c['rois']), 13, c['stds'], (128, 128), 0)
    tail_ok('r > cap')
    a = hip.BboxTailArgs(nc=5, cap=12)
    assert eng.lib.nuhtc_op_bbox_tail(eng.h, ctypes.byref(a), eng._stream()) == hip.E_INVALID
    assert eng.lib.nuhtc_op_bbox_tail(eng.h, None, eng._stream()) == hip.E_INVALID
    tail_ok('null')
    # --- det post
    cn = nms_case(['small', 'wide'])
    gd = _run_det_post(eng, cn, max_per_img=16)

    def det_ok(label):
        r = _run_det_post(eng, cn, max_per_img=16)
        assert all(_same_bits(r[k], gd[k]) for k in ('dets', 'labels', 'counts', 'mask_rois', 'det_off', 'det_total', 'cand_count')), label
    for label, kw in (('nc + 2 > 16', dict(nc=15)), ('max_per_img > 2048', dict(max_per_img=2049)), ('cap % 64', dict(cap=100)), ('cap > 16384', dict(cap=16448))):
        cc = dict(cn, nc=kw.get('nc', cn['nc']))
        with pytest.raises(HipError):
            _run_det_post(eng, cc, max_per_img=kw.get('max_per_img', 16), cap=kw.get('cap'))
        det_ok(label)
    big = dict(cn, off=np.zeros(257, np.int32), cnt=np.zeros(257, np.int32))
    with pytest.raises(HipError):                          # B > 256
        _run_det_post(eng, big, max_per_img=16)
    det_ok('B > 256')
    bad = dict(cn, cnt=cn['cnt'] + 1000)
    with pytest.raises(HipError):                          # roi_off + roi_cnt beyond the rows given
        _run_det_post(eng, bad, max_per_img=16)
    det_ok('counts beyond total')
    assert eng.lib.nuhtc_op_det_post(eng.h, ctypes.byref(hip.DetPostArgs(B=1, nc=5, cap=64, max_per_img=16)), eng._stream()) == hip.E_INVALID
    det_ok('null')
    # --- paste
    cp = paste_case(PASTE_GEOMS[2])
    gm, ga = _run_paste(eng, cp)

    def paste_ok(label):
        m, a = _run_paste(eng, cp)
        assert torch.equal(m, gm) and torch.equal(a, ga), label
    for label, kw in (('max_keep > 2048', dict(max_keep=2049)), ('W % 32', dict(W=48)), ('vW > W', dict(vW=65)), ('vH > H', dict(vH=65))):
        cc = dict(cp, **{k: v for k, v in kw.items() if k != 'max_keep'})
        with pytest.raises(HipError):
            eng.op_paste(dev(cc['prob']), dev(cc['mrois']), cc['off'], cc['counts'], kw.get('max_keep', 24), cc['H'], cc['W'], cc['vH'], cc['vW'], cc['scale'],
                         masks=torch.zeros(2, 24, 64, 2, dtype=torch.int32, device='cuda'), areas=torch.zeros(2, 24, dtype=torch.int32, device='cuda'))
        paste_ok(label)
    with pytest.raises(HipError):                          # B > 256
        eng.op_paste(dev(cp['prob']), dev(cp['mrois']), np.zeros(257, np.int32), np.zeros(257, np.int32), 1, 64, 64, 64, 64, 2.0,
                     masks=torch.zeros(257, 1, 64, 2, dtype=torch.int32, device='cuda'), areas=torch.zeros(257, 1, dtype=torch.int32, device='cuda'))
    with pytest.raises(HipError):                          # more detections than max_keep
        eng.op_paste(dev(cp['prob']), dev(cp['mrois']), cp['off'], cp['counts'], 8, 64, 64, 60, 50, 4.0,
                     masks=torch.zeros(2, 8, 64, 2, dtype=torch.int32, device='cuda'), areas=torch.zeros(2, 8, dtype=torch.int32, device='cuda'))
    assert eng.lib.nuhtc_op_paste(eng.h, ctypes.byref(hip.PasteArgs(B=1, D=1, max_keep=1, H=64, W=64, vH=64, vW=64)), eng._stream()) == hip.E_INVALID
    paste_ok('B > 256 / counts / null')
    # --- tile post
    pd, pl, pm, exp, geo = pinned_tile()
    gk = _run_tile_post(eng, [(pd, pl, pm)], 64, geo)
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device='cuda')
    for label, (B, K, W) in (('max_keep > 2048', (1, 2049, 128)), ('W % 32', (1, 64, 100)), ('B > 256', (257, 4, 128))):
        with pytest.raises(HipError):
            eng.op_tile_post(z(B, K, 5, dt=torch.float32), z(B, K), z(B, K), np.zeros(B, np.int32), z(B, K, 8, 4), 8, W, 8, min(W, 128), 2, 10, 0.05)
        assert (_run_tile_post(eng, [(pd, pl, pm)], 64, geo) == gk).all(), label
    with pytest.raises(HipError):                          # a count beyond max_keep
        eng.op_tile_post(z(1, 4, 5, dt=torch.float32), z(1, 4), z(1, 4), np.asarray([5], np.int32), z(1, 4, 8, 4), 8, 128, 8, 128, 2, 10, 0.05)
    assert eng.lib.nuhtc_op_tile_post(eng.h, ctypes.byref(hip.TilePostArgs(B=1, max_keep=4, H=8, W=128, vH=8, vW=128)), eng._stream()) == hip.E_INVALID
    assert (_run_tile_post(eng, [(pd, pl, pm)], 64, geo) == gk).all()


@pytest.mark.gpu
def test_print_observed_maxima():
    """Summary of the largest errors seen in this module beside their a-priori bounds (run with -s)."""
    print(f'bounds: TOL_TAIL {TOL_TAIL:.3e}, SCORE_REL {SCORE_REL:.3e}, box {BOX_C} u, paste band {PASTE_BAND:g}')
    for key, v in sorted(OBSERVED.items()):
        print(f'max {v:.3e}  {key}')


# ================================================================================================================ host-only self-tests
def test_references_vs_oracle():
    """The float64 references agree with oracle.model / oracle.ops_np (float32 torch) on random inputs."""
    from oracle import model as O
    from oracle import ops_np
    rng = np.random.default_rng(3)
    # delta2bbox
    xy = rng.uniform(-4, 200, (300, 2))
    rois = np.concatenate([xy, xy + rng.uniform(1, 80, (300, 2))], 1).astype(np.float32)
    d = (rng.standard_normal((300, 4)) * 12).astype(np.float32)
    o, t = ref_delta2bbox(rois, d, STDS[0], 256, 192)
    oo = O.delta2bbox(torch.from_numpy(rois), torch.from_numpy(d), STDS[0], (192, 256)).numpy()
    assert (np.abs(o - oo) <= 64 * U * t['geom'] + 1e-6).all() and (np.abs(t['dw']) > MAX_RATIO).any()
    # bbox head tail: the NormedLinear classifier of oracle.model.bbox_head
    h = np.abs(rng.standard_normal((40, 256))).astype(np.float32)
    cw, cb = rng.standard_normal((7, 256)).astype(np.float32), rng.standard_normal(7).astype(np.float32)
    rw, rb = rng.standard_normal((4, 256)).astype(np.float32), rng.standard_normal(4).astype(np.float32)
    cls, reg, mc, mr = ref_bbox_tail(h, cw, cb, rw, rb)
    tw, th = torch.from_numpy(cw), torch.from_numpy(h)
    ocls = torch.nn.functional.linear(th / (th.norm(dim=1, keepdim=True) + 1e-6) * 20, tw / (tw.norm(dim=1, keepdim=True) + 1e-6), torch.from_numpy(cb)).numpy()
    oreg = torch.nn.functional.linear(th, torch.from_numpy(rw), torch.from_numpy(rb)).numpy()
    assert (np.abs(cls - ocls) <= TOL_TAIL * mc).all() and (np.abs(reg - oreg) <= TOL_TAIL * mr).all()
    assert (np.abs(cls) <= mc + 1e-12).all() and (np.abs(reg) <= mr + 1e-12).all()
    # Seesaw scores and detect_post (which also exercises ops_np.batched_nms on the reference's own candidates)
    c = seesaw_case((40, 0, 70), seed=9)
    sc = ref_seesaw(c['cls'][0], c['cls'][1], c['cls'][2], 5)
    mean = (torch.from_numpy(c['cls'][0]) + torch.from_numpy(c['cls'][1]) + torch.from_numpy(c['cls'][2]))[:, :7] / 3.0
    osc = O.seesaw_scores(mean).numpy()
    assert np.abs(sc - osc[:, :5]).max() <= 4 * SCORE_REL
    exp, _ = seesaw_expect(c, PLACED_THR)
    for b in (0, 2):
        sl = slice(int(c['off'][b]), int(c['off'][b]) + int(c['cnt'][b]))
        assert abs(O.STAGE_STDS[2][0] - c['stds'][0]) < 1e-9
        dets, lab = O.detect_post(torch.from_numpy(c['rois'][sl, 1:]), mean[sl], torch.from_numpy(c['reg2'][sl]), c['img_hw'], 2.0, score_thr=PLACED_THR, iou=0.5)
        e = exp[b]
        d5, keep = ops_np.batched_nms(e['box'].astype(np.float32), e['score'].astype(np.float32), e['cls'], 0.5)
        assert len(dets) == len(d5) and np.abs(dets.numpy() - d5).max() <= 1e-3 and (lab.numpy() == e['cls'][keep]).all()
    # paste: oracle.model.paste_masks pastes into an H x W canvas (valid = whole canvas)
    pc = paste_case((64, 64, 64, 64, 2.0), seed=4)
    prob = np.nan_to_num(pc['prob'], nan=0.3)
    ref, vals, hull = ref_paste(prob, pc['boxes'], 64, 64, 64, 64, 0.5)
    om, ov = O.paste_masks(torch.from_numpy(prob)[:, None], torch.from_numpy(pc['boxes'].astype(np.float32)), 64, 64, return_values=True)
    diff = om != ref
    fin = np.isfinite(vals) & np.isfinite(ov)
    assert not (diff & ~(np.abs(vals - 0.5) <= PASTE_BAND)).any()
    assert np.abs(vals - ov)[fin & hull].max() <= 2e-5
    # tile filter + mask-NMS: distinct scores, so every sort agrees
    d, l, m = blob_tile(120, 30, 8, H=64, W=64, vH=64, vW=64, min_area=4)
    keep, nf = ref_tile_post(d, l, m, 64, 64, 2, 4, 0.05)
    bbox_res = [d[l == k] for k in range(5)]
    segm_res = [[m[j] for j in range(len(d)) if l[j] == k] for k in range(5)]
    kb, kl, km = O.tile_filter_and_mask_nms(bbox_res, segm_res, size=64, margin=2, min_area=4, thr=0.05)
    assert nf == 120 and len(kb) == keep.sum() and 0 < keep.sum() < nf
    assert set(map(tuple, kb.tolist())) == set(map(tuple, d[keep == 1].tolist()))


def test_paste_reference_vs_naive_loop():
    """ref_paste against a direct per-pixel loop."""
    pc = paste_case((64, 64, 60, 50, 4.0), seed=6)
    sel = [0, 2, 4, 5, 6, 8, 10, 12, 14, 16, 19, len(pc['boxes']) - 2]
    prob, boxes = pc['prob'][sel].astype(np.float64), pc['boxes'][sel]
    ref, vals, hull = ref_paste(prob, boxes, 64, 64, 60, 50, 0.5)

    def coord(p, lo, hi):
        with np.errstate(all='ignore'):
            g = np.float64(p + 0.5 - lo) / np.float64(hi - lo) * 2 - 1
        g = 0.0 if np.isinf(g) else g
        return ((g + 1) * 28 - 1) / 2
    for d, (x0, y0, x1, y1) in enumerate(boxes):
        for y in range(64):
            for x in range(64):
                inh = max(np.floor(x0) - 1, 0) <= x < min(np.ceil(x1) + 1, 50) and max(np.floor(y0) - 1, 0) <= y < min(np.ceil(y1) + 1, 60)
                assert hull[d, y, x] == inh
                if not inh:
                    assert not ref[d, y, x]
                    continue
                ix, iy = coord(x, x0, x1), coord(y, y0, y1)
                if np.isnan(ix) or np.isnan(iy):
                    assert np.isnan(vals[d, y, x]) and not ref[d, y, x]
                    continue
                v = 0.0
                for yy in (int(np.floor(iy)), int(np.floor(iy)) + 1):
                    for xx in (int(np.floor(ix)), int(np.floor(ix)) + 1):
                        if 0 <= yy < 28 and 0 <= xx < 28:
                            v += prob[d, yy, xx] * (1 - abs(ix - xx)) * (1 - abs(iy - yy))
                assert (np.isnan(v) and np.isnan(vals[d, y, x])) or abs(v - vals[d, y, x]) <= 1e-12, (d, y, x)
                assert ref[d, y, x] == (v >= 0.5)


def test_tile_post_reference_vs_naive_loop():
    """ref_tile_post against a double loop over masks, including the pinned tile's designed verdicts."""
    def naive(d, l, m, vH, vW, mg, mina, thr):
        n = len(d)
        cm = sorted(range(n), key=lambda i: (l[i], i))
        cand = [i for i in cm if d[i, 0] >= mg and d[i, 1] >= mg and d[i, 2] <= vW - mg and d[i, 3] <= vH - mg and m[i].sum() >= mina]
        asc = sorted(range(len(cand)), key=lambda k: (d[cand[k], 4], k))          # stable ascending
        order = [cand[k] for k in asc[::-1]]
        keep, sup = np.zeros(n, np.uint8), set()
        for a, i in enumerate(order):
            if i in sup:
                continue
            keep[i] = 1
            for j in order[a + 1:]:
                inter, uni = int((m[i] & m[j]).sum()), int((m[i] | m[j]).sum())
                if uni > 0 and inter / uni > thr:
                    sup.add(j)
        return keep, len(cand)
    d, l, m = blob_tile(90, 20, 21, H=64, W=64, vH=60, vW=56, min_area=4)
    assert (ref_tile_post(d, l, m, 60, 56, 2, 4, 0.05)[0] == naive(d, l, m, 60, 56, 2, 4, 0.05)[0]).all()
    pd, pl, pm, exp, geo = pinned_tile()
    keep, nf = ref_tile_post(pd, pl, pm, geo['vH'], geo['vW'], geo['margin'], geo['min_area'], 0.05)
    assert (keep == naive(pd, pl, pm, geo['vH'], geo['vW'], geo['margin'], geo['min_area'], 0.05)[0]).all()
    assert all(keep[s] == f for s, f in exp.items()), [(s, int(keep[s]), f) for s, f in exp.items() if keep[s] != f]
    # the pinned pairs are what they claim
    inter = lambda a, b: int((pm[a] & pm[b]).sum())
    union = lambda a, b: int((pm[a] | pm[b]).sum())
    assert (inter(0, 1), union(0, 1)) == (1, 20) and (inter(2, 3), union(2, 3)) == (2, 39)
    assert pm[4].sum() == 9 and pm[5].sum() == 10
    # every mask lies inside the integer hull of its box (the kernel's precondition)
    for dd, mm in ((pd, pm), (d, m)):
        for j in range(len(dd)):
            ys, xs = np.nonzero(mm[j])
            assert xs.min() >= np.floor(dd[j, 0]) - 1 and xs.max() < np.ceil(dd[j, 2]) + 1 and ys.min() >= np.floor(dd[j, 1]) - 1 and ys.max() < np.ceil(dd[j, 3]) + 1


def test_designed_inputs_have_the_claimed_properties():
    """No reference score within the margin of the threshold (placed rows aside); the threshold-band share of every paste case under its
    cap; the filtered counts of the blob lists as stated; the class-offset pairs tell a per-tile offset from a batch-wide one."""
    for counts in SEESAW_COUNTS:
        no_cand = int(np.argmin(counts))                   # the tile with the fewest RoIs (0 or 1): no candidate at all
        c = seesaw_case(counts, seed=sum(counts), no_cand_tile=no_cand)
        exp, sc = seesaw_expect(c, PLACED_THR)
        assert not ((np.abs(sc - PLACED_THR) < SCORE_MARGIN).any(1) & ~c['placed']).any()
        assert np.abs(c['cls']).max() <= L_MAX
        rows = np.nonzero(c['placed'])[0]
        assert len(rows) >= 2 and (np.abs(sc[rows] - 0.1) < 1e-15).all() and np.float32(0.1) == np.float32(PLACED_THR)
        assert len(exp[no_cand]['roi']) == 0 and all(len(exp[b]['roi']) > 0 for b in range(3) if b != no_cand and counts[b] > 1)
        assert c['off'][1] != c['cnt'][0] and (c['off'][1:] >= c['off'][:-1] + c['cnt'][:-1]).all()
    for geom in PASTE_GEOMS:
        pc = paste_case(geom)
        ref, vals, hull = ref_paste(pc['prob'], pc['boxes'], pc['H'], pc['W'], pc['vH'], pc['vW'], 0.5)
        band = _paste_band(vals, hull, 0.5)
        assert band.sum() <= PASTE_BAND_SHARE * hull.sum() and hull.sum() > 3000 and ref.sum() > 1000, (geom, int(band.sum()), int(hull.sum()))
        fin = pc['prob'][np.isfinite(pc['prob'])]
        assert (np.abs(fin - 0.5) >= 0.1 - 1e-6).all()
    for boxes in (const_boxes(),):
        wh = np.concatenate([boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]])
        assert (np.log2(wh) % 1 == 0).all() and (boxes * 4 % 1 == 0).all()
    lists, low, refs_nf = blob_lists_and_refs()
    for k, (d, l, m) in lists.items():
        keep, nf = refs_nf[k]
        assert nf == k and len(d) > k and 0 < keep.sum() < nf and len(d) <= 2048
        assert len(np.unique(d[:, 4])) == len(d)
    assert (np.delete(lists[513][0], low, 0) == lists[511][0]).all() and lists[513][0][low, 4].max() < np.delete(lists[513][0][:, 4], low).min()
    # class-offset pairs of the NMS design
    c = nms_case(['small', 'wide', 'many'])
    tiles = nms_tiles()
    boxes = np.asarray([b for b, sc in tiles['small'] for k in sorted(sc) if sc[k] > 0.05], np.float32)
    ids = np.asarray([k for b, sc in tiles['small'] for k in sorted(sc) if sc[k] > 0.05])
    scores = np.asarray([sc[k] for b, sc in tiles['small'] for k in sorted(sc) if sc[k] > 0.05], np.float32)
    wide_max = max(float(b.max()) for b, _ in tiles['wide'])
    assert wide_max >= 4 * boxes.max() - 1e-3 and (boxes * 2 ** 17 % 1 == 0).all()
    own, other = offset_verdicts(boxes, scores, ids, boxes.max()), offset_verdicts(boxes, scores, ids, wide_max)
    assert set(own.tolist()) != set(other.tolist())
    assert (c['rois'][:, 1:] * 2 ** 16 % 1 == 0).all() and np.abs(c['rois'][:, 1:]).max() < 256
