"""The block of the path that turns RoIs into head features, op by op, on placed boxes: roi_classify_kernel, the two LDS-tile kernels,
roi_feat7_stream_kernel / roi_feat7_stream_few_kernel, roi_feat7_big_kernel and its combine kernel, roi_feat7_giant_kernel, roi_feat14_kernel
and the three routes that build the attention-pool tables G2 / G3 (csrc/roi.hip, csrc/roi_engine.hip).

Engine.op_attn_pool / op_roi_feats (nuhtc_op_*) fill the parameter block run_roi_path fills and call the same functions
(test_ops_are_the_engines_path shows it bit for bit), so a box can be PLACED: on a threshold of the classifier, on a border of the map, with
zero width, with its G centre on a cell edge.  The maps are i.i.d. normal (and offset / mixed-magnitude / zero-channel / index-probe
variants), not the smooth FPN maps of synthetic tiles: a wrong tap, weight, row pitch or table entry is an error of order 0.1 here.

The reference (ref_feats) is numpy.  Geometry -- box scaling, bin sizes, adaptive sample counts, sample coordinates, the validity test,
clamps, tap indices and the bilinear weights hy * hx .. -- is float32 in the expression sequence of roi_geom / roi_bin / make_tap, which is
mmcv's own float arithmetic (roi.hip is compiled with -ffp-contract=off for it).  Values and every sum are float64.  The semantic term is
RoIAlign(14, sampling_ratio 0) average-pooled 2 x 2 for the 7 x 7 features; the G centre is floor((a + b) / (2 stride)) in float32, clamped.

Tolerance, first order in u = 2^-24 and derived here (nothing below was measured):  |got - ref| <= C u mag.
  mag   = the float64 sum of |w v| / count over every tap of the three maps + |G2| + |G3|  (per output element)
  C     = the longest chain of roundings a term passes through in the kernel form the box took (fb_flag):
    LDS tiles (flag 0 / 3, and the one-sample form of the 14 x 14 kernel): product 1, the 4-tap sum 3, the sample sum 4, the division 1,
      the four adds of the two maps and two tables 4, interpolating float32(x0 + sem) instead of the two maps 1            -> C_LDS = 14
    gather forms (giant, flag 4; the 14 x 14 gather form): product 1, 4-tap sum 3, gw * gh sample adds, division 1, the 4 adds of the
      pooled semantic bins (x 0.25 is exact), 3 adds of maps / tables, float32(x0 + sem) 1                                 -> 13 + gw gh
    stream kernels (flag 1): the reference weight hy * hx itself 1; merged x weights: a sum of <= 2 * 4 non-negative terms 7, / Sx 1;
      merged y weights the same 8; the x contraction: an fma chain over SM_J = 5 taps 5; the 49 accumulators run through the rows of all
      three maps: 3 * SM_FH = 96 fma steps; the table sum 1 and its add 1; float32(x0 + sem) 1                             -> C_STREAM = 122
    big-box kernel (flag 2): weight 1; merged weights 2 * (2 * 24 - 1 + 1) = 96; two interleaved fma chains over BG_J = 40 taps and their
      add 21; a row split's BG_FH / 2 = 132 fma steps; the split partial 1; the maps 3; the tables 2; float32(x0 + sem) 1   -> C_BIG = 257
The semantic sample points.  mmcv takes the semantic samples on the 14-grid; the LDS, stream and big-box forms take them on the 7-grid (one
interpolation of x0 + sem at the 2 x 2 points of the 7-grid bins, or 2 g samples per 7-grid bin with bin size 2 bw14).  The points are the
same real numbers, but the two float32 expressions differ by a few ulp of the coordinate, which moves a sample on an i.i.d. map by far more
than C u mag.  So the bound above is held against the reference evaluated at the KERNEL FORM'S OWN float32 points (`val7`: same taps rule,
same float32 weights hy * hx, float64 sums), and the distance between the two references is bounded apart, on the CPU
(test_semantic_grids_agree): each float32 form is within 7 u cmax of the real point (bin size 1, pb * bs 2 in all, the partial sum 1,
(i + 0.5) bs / g 3, the final add 1; cmax = |start| + |side| on the stride-4 map bounds every intermediate), so the forms differ by <=
K_COORD = 14 u cmax per axis; bilinear interpolation is continuous with a slope of at most the largest difference D of adjacent pixels over
the footprint grown by one pixel: |val7 - val14| <= K_COORD u cmax D.  The giant and 14 x 14 forms evaluate mmcv's own expression and are
held to the mmcv-grid reference.  The form a 14 x 14 box takes (LDS or gather) is INFERRED from the reference's footprints -- the kernel
reports none; for one sample per bin both constants are 14.
test_print_observed_maxima prints the observed err / (u mag) per kernel form beside its C."""
import ctypes

import numpy as np
import pytest
import torch

U = 2.0 ** -24
F32 = np.float32
SENTINEL = 0x7fc0dead
SENT_U8 = 0xA5
C_LDS, C_STREAM, C_BIG, K_COORD = 14, 122, 257, 14
TP0, TP1, TS0, TS1, SM_MAXSIDE, BG_S, BG_FH, BG_J, SMF_MAX, BIG_SPLIT_MAX = 12, 7, 8, 5, 112.0, 24, 264, 40, 1024, 512
TAU = 0.25
OBSERVED = {}


def _obs(key, v):
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), float(v))


# ================================================================================================================ reference
def geom(roi, scale, P, sr):
    """roi_geom in float32 -> (x1, y1, bw, bh, gw, gh, rw, rh)."""
    s, h = F32(scale), F32(0.5)
    x1, y1 = F32(roi[1]) * s - h, F32(roi[2]) * s - h
    x2, y2 = F32(roi[3]) * s - h, F32(roi[4]) * s - h
    rw, rh = F32(x2 - x1), F32(y2 - y1)
    bw, bh = F32(rw / F32(P)), F32(rh / F32(P))
    gw = sr if sr > 0 else int(np.ceil(bw))
    gh = sr if sr > 0 else int(np.ceil(bh))
    return x1, y1, bw, bh, gw, gh, rw, rh


def axis_samples(start, bs, P, g, size):
    """The P * g samples of one axis: mmcv's coordinate and axis part of bilinear_interpolate, float32 -> valid, lo, hi, l, h."""
    n = P * g
    pb, i = (np.arange(n) // g).astype(F32), (np.arange(n) % g).astype(F32)
    c = (F32(start) + pb * F32(bs)) + ((i + F32(0.5)) * F32(bs)) / F32(g)
    assert c.dtype == F32
    valid = ~((c < F32(-1.0)) | (c > F32(size)))
    c = np.where(valid, c, F32(0))
    c = np.where(c <= 0, F32(0), c)
    lo = c.astype(np.int32)
    top = lo >= size - 1
    lo = np.where(top, size - 1, lo)
    hi = np.where(top, size - 1, lo + 1)
    c = np.where(top, lo.astype(F32), c)
    l = (c - lo.astype(F32)).astype(F32)
    h = (F32(1.0) - l).astype(F32)
    return valid, lo, hi, l, h


def ref_roi_align(fm, roi, scale, P, sr, grid=None):
    """RoIAlign (avg, aligned) of one box on fm (H, W, C) float32 -> (value, mag) (P, P, C) float64 and the footprint (fx0, fx1, fy0, fy1) or None.
    grid = (bw, bh, gw, gh): bin sizes and sample counts given instead of derived (the 7-grid form of the semantic term)."""
    H, W, C = fm.shape
    x1, y1, bw, bh, gw, gh, _, _ = geom(roi, scale, P, sr)
    if grid is not None:
        bw, bh, gw, gh = grid
    if gw <= 0 or gh <= 0:
        return np.zeros((P, P, C)), np.zeros((P, P, C)), None
    vy, ylo, yhi, ly, hy = axis_samples(y1, bh, P, gh, H)
    vx, xlo, xhi, lx, hx = axis_samples(x1, bw, P, gw, W)
    ok = (vy[:, None] & vx[None, :]).astype(F32)
    w = [np.outer(a, b) * ok for a, b in ((hy, hx), (hy, lx), (ly, hx), (ly, lx))]
    assert all(t.dtype == F32 for t in w)
    f = fm.astype(np.float64)
    val = np.zeros((P * gh, P * gw, C))
    mag = np.zeros((P * gh, P * gw, C))
    for wt, yy, xx in zip(w, (ylo, ylo, yhi, yhi), (xlo, xhi, xlo, xhi)):
        t = wt.astype(np.float64)[:, :, None] * f[yy][:, xx]
        val += t
        mag += np.abs(t)
    cnt = float(gh * gw)
    val = val.reshape(P, gh, P, gw, C).sum((1, 3)) / cnt
    mag = mag.reshape(P, gh, P, gw, C).sum((1, 3)) / cnt
    fp = (int(xlo[vx].min()), int(xhi[vx].max()), int(ylo[vy].min()), int(yhi[vy].max())) if vx.any() and vy.any() else None
    return val, mag, fp


def g_cell(roi, stride, Hl, Wl):
    cx = np.floor((F32(roi[1]) + F32(roi[3])) / (F32(2.0) * F32(stride)))
    cy = np.floor((F32(roi[2]) + F32(roi[4])) / (F32(2.0) * F32(stride)))
    return int(min(max(cy, 0), Hl - 1)), int(min(max(cx, 0), Wl - 1))


def pool2(a):
    return a.reshape(7, 2, 7, 2, -1).mean((1, 3))


def ref_feats(m, roi, P):
    """The fused RoI feature of one box -> dict(val, mag (P, P, 64): mmcv's grids; val7, mag7: the semantic term at the 7-grid points; coord: the K_COORD term's cmax * D (64,), gs: the semantic grid's sample counts,
    fp0 / fp1: the footprints of the 7-grid (2 samples) on levels 0 / 1)."""
    b = int(roi[0])
    sr = 2 if P == 7 else 0
    a0, m0, fp0 = ref_roi_align(m['x0'][b], roi, 0.25, P, sr)
    a1, m1, fp1 = ref_roi_align(m['x1'][b], roi, 0.125, P, sr)
    s, ms, fps = ref_roi_align(m['sem'][b], roi, 0.25, 14, 0)
    if P == 7:
        s, ms = pool2(s), pool2(ms)
    y2, x2 = g_cell(roi, 16, *m['G2'].shape[1:3])
    y3, x3 = g_cell(roi, 32, *m['G3'].shape[1:3])
    g2, g3 = m['G2'][b, y2, x2].astype(np.float64), m['G3'][b, y3, x3].astype(np.float64)
    gx1, gy1, bw14, bh14, gw, gh, rw, rh = geom(roi, 0.25, 14, 0)
    s7, ms7 = s, ms
    if P == 7 and gw > 0 and gh > 0:         # the semantic term at the 7-grid points of the LDS / stream / big-box forms
        s7, ms7, _ = ref_roi_align(m['sem'][b], roi, 0.25, 7, 2) if (gw, gh) == (1, 1) else \
            ref_roi_align(m['sem'][b], roi, 0.25, 7, 0, grid=(F32(2.0) * bw14, F32(2.0) * bh14, 2 * gw, 2 * gh))
    coord = np.zeros(64)
    if fps is not None:
        H, W = m['sem'].shape[1:3]
        reg = m['sem'][b, max(fps[2] - 1, 0):min(fps[3] + 2, H), max(fps[0] - 1, 0):min(fps[1] + 2, W)].astype(np.float64)
        dx = np.abs(np.diff(reg, axis=1)).max((0, 1)) if reg.shape[1] > 1 else np.zeros(64)
        dy = np.abs(np.diff(reg, axis=0)).max((0, 1)) if reg.shape[0] > 1 else np.zeros(64)
        coord = (abs(float(gx1)) + abs(float(rw))) * dx + (abs(float(gy1)) + abs(float(rh))) * dy
    return dict(val=a0 + a1 + s + g2 + g3, mag=m0 + m1 + ms + np.abs(g2) + np.abs(g3), val7=a0 + a1 + s7 + g2 + g3, mag7=m0 + m1 + ms7 + np.abs(g2) + np.abs(g3), coord=coord, gs=(gw, gh), fp0=fp0, fp1=fp1, cells=((y2, x2), (y3, x3)))


def _fwh(fp):
    return (0, 0) if fp is None else (fp[1] - fp[0] + 1, fp[3] - fp[2] + 1)


def expected_flag(roi, r):
    """The class roi_classify_kernel must give, from the reference's footprints and sample counts."""
    gw, gh = r['gs']
    (fw0, fh0), (fw1, fh1) = _fwh(r['fp0']), _fwh(r['fp1'])
    rwn, rhn = F32(roi[3]) - F32(roi[1]), F32(roi[4]) - F32(roi[2])
    if gw == 1 and gh == 1 and fw0 <= TP0 and fh0 <= TP0 and fw1 <= TP1 and fh1 <= TP1:
        return 0 if fw0 <= TS0 and fh0 <= TS0 and fw1 <= TS1 and fh1 <= TS1 else 3
    if gw <= 2 and gh <= 2 and rwn <= SM_MAXSIDE and rhn <= SM_MAXSIDE:
        return 1
    if 2 * gw > BG_S or 2 * gh > BG_S or rhn * F32(0.25) + F32(4) > BG_FH or rwn * F32(0.25) / F32(7) + F32(3) > BG_J:
        return 4
    return 2


def tolerance(r, flag, P):
    """-> (C, the name of the kernel form, the reference value and magnitude that form is held to)."""
    gw, gh = r['gs']
    if P == 14:
        lds = gw == 1 and gh == 1 and _fwh(r['fp0'])[0] <= TP0 and _fwh(r['fp0'])[1] <= TP0 and _fwh(r['fp1'])[0] <= TP1 and _fwh(r['fp1'])[1] <= TP1
        return (C_LDS if lds else 13 + max(gw * gh, 1)), 'P14 lds' if lds else 'P14 gather', r['val'], r['mag']
    if flag == 4:
        return 13 + max(gw * gh, 4), 'P7 flag 4', r['val'], r['mag']
    return {0: C_LDS, 3: C_LDS, 1: C_STREAM, 2: C_BIG}[flag], f'P7 flag {flag}', r['val7'], r['mag7']


def naive_roi_align(fm, roi, scale, P, sr, chans):
    """mmcv's sample loop, one sample at a time (roi_bin / make_tap), float32 geometry and float64 sums, on a few channels."""
    H, W, _ = fm.shape
    x1, y1, bw, bh, gw, gh, _, _ = geom(roi, scale, P, sr)
    out = np.zeros((P, P, len(chans)))
    for ph in range(P):
        for pw in range(P):
            acc = np.zeros(len(chans))
            for iy in range(gh):
                y = F32(F32(y1 + F32(ph) * bh) + F32(F32(F32(iy) + F32(0.5)) * bh) / F32(gh))
                for ix in range(gw):
                    x = F32(F32(x1 + F32(pw) * bw) + F32(F32(F32(ix) + F32(0.5)) * bw) / F32(gw))
                    if y < -1.0 or y > H or x < -1.0 or x > W:
                        continue
                    yy, xx = max(y, F32(0)), max(x, F32(0))
                    yl, xl = int(yy), int(xx)
                    if yl >= H - 1:
                        yh = yl = H - 1
                        yy = F32(yl)
                    else:
                        yh = yl + 1
                    if xl >= W - 1:
                        xh = xl = W - 1
                        xx = F32(xl)
                    else:
                        xh = xl + 1
                    ly, lx = F32(yy - F32(yl)), F32(xx - F32(xl))
                    hy, hx = F32(F32(1) - ly), F32(F32(1) - lx)
                    for wt, a, c in ((F32(hy * hx), yl, xl), (F32(hy * lx), yl, xh), (F32(ly * hx), yh, xl), (F32(ly * lx), yh, xh)):
                        acc += float(wt) * fm[a, c, chans].astype(np.float64)
            out[ph, pw] = acc / max(gh * gw, 1)
    return out


def ref_attn_pool(Fm, tau):
    """G[b, q] = mean_p F[b, p] (relu(cos(F[b, q], F[b, p]) - tau) + tau) in float64, and the per-pair cosines."""
    f = Fm.astype(np.float64)
    n = np.maximum(np.sqrt((f * f).sum(-1)), 1e-8)
    cos = np.einsum('bqc,bpc->bqp', f / n[..., None], f / n[..., None])
    sim = np.maximum(cos - tau, 0) + tau
    return np.einsum('bqp,bpc->bqc', sim, f) / f.shape[1], np.einsum('bqp,bpc->bqc', sim, np.abs(f)) / f.shape[1], cos


# ================================================================================================================ maps and boxes
SHAPES = {'a': (2, [(64, 64), (32, 32), (16, 16), (8, 8)]), 'b': (3, [(50, 34), (25, 17), (13, 9), (7, 5)]), 'c': (1, [(256, 256), (128, 128), (64, 64), (32, 32)])}
_CTX = {}


def probe(B, H, W):
    """value = c + 64 (x + W (y + H b)): (b, y, x, c) exactly in float32 (below 2^24 for every shape here)."""
    b, y, x, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(64), indexing='ij')
    v = c + 64 * (x + W * (y + H * b))
    assert v.max() < 2 ** 24
    return v.astype(F32)


def make_maps(shape, kind):
    """kind 'normal': i.i.d. normal; 'hard': x0 a large offset plus a small signal, x1 mixed magnitudes over six decades, channel 7 exactly zero
    everywhere and channel 5 of sem too; 'probe': index-probe maps.  The G tables are random inputs (their values are tested by the attention-pool tests)."""
    key = (shape, kind)
    if key in _CTX:
        return _CTX[key]
    B, lv = SHAPES[shape]
    rng = np.random.default_rng(['a', 'b', 'c'].index(shape) * 10 + ['normal', 'hard', 'probe'].index(kind))
    n = lambda l: rng.standard_normal((B,) + lv[l] + (64,)).astype(F32)
    m = dict(x0=n(0), x1=n(1), sem=n(0), G2=n(2), G3=n(3))
    if kind == 'hard':
        m['x0'] = (F32(1000.0) + F32(1e-2) * m['x0']).astype(F32)
        m['x1'] = (m['x1'] * (10.0 ** rng.uniform(-3, 3, m['x1'].shape)).astype(F32)).astype(F32)
        for k in ('x0', 'x1', 'sem', 'G2', 'G3'):
            m[k][..., 7] = 0
        m['sem'][..., 5] = 0
    elif kind == 'probe':
        m['x0'], m['x1'], m['sem'] = probe(B, *lv[0]), probe(B, *lv[1]) * F32(0.5), probe(B, *lv[0]) * F32(0.25)
    m['x0sem'] = (m['x0'] + m['sem']).astype(F32)
    m['B'], m['img'] = B, (lv[0][0] * 4, lv[0][1] * 4)
    _CTX[key] = m
    return m


def box(b, x, y, w, h):
    return [float(b), x, y, x + w, y + h]


def boxes_adaptive():
    """group 1 -> {shape: [(roi, (gw, gh), flag)]}: the semantic sample count and the class on either side of 56, 112 and 672 px, crossed on x, on y, on both."""
    out = {'a': [], 'c': []}
    for lo, hi, glo, ghi, shape, x0 in ((56.0, 56.125, 1, 2, 'a', 24.0), (112.0, 112.125, 2, 3, 'a', 40.0), (672.0, 672.125, 12, 13, 'c', 100.0)):
        for w, h in ((lo, lo), (hi, lo), (lo, hi), (hi, hi)):
            g = (glo if w == lo else ghi, glo if h == lo else ghi)
            big = max(w, h)
            flag = 1 if big <= 112.0 else 2 if big <= 672.0 else 4
            out[shape].append((box(0, x0, x0 + 8.0, w, h), g, flag))
    for (w, h), g in (((40.0, 100.0), (1, 2)), ((100.0, 40.0), (2, 1))):
        out['a'].append((box(1, 16.0, 24.0, w, h), g, 1))
    for (w, h), g in (((40.0, 300.0), (1, 6)), ((300.0, 40.0), (6, 1)), ((100.0, 700.0), (2, 13)), ((700.0, 100.0), (13, 2))):
        out['c'].append((box(0, 60.0, 90.0, w, h), g, 4 if max(g) > 12 else 2))
    return out


def boxes_footprint(img_hw):
    """group 2: 24-px and 44-px boxes at the 8 x 8 alignments to the stride-8 pixel grid (which hold the 4 x 4 of stride 4)."""
    rois = []
    for side in (24.0, 44.0):
        for ay in range(8):
            for ax in range(8):
                rois.append(box((ax + ay) % 2, 40.0 + ax, 48.0 + ay, side, side))
    return rois


def boxes_border(H, W, b=0):
    """group 3 on an image of H x W network pixels."""
    r = [box(b, W - 30.0, H - 40.0, 30.0, 40.0), box(b, W - 3.0, H - 2.0, 2.0, 1.0), box(b, W - 1.0, H - 1.0, 1.0, 1.0), box(b, 0.0, 0.0, 1.0, 1.0),
         box(b, -10.0, 20.0, 30.0, 30.0), box(b, 20.0, -10.0, 30.0, 30.0), box(b, W - 20.0, 20.0, 30.0, 30.0), box(b, 20.0, H - 20.0, 30.0, 30.0),
         box(b, -20.0, -20.0, W + 40.0, H + 40.0) if max(H, W) + 40 <= 672 else box(b, -20.0, -20.0, 100.0, 100.0),
         box(b, 8.0, -4.0, 56.0, 56.0), box(b, 8.0, -4.5, 56.0, 56.5), box(b, 8.0, H - 52.0, 56.0, 56.0), box(b, 8.0, H - 52.0, 56.0, 56.5),
         box(b, -4.0, 8.0, 56.0, 56.0), box(b, W - 52.0, 8.0, 56.5, 56.0),
         box(b, -80.0, 10.0, 40.0, 40.0), box(b, W + 30.0, 10.0, 40.0, 40.0), box(b, 10.0, -90.0, 60.0, 60.0), box(b, 10.0, H + 30.0, 20.0, 20.0),
         box(b, -300.0, -300.0, 200.0, 200.0)]
    return r


def boxes_degenerate(shape):
    """group 4: zero width, zero height, both, interior and border, the other side in each range; sub-pixel boxes."""
    H, W = [4 * v for v in SHAPES[shape][1][0]]
    sides = (40.0, 100.0) + ((300.0, 700.0) if shape == 'c' else ())
    r = []
    for s in sides:
        for x, y in ((24.0, 16.0), (0.0, 0.0), (float(W), 8.0), (8.0, float(H))):
            r += [box(0, x, y, 0.0, s), box(0, y, x, s, 0.0)]
    r += [box(0, 24.0, 24.0, 0.0, 0.0), box(0, 0.0, 0.0, 0.0, 0.0), box(0, float(W), float(H), 0.0, 0.0)]
    for s in (0.125, 1.0, 3.0):
        r += [box(0, 33.0, 21.0, s, s), box(0, 33.5, 21.25, s, 3.0)]
    return r


def boxes_degenerate_lists():
    """Zero width, zero height and both for the list forms: the other side <= 112 px (stream class; adaptive counts (0, 0), (0, 1), (1, 0), (0, 2),
    (2, 0)) and in (112, 672] px (big-box class) -> (stream boxes, big boxes)."""
    mid, big = [box(0, 60.0, 70.0, 0.0, 0.0), box(1, 0.0, 256.0, 0.0, 0.0)], []
    for k, s_ in enumerate((40.0, 56.0, 100.0, 112.0)):
        mid += [box(k % 2, 30.0 + k, 20.0, 0.0, s_), box(k % 2, 20.0, 30.0 + k, s_, 0.0), box(1, 256.0, 8.0 * k, 0.0, s_), box(0, 8.0 * k, 0.0, s_, 0.0)]
    for k, s_ in enumerate((112.125, 150.0, 200.0, 280.0)):
        big += [box(k % 2, 30.0 + k, 10.0, 0.0, s_), box(k % 2, 10.0, 30.0 + k, s_, 0.0), box(1, 256.0, -20.0, 0.0, s_), box(0, -20.0, 0.0, s_, 0.0)]
    return mid, big


def boxes_mid(n, rng, H, W, B):
    """mid-size boxes (stream class): sides 57 .. 112 px, dyadic coordinates."""
    wh = rng.integers(57 * 8, 112 * 8 + 1, (n, 2)) / 8.0
    xy = rng.integers(-8 * 8, (min(H, W) - 60) * 8, (n, 2)) / 8.0
    return [box(int(rng.integers(0, B)), xy[i, 0], xy[i, 1], wh[i, 0], wh[i, 1]) for i in range(n)]


def boxes_big(n, rng, H, W, B):
    wh = rng.integers(113 * 8, (max(H, W) + 30) * 8, (n, 2)) / 8.0
    xy = rng.integers(-20 * 8, 100 * 8, (n, 2)) / 8.0
    return [box(int(rng.integers(0, B)), xy[i, 0], xy[i, 1], wh[i, 0], wh[i, 1]) for i in range(n)]


# ================================================================================================================ CPU cross-checks
def test_reference_matches_oracle():
    """ref_feats against oracle.model.bbox_feats (P = 7) and roi_extract + semantic_roi (P = 14), the tables from oracle.model.attention_pool: the
    oracle is float32 and sums in another order, so the agreement is held to 1e-5 (1 + mag) -- what this pins is the semantics."""
    from oracle import model as O
    B, lv = 2, [(24, 20), (12, 10), (6, 5), (3, 3)]
    rng = np.random.default_rng(3)
    x = [rng.standard_normal((B,) + s + (64,)).astype(F32) for s in lv]
    sem = rng.standard_normal((B,) + lv[0] + (64,)).astype(F32)
    G = [ref_attn_pool(x[l].reshape(B, -1, 64), O.ATT_THRES)[0].reshape(x[l].shape).astype(F32) for l in (2, 3)]
    m = dict(x0=x[0], x1=x[1], sem=sem, G2=G[0], G3=G[1])
    rois = np.asarray([box(0, 10.0, 12.0, 20.0, 24.0), box(1, 3.5, 7.25, 50.0, 61.0), box(0, -6.0, 30.0, 40.0, 70.0), box(1, 20.0, 20.0, 0.0, 30.0),
                       box(0, 60.0, 70.0, 30.0, 40.0), box(1, 0.0, 0.0, 80.0, 96.0), box(0, 5.0, 5.0, 0.125, 1.0)], F32)
    nchw = lambda a: torch.from_numpy(a).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        o7 = O.bbox_feats([nchw(a) for a in x], nchw(sem), torch.from_numpy(rois)).permute(0, 2, 3, 1).numpy()
        o14 = (O.roi_extract([nchw(a) for a in x], torch.from_numpy(rois), 14, 0) + O.semantic_roi(nchw(sem), torch.from_numpy(rois))).permute(0, 2, 3, 1).numpy()
    for i, roi in enumerate(rois):
        for P, o in ((7, o7), (14, o14)):
            r = ref_feats(m, roi, P)
            assert (np.abs(r['val'] - o[i]) <= 1e-5 * (1 + r['mag'])).all(), (i, P, np.abs(r['val'] - o[i]).max())


def test_reference_matches_naive_sample_loop():
    rng = np.random.default_rng(4)
    fm = rng.standard_normal((17, 13, 64)).astype(F32)
    ch = [0, 31, 63]
    for roi in (box(0, 10.0, 12.0, 20.0, 24.0), box(0, -7.5, -3.0, 30.0, 90.0), box(0, 40.0, 50.0, 30.0, 30.0), box(0, 8.0, -4.0, 56.0, 56.0), box(0, 5.0, 5.0, 0.0, 9.0)):
        for P, sr, sc in ((7, 2, 0.25), (14, 0, 0.25), (7, 2, 0.125), (14, 0, 0.125)):
            v, mag, _ = ref_roi_align(fm, roi, sc, P, sr)
            nv = naive_roi_align(fm, roi, sc, P, sr, ch)
            assert (np.abs(v[..., ch] - nv) <= 1e-12 * (1 + mag[..., ch])).all(), (roi, P, sr, sc)


def test_semantic_grids_agree():
    """The semantic term at the 7-grid points (what the LDS, stream and big-box forms evaluate) against mmcv's 14-grid, reference against reference:
    |val7 - val| <= K_COORD u cmax D (module docstring), on the designed boxes of shape (a) and on random lists."""
    m = make_maps('a', 'normal')
    rng = np.random.default_rng(2)
    rois = [r[0] for r in boxes_adaptive()['a']] + boxes_footprint(m['img'])[::5] + boxes_degenerate('a') + boxes_border(256, 256) + \
        boxes_mid(20, rng, 256, 256, 2) + boxes_big(20, rng, 256, 256, 2) + sum(boxes_degenerate_lists(), [])
    worst = 0.0
    for roi in rois:
        r = ref_feats(m, np.asarray(roi, F32), 7)
        d = np.abs(r['val7'] - r['val'])
        bound = K_COORD * U * r['coord'][None, None] + 1e-13 * r['mag']
        assert (d <= bound).all(), (roi, d.max(), bound.min())
        if 0 in r['gs']:
            assert not d.any()
        worst = max(worst, float((d / np.maximum(U * r['mag'], 1e-300)).max()))
    print(f'7-grid against 14-grid semantic term: up to {worst:.0f} u mag apart')
    assert worst > C_LDS                               # the reason the kernel forms are held to their own points


def test_designed_boxes_have_their_properties():
    """Sample counts and classes of group 1, the three LDS / stream classes of group 2, the valid / invalid first sample row of group 3, the
    zero sample counts of group 4, the G cells of group 5 -- from the reference alone."""
    for shape, rows in boxes_adaptive().items():
        m = make_maps(shape, 'normal')
        for roi, g, flag in rows:
            r = ref_feats(m, roi, 7)
            assert r['gs'] == g and expected_flag(roi, r) == flag, (roi, r['gs'], g, expected_flag(roi, r), flag)
    m = make_maps('a', 'normal')
    flags = {}
    for roi in boxes_footprint(m['img']):
        flags.setdefault(roi[3] - roi[1], set()).add(expected_flag(roi, ref_feats(m, roi, 7)))
    assert set().union(*flags.values()) == {0, 3, 1}, flags
    H = m['img'][0]
    for y0, h, first_valid, at in ((-4.0, 56.0, True, 0), (-4.5, 56.5, False, 0), (H - 52.0, 56.0, True, -1), (H - 52.0, 56.5, False, -1)):
        _, y1, _, bh, _, gh, _, _ = geom(box(0, 8.0, y0, 56.0, h), 0.25, 7, 2)
        v, lo, hi, l, hh = axis_samples(y1, bh, 7, gh, H // 4)
        assert bool(v[at]) == first_valid, (y0, h)
        if first_valid:                                   # exactly -1.0 is clamped to row 0, exactly H to the last row: the value is that row's
            assert (lo[at] == 0 and l[at] == 0) if at == 0 else (lo[at] == hi[at] == H // 4 - 1)
    for roi in boxes_degenerate('a') + boxes_degenerate('c'):
        gw, gh = ref_feats(make_maps('c', 'normal'), roi, 7)['gs']
        w, h = roi[3] - roi[1], roi[4] - roi[2]
        assert (gw == 0) == (w == 0) and (gh == 0) == (h == 0), roi
    for c, cell in ((32.0, 2), (31.875, 1), (16.0, 1), (15.875, 0), (0.0, 0), (-40.0, 0), (256.0, 15), (400.0, 15)):
        assert g_cell(box(0, c - 4.0, c - 4.0, 8.0, 8.0), 16, 16, 16) == (cell, cell), c


# ================================================================================================================ GPU helpers
@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    return Engine(weights.seeded_state_dict(0), device=0, max_batch=1, tile=(64, 64))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def dev_maps(m):
    if '_dev' not in m:
        m['_dev'] = {n: dev(m[n]) for n in ('x0', 'x1', 'sem', 'x0sem', 'G2', 'G3')}
    return m['_dev']


def run(eng, m, rois, P, r=None, cap=None):
    rois = np.asarray(rois, F32).reshape(-1, 5)
    cap = len(rois) if cap is None else cap
    rr = np.zeros((cap, 5), F32)
    rr[:len(rois)] = rois
    d = dev_maps(m)
    out = sentinel(cap, P * P, 64)
    flag = torch.full((cap,), SENT_U8, dtype=torch.uint8, device='cuda')
    res = eng.op_roi_feats(d['x0'], d['x1'], d['sem'], d['x0sem'], d['G2'], d['G3'], dev(rr), len(rois) if r is None else r, P, out=out, fb_flag=flag)
    return res


def check(eng, m, rois, P, tag, want_flags=None):
    """Runs the boxes, asserts the class of each (P = 7) and the derived bound against the reference; returns (out, flags, refs, forms)."""
    rois = np.asarray(rois, F32).reshape(-1, 5)
    res = run(eng, m, rois, P)
    out, flags = res['out'].cpu().numpy().astype(np.float64), res['fb_flag'].cpu().numpy()
    assert np.isfinite(out).all(), f'{tag}: non-finite features'
    refs = [ref_feats(m, roi, P) for roi in rois]
    forms = set()
    for i, (roi, r) in enumerate(zip(rois, refs)):
        fl = int(flags[i]) if P == 7 else -1
        if P == 7:
            assert fl == expected_flag(roi, r), f'{tag}: box {i} {roi.tolist()} class {fl}, expected {expected_flag(roi, r)}'
            if want_flags is not None:
                assert fl == want_flags[i], f'{tag}: box {i} {roi.tolist()} took form {fl}, designed for {want_flags[i]}'
        C, form, val, mag = tolerance(r, fl, P)
        forms.add(form)
        err = np.abs(out[i].reshape(P, P, 64) - val)
        mm = mag > 0
        ratio = (err[mm] / (U * mag[mm])).max() if mm.any() else 0.0
        _obs(f'{form} (C = {C if "gather" not in form and form != "P7 flag 4" else "13 + gw gh"}): err / (u mag)', ratio)
        _obs(f'{form}: err / (C u mag)', ratio / C)
        bad = err > C * U * mag
        assert not bad.any(), (f'{tag}: box {i} {roi.tolist()} form {form} gs {r["gs"]}: {int(bad.sum())} of {bad.size} values beyond C u mag, C = {C}, '
                               f'worst err {err[bad].max():.3e}, err / (u mag) {ratio:.1f}')
    if P == 7:
        c = res['counts'].cpu().numpy()
        assert (c == [int((flags == 2).sum()), int((flags == 1).sum()), int((flags == 4).sum())]).all(), (tag, c)
    return res['out'], flags, refs, forms


# ================================================================================================================ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['normal', 'hard', 'probe'])
def test_adaptive_semantic_count(eng, kind):
    """group 1: sides on either side of 56, 112 and 672 px, crossed on x only, y only and both, and the mixed pairs (1,2) .. (13,2)."""
    for shape, rows in boxes_adaptive().items():
        if shape == 'c' and kind == 'hard':
            continue                                   # (the 1024-px maps are run on two map kinds: the references of their boxes are the slow part)
        forms = check(eng, make_maps(shape, kind), [r[0] for r in rows], 7, f'adaptive {shape} {kind}', want_flags=[r[2] for r in rows])[3]
        assert forms == ({'P7 flag 1', 'P7 flag 2'} if shape == 'a' else {'P7 flag 2', 'P7 flag 4'}), forms      # stream, big-box and giant forms ran


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['normal', 'hard', 'probe'])
def test_footprint_splits(eng, kind):
    """group 2: the same 24- and 44-px boxes at every alignment to the pixel grids: flags 0, 3 and 1 all occur."""
    m = make_maps('a', kind)
    _, flags, _, _ = check(eng, m, boxes_footprint(m['img']), 7, f'footprint {kind}')
    assert set(flags.tolist()) == {0, 3, 1}, set(flags.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('shape,kind', [('a', 'normal'), ('a', 'hard'), ('b', 'normal'), ('b', 'probe')])
def test_borders(eng, shape, kind):
    """group 3: boxes ending on the image edge, inside the last pixel, in the corners, over every side, first sample row at -1.0 / beyond, the
    same at y == H, and boxes wholly outside (only the G term remains)."""
    m = make_maps(shape, kind)
    H, W = m['img']
    rois = [q for b in range(m['B']) for q in boxes_border(H, W, b)]
    out, _, refs, _ = check(eng, m, rois, 7, f'borders {shape} {kind}')
    outside = [i for i, r in enumerate(refs) if r['fp0'] is None and r['fp1'] is None]
    assert len(outside) >= 4 * m['B']
    o = out.cpu().numpy()
    for i in outside:                                      # every kernel form adds the two table rows in float32 and nothing else
        (y2, x2), (y3, x3) = refs[i]['cells']
        b = int(rois[i][0])
        assert (o[i] == (m['G2'][b, y2, x2] + m['G3'][b, y3, x3])[None]).all(), rois[i]


@pytest.mark.gpu
@pytest.mark.parametrize('shape,kind', [('a', 'normal'), ('a', 'hard'), ('c', 'normal')])
def test_degenerate_boxes(eng, shape, kind):
    """group 4: zero width, zero height and both (mmcv's adaptive grid takes no sample on that axis: the semantic term is exactly 0; the level
    maps keep their fixed 2 x 2 samples), and sub-pixel boxes.  Before the stream kernels decided on "the semantic grid
    differs from one sample per bin" the boxes with adaptive counts (0, 0), (0, 1), (1, 0) carried an interpolated semantic term here."""
    m = make_maps(shape, kind)
    rois = boxes_degenerate(shape)
    out, flags, refs, _ = check(eng, m, rois, 7, f'degenerate {shape} {kind}')
    n0 = 0
    for i, (roi, r) in enumerate(zip(rois, refs)):
        if 0 in r['gs']:
            n0 += 1
            # (the level maps keep their fixed 2 x 2 samples, all on one line; the bound above, against a reference whose semantic term is exactly 0, is the check)
            assert not ref_roi_align(m['sem'][0], np.asarray(roi, F32), 0.25, 14, 0)[1].any(), roi
    assert n0 >= 16 and {1, 4}.issubset(set(flags.tolist())) if shape == 'c' else n0 >= 16


@pytest.mark.gpu
def test_g_centre_cells(eng):
    """group 5: with zero maps and index-probe tables (G2 = cell index, G3 = cell index / 128) the feature IS the pair of picked cells: centres on
    multiples of 16 and 32 and 1/8 below, at 0, at the image size (clamped) and outside, for every kernel form of shape (a)."""
    B, lv = SHAPES['a']
    z = lambda l: np.zeros((B,) + lv[l] + (64,), F32)
    cell = lambda l: np.broadcast_to(np.arange(B * lv[l][0] * lv[l][1], dtype=F32).reshape((B,) + lv[l] + (1,)), (B,) + lv[l] + (64,)).copy()
    m = dict(x0=z(0), x1=z(1), sem=z(0), x0sem=z(0), G2=cell(2), G3=cell(3) / F32(128.0), B=B, img=(256, 256))
    rois = []
    for c in (32.0, 31.875, 16.0, 15.875, 48.0, 64.0, 63.875, 0.0, 0.125, -40.0, 255.875, 256.0, 400.0):
        for s in (8.0, 30.0, 80.0, 200.0):
            rois += [box(1, c - s / 2, 100.0 - s / 2, s, s), box(0, 100.0 - s / 2, c - s / 2, s, s)]
    for P in (7, 14):
        res = run(eng, m, rois, P)
        o = res['out'].cpu().numpy()
        for i, roi in enumerate(rois):
            (y2, x2), (y3, x3) = g_cell(roi, 16, 16, 16), g_cell(roi, 32, 8, 8)
            b = int(roi[0])
            want = F32((b * 16 + y2) * 16 + x2) + F32((b * 8 + y3) * 8 + x3) / F32(128.0)
            assert (o[i] == want).all(), (P, roi, float(o[i].flat[0]), float(want))
        if P == 7:
            fl = set(res['fb_flag'].cpu().numpy().tolist())
            assert {1, 2} <= fl and fl & {0, 3}, fl


@pytest.mark.gpu
def test_list_forms(eng):
    """group 6: 150 mid-size and 150 big boxes alone (stream_few, the big-box split) and inside lists of more than 1024 mid-size and more than 512
    big boxes (roi_feat7_stream_kernel, the unsplit big-box form): bit-identical features, each within the bound.  Both sets hold the zero-width /
    zero-height boxes of group 4, so every list form meets a box whose semantic grid has no sample."""
    from nuhtc_amd import hip
    # the engine's settings are in force (the switches exist in development builds only, where this sets them to their defaults): short lists go to
    # stream_few and the split, so the comparison below is between two different kernels
    for knob in (b'STREAM_FEW', b'BIG_SPLIT'):
        assert eng.lib.nuhtc_dev_knob(knob, 1) in (0, hip.E_STATE)
    m = make_maps('a', 'normal')
    rng = np.random.default_rng(11)
    H, W = m['img']
    dmid, dbig = boxes_degenerate_lists()
    mid, big = dmid + boxes_mid(150 - len(dmid), rng, H, W, m['B']), dbig + boxes_big(150 - len(dbig), rng, H, W, m['B'])
    short = mid + big
    out_s, flags, refs, forms = check(eng, m, short, 7, 'short lists', want_flags=[1] * 150 + [2] * 150)
    assert forms == {'P7 flag 1', 'P7 flag 2'}
    assert sum(0 in r['gs'] for r in refs[:150]) == len(dmid) and sum(0 in r['gs'] for r in refs[150:]) == len(dbig)
    assert {r['gs'] for r in refs[:150]} >= {(0, 0), (0, 1), (1, 0), (0, 2), (2, 0)}
    cs = run(eng, m, short, 7)['counts'].cpu().numpy()
    assert 0 < cs[0] <= BIG_SPLIT_MAX and 0 < cs[1] <= SMF_MAX, cs                 # the short forms: stream_few, the big-box split + combine
    filler = boxes_mid(SMF_MAX - 150 + 40, rng, H, W, m['B']) + boxes_big(BIG_SPLIT_MAX - 150 + 30, rng, H, W, m['B'])
    order = rng.permutation(len(short) + len(filler))
    long_rois = np.asarray(short + filler, F32)[np.argsort(order)]           # row i of `short` sits at row order[i]
    res = run(eng, m, long_rois, 7)
    c = res['counts'].cpu().numpy()
    assert c[0] > BIG_SPLIT_MAX and c[1] > SMF_MAX and c[2] == 0, c          # the long forms: roi_feat7_stream_kernel, the unsplit big-box kernel
    pos = torch.from_numpy(order[:len(short)].copy()).cuda()
    assert torch.equal(_bits(res['out'][pos]), _bits(out_s)), "a box's features depend on the length of its list"
    assert (res['fb_flag'][pos].cpu().numpy() == flags).all()


@pytest.mark.gpu
@pytest.mark.parametrize('shape,kind', [('a', 'normal'), ('a', 'hard'), ('b', 'probe'), ('c', 'normal')])
def test_mask_features_14(eng, shape, kind):
    """group 7: the one-sample LDS form and the gather form of roi_feat14_kernel (`one` true and false, l0.ok false at the worst alignment, a large
    box split over gridDim.y), zero-width boxes (only the G term is left), borders."""
    m = make_maps(shape, kind)
    H, W = m['img']
    rois = [box(0, 40.0 + a, 48.0 + a2, s, s2) for a, a2 in ((0.0, 0.0), (3.0, 7.0), (7.0, 3.0), (7.875, 7.875)) for s, s2 in ((12.0, 12.0), (14.0, 13.0), (14.0, 14.125), (14.125, 6.0), (40.0, 52.0))]
    rois += [box(m['B'] - 1, 10.0, 20.0, 100.0, 90.0), box(0, 5.0, 5.0, min(H, W) - 10.0, min(H, W) - 20.0), box(0, 30.0, 30.0, 0.0, 40.0), box(0, 30.0, 30.0, 12.0, 0.0)]
    rois += boxes_border(H, W, m['B'] - 1)
    if shape == 'c':
        rois = rois[:8] + [box(0, 100.0, 60.0, 700.0, 500.0), box(0, -20.0, -20.0, 1000.0, 300.0), box(0, 500.0, 500.0, 0.0, 400.0)]
    rois.append(box(0, 43.0, 47.0, 56.0, 56.0))            # one sample per bin (`one` true) and a 14-15 pixel footprint: l0.ok false, the gather form
    out, _, refs, forms = check(eng, m, rois, 14, f'P14 {shape} {kind}')
    assert forms == {'P14 lds', 'P14 gather'}, forms
    assert refs[-1]['gs'] == (1, 1) and max(_fwh(refs[-1]['fp0'])) > TP0 and tolerance(refs[-1], -1, 14)[1] == 'P14 gather'
    for i, r in enumerate(refs):
        if 0 in r['gs']:
            (y2, x2), (y3, x3) = r['cells']
            b = int(rois[i][0])
            assert (out[i].cpu().numpy() == (m['G2'][b, y2, x2] + m['G3'][b, y3, x3])[None]).all(), rois[i]


@pytest.mark.gpu
def test_rows_from_r_dev_on_are_not_written(eng):
    """group 8: out, fb_flag and everything from *r_dev on keep the sentinel, for *r_dev in {0, 1, 15, 16, 17, cap}; the live rows do not depend on it."""
    m = make_maps('a', 'normal')
    rng = np.random.default_rng(5)
    H, W = m['img']
    rois = (boxes_footprint(m['img'])[::7] + boxes_mid(6, rng, H, W, 2) + boxes_big(6, rng, H, W, 2))
    rois = [rois[i] for i in rng.permutation(len(rois))][:21]
    cap = len(rois)
    full = {P: run(eng, m, rois, P) for P in (7, 14)}
    for P in (7, 14):
        for r in (0, 1, 15, 16, 17, cap):
            res = run(eng, m, rois, P, r=r)
            assert bool((_bits(res['out'][r:]) == SENTINEL).all()), (P, r)
            assert torch.equal(_bits(res['out'][:r]), _bits(full[P]['out'][:r])), (P, r)
            if P == 7:
                assert bool((res['fb_flag'][r:] == SENT_U8).all()) and torch.equal(res['fb_flag'][:r], full[7]['fb_flag'][:r]), r


# ---------------------------------------------------------------------------------------------------------------- attention-pool tables
# G[q, c] = (1 / HW) sum_p F[p, c] sim(q, p), sim = relu(cos - tau) + tau in [tau, 1].  Bound |got - ref| <= C_AP(HW) u magG, magG = (1 / HW) sum_p |F[p, c]| sim:
#   cos: each squared norm a 64-term sum 64 u, sqrt halves and rounds 33, the division 34 per vector; the dot product of the two unit vectors 65 more: the cosine's
#   ABSOLUTE error is <= (2 * 34 + 65) u = 133 u (|cos| <= 1), and so is sim's; relative to sim >= tau that is 133 / tau u.  The product F sim 1, the HW-term sum
#   HW (any order), the division 1.  The GEMM route multiplies the dot product by the two reciprocal norms instead (the same count) and rounds S once more: + 2.
#   C_AP = 133 / tau + HW + 4.  A pair whose cosine lies within COS_MARGIN = 133 u of tau may take the other relu branch: the placed pairs stay 64 times further away.
COS_ABS = 133


def c_ap(HW):
    return COS_ABS / TAU + HW + 4


def attn_case(HW, B=2):
    """Normal pixels; pixel 0 all zero (the norm clamp); pixels 1, 2 identical (cos = 1); pixels 3, 4 / 3, 5: cosines placed on either side of tau."""
    rng = np.random.default_rng(HW)
    Fm = rng.standard_normal((B, HW, 64)).astype(F32)
    if HW >= 6:
        Fm[:, 0] = 0
        Fm[:, 2] = Fm[:, 1]
        e = np.zeros((3, 64), F32)
        e[0, 0] = e[1, 1] = 1
        d = 64 * COS_ABS * U
        for k, cs in ((4, TAU + d), (5, TAU - d)):
            Fm[:, k] = F32(2.0) * (F32(cs) * e[0] + F32(np.sqrt(1 - cs * cs)) * e[1])
        Fm[:, 3] = F32(3.0) * e[0]
    return Fm


@pytest.mark.gpu
@pytest.mark.parametrize('HW', [1, 35, 64, 117, 256])
def test_attn_pool_routes(eng, HW):
    """attn_pool_kernel, the GEMM pair (HW % 32 == 0) and `auto` against float64 within C_AP u magG; `auto` is the route the engine picks, bit for
    bit; both routes agree within the sum of their bounds; the fp16 route against oracle.model.attention_pool(fp16=True) to one fp16 unit."""
    from nuhtc_amd.engine import HipError
    from oracle import model as O
    Fm = attn_case(HW)
    ref, mag, cos = ref_attn_pool(Fm, TAU)
    if HW >= 6:
        assert (cos[:, 3, 4] > TAU + 32 * COS_ABS * U).all() and (cos[:, 3, 5] < TAU - 32 * COS_ABS * U).all() and (np.abs(cos[:, 1, 2] - 1) < 1e-12).all()
    d = dev(Fm)
    got = {'kernel': eng.op_attn_pool(d, TAU, 'kernel'), 'auto': eng.op_attn_pool(d, TAU, 'auto')}
    if HW % 32 == 0:
        got['gemm'] = eng.op_attn_pool(d, TAU, 'gemm')
    else:
        with pytest.raises(HipError):
            eng.op_attn_pool(d, TAU, 'gemm')
    assert torch.equal(_bits(got['auto']), _bits(got['gemm' if HW % 32 == 0 else 'kernel']))
    tol = c_ap(HW) * U * mag
    for k, g in got.items():
        err = np.abs(g.cpu().numpy().astype(np.float64) - ref)
        pos = tol > 0
        _obs(f'attn_pool {k}: err / tolerance', (err[pos] / tol[pos]).max() if pos.any() else 0.0)
        assert (err <= tol).all(), f'{k} HW={HW}: worst err / tol {(err[pos] / tol[pos]).max():.2f}'
    if 'gemm' in got:
        assert (np.abs(got['gemm'].cpu().numpy().astype(np.float64) - got['kernel'].cpu().numpy()) <= 2 * tol).all()
    # fp16 route: the reference's own tensor expressions on fp16 tensors; one fp16 unit (tests/test_hip_full.py)
    # (a zero pixel gives 0 / 0 there and its NaN spreads to every mean: the zero pixel is replaced for this route)
    F16 = Fm.copy()
    F16[:, 0] = np.random.default_rng(1).standard_normal((2, 64)).astype(F32)
    g16 = eng.op_attn_pool(dev(F16), TAU, 'fp16').cpu()
    x = torch.from_numpy(F16).reshape(2, 1, HW, 64).permute(0, 3, 1, 2).contiguous()
    cx = np.arange(HW, dtype=np.float64)
    one = np.stack([cx + 0.25, np.full(HW, 0.25), cx + 0.75, np.full(HW, 0.75)], -1)
    rois = torch.from_numpy(np.concatenate([np.concatenate([np.full((HW, 1), float(b)), one], 1) for b in range(2)]).astype(F32))
    with torch.no_grad():
        ref16 = O.attention_pool(x, rois, 1, thres=TAU, fp16=True).reshape(2, HW, 64)
    assert bool(torch.isfinite(ref16).all()) and torch.equal(g16, g16.half().float())
    if HW >= 6:                                            # with the zero pixel: the NaN of 0 / 0 spreads exactly as in the reference's expressions
        xz = torch.from_numpy(Fm).reshape(2, 1, HW, 64).permute(0, 3, 1, 2).contiguous()
        with torch.no_grad():
            nan_ref = torch.isnan(O.attention_pool(xz, rois, 1, thres=TAU, fp16=True).reshape(2, HW, 64))
        nan_got = torch.isnan(eng.op_attn_pool(d, TAU, 'fp16').cpu())
        assert bool(nan_ref.any()) and torch.equal(nan_got, nan_ref)
    unit = torch.maximum(ref16.abs(), torch.tensor(2.0 ** -14)) * 2.0 ** -10
    off = (g16 - ref16).abs()
    _obs('attn_pool fp16: err / fp16 unit', float((off / unit).max()))
    assert bool((off <= unit).all())


# ---------------------------------------------------------------------------------------------------------------- the ops are the engine's path
@pytest.mark.gpu
def test_ops_are_the_engines_path(hip_device):
    """One engine on the small_b2 golden with the token dump on: its own x0..x3, sem_feat, x0sem, rois_stage2 and mask_rois through the two ops
    give its G2, G3, bbox_feats and mask_feats bit for bit."""
    import golden_util as G
    from nuhtc_amd.engine import Engine
    g = G.load('small_b2')
    sd, tiles = G.seeded_sd(g), g['tiles']
    B = len(tiles)
    e = Engine(sd, device=0, max_batch=B, tile=tiles.shape[1:3])
    e.enable_token_dump()
    e.infer_async(e.to_device(tiles), int(g['channel_mode']))
    e.check()
    x = [e.buffer(f'x{l}')[:B] for l in range(4)]
    tau = float(e.cfg.att_thres)
    G2, G3 = e.op_attn_pool(x[2], tau), e.op_attn_pool(x[3], tau)
    assert torch.equal(_bits(G2.reshape(B, -1, 64)), _bits(e.buffer('G2')[:B])) and torch.equal(_bits(G3.reshape(B, -1, 64)), _bits(e.buffer('G3')[:B]))
    R, D = int(e.buffer('roi_total').item()), int(e.buffer('det_total').item())
    assert R > 0 and D > 0
    sem, x0sem = e.buffer('sem_feat')[:B], e.buffer('x0sem')[:B]
    r7 = e.op_roi_feats(x[0], x[1], sem, x0sem, G2, G3, e.buffer('rois_stage2'), e.buffer('roi_total'), 7)
    assert torch.equal(_bits(r7['out'][:R]), _bits(e.buffer('bbox_feats')[:R]))
    r14 = e.op_roi_feats(x[0], x[1], sem, x0sem, G2, G3, e.buffer('mask_rois'), e.buffer('det_total'), 14)
    assert torch.equal(_bits(r14['out'][:D]), _bits(e.buffer('mask_feats')[:D]))
    print(f'engine path: {R} RoIs (forms {sorted(set(r7["fb_flag"][:R].cpu().numpy().tolist()))}), {D} detections')
    e.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_refusals_leave_the_engine_usable(eng):
    """Null pointers, P not in {7, 14}, *r_dev > cap, B above the limit, an image index outside the batch and a forced GEMM route at HW % 32 != 0 are
    refused with the error code and nothing written; the next valid call gives the same bits as before."""
    from nuhtc_amd import hip
    from nuhtc_amd.engine import HipError
    m = make_maps('a', 'normal')
    rois = boxes_footprint(m['img'])[:9]
    good = run(eng, m, rois, 7)

    def still_ok(label):
        r = run(eng, m, rois, 7)
        assert torch.equal(_bits(r['out']), _bits(good['out'])) and torch.equal(r['fb_flag'], good['fb_flag']), label
    d = dev_maps(m)
    for label, kw in (('P = 8', dict(P=8)), ('r > cap', dict(r=10)), ('r < 0', dict(r=-1))):
        out, flag = sentinel(9, 196, 64), torch.full((9,), SENT_U8, dtype=torch.uint8, device='cuda')
        with pytest.raises(HipError):
            eng.op_roi_feats(d['x0'], d['x1'], d['sem'], d['x0sem'], d['G2'], d['G3'], dev(np.asarray(rois, F32)), kw.get('r', 9), kw.get('P', 7), out=out, fb_flag=flag)
        assert bool((_bits(out) == SENTINEL).all()) and bool((flag == SENT_U8).all()), label
        still_ok(label)
    bad = np.asarray(rois, F32)
    bad[4, 0] = 2.0                                        # image index == B
    out = sentinel(9, 49, 64)
    with pytest.raises(HipError):
        eng.op_roi_feats(d['x0'], d['x1'], d['sem'], d['x0sem'], d['G2'], d['G3'], dev(bad), 9, 7, out=out)
    assert bool((_bits(out) == SENTINEL).all())
    still_ok('image index')
    a = hip.RoiFeatsArgs(B=2, cap=9, P=7)
    assert eng.lib.nuhtc_op_roi_feats(eng.h, ctypes.byref(a), eng._stream()) == hip.E_INVALID
    assert eng.lib.nuhtc_op_roi_feats(eng.h, None, eng._stream()) == hip.E_INVALID
    full = dict(x0=d['x0'].data_ptr(), x1=d['x1'].data_ptr(), sem=d['sem'].data_ptr(), x0sem=d['x0sem'].data_ptr(), G2=d['G2'].data_ptr(), G3=d['G3'].data_ptr(),
                rois=dev(np.asarray(rois, F32)).data_ptr(), r_dev=torch.tensor([9], dtype=torch.int32, device='cuda').data_ptr(), cap=9, P=7,
                H=(ctypes.c_int32 * 4)(64, 32, 16, 8), W=(ctypes.c_int32 * 4)(64, 32, 16, 8))
    out, flag, cnt = sentinel(9, 49, 64), torch.zeros(9, dtype=torch.uint8, device='cuda'), torch.zeros(3, dtype=torch.int32, device='cuda')
    a = hip.RoiFeatsArgs(B=257, out=out.data_ptr(), fb_flag=flag.data_ptr(), counts=cnt.data_ptr(), **full)
    assert eng.lib.nuhtc_op_roi_feats(eng.h, ctypes.byref(a), eng._stream()) == hip.E_INVALID
    a = hip.RoiFeatsArgs(B=2, out=out.data_ptr(), fb_flag=None, counts=cnt.data_ptr(), **full)          # P = 7 needs fb_flag
    assert eng.lib.nuhtc_op_roi_feats(eng.h, ctypes.byref(a), eng._stream()) == hip.E_INVALID
    assert bool((_bits(out) == SENTINEL).all())
    still_ok('null / B > 256')
    # attention pool
    Fm = dev(attn_case(35))
    g0 = eng.op_attn_pool(Fm, TAU)
    G = sentinel(2, 35, 64)
    assert eng.lib.nuhtc_op_attn_pool(eng.h, None, 2, 35, TAU, 0, G.data_ptr(), eng._stream()) == hip.E_INVALID
    assert eng.lib.nuhtc_op_attn_pool(eng.h, Fm.data_ptr(), 2, 35, TAU, 0, None, eng._stream()) == hip.E_INVALID
    for B_, HW_, route in ((257, 35, 0), (2, 0, 0), (2, 35, 1), (2, 35, 4)):
        assert eng.lib.nuhtc_op_attn_pool(eng.h, Fm.data_ptr(), B_, HW_, TAU, route, G.data_ptr(), eng._stream()) == hip.E_INVALID, (B_, HW_, route)
    assert bool((_bits(G) == SENTINEL).all())
    assert torch.equal(_bits(eng.op_attn_pool(Fm, TAU)), _bits(g0))


@pytest.mark.gpu
def test_print_observed_maxima(eng):
    """Prints the observed maxima of the tests that ran before it in this process: err / (u mag) per kernel form beside the derived C."""
    for k in sorted(OBSERVED):
        print(f'  {k}: {OBSERVED[k]:.3f}')
