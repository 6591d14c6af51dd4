"""The separable form of the small-box RoI features (roi_feat7_lds_kernel, flags 0 and 3 of roi_classify_kernel; csrc/roi.hip: sep_build,
sep_column) on placed boxes, one tile with 64-channel maps of 32 x 32 / 16 x 16 pixels (a 128 x 128 network input, the smallest the op
entry accepts).

A bin of RoIAlign is  sum_y sum_x wy[y] wx[x] F[y][x]  with per-axis weights that merge the bilinear weights of the bin's two samples; on a
footprint that fits the LDS tiles (8 x 8 / 12 x 12 pixels on stride 4, 5 x 5 / 7 x 7 on stride 8) a bin touches at most 3 pixels per axis.
test_merged_weight_algebra pins that algebra on the CPU, in float64, with a numpy restatement of the tables; the GPU tests hold the kernel
to the float64 reference, the classes and the bound C u mag of tests/test_hip_roifeat.py (its helpers are imported, C_LDS = 14 for flags 0
and 3: the separable chain -- reference weight 1, merged x and y weights 1 each, x chain 3, y chain 3, maps and tables 4, x0 + sem 1 -- has
the same first-order length as the sample loop's).

A box whose semantic grid is not one sample per 14 x 14 bin (sem_separate) and whose footprint fits a tile can only be a box of zero width
or height (two samples per bin mean a side above 56 px, a footprint of 14 pixels): the classes do not change, so it takes the stream form
(flag 1, three maps, a semantic term of exactly 0) and is held to that form's bound."""
import numpy as np
import pytest
import torch

import test_hip_roifeat as R
from test_hip_roifeat import F32, SENTINEL, SENT_U8, box

LV = [(32, 32), (16, 16), (8, 8), (4, 4)]
IMG = 128.0
_MAPS = {}


def small_maps(kind):
    """One tile of the smallest maps: 'normal' i.i.d. normal; 'hard' as test_hip_roifeat.make_maps (x0 a large offset plus a small signal, x1 over
    six decades, channel 7 zero everywhere, channel 5 of sem zero)."""
    if kind in _MAPS:
        return _MAPS[kind]
    rng = np.random.default_rng(100 + ['normal', 'hard'].index(kind))
    n = lambda l: rng.standard_normal((1,) + LV[l] + (64,)).astype(F32)
    m = dict(x0=n(0), x1=n(1), sem=n(0), G2=n(2), G3=n(3))
    if kind == 'hard':
        m['x0'] = (F32(1000.0) + F32(1e-2) * m['x0']).astype(F32)
        m['x1'] = (m['x1'] * (10.0 ** rng.uniform(-3, 3, m['x1'].shape)).astype(F32)).astype(F32)
        for k in ('x0', 'x1', 'sem', 'G2', 'G3'):
            m[k][..., 7] = 0
        m['sem'][..., 5] = 0
    m['x0sem'] = (m['x0'] + m['sem']).astype(F32)
    m['B'], m['img'] = 1, (int(IMG), int(IMG))
    _MAPS[kind] = m
    return m


# ---------------------------------------------------------------------------------------------------------------- the placed boxes
# (roi, footprint on stride 4 (w, h), footprint on stride 8, class): exactly at each tile limit and one pixel over it
LIMITS = [
    ([0.0, 24.125, 25.125, 47.125, 48.125], (8, 8), (5, 5), 0),
    ([0.0, 34.25, 35.25, 54.25, 52.75], (6, 6), (5, 5), 0),
    ([0.0, 29.0, 30.0, 55.0, 56.0], (9, 8), (5, 5), 3),
    ([0.0, 20.0, 21.0, 46.0, 47.0], (8, 9), (5, 5), 3),
    ([0.0, 35.0, 36.0, 61.0, 62.0], (8, 8), (6, 5), 3),
    ([0.0, 26.0, 27.0, 52.0, 53.0], (8, 8), (5, 6), 3),
    ([0.0, 25.625, 26.625, 61.625, 62.625], (10, 10), (7, 7), 3),
    ([0.0, 23.0, 24.0, 63.5, 64.5], (12, 12), (7, 7), 3),
    ([0.0, 20.375, 21.375, 63.875, 64.875], (13, 12), (7, 7), 1),
    ([0.0, 23.375, 24.375, 66.875, 67.875], (12, 13), (7, 7), 1),
    ([0.0, 26.375, 27.375, 69.875, 70.875], (12, 12), (8, 7), 1),
    ([0.0, 25.25, 26.25, 68.75, 69.75], (12, 12), (7, 8), 1),
]
# bins far narrower than a pixel (both samples of a bin between the same two pixels, several bins per pixel) and bins over a pixel wide
# (the two samples' low pixels differ: three pixels per bin and axis)
NARROW = [box(0, 40.0, 40.0, 6.0, 6.0), box(0, 41.5, 42.25, 3.0, 9.0), box(0, 64.0, 32.0, 1.0, 1.0), box(0, 33.0, 21.0, 0.125, 0.125)]
WIDE = [box(0, 20.5, 30.25, 36.0, 40.0), box(0, 50.125, 40.5, 40.0, 33.0), box(0, 30.0, 60.0, 38.5, 39.5)]
# the four borders and corners (samples between -1 and 0 and between H - 1 and H are clamped, beyond they are dropped), boxes ending on the edge
BORDER = [box(0, 0.0, 0.0, 20.0, 20.0), box(0, IMG - 20.0, IMG - 20.0, 20.0, 20.0), box(0, -6.0, 50.0, 24.0, 20.0), box(0, IMG - 18.0, 50.0, 24.0, 20.0),
          box(0, 50.0, -6.0, 20.0, 24.0), box(0, 50.0, IMG - 18.0, 20.0, 24.0), box(0, -6.0, -6.0, 24.0, 24.0), box(0, IMG - 18.0, -6.0, 24.0, 24.0),
          box(0, -6.0, IMG - 18.0, 24.0, 24.0), box(0, IMG - 18.0, IMG - 18.0, 24.0, 24.0), box(0, -3.0, -2.0, 36.0, 38.0), box(0, IMG - 2.0, IMG - 1.0, 2.0, 1.0)]
ZERO = [box(0, 40.0, 40.0, 0.0, 20.0), box(0, 40.0, 40.0, 20.0, 0.0), box(0, 40.0, 40.0, 0.0, 0.0), box(0, 0.0, 70.0, 0.0, 12.0), box(0, 30.0, IMG, 16.0, 0.0)]
OUTSIDE = [box(0, -60.0, 20.0, 30.0, 30.0), box(0, IMG + 22.0, IMG + 22.0, 20.0, 20.0), box(0, 20.0, -50.0, 24.0, 24.0)]


def samples_of(roi, scale, size_hw):
    """The 14 samples per axis of the 7-grid with 2 samples per bin -> (x samples, y samples), each (valid, lo, hi, l, h)."""
    x1, y1, bw, bh, _, _, _, _ = R.geom(roi, scale, 7, 2)
    return R.axis_samples(x1, bw, 7, 2, size_hw[1]), R.axis_samples(y1, bh, 7, 2, size_hw[0])


def test_placed_boxes_have_their_properties():
    """The footprints and classes of LIMITS, the bins of NARROW and WIDE, the clamped and dropped samples of BORDER, the empty semantic grid of ZERO
    and the empty footprints of OUTSIDE -- from the reference alone."""
    m = small_maps('normal')
    for roi, fp0, fp1, flag in LIMITS:
        r = R.ref_feats(m, np.asarray(roi, F32), 7)
        assert (R._fwh(r['fp0']), R._fwh(r['fp1']), R.expected_flag(np.asarray(roi, F32), r), r['gs']) == (fp0, fp1, flag, (1, 1)), roi
    for rois, want in ((NARROW, 0), (WIDE, 1)):
        for roi in rois:
            (v, lo, hi, l, h), _ = samples_of(roi, 0.25, LV[0])
            assert v.all() and set((lo[1::2] - lo[0::2]).tolist()) >= {want}, roi
            r = R.ref_feats(m, np.asarray(roi, F32), 7)
            assert R.expected_flag(np.asarray(roi, F32), r) in (0, 3), roi
    one_pixel = clamp_lo = clamp_hi = dropped = 0
    for roi in BORDER:
        r = R.ref_feats(m, np.asarray(roi, F32), 7)
        assert R.expected_flag(np.asarray(roi, F32), r) in (0, 3), roi
        for scale, size in ((0.25, LV[0]), (0.125, LV[1])):
            for (v, lo, hi, l, h), n in zip(samples_of(roi, scale, size), (size[1], size[0])):
                dropped += int(v.any() and not v.all())
                clamp_lo += int((v & (lo == 0) & (l == 0)).any())
                clamp_hi += int((v & (lo == n - 1) & (hi == n - 1)).any())
                one_pixel += int(any(v[2 * q] and v[2 * q + 1] and lo[2 * q] == lo[2 * q + 1] and l[2 * q] == 0 and l[2 * q + 1] == 0 for q in range(7)))
    assert dropped >= 8 and clamp_lo >= 8 and clamp_hi >= 8 and one_pixel >= 8, (dropped, clamp_lo, clamp_hi, one_pixel)      # (one_pixel: a merged weight on a single pixel)
    for roi in ZERO:
        r = R.ref_feats(m, np.asarray(roi, F32), 7)
        assert 0 in r['gs'] and R.expected_flag(np.asarray(roi, F32), r) == 1, roi
        assert max(R._fwh(r['fp0'])) <= R.TP0 and max(R._fwh(r['fp1'])) <= R.TP1, roi      # sem_separate, and the footprint would fit
    for roi in OUTSIDE:
        r = R.ref_feats(m, np.asarray(roi, F32), 7)
        assert r['fp0'] is None and r['fp1'] is None and R.expected_flag(np.asarray(roi, F32), r) == 0, roi


# ---------------------------------------------------------------------------------------------------------------- the algebra, on the CPU
def merged_tables(valid, lo, hi, l, h):
    """sep_build restated: per bin its first pixel and the merged weights of the 3 pixels from there (sample order, / samples per axis), float64;
    also whether every valid sample of the bin lies on those 3 pixels."""
    first, w, fits = np.zeros(7, np.int64), np.zeros((7, 3)), True
    for q in range(7):
        s = [i for i in (2 * q, 2 * q + 1) if valid[i]]
        first[q] = min(int(lo[i]) for i in s) if s else 0
        for j in range(3):
            px = first[q] + j
            acc = 0.0
            for i in s:
                if lo[i] == px:
                    acc += float(h[i])
                if hi[i] == px:
                    acc += float(l[i])
            w[q, j] = acc / 2.0
        fits = fits and all(first[q] <= lo[i] and hi[i] <= first[q] + 2 for i in s)
    return first, w, fits


def sample_loop(fm, sx, sy):
    """mmcv's sample loop on one map, float64 products of the float32 axis weights -> (value, magnitude) (7, 7)."""
    (vx, xlo, xhi, lx, hx), (vy, ylo, yhi, ly, hy) = sx, sy
    f = fm.astype(np.float64)
    ok = (vy[:, None] & vx[None, :]).astype(np.float64)
    val, mag = np.zeros((14, 14)), np.zeros((14, 14))
    for a, b_, yy, xx in ((hy, hx, ylo, xlo), (hy, lx, ylo, xhi), (ly, hx, yhi, xlo), (ly, lx, yhi, xhi)):
        t = np.outer(a.astype(np.float64), b_.astype(np.float64)) * ok * f[yy][:, xx]
        val += t
        mag += np.abs(t)
    return val.reshape(7, 2, 7, 2).sum((1, 3)) / 4.0, mag.reshape(7, 2, 7, 2).sum((1, 3)) / 4.0


def test_merged_weight_algebra():
    """1000 seeded random small boxes, inside, over the borders and partly outside, on both levels: the two contractions with the merged-weight
    tables equal the sample loop to 1e-12 relative in float64, and no sample of a bin lies beyond its 3 pixels when the footprint fits a tile."""
    rng = np.random.default_rng(7)
    maps = [rng.standard_normal(LV[0]), rng.standard_normal(LV[1])]
    done = clamped = invalid = 0
    while done < 1000:
        w, h = rng.integers(1, 40 * 8 + 1, 2) / 8.0
        x, y = rng.integers(-30 * 8, 140 * 8, 2) / 8.0
        roi = np.asarray(box(0, x, y, w, h), F32)
        for scale, size, fm, tp in ((0.25, LV[0], maps[0], R.TP0), (0.125, LV[1], maps[1], R.TP1)):
            sx, sy = samples_of(roi, scale, size)
            if not (sx[0].any() and sy[0].any()):
                continue
            if max(sx[2][sx[0]].max() - sx[1][sx[0]].min(), sy[2][sy[0]].max() - sy[1][sy[0]].min()) + 1 > tp:
                continue                                  # the footprint does not fit: another kernel form
            fx, wx, okx = merged_tables(*sx)
            fy, wy, oky = merged_tables(*sy)
            assert okx and oky, roi
            H, W = size
            got = np.zeros((7, 7))
            for ph in range(7):
                for pw in range(7):
                    rows = np.minimum(fy[ph] + np.arange(3), H - 1)      # (a tap past the map has weight 0)
                    cols = np.minimum(fx[pw] + np.arange(3), W - 1)
                    got[ph, pw] = wy[ph] @ fm[np.ix_(rows, cols)] @ wx[pw]
            val, mag = sample_loop(fm, sx, sy)
            assert (np.abs(got - val) <= 1e-12 * mag + 1e-300).all(), (roi, np.abs(got - val).max())
            clamped += int(((sx[1] == sx[2]) & sx[0]).any() or ((sy[1] == sy[2]) & sy[0]).any())
            invalid += int(not sx[0].all() or not sy[0].all())
        done += 1
    assert clamped >= 20 and invalid >= 20, (clamped, invalid)


# ---------------------------------------------------------------------------------------------------------------- GPU tests
@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    return Engine(weights.seeded_state_dict(0), device=0, max_batch=1, tile=(64, 64))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['normal', 'hard'])
def test_tile_limits(eng, kind):
    """Footprints exactly at 8 x 8 / 5 x 5 and 12 x 12 / 7 x 7 and one pixel over on either axis and either level: the class of each, and the box
    over the last limit takes the stream form."""
    flags = R.check(eng, small_maps(kind), [r[0] for r in LIMITS], 7, f'limits {kind}', want_flags=[r[3] for r in LIMITS])[1]
    assert set(flags.tolist()) == {0, 3, 1}


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['normal', 'hard'])
def test_narrow_and_wide_bins(eng, kind):
    flags = R.check(eng, small_maps(kind), NARROW + WIDE, 7, f'bins {kind}')[1]
    assert set(flags.tolist()) <= {0, 3}


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['normal', 'hard'])
def test_borders_zero_sides_and_outside(eng, kind):
    m = small_maps(kind)
    rois = BORDER + ZERO + OUTSIDE
    out, flags, refs, forms = R.check(eng, m, rois, 7, f'borders {kind}')
    assert forms == {'P7 flag 0', 'P7 flag 3', 'P7 flag 1'} or forms == {'P7 flag 0', 'P7 flag 1'}, forms
    assert flags[len(BORDER):len(BORDER) + len(ZERO)].tolist() == [1] * len(ZERO)          # sem_separate: three maps, the stream form
    o = out.cpu().numpy()
    for i in range(len(BORDER) + len(ZERO), len(rois)):                                     # all weights 0: the two table rows and nothing else
        (y2, x2), (y3, x3) = refs[i]['cells']
        assert (o[i] == (m['G2'][0, y2, x2] + m['G3'][0, y3, x3])[None]).all(), rois[i]


@pytest.mark.gpu
def test_rows_do_not_depend_on_the_list(eng):
    """The same list twice and in reversed order: bitwise-equal rows per box."""
    m = small_maps('normal')
    rois = [r[0] for r in LIMITS] + NARROW + WIDE + BORDER + ZERO + OUTSIDE
    a, b_ = R.run(eng, m, rois, 7), R.run(eng, m, rois, 7)
    c = R.run(eng, m, rois[::-1], 7)
    assert torch.equal(R._bits(a['out']), R._bits(b_['out'])) and torch.equal(a['fb_flag'], b_['fb_flag'])
    assert torch.equal(R._bits(c['out'].flip(0)), R._bits(a['out'])) and torch.equal(c['fb_flag'].flip(0), a['fb_flag'])
    assert {0, 3} <= set(a['fb_flag'].cpu().numpy().tolist())


@pytest.mark.gpu
def test_rows_from_r_dev_on_keep_the_sentinel(eng):
    m = small_maps('normal')
    rois = ([r[0] for r in LIMITS] + NARROW + WIDE + BORDER)[:24]
    cap = len(rois)
    full = R.run(eng, m, rois, 7)
    for r in (0, 1, 7, cap - 1, cap):
        res = R.run(eng, m, rois, 7, r=r)
        assert bool((R._bits(res['out'][r:]) == SENTINEL).all()) and bool((res['fb_flag'][r:] == SENT_U8).all()), r
        assert torch.equal(R._bits(res['out'][:r]), R._bits(full['out'][:r])) and torch.equal(res['fb_flag'][:r], full['fb_flag'][:r]), r
