"""The 3x3 convolution of the path (64 -> 64 channels, zero padding 1) and its fused epilogues, op by op, against
torch.nn.functional.conv2d in float64 on the CPU.

Every 3x3 convolution of nuhtc_infer -- FPN output convs, the RPN conv, the four semantic-head convs, the four mask-head convs --
runs through conv3_split_kernel (csrc/conv.hip) on the split pipe and through the implicit-GEMM gemm_kernel (csrc/gemm.hip, A_CONV3)
on the fp32 pipe.  Engine.op_conv3 (nuhtc_op_conv3) packs the weights as nuhtc_finalize does and launches through the engine's GEMM
dispatch, so these tests reach what the end-to-end tests cannot: workgroups that walk several tiles (halo prefetch, weight double
buffer across a tile boundary, deferred stores flushed after the last tile), device-side image counts below the capacity, image
boundaries in the flattened batch, the multi-map launch of the RPN, the fused pointwise layers, and the operand classes the
"exact bf16 split = fp32 arithmetic" claim rests on.

Error bound: |got - ref| <= TOL * mag per element, mag = conv2d(|x|, |w|) + |b| (what any fp32 summation of the 576 products can be
held to); the fused outputs take the propagated magnitudes (see _fused_refs).  The observed maxima are printed per class and pipe."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

TOL = 1e-6
SENTINEL = 0x7fc0dead                  # a quiet NaN with a payload: outputs that must not be written keep it bit for bit
PIPES = ('split', 'fp32')
# the engine's image geometries (tile h, tile w, scale factor): tests/golden small_b2 / five_b2 / pad_b2, a 96-pixel tile, a
# 251x253 tile at 1x and the 256-pixel tile at 4x (level 0 is 256x256)
GEOMS = [(64, 64, 2), (96, 96, 2), (256, 256, 2), (72, 90, 2), (251, 253, 1), (256, 256, 4)]
EDGE_SHAPES = [(14, 14), (1, 1), (1, 17), (17, 1), (2, 2), (7, 9), (8, 16), (9, 17), (15, 31), (16, 32), (33, 65)]


# ----------------------------------------------------------------------------------------------------------- references
def levels(th, tw, sf):
    """FPN level sizes of an engine built for (th, tw) tiles at scale factor sf (engine.hip: resize, Pad(32), strides 4 .. 32)."""
    hn, wn = (int(th * sf + 0.5) + 31) // 32 * 32, (int(tw * sf + 0.5) + 31) // 32 * 32
    return [(hn >> (2 + s), wn >> (2 + s)) for s in range(4)]


def ref_conv(x, w, b=None, act=0):
    """fp64 3x3 convolution, zero padding 1, of NHWC x (nimg, H, W, 64) with OIHW w; act 1 = ReLU.  -> NHWC float64 (CPU)."""
    y = F.conv2d(x.detach().cpu().double().permute(0, 3, 1, 2), w.detach().cpu().double(), None if b is None else b.detach().cpu().double(), padding=1)
    y = y.permute(0, 2, 3, 1).contiguous()
    return torch.relu(y) if act else y


def mag_conv(x, w, b=None):
    """conv2d(|x|, |w|) + |b| in fp64: the magnitude the error of any fp32 evaluation of the convolution is measured against."""
    m = ref_conv(x.detach().cpu().double().abs(), w.detach().cpu().double().abs())
    return m + b.detach().cpu().double().abs() if b is not None else m


def _fused_refs(y, magy, w2, b2, act2, res2=None, wn1=None, bn1=None):
    """fp64 outputs of the fused epilogue on the activated convolution output y (fp64) and their magnitudes:
    out2 = act2(y w2^T + b2), bound |w2| magy + |b2|;  out3 = res2 + out2, bound that plus |res2|;  outn1 = y wn1 + bn1, bound
    |wn1| magy + |bn1|."""
    d = lambda t: t.detach().cpu().double()
    r = {}
    o2 = y @ d(w2).T + (d(b2) if b2 is not None else 0.0)
    r['out2'] = torch.relu(o2) if act2 else o2
    r['mag2'] = magy @ d(w2).abs().T + (d(b2).abs() if b2 is not None else 0.0)
    if res2 is not None:
        r['out3'] = d(res2) + r['out2']
        r['mag3'] = r['mag2'] + d(res2).abs()
    if wn1 is not None:
        r['outn1'] = y @ d(wn1) + (d(bn1) if bn1 is not None else 0.0)
        r['magn1'] = magy @ d(wn1).abs() + (d(bn1).abs() if bn1 is not None else 0.0)
    return r


OBSERVED = {}


def _within(tag, pipe, got, ref, mag, bad=None):
    """got (any device) vs fp64 ref within TOL * mag; `bad` (bool, broadcastable) masks out elements expected non-finite.
    Records and returns the largest err / mag."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (tag, pipe, got.shape, ref.shape)
    ok = torch.ones_like(got, dtype=torch.bool) if bad is None else ~bad.expand_as(got)
    assert torch.isfinite(got[ok]).all(), f'{tag} [{pipe}]: {int((~torch.isfinite(got[ok])).sum())} non-finite outputs'
    err = (got - ref).abs()[ok]
    m = mag.expand_as(got)[ok]
    over = err > TOL * m
    rel = float((err / m.clamp_min(1e-300)).max()) if err.numel() else 0.0
    key = (tag, pipe)
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), rel)
    print(f'conv3 {tag} [{pipe}]: max err/mag {rel:.3e}')
    assert not over.any(), f'{tag} [{pipe}]: {int(over.sum())}/{over.numel()} outside {TOL:g} * mag (max err/mag {rel:.3e})'
    return rel


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)


def _keeps_sentinel(t):
    return bool((_bits(t) == SENTINEL).all())


def _operands(gen, nimg, H, W, bias=True):
    x = torch.randn(nimg, H, W, 64, generator=gen)
    w = torch.randn(64, 64, 3, 3, generator=gen) / 24.0
    b = 0.5 * torch.randn(64, generator=gen) if bias else None
    return x, w, b


# ----------------------------------------------------------------------------------------------------------- GPU fixtures
@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    return Engine(weights.seeded_state_dict(0), device=0, max_batch=1, tile=(64, 64))


def _conv(eng, x, w, b, act, pipe, **kw):
    """op_conv3 into a sentinel-filled output (an unwritten pixel fails the finiteness check)."""
    out = sentinel(*x.shape)
    return eng.op_conv3(x, w, b, act, pipe=pipe, out=out, **kw)['out']


# ----------------------------------------------------------------------------------------------------------- plain convolution
@pytest.mark.gpu
def test_plain_conv_shapes_vs_fp64(eng):
    """Bias / no bias x none / ReLU on both pipes over every FPN level size the engine builds, the mask head's 14x14 and degenerate
    and tile-boundary maps (the halo tile is 8 x 16 pixels)."""
    gen = torch.Generator().manual_seed(1)
    shapes = sorted({hw for g in GEOMS for hw in levels(*g)} | set(EDGE_SHAPES))
    for H, W in shapes:
        nimg = 1 if H * W > 128 * 128 else 2 if H * W > 4096 else 3
        x, w, b = _operands(gen, nimg, H, W)
        r0, m0 = ref_conv(x, w), mag_conv(x, w)
        xd = x.cuda()
        for bias in (None, b):
            ref = r0 + bias.double() if bias is not None else r0
            mag = m0 + bias.double().abs() if bias is not None else m0
            for act in (0, 1):
                for pipe in PIPES:
                    got = _conv(eng, xd, w, bias, act, pipe)
                    _within(f'plain {nimg}x{H}x{W} bias{int(bias is not None)} act{act}', pipe, got, torch.relu(ref) if act else ref, mag)


@pytest.mark.gpu
def test_tile_counts_around_the_grid(eng):
    """One-tile 8x16 maps give exact tile counts around the persistent grid (one workgroup per CU, dealt over 8 XCDs), then the
    production level 0 (B = 16 at 128x128, 2048 tiles): several tiles per workgroup."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    gen = torch.Generator().manual_seed(2)
    cases = [(n, 8, 16) for n in sorted({1, 7, 8, 9, cus - 1, cus, cus + 1, 2 * cus + 3})] + [(16, 128, 128)]
    for nimg, H, W in cases:
        x, w, b = _operands(gen, nimg, H, W)
        act = 1 if H == 128 else 0
        ref, mag = ref_conv(x, w, b, act), mag_conv(x, w, b)
        xd = x.cuda()
        for pipe in PIPES:
            _within(f'tiles {nimg}x{H}x{W}', pipe, _conv(eng, xd, w, b, act, pipe), ref, mag)


# ----------------------------------------------------------------------------------------------------------- hard operands
def _hard_classes(gen, nimg, H, W):
    """(label, x, w) of the operand classes of test_hip_dense.py::test_split_pipe_hard_operand_classes, laid out for a convolution
    (k = tap * 64 + channel)."""
    sgn = lambda *s: torch.randint(0, 2, s, generator=gen).float() * 2 - 1
    out = []
    # cancellation: channel pairs (a, a) x (w, -w (1 + d)), d ~ 1e-6: every tap's sum cancels to ~1e-6 of sum |a w|
    a = torch.randn(nimg, H, W, 32, generator=gen)
    wv = torch.randn(64, 32, 3, 3, generator=gen)
    d = 1e-6 * torch.randn(64, 32, 3, 3, generator=gen)
    out.append(('cancellation', torch.stack([a, a], -1).reshape(nimg, H, W, 64), torch.stack([wv, -wv * (1 + d)], 2).reshape(64, 64, 3, 3)))
    # just below powers of two: the first round-to-nearest split rounds up a binade (negative residual planes)
    x = torch.exp2(torch.randint(-6, 7, (nimg, H, W, 64), generator=gen).float()) * (2.0 - torch.rand(nimg, H, W, 64, generator=gen) * 2e-3) * sgn(nimg, H, W, 64)
    w = torch.exp2(torch.randint(-6, 7, (64, 64, 3, 3), generator=gen).float()) * (2.0 - torch.rand(64, 64, 3, 3, generator=gen) * 2e-3) * sgn(64, 64, 3, 3)
    out.append(('below powers of two', x, w / 64))
    # subnormal third planes: |v| ~ 2^-110 puts the third bf16 plane below the smallest normal number; products and sums stay normal
    out.append(('x third plane subnormal', torch.randn(nimg, H, W, 64, generator=gen) * 2.0 ** -110, torch.randn(64, 64, 3, 3, generator=gen)))
    out.append(('w third plane subnormal', torch.randn(nimg, H, W, 64, generator=gen), torch.randn(64, 64, 3, 3, generator=gen) * 2.0 ** -110))
    # the top binade: |x| up to 3.38e38 (below 0x7f7f8000, where the first split would round to Inf: the pipe's documented domain
    # limit), weights small enough for finite sums
    x = (torch.rand(nimg, H, W, 64, generator=gen) * 0.5 + 0.5) * 3.38e38 * sgn(nimg, H, W, 64)
    out.append(('top binade', x, torch.randn(64, 64, 3, 3, generator=gen) * 1e-5))
    return out


@pytest.mark.gpu
def test_hard_operand_classes_vs_fp64(eng):
    """Split pipe beside the fp32 pipe, both against fp64, class by class, on a ragged multi-tile map."""
    gen = torch.Generator().manual_seed(3)
    nimg, H, W = 3, 17, 35
    for label, x, w in _hard_classes(gen, nimg, H, W):
        assert torch.isfinite(x).all() and torch.isfinite(w).all()
        ref, mag = ref_conv(x, w), mag_conv(x, w)
        xd = x.cuda()
        for pipe in PIPES:
            _within(f'hard: {label}', pipe, _conv(eng, xd, w, None, 0, pipe), ref, mag)


def _nonfinite_case(nimg=3, H=12, W=20):
    """Inputs with NaN / +-Inf at image corners and edges, on the last row of image i and the first row of image i + 1 (adjacent
    in memory) -> (x, the fp64-referenceable copy with zeros there, expected non-finite mask (nimg, H, W, 1))."""
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(nimg, H, W, 64, generator=gen)
    spots = [(0, 0, 0), (0, 0, W - 1), (1, H - 1, 0), (1, H - 1, W - 1), (0, 5, 0), (2, 0, 7), (2, H - 1, 11), (0, H - 1, 9), (1, 0, 9),
             (1, H - 1, 3), (2, 0, 15), (2, 6, W - 1)]
    vals = [float('nan'), float('inf'), float('-inf')]
    bad = torch.zeros(nimg, H, W, 1, dtype=torch.bool)
    for k, (i, y, xx) in enumerate(spots):
        x[i, y, xx, (7 * k) % 64] = vals[k % 3]
        bad[i, max(y - 1, 0):y + 2, max(xx - 1, 0):xx + 2] = True
    return x, torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0), bad


@pytest.mark.gpu
def test_nonfinite_inputs_stay_in_their_neighbourhood(eng):
    """A NaN / Inf input makes exactly its 3x3 neighbourhood within its own image non-finite (all 64 channels; an Inf may come out as
    NaN on the split pipe); nothing leaks across image boundaries and everything else stays inside the bound."""
    x, xz, bad = _nonfinite_case()
    gen = torch.Generator().manual_seed(5)
    _, w, b = _operands(gen, 1, 1, 1)
    ref, mag = ref_conv(xz, w, b), mag_conv(xz, w, b)
    xd = x.cuda()
    for pipe in PIPES:
        got = _conv(eng, xd, w, b, 0, pipe).cpu()
        nf = ~torch.isfinite(got)
        assert torch.equal(nf, bad.expand_as(got)), (pipe, int((nf != bad.expand_as(got)).sum()))
        _within('non-finite inputs (other outputs)', pipe, got, ref, mag, bad=bad)


# ----------------------------------------------------------------------------------------------------------- device image count
@pytest.mark.gpu
def test_device_image_count(eng):
    """nimg_dev below the capacity (the mask head's det_total): images >= count keep the sentinel bit for bit, images < count are
    bitwise the launch with nimg = count (a count above the capacity is clamped to it); the full count against fp64."""
    gen = torch.Generator().manual_seed(6)
    for cap, H, W in [(1200, 14, 14), (4, 128, 128)]:
        x, w, b = _operands(gen, cap, H, W)
        xd = x.cuda()
        ref, mag = ref_conv(x, w, b, 1), mag_conv(x, w, b)
        for pipe in PIPES:
            for count in sorted({c for c in (0, 1, 7, cap - 1, cap) if c <= cap}) + [cap + 5]:
                n_dev = torch.tensor([count], dtype=torch.int32, device='cuda')
                got = _conv(eng, xd, w, b, 1, pipe, nimg_dev=n_dev)
                assert _keeps_sentinel(got[count:]), (pipe, cap, count)
                if count:
                    assert _same_bits(got[:count], _conv(eng, xd[:count].contiguous(), w, b, 1, pipe)), (pipe, cap, count)
                if count >= cap:
                    _within(f'device count {cap}x{H}x{W}', pipe, got, ref, mag)


# ----------------------------------------------------------------------------------------------------------- fused pointwise layer
@pytest.mark.gpu
def test_fused_pointwise_vs_fp64(eng):
    """N2 in {32, 64} x act2 x store_out (x conv act), on a ragged map and on one where every workgroup takes two tiles: out2 against
    fp64; store_out = 0 leaves `out` alone, store_out = 1 stores bitwise what the plain launch (N2 = 0) stores."""
    gen = torch.Generator().manual_seed(7)
    for nimg, H, W in [(3, 20, 36), (16, 64, 64)]:
        x, w, b = _operands(gen, nimg, H, W)
        xd = x.cuda()
        r0, magy = ref_conv(x, w, b), mag_conv(x, w, b)
        for act in (0, 1):
            y = torch.relu(r0) if act else r0
            plain = _conv(eng, xd, w, b, act, 'split')
            for N2 in (32, 64):
                w2 = torch.randn(N2, 64, generator=gen) / 8.0
                b2 = 0.5 * torch.randn(N2, generator=gen)
                for act2 in (0, 1):
                    ref = _fused_refs(y, magy, w2, b2, act2)
                    for store_out in (0, 1):
                        r = eng.op_conv3(xd, w, b, act, pipe='split', N2=N2, w2=w2, b2=b2, act2=act2, store_out=store_out,
                                         out=sentinel(nimg, H, W, 64), out2=sentinel(nimg, H, W, N2))
                        tag = f'fused {nimg}x{H}x{W} act{act} N2={N2} act2={act2} store_out={store_out}'
                        _within(tag + ' out2', 'split', r['out2'], ref['out2'], ref['mag2'])
                        if store_out:
                            assert _same_bits(r['out'], plain), tag
                        else:
                            assert _keeps_sentinel(r['out']), tag


@pytest.mark.gpu
def test_fused_semantic_head_epilogue_vs_fp64(eng):
    """The semantic head's last conv (engine.hip run_neck_heads): ReLU conv, conv_embedding 64 -> 64 + ReLU (out2), x0 + sem (res2 /
    out3) and the 64 -> 1 logits (wn1 / outn1), with store_out = 0; and the same options with store_out = 1 and no activations."""
    gen = torch.Generator().manual_seed(8)
    for nimg, H, W in [(2, 24, 40), (16, 64, 64)]:
        x, w, b = _operands(gen, nimg, H, W)
        xd = x.cuda()
        r0, magy = ref_conv(x, w, b), mag_conv(x, w, b)
        res2 = torch.randn(nimg, H, W, 64, generator=gen)
        w2, b2 = torch.randn(64, 64, generator=gen) / 8.0, 0.5 * torch.randn(64, generator=gen)
        wn1, bn1 = torch.randn(64, generator=gen) / 8.0, torch.randn(1, generator=gen)
        for act, act2, store_out, with_bn1 in [(1, 1, 0, True), (0, 0, 1, False)]:
            y = torch.relu(r0) if act else r0
            ref = _fused_refs(y, magy, w2, b2, act2, res2=res2, wn1=wn1, bn1=bn1 if with_bn1 else None)
            r = eng.op_conv3(xd, w, b, act, pipe='split', N2=64, w2=w2, b2=b2, act2=act2, store_out=store_out, res2=res2.cuda(), wn1=wn1,
                             bn1=bn1 if with_bn1 else None, out=sentinel(nimg, H, W, 64), out2=sentinel(nimg, H, W, 64),
                             out3=sentinel(nimg, H, W, 64), outn1=sentinel(nimg, H, W))
            tag = f'semantic {nimg}x{H}x{W} act{act} act2={act2} store_out={store_out}'
            _within(tag + ' out2', 'split', r['out2'], ref['out2'], ref['mag2'])
            _within(tag + ' out3', 'split', r['out3'], ref['out3'], ref['mag3'])
            _within(tag + ' outn1', 'split', r['outn1'], ref['outn1'], ref['magn1'])
            if store_out:
                assert _same_bits(r['out'], _conv(eng, xd, w, b, act, 'split')), tag
            else:
                assert _keeps_sentinel(r['out']), tag


@pytest.mark.gpu
def test_multi_map_launch_equals_single_maps(eng):
    """n_more = 1, 2, 3 with the FPN level sizes of three engine geometries at B = 2 and 16: every map's out2 is bitwise what a launch
    of that map alone gives (the RPN's one launch over four levels relies on it), `out` is never written."""
    gen = torch.Generator().manual_seed(9)
    _, w, b = _operands(gen, 1, 1, 1)
    w2, b2 = torch.randn(32, 64, generator=gen) / 8.0, 0.5 * torch.randn(32, generator=gen)
    kw = dict(pipe='split', N2=32, w2=w2, b2=b2, act2=0, store_out=0)
    for th, tw, sf in [(64, 64, 2), (72, 90, 2), (256, 256, 2)]:
        lv = levels(th, tw, sf)
        for B in (2, 16):
            xs = [torch.randn(B, H, W, 64, generator=gen).cuda() for H, W in lv]
            single = [eng.op_conv3(xk, w, b, 1, **kw)['out2'] for xk in xs]
            for n in (1, 2, 3):
                out = sentinel(*xs[0].shape)
                r = eng.op_conv3(xs[0], w, b, 1, more=xs[1:1 + n], out=out, **kw)
                tag = (th, tw, B, n)
                assert _same_bits(r['out2'], single[0]), tag
                for k in range(n):
                    assert _same_bits(r['more_out2'][k], single[k + 1]), (tag, k)
                assert _keeps_sentinel(out), tag


# ----------------------------------------------------------------------------------------------------------- batch independence
@pytest.mark.gpu
def test_batch_independence_and_determinism(eng):
    """An image's outputs are bitwise the same whatever nimg and its position in the batch (the tile distribution over the
    persistent grid changes), and two identical launches are bitwise equal: B = 16 at 128x128 and 1200 images of 14x14."""
    gen = torch.Generator().manual_seed(10)
    w2, b2 = torch.randn(64, 64, generator=gen) / 8.0, 0.5 * torch.randn(64, generator=gen)
    for nimg, H, W in [(16, 128, 128), (1200, 14, 14)]:
        x, w, b = _operands(gen, nimg, H, W)
        xd = x.cuda()
        perm = torch.randperm(nimg, generator=gen).cuda()
        subs = [slice(0, 1), slice(nimg - 1, nimg), slice(3, 8), slice(nimg // 2, nimg)]
        runs = [(pipe, lambda t, pipe=pipe: _conv(eng, t, w, b, 1, pipe)) for pipe in PIPES]
        runs.append(('split fused', lambda t: eng.op_conv3(t, w, b, 1, pipe='split', N2=64, w2=w2, b2=b2, act2=1, store_out=1)['out2']))
        for label, run in runs:
            full = run(xd)
            assert _same_bits(full, run(xd)), (label, nimg, 'repeat')
            assert _same_bits(full[perm], run(xd[perm].contiguous())), (label, nimg, 'permuted')
            for s in subs:
                assert _same_bits(full[s], run(xd[s].contiguous())), (label, nimg, s)


# ----------------------------------------------------------------------------------------------------------- the engine's path
def _engine_cases():
    import golden_util as G
    from nuhtc_amd import synth, weights
    for name in ('small_b2', 'five_b2'):
        g = G.load(name)
        yield name, G.seeded_sd(g), g['tiles']
    yield 'bench B16 256', weights.bench_state_dict(0), synth.nuclei_tiles(16, 256, start=0)


@pytest.mark.gpu
def test_op_is_the_engines_path(hip_device):
    """op_conv3 on the engine's buffers with the checkpoint's weights reproduces the engine bitwise: x{i} = fpn_convs.i(lat{i})
    (fused with the semantic lateral on the split pipe), and rpn{i} = the RPN conv + cls / reg layer (one fused launch over the four
    levels on the split pipe; conv, then the 1x1 product on the fp32 pipe)."""
    from nuhtc_amd.engine import Engine
    for name, sd, tiles in _engine_cases():
        wcat, bcat = torch.zeros(32, 64), torch.zeros(32)
        wcat[:3], wcat[3:15] = sd['rpn_head.rpn_cls.weight'].reshape(3, 64), sd['rpn_head.rpn_reg.weight'].reshape(12, 64)
        bcat[:3], bcat[3:15] = sd['rpn_head.rpn_cls.bias'], sd['rpn_head.rpn_reg.bias']
        rw, rb = sd['rpn_head.rpn_conv.weight'], sd['rpn_head.rpn_conv.bias']
        for pipe, mp in (('split', 0), ('fp32', 1)):
            e = Engine(sd, device=0, max_batch=len(tiles), tile=tiles.shape[1:3], matrix_pipe=mp)
            e(tiles)
            xs = [e.buffer(f'x{i}') for i in range(4)]
            for i in range(4):
                got = _conv(e, e.buffer(f'lat{i}'), sd[f'neck.fpn_convs.{i}.conv.weight'], sd[f'neck.fpn_convs.{i}.conv.bias'], 0, pipe)
                assert _same_bits(got, xs[i]), (name, pipe, i)
            rpn = [e.buffer(f'rpn{i}') for i in range(4)]
            if pipe == 'split':
                r = e.op_conv3(xs[0], rw, rb, 1, pipe='split', N2=32, w2=wcat, b2=bcat, act2=0, store_out=0, more=xs[1:])
                for i, got in enumerate([r['out2']] + r['more_out2']):
                    assert _same_bits(got, rpn[i]), (name, pipe, 'rpn', i)
            else:
                for i in range(4):
                    t = _conv(e, xs[i], rw, rb, 1, 'fp32')
                    got = e.op_gemm(t.reshape(-1, 64), wcat.cuda(), bcat.cuda(), 0, pipe='fp32')
                    assert _same_bits(got, rpn[i].reshape(-1, 32)), (name, pipe, 'rpn', i)
            e.close()
            del e


# ----------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_refusals_leave_the_engine_usable(eng):
    """What the path does not serve is refused with an error (no launch), and the next correct call gives the same bits as before."""
    from nuhtc_amd import hip
    from nuhtc_amd.engine import HipError
    gen = torch.Generator().manual_seed(12)
    x, w, b = _operands(gen, 2, 16, 24)
    xd = x.cuda()
    w2_32, w2_16 = torch.randn(32, 64, generator=gen), torch.randn(16, 64, generator=gen)
    w2_64 = torch.randn(64, 64, generator=gen)
    res2, m1 = torch.randn(2, 16, 24, 64, generator=gen).cuda(), torch.randn(2, 8, 12, 64, generator=gen).cuda()
    good = _conv(eng, xd, w, b, 1, 'split')
    bad_calls = {
        'N2 = 16': dict(N2=16, w2=w2_16),
        'out3 with N2 = 32': dict(N2=32, w2=w2_32, res2=res2),
        'n_more with store_out': dict(N2=32, w2=w2_32, store_out=1, more=[m1]),
        'n_more with out3': dict(N2=64, w2=w2_64, store_out=0, res2=res2, more=[m1]),
        'n_more with outn1': dict(N2=32, w2=w2_32, store_out=0, wn1=torch.randn(64), more=[m1]),
        'n_more = 4': dict(N2=32, w2=w2_32, store_out=0, more=[m1] * 4),
        'fused on the fp32 pipe': dict(N2=32, w2=w2_32, pipe='fp32'),
        'fused N2 = 64 on the fp32 pipe': dict(N2=64, w2=w2_64, store_out=1, pipe='fp32'),
    }
    for label, kw in bad_calls.items():
        kw = dict(kw)
        pipe = kw.pop('pipe', 'split')
        with pytest.raises(HipError):
            eng.op_conv3(xd, w, b, 1, pipe=pipe, **kw)
        assert _same_bits(_conv(eng, xd, w, b, 1, 'split'), good), label
    # maps of H or W <= 0, the launch's own and a further map's (built by hand: the wrapper takes sizes from the tensors)
    wh = np.ascontiguousarray(w.numpy(), dtype=np.float32)
    w2h = np.ascontiguousarray(w2_32.numpy(), dtype=np.float32)
    out, out2, mo2 = sentinel(2, 16, 24, 64), sentinel(2, 16, 24, 32), sentinel(2, 8, 12, 32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for H, W, mH, mW, n_more in [(0, 24, 8, 12, 0), (16, -1, 8, 12, 0), (16, 24, 0, 12, 1), (16, 24, 8, -3, 1)]:
        a = hip.Conv3Args(inp=xd.data_ptr(), out=out.data_ptr(), w=vp(wh), nimg=2, H=H, W=W, act=1, pipe=hip.PIPE_BF16_SPLIT, N2=32 if n_more else 0,
                          w2=vp(w2h) if n_more else None, out2=out2.data_ptr() if n_more else None, n_more=n_more)
        a.more_in[0], a.more_out2[0], a.more_H[0], a.more_W[0] = m1.data_ptr(), mo2.data_ptr(), mH, mW
        assert eng.lib.nuhtc_op_conv3(eng.h, ctypes.byref(a), eng._stream()) == hip.E_INVALID, (H, W, mH, mW)
        assert _same_bits(_conv(eng, xd, w, b, 1, 'split'), good), (H, W, mH, mW)
    assert _keeps_sentinel(out) and _keeps_sentinel(out2) and _keeps_sentinel(mo2)


@pytest.mark.gpu
def test_print_observed_maxima():
    """Summary of the largest err / mag seen per class and pipe in this module (run with -s)."""
    for (tag, pipe), rel in sorted(OBSERVED.items()):
        print(f'max err/mag {rel:.3e}  [{pipe}]  {tag}')


# ----------------------------------------------------------------------------------------------------------- host-only
def _naive(x, w, b, act):
    n, H, W, C = x.shape
    y = np.zeros((n, H, W, w.shape[0]))
    m = np.zeros_like(y)
    for i in range(n):
        for yy in range(H):
            for xx in range(W):
                for ky in range(3):
                    for kx in range(3):
                        sy, sx = yy + ky - 1, xx + kx - 1
                        if 0 <= sy < H and 0 <= sx < W:
                            y[i, yy, xx] += w[:, :, ky, kx] @ x[i, sy, sx]
                            m[i, yy, xx] += np.abs(w[:, :, ky, kx]) @ np.abs(x[i, sy, sx])
    y += b
    m += np.abs(b)
    return (np.maximum(y, 0) if act else y), m


def test_reference_and_bound_vs_naive_loop():
    """ref_conv / mag_conv (NHWC in, OIHW weights, zero padding 1) against a direct loop, and the fused references against a
    direct evaluation."""
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(2, 3, 5, 64, generator=gen)
    w = torch.randn(64, 64, 3, 3, generator=gen)
    b = torch.randn(64, generator=gen)
    for act in (0, 1):
        y, m = _naive(x.double().numpy(), w.double().numpy(), b.double().numpy(), act)
        assert np.allclose(ref_conv(x, w, b, act).numpy(), y, rtol=1e-12, atol=1e-10)
        assert np.allclose(mag_conv(x, w, b).numpy(), m, rtol=1e-12, atol=1e-10)
    y = ref_conv(x, w, b, 1)
    mag = mag_conv(x, w, b)
    assert (y.abs() <= mag + 1e-9).all()
    w2, b2, res2 = torch.randn(32, 64, generator=gen), torch.randn(32, generator=gen), torch.randn(2, 3, 5, 32, generator=gen)
    wn1, bn1 = torch.randn(64, generator=gen), torch.randn(1, generator=gen)
    r = _fused_refs(y, mag, w2, b2, 1, res2=res2, wn1=wn1, bn1=bn1)
    yn, w2n = y.numpy(), w2.double().numpy()
    o2 = np.maximum(np.einsum('nhwc,oc->nhwo', yn, w2n) + b2.double().numpy(), 0)
    assert np.allclose(r['out2'].numpy(), o2, rtol=1e-12, atol=1e-10)
    assert np.allclose(r['out3'].numpy(), o2 + res2.double().numpy(), rtol=1e-12, atol=1e-10)
    assert np.allclose(r['outn1'].numpy(), yn @ wn1.double().numpy() + float(bn1), rtol=1e-12, atol=1e-10)
    assert (r['out2'].abs() <= r['mag2'] + 1e-9).all() and (r['outn1'].abs() <= r['magn1'] + 1e-9).all()
    assert (r['out3'].abs() <= r['mag3'] + 1e-9).all()


def test_levels_and_hard_operands():
    """The level sizes the engine builds, and the hard operand classes are what they claim (finite, in range)."""
    assert levels(64, 64, 2) == [(32, 32), (16, 16), (8, 8), (4, 4)]
    assert levels(72, 90, 2) == [(40, 48), (20, 24), (10, 12), (5, 6)]
    assert levels(251, 253, 1) == [(64, 64), (32, 32), (16, 16), (8, 8)]
    assert levels(256, 256, 4)[0] == (256, 256)
    gen = torch.Generator().manual_seed(14)
    cls = dict((label, (x, w)) for label, x, w in _hard_classes(gen, 1, 4, 5))
    for label, (x, w) in cls.items():
        assert torch.isfinite(x).all() and torch.isfinite(w).all(), label
    x, _ = cls['top binade']
    assert float(x.abs().max()) < 3.3895e38 and float(x.abs().min()) >= 1.69e38
    assert float(cls['x third plane subnormal'][0].abs().max()) < 2.0 ** -100
    x, w = cls['cancellation']
    assert torch.equal(x[..., 0::2], x[..., 1::2])
    xz, x0, bad = _nonfinite_case()
    assert int((~torch.isfinite(xz)).sum()) == 12 and torch.isfinite(x0).all() and bad.sum() > 12
