"""The kernels of the default path that only whole-engine runs reached, op by op on designed inputs (cases and references: front_cases.py,
checked on the CPU by test_front_reference.py): patch_embed_tiles_kernel and preproc_kernel with their host tables, the plain LayerNorm
kernels, merge_ln_kernel, the FPN top-down add in the GEMM epilogue, sem_fuse_kernel, conv1x1_n1_kernel in both forms and the mean pooling.

Every op goes through the host code the engine uses for the same launch (Engine.op_* -> nuhtc_op_*).  Float results are asserted beside torch's
own float32 CPU evaluation of the same inputs: e_hip <= 4 e_f32 + 2e-6 max|ref| (the project's margin for another summation order, as
test_fused_mlp_kernel_vs_fp64); integers exactly.  The observed maxima are printed (run with -s)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import front_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng(hip_device):
    import golden_util as G
    from nuhtc_amd.engine import Engine
    g = G.load('small_b2')
    e = Engine(G.seeded_sd(g), device=0, max_batch=1, tile=g['tiles'].shape[1:3])
    yield e
    e.close()


def _beside_f32(tag, got, r64, r32, factor=4.0):
    """e_hip <= factor * e_f32 + 2e-6 max|ref|, both maxima printed."""
    got = got.detach().cpu().double()
    assert got.shape == r64.shape, (tag, got.shape, r64.shape)
    assert torch.isfinite(got).all(), tag
    e_hip, e_f32, mag = float((got - r64).abs().max()), float((r32.double() - r64).abs().max()), float(r64.abs().max())
    print(f'{tag}: max abs err {e_hip:.2e} (torch fp32 {e_f32:.2e}), |ref| max {mag:.3g}')
    assert e_hip <= factor * e_f32 + 2e-6 * mag, (tag, e_hip, e_f32, mag)
    return e_hip, e_f32


def _sentinel(*shape):
    return torch.full(shape, FC.SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)


def _is_sentinel(t):
    return bool((t.view(torch.int32) == FC.SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------- resize, Normalize, Pad
@pytest.mark.parametrize('case', FC.RESIZE_CASES, ids=lambda c: f'{c[2]}x{c[3]}in{c[0]}x{c[1]}s{c[4]}')
def test_resize_normalize_pad_exact(eng, case):
    """preproc_kernel with the tables of cv_linear_tables against cv2's 8-bit linear resize (oracle.model.cv2_resize_linear_u8, pinned by the
    committed cv2 goldens): the integer u = rint(img * std + mean) equals the reference for every pixel and channel, the float equals numpy's
    float32 (u - mean) * float32(1 / std) within 1e-6, every pixel right of or below the valid size is exactly 0.0, and scale 1 returns the
    input.  Factors 1, 1.25, 1.5, 2, 4, 8, three different tiles per call, both channel modes, seven image kinds."""
    th, tw, vh, vw, scale = case
    Hv, Wv, Hn, Wn = FC.net_shape(vh, vw, scale)
    wt = FC.embed_weights(1)
    for kind in FC.IMAGE_KINDS:
        tiles = FC.images(kind, th, tw, seed=3)
        ref_u = FC.ref_resized_u8(tiles, vh, vw, scale)
        if scale == 1.0:
            assert np.array_equal(ref_u, tiles[:, :vh, :vw])
        dev = torch.from_numpy(tiles).cuda()
        for mode in (0, 1):
            _, img = eng.op_patch_embed(dev, (vh, vw), scale, mode, FC.MEAN, FC.STD, wt['w'], wt['b'], wt['g'], wt['beta'])
            img = img.cpu().numpy()
            want = FC.ref_img(ref_u, mode, Hn, Wn)
            got_u = FC.recover_u8(img, Hv, Wv)
            exp_u = (ref_u[..., ::-1] if mode else ref_u).astype(np.int64)
            bad = got_u != exp_u
            assert not bad.any(), (kind, mode, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert np.abs(img.astype(np.float64) - want).max() <= 1e-6, (kind, mode)
            pad = np.ones((Hn, Wn), bool)
            pad[:Hv, :Wv] = False
            assert (img[:, pad] == 0.0).all(), (kind, mode)


def test_patch_embed_refuses_what_create_refuses(eng):
    """A scale outside [1, 8] or a non-integer scale * valid size is NUHTC_E_INVALID, and nothing is written."""
    from nuhtc_amd import hip
    wt = FC.embed_weights(1)
    tiles = torch.from_numpy(FC.images('random', 20, 28)).cuda()
    h = lambda t: np.ascontiguousarray(t.numpy(), dtype=np.float32)
    wh, bh, gh, lbh = h(wt['w']), h(wt['b']), h(wt['g']), h(wt['beta'])
    f3 = lambda v: (ctypes.c_float * 3)(*v)
    tok = _sentinel(3 * 64 * 64, 96)
    for vh, vw, scale in [(20, 28, 0.5), (20, 28, 8.5), (20, 28, 1.3), (21, 28, 1.5), (20, 27, 1.25), (20, 28, float('nan')), (24, 28, 2.0), (20, 32, 2.0)]:
        rc = eng.lib.nuhtc_op_patch_embed(eng.h, tiles.data_ptr(), 3, 20, 28, vh, vw, scale, 0, f3(FC.MEAN), f3(FC.STD), wh.ctypes.data, bh.ctypes.data,
                                          gh.ctypes.data, lbh.ctypes.data, tok.data_ptr(), None, eng._stream())
        assert rc == hip.E_INVALID, (vh, vw, scale, rc)
    torch.cuda.synchronize()
    assert _is_sentinel(tok)


# ----------------------------------------------------------------------------------------------------------- patch embedding
@pytest.mark.parametrize('case', FC.RESIZE_CASES, ids=lambda c: f'{c[2]}x{c[3]}in{c[0]}x{c[1]}s{c[4]}')
def test_patch_embed_vs_fp64(eng, case):
    """patch_embed_tiles_kernel (resize + Normalize + Pad + Conv2d(3, 96, 4, 4) + LayerNorm(96) from the uint8 tiles) against the float64
    convolution and norm of the reference image, beside torch's float32 CPU chain on the same image.  Random weights with a non-constant bias
    (a transposed (kh, kw, c) order cannot match); valid sizes that are no multiple of 4 network pixels (patches that straddle the edge) and
    patches wholly in the Pad, whose 48 inputs are 0, so the norm sees the bias alone.  With a constant bias those tokens have zero variance:
    they must be finite and equal beta (the float64 reference is beta exactly) within the same bound.  They are not bit-equal: the kernel's
    mean is sum * fl(1 / 96), 2^-25 relative above the bias, the fused multiply-add of acc - sum * fl(1 / 96) keeps that difference, and
    1 / sqrt(eps) = 316 scales it: observed 7.0e-6 for the bias 0.5, below the bound's floor of 2e-6 max|ref|.  No ragged block exists to
    test: the token count B * Hn/4 * Wn/4 is a multiple of 64 because Hn and Wn are multiples of 32, and the kernel takes 32 tokens per block."""
    th, tw, vh, vw, scale = case
    Hv, Wv, Hn, Wn = FC.net_shape(vh, vw, scale)
    assert (3 * (Hn // 4) * (Wn // 4)) % 64 == 0
    padtok = FC.pad_tokens(vh, vw, scale)
    for kind, mode, wt in [('random', 0, FC.embed_weights(11)), ('checker', 1, FC.embed_weights(12)), ('random', 1, FC.embed_weights(13, const_bias=0.5))]:
        tiles = FC.images(kind, th, tw, seed=5)
        img = FC.ref_img(FC.ref_resized_u8(tiles, vh, vw, scale), mode, Hn, Wn)
        r64, r32 = FC.ref_patch_embed(img, wt), FC.ref_patch_embed(img, wt, torch.float32)
        tok, _ = eng.op_patch_embed(torch.from_numpy(tiles).cuda(), (vh, vw), scale, mode, FC.MEAN, FC.STD, wt['w'], wt['b'], wt['g'], wt['beta'], want_img=False)
        _, e_f32 = _beside_f32(f'patch_embed {case} {kind} mode {mode}', tok, r64, r32)
        if float(wt['b'].std()) == 0.0 and padtok.any():
            rows = tok.cpu()[torch.from_numpy(padtok)]
            assert torch.equal(r64[torch.from_numpy(padtok)], wt['beta'].double().expand_as(rows))
            e_pad = float((rows.double() - wt['beta'].double()).abs().max())
            print(f'patch_embed {case}: {int(padtok.sum())} tokens wholly in the Pad, constant bias: max |tok - beta| {e_pad:.2e}')
            assert torch.isfinite(rows).all() and e_pad <= 4.0 * e_f32 + 2e-6 * float(r64.abs().max()), e_pad


# ----------------------------------------------------------------------------------------------------------- plain LayerNorm
@pytest.mark.parametrize('C,rows', FC.LN_CASES)
def test_plain_layernorm_vs_fp64(eng, C, rows):
    """layernorm96_kernel (four rows per half-wave, tail reads clamped to rows - 1) and layernorm_kernel<1, 2, 3> without maps against float64,
    beside torch's float32 layer_norm: normal rows, a common offset of 50 sigma, a constant row (variance 0), a row of 1e-20 (eps dominates).
    The output sits between guard rows of sentinels, which must keep their bits."""
    G_ = 2
    for kind in FC.LN_KINDS:
        x, g, b = FC.ln_input(kind, rows, C, seed=7)
        r64 = FC.ln_ref(x.double(), g.double(), b.double())
        r32 = F.layer_norm(x, (C,), g, b, 1e-5)
        buf = _sentinel(rows + 2 * G_, C)
        eng.op_layernorm(x.cuda(), g.cuda(), b.cuda(), out=buf[G_:G_ + rows])
        assert _is_sentinel(buf[:G_]) and _is_sentinel(buf[G_ + rows:]), (kind, 'guard rows written')
        _beside_f32(f'layernorm C{C} rows {rows} {kind}', buf[G_:G_ + rows], r64, r32)


# ----------------------------------------------------------------------------------------------------------- PatchMerging gather + LN(4C)
@pytest.mark.parametrize('case', FC.MERGE_CASES, ids=str)
def test_merge_ln_vs_fp64(eng, case):
    """merge_ln_kernel<6, 12, 24> (PatchMerging on the fp32 pipe) against float64 LayerNorm over the 2 x 2 gather in the kernel's order
    (which test_front_reference.py ties to nn.Unfold and the engine's permutation), beside torch's float32 layer_norm.  Tokens carry their
    index, so a wrong (kh, kw) or swapped H / W moves values; with and without a common offset of 50 sigma; guard rows of sentinels."""
    B, H, W, C = case
    rows = B * (H // 2) * (W // 2)
    for offset in (0.0, 50.0):
        x, g_u, b_u = FC.merge_input(B, H, W, C, seed=9, offset=offset)
        g, b = FC.unfold_to_kernel_order(g_u, C), FC.unfold_to_kernel_order(b_u, C)
        r64, r32 = FC.ref_merge_ln(x, g, b), FC.ref_merge_ln(x, g, b, torch.float32)
        buf = _sentinel(rows + 4, 4 * C)
        eng.op_merge_ln(x.cuda(), g.contiguous().cuda(), b.contiguous().cuda(), out=buf[2:2 + rows])
        assert _is_sentinel(buf[:2]) and _is_sentinel(buf[2 + rows:])
        _beside_f32(f'merge_ln {case} offset {offset}', buf[2:2 + rows], r64, r32)


def test_merge_ln_refuses_odd_sides(eng):
    from nuhtc_amd import hip
    x = torch.randn(1, 6, 6, 96).cuda()
    g = torch.ones(384).cuda()
    out = _sentinel(9, 384)
    for H, W in [(5, 6), (6, 5), (3, 3)]:
        rc = eng.lib.nuhtc_op_merge_ln(eng.h, x.data_ptr(), g.data_ptr(), g.data_ptr(), out.data_ptr(), 1, H, W, 96, eng._stream())
        assert rc == hip.E_INVALID, (H, W, rc)
    torch.cuda.synchronize()
    assert _is_sentinel(out)


# ----------------------------------------------------------------------------------------------------------- FPN lateral + top-down add
@pytest.mark.parametrize('case', FC.LATERAL_CASES, ids=str)
def test_fpn_lateral_top_down_vs_fp64(eng, case):
    """The FPN laterals as run_fpn launches them, with and without the stage's output norm in the A path and with and without the parent
    (GemmParams::up: the nearest-upsampled coarser lateral added in the epilogue), against float64 LN(x) W^T + b + parent[b, y // 2, x // 2].
    Error relative to |LN x| |W|^T + |b| + |parent|, beside the two-kernel form (torch LN, the split GEMM op, the add on the host) with the
    limits of test_ln_gemm_kernel_vs_fp64: rms <= 1.5x + 2e-8, max <= 2e-6 (2e-5 with a 50 sigma offset)."""
    B, H, W, C = case
    for offset in (0.0, 50.0):
        d = FC.lateral_input(B, H, W, C, seed=21, offset=offset)
        xd, pd = d['x'].cuda(), d['parent'].cuda()
        for norm in (True, False):
            xin = F.layer_norm(d['x'].reshape(-1, C), (C,), d['lg'], d['lb'], 1e-5) if norm else d['x'].reshape(-1, C)
            two0 = eng.op_gemm(xin.cuda(), d['w'].cuda(), d['b'].cuda(), 0, pipe='split').cpu()
            for with_parent in (True, False):
                ref, mag = FC.ref_lateral(d, norm, with_parent)
                out = eng.op_fpn_lateral(xd, d['w'], d['b'], d['lg'] if norm else None, d['lb'] if norm else None, pd if with_parent else None)
                out = out.cpu().reshape(-1, 64).double()
                two = (two0 + FC.upsample_parent(d['parent'], H, W).reshape(-1, 64) if with_parent else two0).double()
                e1, e2 = (out - ref).abs() / mag, (two - ref).abs() / mag
                rms1, rms2 = float((e1 ** 2).mean().sqrt()), float((e2 ** 2).mean().sqrt())
                print(f'fpn lateral {case} offset {offset} norm {norm} parent {with_parent}: max {float(e1.max()):.2e} rms {rms1:.2e} | two-kernel form max {float(e2.max()):.2e} rms {rms2:.2e}')
                assert torch.isfinite(out).all()
                assert rms1 <= 1.5 * rms2 + 2e-8, (case, offset, norm, with_parent, rms1, rms2)
                assert float(e1.max()) <= (2e-5 if offset >= 50 else 2e-6), (case, offset, norm, with_parent, float(e1.max()))


# ----------------------------------------------------------------------------------------------------------- semantic fusion
@pytest.mark.parametrize('case', FC.SEM_CASES, ids=str)
def test_sem_fuse_vs_fp64(eng, case):
    """sem_fuse_kernel (align-corners bilinear upsampling of three levels with float32 coordinates, ReLU after the interpolation, the h > 1
    guard of a 1 x 1 or 1 x w level) against float64 F.interpolate per level, beside torch's float32 CPU evaluation.  The last row and column
    of the output are also compared with the ReLU of the coarse maps' last row and column interpolated along the other axis with exact rational
    coordinates: float32 sy * y may land just below an integer there, and the result must not move by more than the bound."""
    B, H, W = case
    for kind in FC.SEM_KINDS:
        gs = FC.sem_input(kind, B, H, W, seed=31)
        r64, r32 = FC.ref_sem_fuse(gs), FC.ref_sem_fuse(gs, torch.float32)
        out = eng.op_sem_fuse(*[g.cuda() for g in gs]).cpu()
        e_hip, e_f32 = _beside_f32(f'sem_fuse {case} {kind}', out, r64, r32)
        bound = 4.0 * e_f32 + 2e-6 * float(r64.abs().max())
        last_row = torch.relu(gs[0][:, -1].double()) + sum(torch.relu(FC.interp_line_ac(g[:, -1], W)) for g in gs[1:])
        last_col = torch.relu(gs[0][:, :, -1].double()) + sum(torch.relu(FC.interp_line_ac(g[:, :, -1], H)) for g in gs[1:])
        assert float((out[:, -1].double() - last_row).abs().max()) <= bound, (case, kind, 'last row')
        assert float((out[:, :, -1].double() - last_col).abs().max()) <= bound, (case, kind, 'last column')
        if kind == 'neg_level':        # the negative level adds nothing: the same output without it
            zero = [gs[0], gs[1], torch.full_like(gs[2], -1.0), gs[3]]
            assert torch.equal(eng.op_sem_fuse(*[g.cuda() for g in zero]).cpu(), out)


# ----------------------------------------------------------------------------------------------------------- pointwise 64 -> 1
def _pw_bounds(x, w, b):
    ref, mag = FC.ref_pointwise(x, w, b)
    return ref, 4e-7 * mag


@pytest.mark.parametrize('rows', FC.PW_FIXED_ROWS)
def test_pointwise64_fixed_rows_vs_fp64(eng, rows):
    """conv1x1_n1_kernel in its fixed-row form (sem_pred on the fp32 pipe): |err| <= 4e-7 (|x| . |w| + |b|), the split-pipe test's fp32
    level; the row behind the last keeps the sentinel."""
    x, w, b = FC.pointwise_input(rows, seed=41)
    ref, bound = _pw_bounds(x, w, b)
    y = _sentinel(rows + 16)
    eng.op_pointwise64(x.cuda(), w.cuda(), b.cuda(), y[:rows])
    err = (y[:rows].cpu().double() - ref).abs()
    print(f'pointwise64 fixed rows {rows}: max err / (|x|.|w| + |b|) {float((err / (bound / 4e-7)).max()):.2e}')
    assert (err <= bound).all(), float((err / bound).max())
    assert _is_sentinel(y[rows:])


def test_pointwise64_device_count_and_sigmoid(eng):
    """The device-count form (the 28 x 28 mask probabilities of every tile): a capacity of 784 * 200 rows is 9800 blocks, over the 8192-block
    cap, so the stride loop runs; *rows_dev = 0, 1, 37, 200 and 500 (clamped to the capacity) with rows_mul = 784.  Rows at and beyond the count
    keep the sentinel.  Before the sigmoid |err| <= 4e-7 (|x| . |w| + |b|); after it the output is within 2 ulp of float32 at the float64 value
    plus a quarter of that bound (d sigma <= 1 / 4), lies in [0, 1] and is never NaN, with pre-activations of +-100 and +-1e4 among the rows."""
    cap, mul = FC.PW_CAP, 784
    x, w, b = FC.pointwise_input(cap, seed=43, extremes=True)
    ref, bound = _pw_bounds(x, w, b)
    assert [round(float(v)) for v in ref[:4]] == [100, -100, 10000, -10000]
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    sig = torch.sigmoid(ref)
    sig_bound = 2.0 * torch.from_numpy(np.spacing(sig.float().numpy()).astype(np.float64)) + 0.25 * bound
    for count in FC.PW_COUNTS:
        live = min(count * mul, cap)
        cnt = torch.tensor([count], dtype=torch.int32, device='cuda')
        for sigmoid in (False, True):
            y = _sentinel(cap)
            eng.op_pointwise64(xd, wd, bd, y, rows_dev=cnt, rows_mul=mul, sigmoid=sigmoid)
            assert _is_sentinel(y[live:]), (count, sigmoid, 'rows beyond the count written')
            got = y[:live].cpu().double()
            assert torch.isfinite(got).all(), (count, sigmoid)
            if sigmoid:
                assert bool(((got >= 0.0) & (got <= 1.0)).all()), (count, 'outside [0, 1]')
                err, lim = (got - sig[:live]).abs(), sig_bound[:live]
            else:
                err, lim = (got - ref[:live]).abs(), bound[:live]
            if live:
                print(f'pointwise64 count {count} sigmoid {sigmoid}: max err / bound {float((err / lim).max()):.3f}')
            assert bool((err <= lim).all()), (count, sigmoid, float((err / lim).max()))


# ----------------------------------------------------------------------------------------------------------- mean pooling
@pytest.mark.parametrize('hw', FC.POOL_CASES, ids=str)
def test_fpn_mean_pool_rounding_and_placement(eng, hw):
    """fpn_mean_pool_kernel + fpn_mean_pool_final_kernel on maps with a large common offset (1e4 + noise): the output is float32 of the float64
    mean or its neighbour (the file's claim: a correctly rounded mean up to one fp32 rounding), and the same tile at batch positions 0 and 2
    gives the same bits.  One pixel per level; one pixel over a chunk; whole chunks and a chunk less one pixel."""
    maps = FC.pool_input(hw, seed=51)
    feat = eng.op_fpn_mean_pool([m.cuda() for m in maps]).cpu()
    ref = FC.ref_pool(maps)
    r32 = ref.float().numpy()
    got = feat.numpy()
    ulps = np.abs(got.astype(np.float64) - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)
    print(f'fpn_mean_pool hw {hw}: max distance from float32(float64 mean) {ulps.max():.2f} ulp, exact in {float((ulps == 0).mean()):.3f}')
    assert np.isfinite(got).all() and ulps.max() <= 1.0, float(ulps.max())
    assert np.abs(got.astype(np.float64) - ref.numpy()).max() <= 1.5 * float(np.spacing(np.float32(1e4)))
    assert torch.equal(feat[0].view(torch.int32), feat[2].view(torch.int32))
    assert not torch.equal(feat[0], feat[1])
