"""Host-only checks of what tests/test_hip_front.py compares the kernels with: every reference of front_cases.py against an independent form,
and the properties its designed inputs claim.  A wrong reference must not be able to pass quietly on the GPU."""
import numpy as np
import torch
import torch.nn.functional as F

import front_cases as FC


def _resize2x_closed(img):
    """cv2's 8-bit linear resize for an exact x2 factor, from the closed formula in oracle.model.resize2x_u8's docstring:
    (((a + 3 b) >> 2) + ((3 c + 9 d) >> 2) + 2) >> 2 with (a, b) the far row's (far, near) columns and (c, d) the near row's; the far
    neighbour of output index 2 k is k - 1, of 2 k + 1 it is k + 1, clamped to the image."""
    h, w = img.shape[:2]
    s = img.astype(np.int64)

    def near_far(n, size):
        i = np.arange(n)
        near = i // 2
        far = np.clip(np.where(i % 2 == 0, near - 1, near + 1), 0, size - 1)
        return near, far
    yn, yf = near_far(2 * h, h)
    xn, xf = near_far(2 * w, w)
    a, b = s[yf][:, xf], s[yf][:, xn]
    c, d = s[yn][:, xf], s[yn][:, xn]
    return ((((a + 3 * b) >> 2) + ((3 * c + 9 * d) >> 2) + 2) >> 2).astype(np.uint8)


def test_resize_reference_vs_closed_x2_formula_and_copy():
    """The x2 cases of every image kind equal the closed formula, pixel for pixel; scale 1 is the input; the tiles of a call differ and the
    ramps vary along one axis only."""
    for (th, tw, vh, vw, scale) in FC.RESIZE_CASES:
        for kind in FC.IMAGE_KINDS:
            tiles = FC.images(kind, th, tw, seed=3)
            ref = FC.ref_resized_u8(tiles, vh, vw, scale)
            Hv, Wv, Hn, Wn = FC.net_shape(vh, vw, scale)
            assert ref.shape == (FC.B_TILES, Hv, Wv, 3) and Hn % 32 == 0 and Wn % 32 == 0 and 0 <= Hn - Hv < 32 and 0 <= Wn - Wv < 32
            if scale == 2.0:
                for b in range(FC.B_TILES):
                    assert np.array_equal(ref[b], _resize2x_closed(tiles[b, :vh, :vw])), (kind, b)
            if scale == 1.0:
                assert np.array_equal(ref, tiles[:, :vh, :vw])
    # the tiles of a call differ (a wrong tile stride moves values) wherever the kind allows it
    for kind in ('random', 'hramp', 'vramp', 'checker', 'border'):
        t = FC.images(kind, 20, 28, seed=3)
        assert not np.array_equal(t[0], t[1]) and not np.array_equal(t[1], t[2]), kind
    # ramps separate the axes
    assert (np.diff(FC.images('hramp', 20, 28)[0].astype(int), axis=0) == 0).all() and (np.diff(FC.images('vramp', 20, 28)[0].astype(int), axis=1) == 0).all()


def test_normalize_pad_and_recovery():
    """ref_img is the oracle's preprocess (same floats, NCHW there), zero outside the valid part; recover_u8 inverts it exactly."""
    from oracle import model as O
    for mode in (0, 1):
        tiles = FC.images('random', 20, 28, seed=4)
        u = FC.ref_resized_u8(tiles, 20, 28, 2.0)
        Hv, Wv, Hn, Wn = FC.net_shape(20, 28, 2.0)
        img = FC.ref_img(u, mode, Hn, Wn)
        want = O.preprocess(tiles, mode).permute(0, 2, 3, 1).numpy()
        assert img.shape == want.shape and np.array_equal(img, want)
        assert (img[:, Hv:] == 0).all() and (img[:, :, Wv:] == 0).all()
        assert np.array_equal(FC.recover_u8(img, Hv, Wv), (u[..., ::-1] if mode else u).astype(np.int64))


def test_patch_embed_reference_vs_explicit_patches():
    """The convolution of the reference is the dot product of every 4 x 4 x 3 patch with w[o, c, kh, kw] (an explicit gather, no conv2d), the
    norm is torch's; the wholly padded tokens of the cases are where they are claimed, and with a constant bias they come out as beta."""
    th, tw, vh, vw, scale = FC.RESIZE_CASES[-1]
    Hv, Wv, Hn, Wn = FC.net_shape(vh, vw, scale)
    assert Hv % 4 and Wv % 4            # patches straddle the valid edge
    img = FC.ref_img(FC.ref_resized_u8(FC.images('random', th, tw, seed=5), vh, vw, scale), 1, Hn, Wn)
    for wt in (FC.embed_weights(11), FC.embed_weights(13, const_bias=0.5)):
        x = torch.from_numpy(img).double()                                       # (B, Hn, Wn, 3)
        p = x.reshape(FC.B_TILES, Hn // 4, 4, Wn // 4, 4, 3).permute(0, 1, 3, 2, 4, 5)      # (B, ty, tx, kh, kw, c)
        y = torch.einsum('byxhwc,ochw->byxo', p, wt['w'].double()) + wt['b'].double()
        want = F.layer_norm(y.reshape(-1, 96), (96,), wt['g'].double(), wt['beta'].double(), 1e-5)
        got = FC.ref_patch_embed(img, wt)
        assert float((got - want).abs().max()) <= 1e-12
        pad = FC.pad_tokens(vh, vw, scale)
        zero_in = (p.abs().sum((3, 4, 5)) == 0).reshape(-1).numpy()
        assert pad.any() and np.array_equal(pad & zero_in, pad)                   # every claimed token has 48 zero inputs
        if float(wt['b'].std()) == 0.0:
            assert torch.equal(got[torch.from_numpy(pad)].float(), wt['beta'].expand(int(pad.sum()), 96))
        f32 = FC.ref_patch_embed(img, wt, torch.float32)
        assert f32.dtype == torch.float32 and float((f32.double() - got).abs().max()) < 1e-4
    assert any(FC.pad_tokens(c[2], c[3], c[4]).any() for c in FC.RESIZE_CASES[:1])


def test_layernorm_reference_vs_torch():
    for C, rows in FC.LN_CASES:
        for kind in FC.LN_KINDS:
            x, g, b = FC.ln_input(kind, rows, C, seed=7)
            got = FC.ln_ref(x.double(), g.double(), b.double())
            want = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-5)
            assert float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max())), (C, rows, kind)
            if kind == 'const_row':
                assert float((got[rows // 2] - b.double()).abs().max()) <= 1e-12
            if kind == 'offset50':
                assert float((x.mean(1).abs() / x.std(1)).min()) > 20


def test_merge_reference_vs_unfold():
    """The gather order of the reference is nn.Unfold(2, stride 2) with the engine's channel permutation: LayerNorm in Unfold's order with the
    checkpoint's gamma / beta, its columns permuted, equals the reference with the permuted gamma / beta."""
    for (B, H, W, C) in FC.MERGE_CASES + [(1, 4, 2, 96)]:
        x, g_u, b_u = FC.merge_input(B, H, W, C, seed=9, offset=50.0)
        u = F.unfold(x.double().permute(0, 3, 1, 2), kernel_size=2, stride=2).transpose(1, 2).reshape(-1, 4 * C)      # k = c*4 + kh*2+kw
        want = FC.unfold_to_kernel_order(F.layer_norm(u, (4 * C,), g_u.double(), b_u.double(), 1e-5), C)
        got = FC.ref_merge_ln(x, FC.unfold_to_kernel_order(g_u, C), FC.unfold_to_kernel_order(b_u, C))
        assert got.shape == (B * (H // 2) * (W // 2), 4 * C)
        assert float((got - want).abs().max()) <= 1e-10
        # the permutation is the engine's: m.g[q * C + c] = g[c * 4 + q]
        gk = FC.unfold_to_kernel_order(g_u, C)
        assert all(float(gk[q * C + c]) == float(g_u[c * 4 + q]) for q in range(4) for c in (0, 1, C - 1))
        # swapping H and W, or kh and kw, moves the reference
        swapped = FC.ref_merge_ln(x.transpose(1, 2), FC.unfold_to_kernel_order(g_u, C), FC.unfold_to_kernel_order(b_u, C))
        assert swapped.shape != got.shape or float((swapped - got).abs().max()) > 1e-2


def test_lateral_reference_parent_index():
    d = FC.lateral_input(2, 8, 12, 96, seed=21)
    up = FC.upsample_parent(d['parent'], 8, 12)
    want = F.interpolate(d['parent'].permute(0, 3, 1, 2), scale_factor=2, mode='nearest').permute(0, 2, 3, 1)
    assert torch.equal(up, want)
    ref, mag = FC.ref_lateral(d, True, True)
    x = d['x'].double().reshape(-1, 96)
    y = F.layer_norm(x, (96,), d['lg'].double(), d['lb'].double(), 1e-5)
    want = y @ d['w'].double().T + d['b'].double() + up.double().reshape(-1, 64)
    assert float((ref - want).abs().max()) <= 1e-9 and bool((mag >= ref.abs() - 1e-9).all())
    # the parent is asymmetric: another (b, y, x) is another value
    assert len(torch.unique(d['parent'])) == d['parent'].numel()


def _sem_fuse_loop(gs):
    """relu(g0) + sum_i relu(bilinear, align_corners=True) by a plain loop over output pixels (at::upsample_bilinear2d: source index
    y (h - 1) / (H - 1), 0 when h == 1)."""
    B, H, W, C = gs[0].shape
    out = np.maximum(gs[0].double().numpy(), 0)
    for g in gs[1:]:
        a = g.double().numpy()
        h, w = a.shape[1:3]
        for y in range(H):
            fy = y * (h - 1) / (H - 1) if h > 1 else 0.0
            y0 = min(int(fy), h - 1)
            y1, ly = min(y0 + 1, h - 1), fy - y0
            for x in range(W):
                fx = x * (w - 1) / (W - 1) if w > 1 else 0.0
                x0 = min(int(fx), w - 1)
                x1, lx = min(x0 + 1, w - 1), fx - x0
                v = (1 - ly) * ((1 - lx) * a[:, y0, x0] + lx * a[:, y0, x1]) + ly * ((1 - lx) * a[:, y1, x0] + lx * a[:, y1, x1])
                out[:, y, x] += np.maximum(v, 0)
    return out


def test_sem_fuse_reference_vs_plain_loop():
    for (B, H, W) in FC.SEM_CASES:
        for kind in FC.SEM_KINDS:
            gs = FC.sem_input(kind, B, H, W, seed=31)
            ref = FC.ref_sem_fuse(gs)
            assert float(np.abs(ref.numpy() - _sem_fuse_loop(gs)).max()) <= 1e-12, (B, H, W, kind)
            last_row = torch.relu(gs[0][:, -1].double()) + sum(torch.relu(FC.interp_line_ac(g[:, -1], W)) for g in gs[1:])
            last_col = torch.relu(gs[0][:, :, -1].double()) + sum(torch.relu(FC.interp_line_ac(g[:, :, -1], H)) for g in gs[1:])
            assert float((ref[:, -1] - last_row).abs().max()) <= 1e-12 and float((ref[:, :, -1] - last_col).abs().max()) <= 1e-12
            corner = sum(torch.relu(g[:, -1, -1].double()) for g in gs)
            assert float((ref[:, -1, -1] - corner).abs().max()) <= 1e-12
            if kind == 'mixed':       # ReLU after the interpolation is not ReLU before it
                before = FC.ref_sem_fuse([gs[0]] + [torch.relu(g) for g in gs[1:]])
                assert float((before - ref).abs().max()) > 0.1
            if kind == 'neg_level':
                assert float(gs[2].max()) < 0
            if kind == 'probe':
                assert float(ref.sum()) > 0 and int((ref > 0).sum()) <= 25 and float(ref.max()) <= 1.0      # the hat of one coarse pixel: under 5 x 5 fine pixels
    assert FC.SEM_CASES[0][1] >> 3 == 1 and FC.SEM_CASES[0][2] >> 3 == 1 and FC.SEM_CASES[2][1] >> 3 == 1 and FC.SEM_CASES[2][2] >> 3 > 1


def test_pointwise_and_pool_inputs():
    x, w, b = FC.pointwise_input(64, seed=43, extremes=True)
    ref, mag = FC.ref_pointwise(x, w, b)
    assert [round(float(v)) for v in ref[:4]] == [100, -100, 10000, -10000]
    want = np.array([float(np.dot(x[i].double().numpy(), w.double().numpy()) + 0.3) for i in range(64)])
    assert np.abs(ref.numpy() - want).max() <= 1e-9 * np.abs(want).max() and bool((mag >= ref.abs()).all())
    assert (FC.PW_CAP * 16 + 255) // 256 > 8192 and FC.PW_CAP == 784 * 200 and max(FC.PW_COUNTS) * 784 > FC.PW_CAP
    for hw in FC.POOL_CASES:
        maps = FC.pool_input(hw, seed=51)
        ref = FC.ref_pool(maps)
        want = np.concatenate([m.double().numpy().sum(1) / m.shape[1] for m in maps], 1)
        assert ref.shape == (FC.B_TILES, 256) and np.abs(ref.numpy() - want).max() <= 1e-9
        assert torch.equal(ref[0], ref[2]) and not torch.equal(ref[0], ref[1])
        assert float(ref.min()) > 9990
