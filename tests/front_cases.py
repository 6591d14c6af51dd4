"""Designed inputs and plain references of tests/test_hip_front.py: the front of the path (cv2's 8-bit linear resize, channel swap, Normalize,
zero Pad, patch embedding, the plain LayerNorms, PatchMerging's gather + norm), the FPN top-down add, the semantic fusion, the 64 -> 1 pointwise
layer and the mean pooling.  Every reference is a float64 (or integer) restatement written from the mmdet / OpenCV semantics it cites, not from
the kernels; tests/test_front_reference.py checks each against an independent form on the CPU.

Shapes are the smallest at which the named edge exists (see the lists below)."""
import numpy as np
import torch
import torch.nn.functional as F

MEAN = (123.675, 116.28, 103.53)     # the config's img_norm_cfg
STD = (58.395, 57.12, 57.375)
SENTINEL = 0x7fc0dead                # a quiet NaN with a payload: memory that must not be written keeps it bit for bit
POOL_CHUNK = 256                     # csrc/common.h

# ----------------------------------------------------------------------------------------------------------- resize, Normalize, Pad
# (buffer h, buffer w, valid h, valid w, scale): the network input is ceil32 of scale * valid
#   20 x 28 x2    the path's factor; 40 x 56 in a 64 x 64 input: the right-hand and bottom patches lie wholly in the Pad
#   16 x 16 x1    cv2 copies
#   8 x 12 x4, 4 x 4 x8   the other integer factors, 8 the largest the header allows; 32 x 48 and 32 x 32 have no Pad at all
#   20 x 28 x1.5, 16 x 24 x1.25   fractional factors with integer scale * valid: weights other than 512 / 1536
#   21 x 27 x2 in a 24 x 32 buffer: 42 x 54 is no multiple of 4 network pixels, so patches straddle the valid edge (and others lie
#                 wholly in the Pad), and the buffer's row pitch differs from the image's width
RESIZE_CASES = [(20, 28, 20, 28, 2.0), (16, 16, 16, 16, 1.0), (8, 12, 8, 12, 4.0), (20, 28, 20, 28, 1.5), (16, 24, 16, 24, 1.25), (4, 4, 4, 4, 8.0),
                (24, 32, 21, 27, 2.0)]
IMAGE_KINDS = ('random', 'zeros', 'full', 'hramp', 'vramp', 'checker', 'border')
B_TILES = 3


def images(kind, h, w, seed=0, B=B_TILES):
    """(B, h, w, 3) uint8, different content per tile where the kind allows it (a wrong tile stride then moves values)."""
    rng = np.random.RandomState(seed)
    t = np.zeros((B, h, w, 3), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for b in range(B):
        if kind == 'random':
            t[b] = rng.randint(0, 256, (h, w, 3))
        elif kind == 'full':
            t[b] = 255
        elif kind == 'hramp':          # varies along x only; the three channels differ, so a swap shows
            t[b] = ((xx * 255 // max(w - 1, 1) + 37 * b)[..., None] + np.array([0, 85, 170])) % 256
        elif kind == 'vramp':
            t[b] = ((yy * 255 // max(h - 1, 1) + 37 * b)[..., None] + np.array([0, 85, 170])) % 256
        elif kind == 'checker':        # 0 / 255 at every neighbour: the largest truncation in the two >> 16 products
            t[b] = (((yy + xx + b) & 1) * 255)[..., None]
        elif kind == 'border':         # the border taps: first / last rows and columns against the rest
            ring = (yy == 0) | (yy == h - 1) | (xx == 0) | (xx == w - 1)
            if b == 0:
                t[b] = np.where(ring, 255, 0)[..., None]
            elif b == 1:
                t[b] = np.where(ring, 0, 255)[..., None]
            else:
                t[b] = np.where(ring[..., None], 255, rng.randint(0, 256, (h, w, 3)))
    return t


def net_shape(vh, vw, scale):
    """img_shape (mmcv.rescale_size: int(size * scale + 0.5)) and pad_shape (Pad(size_divisor=32))."""
    Hv, Wv = int(vh * scale + 0.5), int(vw * scale + 0.5)
    return Hv, Wv, -(-Hv // 32) * 32, -(-Wv // 32) * 32


def ref_resized_u8(tiles, vh, vw, scale):
    """(B, Hv, Wv, 3) uint8: cv2.resize(INTER_LINEAR) of the valid part of every tile (mmdet transforms.py:207-236 -> mmcv.imrescale), by the
    oracle's restatement that the committed cv2 goldens pin."""
    from oracle import model as O
    Hv, Wv, _, _ = net_shape(vh, vw, scale)
    return np.stack([O.cv2_resize_linear_u8(t[:vh, :vw], Wv, Hv) for t in tiles])


def ref_img(u8, mode, Hn, Wn):
    """Normalize (mmcv.imnormalize: channel swap first, then float32 (x - mean) * float32(1 / std), transforms.py:686-700) and the zero Pad to
    (Hn, Wn) (transforms.py:570-) of resized uint8 images (B, Hv, Wv, 3) -> float32 (B, Hn, Wn, 3)."""
    B, Hv, Wv, _ = u8.shape
    u = u8[..., ::-1] if mode else u8
    v = (u.astype(np.float32) - np.array(MEAN, np.float32)) * (1.0 / np.array(STD, np.float64)).astype(np.float32)
    out = np.zeros((B, Hn, Wn, 3), np.float32)
    out[:, :Hv, :Wv] = v
    return out


def recover_u8(img, Hv, Wv):
    """The integers behind a normalised image: rint(img * std + mean) over the valid part (float64)."""
    return np.rint(img[:, :Hv, :Wv].astype(np.float64) * np.array(STD) + np.array(MEAN)).astype(np.int64)


# ----------------------------------------------------------------------------------------------------------- patch embedding
def embed_weights(seed, const_bias=None):
    """Random 4x4 stride-4 convolution (96, 3, 4, 4) with a non-constant bias (or the constant `const_bias`) and LN gamma / beta.  Random
    weights are the layout check: a transposed (kh, kw, c) order cannot match the reference."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(96, 3, 4, 4, generator=gen) / 48 ** 0.5
    b = torch.full((96,), float(const_bias)) if const_bias is not None else 0.5 * torch.randn(96, generator=gen)
    return dict(w=w, b=b, g=1.0 + 0.2 * torch.randn(96, generator=gen), beta=0.2 * torch.randn(96, generator=gen))


def ln_ref(x, g, b, eps=1e-5):
    """LayerNorm over the last axis in the dtype of x (biased variance, torch.nn.LayerNorm)."""
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g.to(x.dtype) + b.to(x.dtype)


def ref_patch_embed(img, wt, dtype=torch.float64):
    """PatchEmbed (mmdet/models/utils/transformer.py:236-257): Conv2d(3, 96, 4, stride 4) of the padded image (B, Hn, Wn, 3), tokens in raster
    order, LayerNorm(96) -> (B * Hn/4 * Wn/4, 96) in `dtype` (float32: torch's own CPU chain on the same inputs)."""
    x = torch.from_numpy(np.ascontiguousarray(img)).permute(0, 3, 1, 2).to(dtype)
    y = F.conv2d(x, wt['w'].to(dtype), wt['b'].to(dtype), stride=4).permute(0, 2, 3, 1).reshape(-1, 96)
    if dtype == torch.float64:
        return ln_ref(y, wt['g'].double(), wt['beta'].double())
    return F.layer_norm(y, (96,), wt['g'], wt['beta'], 1e-5)


def pad_tokens(vh, vw, scale, B=B_TILES):
    """Boolean (B * Hn/4 * Wn/4,): the tokens whose 4 x 4 patch lies wholly in the Pad (all 48 inputs are 0)."""
    Hv, Wv, Hn, Wn = net_shape(vh, vw, scale)
    ty, tx = np.mgrid[0:Hn // 4, 0:Wn // 4]
    m = (4 * ty >= Hv) | (4 * tx >= Wv)
    return np.broadcast_to(m, (B,) + m.shape).reshape(-1)


# ----------------------------------------------------------------------------------------------------------- plain LayerNorm
# C = 96: four rows per half-wave, eight half-waves per block: the tails 1, 3, 4, 5 of a group, 31, 32, 33 of a block, 257 = several blocks
# C = 192 / 384 / 768: one row per wave, four per block (layernorm_kernel<1, 2, 3>)
LN_CASES = [(96, r) for r in (1, 3, 4, 5, 31, 32, 33, 257)] + [(C, r) for C in (192, 384, 768) for r in (1, 4, 5, 130)]
LN_KINDS = ('normal', 'offset50', 'const_row', 'tiny_row')


def ln_input(kind, rows, C, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=gen) * (1.0 + torch.rand(rows, 1, generator=gen))
    if kind == 'offset50':             # a common offset of 50 sigma per row
        x = x + 50.0 * (1.0 + torch.rand(rows, 1, generator=gen)) * torch.randn(rows, 1, generator=gen).sign()
    elif kind == 'const_row':          # variance 0: the row comes out as beta
        x[rows // 2] = 3.25
    elif kind == 'tiny_row':           # eps dominates the variance
        x[rows // 2] = 1e-20 * torch.randn(C, generator=gen).sign()
    g = 1.0 + 0.2 * torch.randn(C, generator=gen)
    b = 0.2 * torch.randn(C, generator=gen)
    return x, g, b


# ----------------------------------------------------------------------------------------------------------- PatchMerging gather + LN(4C)
MERGE_CASES = [(2, 4, 6, 96), (1, 2, 2, 192), (3, 6, 4, 384)]


def merge_input(B, H, W, C, seed, offset=0.0):
    """Tokens that carry their own index -- (b, y, x) in the integer part of every channel -- plus noise, so a wrong (kh, kw) or swapped H / W
    moves values by >= 1; `offset`: a common offset per token, as for the plain norm.  g / b (4C,) in nn.Unfold's order k = c*4 + kh*2+kw."""
    gen = torch.Generator().manual_seed(seed)
    idx = torch.arange(B * H * W, dtype=torch.float32).reshape(B, H, W, 1)
    x = idx + torch.randn(B, H, W, C, generator=gen) + offset * torch.randn(B, H, W, 1, generator=gen).sign()
    g = 1.0 + 0.2 * torch.randn(4 * C, generator=gen)
    b = 0.2 * torch.randn(4 * C, generator=gen)
    return x, g, b


def unfold_to_kernel_order(v, C):
    """A (..., 4C) vector from nn.Unfold's column order k = c*4 + q to the gather order k' = q*C + c (q = kh*2+kw): the permutation the
    engine applies to the merging norm and reduction weight (transformer.py:363-385)."""
    return v.reshape(*v.shape[:-1], C, 4).transpose(-1, -2).reshape(*v.shape[:-1], 4 * C)


def ref_merge_ln(x, g_k, b_k, dtype=torch.float64):
    """LayerNorm(4C) of the 2 x 2 gather in the kernel's order: row (b, y2, x2), column (kh*2+kw)*C + c = x[b, 2 y2 + kh, 2 x2 + kw, c]."""
    B, H, W, C = x.shape
    xd = x.to(dtype)
    parts = [xd[:, kh::2, kw::2, :] for kh in (0, 1) for kw in (0, 1)]
    u = torch.cat(parts, -1).reshape(-1, 4 * C)
    if dtype == torch.float64:
        return ln_ref(u, g_k.double(), b_k.double())
    return F.layer_norm(u, (4 * C,), g_k, b_k, 1e-5)


# ----------------------------------------------------------------------------------------------------------- FPN lateral + top-down add
LATERAL_CASES = [(2, 8, 12, 96), (3, 4, 4, 768), (1, 16, 8, 192)]


def lateral_input(B, H, W, C, seed, offset=0.0):
    gen = torch.Generator().manual_seed(seed)
    T = B * H * W
    x = torch.randn(T, C, generator=gen) * (1.0 + torch.rand(T, 1, generator=gen)) + offset * torch.randn(T, 1, generator=gen).sign()
    w = torch.randn(64, C, generator=gen) / C ** 0.5
    b = 0.1 * torch.randn(64, generator=gen)
    lg = 1.0 + 0.2 * torch.randn(C, generator=gen)
    lb = 0.1 * torch.randn(C, generator=gen)
    n = B * (H // 2) * (W // 2) * 64
    parent = (torch.arange(n, dtype=torch.float32) / 7.0).reshape(B, H // 2, W // 2, 64)      # asymmetric: (y >> 1, x >> 1, b) errors show
    return dict(x=x.reshape(B, H, W, C), w=w, b=b, lg=lg, lb=lb, parent=parent)


def upsample_parent(parent, H, W):
    """F.interpolate(scale_factor=2, mode='nearest') of the coarser lateral (fpn.py:166-173): out[b, y, x] = parent[b, y // 2, x // 2]."""
    return parent[:, torch.arange(H) // 2][:, :, torch.arange(W) // 2]


def ref_lateral(d, norm, with_parent):
    """float64 LN(x) W^T + b + parent[b, y // 2, x // 2] and the magnitude its error is relative to, (B*H*W, 64) each."""
    B, H, W, C = d['x'].shape
    x = d['x'].double().reshape(-1, C)
    y = ln_ref(x, d['lg'].double(), d['lb'].double()) if norm else x
    ref = y @ d['w'].double().T + d['b'].double()
    mag = y.abs() @ d['w'].double().abs().T + d['b'].double().abs()
    if with_parent:
        up = upsample_parent(d['parent'].double(), H, W).reshape(-1, 64)
        ref, mag = ref + up, mag + up.abs()
    return ref, mag


# ----------------------------------------------------------------------------------------------------------- semantic fusion
# (1, 8, 8): level 3 is 1 x 1 (both scales of the h > 1 guard); (2, 16, 24): more than one block, W != H; (2, 8, 40): only the height of level 3 is 1
SEM_CASES = [(1, 8, 8), (2, 16, 24), (2, 8, 40)]
SEM_KINDS = ('mixed', 'neg_level', 'probe')


def sem_input(kind, B, H, W, seed):
    """g0..g3 (B, H >> i, W >> i, 64).  mixed: signs differ at neighbouring coarse pixels, so ReLU after the interpolation differs from ReLU
    before it; neg_level: level 2 is negative everywhere (it must add nothing); probe: a single coarse pixel of level 1 is 1, all else 0."""
    gen = torch.Generator().manual_seed(seed)
    gs = [torch.randn(B, H >> i, W >> i, 64, generator=gen) for i in range(4)]
    if kind == 'neg_level':
        gs[2] = -gs[2].abs() - 0.1
    elif kind == 'probe':
        gs = [torch.zeros_like(g) for g in gs]
        gs[1][B - 1, (H >> 1) - 2, (W >> 1) - 3, 5] = 1.0
    return gs


def ref_sem_fuse(gs, dtype=torch.float64):
    """FusedSemanticHead's fusion (fused_semantic_head.py:97-104) on maps that already went through their 1x1 lateral:
    relu(g0) + sum_i relu(F.interpolate(g_i, size, mode='bilinear', align_corners=True))."""
    B, H, W, _ = gs[0].shape
    out = torch.relu(gs[0].to(dtype))
    for g in gs[1:]:
        up = F.interpolate(g.to(dtype).permute(0, 3, 1, 2), size=(H, W), mode='bilinear', align_corners=True)
        out = out + torch.relu(up).permute(0, 2, 3, 1)
    return out


def interp_line_ac(v, n):
    """Align-corners linear interpolation of v (..., m, C) along its second-to-last axis to n samples, float64, coordinates as exact rationals
    i (m - 1) / (n - 1) (integer arithmetic picks the cell: the last sample is exactly the last input)."""
    m = v.shape[-2]
    v = v.double()
    if m == 1:
        return v.expand(*v.shape[:-2], n, v.shape[-1]).clone()
    i = torch.arange(n)
    num = i * (m - 1)
    i0 = torch.clamp(num // (n - 1), max=m - 1)
    i1 = torch.clamp(i0 + 1, max=m - 1)
    fr = ((num - i0 * (n - 1)).double() / (n - 1))[:, None]
    return v[..., i0, :] * (1 - fr) + v[..., i1, :] * fr


# ----------------------------------------------------------------------------------------------------------- pointwise 64 -> 1
PW_FIXED_ROWS = (1, 17, 4099)          # one row, one ragged block, several blocks and a ragged last one
PW_CAP = 784 * 200                     # 9800 blocks of 16 rows: over the 8192-block cap, so the stride loop runs
PW_COUNTS = (0, 1, 37, 200, 500)       # *rows_dev; rows_mul = 784; 500 clamps to the capacity
PW_EXTREMES = (100.0, -100.0, 1e4, -1e4)


def pointwise_input(rows, seed, extremes=False):
    """x (rows, 64), w (64,), b (1,); with `extremes` the first rows of x are scaled so that w . x + b is +-100 and +-1e4."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, 64, generator=gen)
    w = torch.randn(64, generator=gen) / 8.0
    b = torch.tensor([0.3])
    if extremes:
        for i, t in enumerate(PW_EXTREMES):
            if i < rows:
                x[i] = (t - 0.3) * w / float(w @ w)
    return x, w, b


def ref_pointwise(x, w, b):
    """float64 w . x + b and the magnitude |x| . |w| + |b| per row."""
    return x.double() @ w.double() + b.double(), x.double().abs() @ w.double().abs() + b.double().abs()


# ----------------------------------------------------------------------------------------------------------- mean pooling
# one pixel per level; one pixel over a chunk, sizes below it; whole chunks, a chunk less one pixel
POOL_CASES = [(1, 1, 1, 1), (POOL_CHUNK + 1, 7, 3, 1), (2 * POOL_CHUNK, POOL_CHUNK, POOL_CHUNK - 1, 5)]


def pool_input(hw, seed, B=B_TILES):
    """Four maps (B, hw_l, 64) with a large common offset (1e4 + noise); the tiles at batch positions 0 and B - 1 are the same."""
    gen = torch.Generator().manual_seed(seed)
    maps = [1e4 + torch.randn(B, n, 64, generator=gen) for n in hw]
    for m in maps:
        m[B - 1] = m[0]
    return maps


def ref_pool(maps):
    """float64 per-channel means, level-major (B, 256) (tools/extract_features_nuhtc.py: features_lvl[l].mean(dim=(2, 3)))."""
    return torch.cat([m.double().mean(1) for m in maps], 1)
