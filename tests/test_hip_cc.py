"""The connected-component ("watershed") proposal chain of csrc/proposals.hip, op by op, against plain references:
numpy in fp64 for the thresholded mask (bilinear x4 align_corners, reflect-padded 5x5 Gaussian, > 0) and scipy.ndimage for
opening, hole filling, 4-connected labelling, areas and boxes (nuhtc/models/htc_roi_head_cus.py:283-335).

The GPU tests drive the two halves through Engine.op_cc_mask / Engine.op_cc_proposals (nuhtc_op_cc_mask / nuhtc_op_cc_proposals)
on designed masks that reach what the end-to-end tests cannot: long union chains, runs across 64-pixel wave chunks, rows and
images of the flattened batch, holes that leak only diagonally, the statistics hash table overflowing, more components than the
caps, odd sizes and the area bounds.  The host tests check the references and the designed masks themselves."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

U = 2.0 ** -24          # unit roundoff of fp32
CC_LIST_CAP = 4096      # csrc/proposals.h


# ----------------------------------------------------------------------------------------------------------- references
def gauss5():
    """torchvision gaussian_blur(kernel_size=5)'s kernel: sigma = 0.15*5+0.35 = 1.1, built in fp32 as torchvision builds it."""
    x = torch.linspace(-2, 2, 5)
    pdf = torch.exp(-0.5 * (x / 1.1).pow(2))
    k1 = pdf / pdf.sum()
    return torch.mm(k1[:, None], k1[None, :]).double().numpy()


def _axis(n_in, n_out):
    src = np.arange(n_out) * (n_in - 1) / (n_out - 1) if n_in > 1 else np.zeros(n_out)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def blur_ref64(pred, H, W):
    """fp64 blurred field of (B, h, w) logits at (H, W), and the device's fp32 error bound for it (pixels with
    |blur| <= bound are ambiguous: their sign may legitimately differ).

    The bound, per pixel, is tau * sum_ij k_ij * M_ij, M_ij the largest |logit| of the 3x3 source cells around tap ij's bilinear
    cell (the fp32 source coordinate may fall into a neighbouring cell).  tau, in units of u = 2^-24:
      - bilinear: sy = fl((h-1)/(H-1)) and fy = fl(sy*Y) are each one rounding, so |dfy| <= 2.01 u (h-1); a coordinate error moves the
        value by at most |dfy| * 2M (the slope across a cell is at most |a - b| <= 2M); likewise in x; 1 - ly1 and 1 - lx1 round once
        each (2 u M), the three products and sums once each (3 u M):  4.02 (h + w) + 5;
      - blur: 25 products accumulated in fp32 from 0 in a fixed order, gamma_26 of sum |k_ij * up_ij| <= sum k_ij M_ij:  26;
      - kernel: the device builds k with expf and its own divisions: at most 8 u relative per tap against torch's fp32 kernel:  8.
    The fp64 reference's own error is ~2^-53 and is ignored."""
    pred = np.asarray(pred, np.float64)
    B, h, w = pred.shape
    y0, y1, wy = _axis(h, H)
    x0, x1, wx = _axis(w, W)
    wy, wx = wy[None, :, None], wx[None, None, :]
    g = lambda ys, xs: pred[:, ys[:, None], xs[None, :]]
    up = (1 - wy) * ((1 - wx) * g(y0, x0) + wx * g(y0, x1)) + wy * ((1 - wx) * g(y1, x0) + wx * g(y1, x1))
    M = ndi.maximum_filter(np.abs(pred), size=(1, 3, 3), mode='nearest')[:, y0[:, None], x0[None, :]]
    k = gauss5()
    pu = np.pad(up, ((0, 0), (2, 2), (2, 2)), mode='reflect')
    pm = np.pad(M, ((0, 0), (2, 2), (2, 2)), mode='reflect')
    blur, S = np.zeros((B, H, W)), np.zeros((B, H, W))
    for i in range(5):
        for j in range(5):
            blur += k[i, j] * pu[:, i:i + H, j:j + W]
            S += k[i, j] * pm[:, i:i + H, j:j + W]
    tau = U * (4.02 * (h + w) + 5 + 26 + 8)
    return blur, tau * S


def open_ref(m):
    """open(5x5 ones, 2 iterations) of the reference (two zero-padded 5x5 erosions, two dilations) == 9x9 erode then dilate, zero outside."""
    st = np.ones((9, 9), bool)
    e = ndi.binary_erosion(m.astype(bool), st, border_value=0)
    return ndi.binary_dilation(e, st, border_value=0)


def cc_ref(mask, open, min_area, cap):
    """Per image: (opened, filled, labels as the device numbers them, area / box statistics at each root, boxes, count, overflow)."""
    out = []
    for m in mask:
        H, W = m.shape
        o = open_ref(m) if open else m.astype(bool)
        f = ndi.binary_fill_holes(o)
        lab, n = ndi.label(f)
        ids, first = np.unique(lab.reshape(-1), return_index=True)
        root = np.full(n + 1, -1, np.int64)
        root[ids] = first
        root[0] = -1
        areas = np.bincount(lab.reshape(-1), minlength=n + 1)
        objs = ndi.find_objects(lab)
        stats = np.array([[areas[i + 1], s[1].start, s[0].start, s[1].stop - 1, s[0].stop - 1] for i, s in enumerate(objs)],
                         np.int64).reshape(-1, 5)
        keep = (areas[1:] > min_area) & (areas[1:] < H * W / 4)        # the reference's rule, true division (htc_roi_head_cus.py:302,332)
        boxes = (stats[keep][:, 1:] + [0, 0, 1, 1]).astype(np.float32)
        out.append(dict(opened=o, filled=f, labels=root[lab], roots=root[1:], stats=stats, boxes=boxes, n=len(boxes)))
    return out


def holes(m):
    """Background components (4-connected) not touching the border."""
    lab, n = ndi.label(~m.astype(bool))
    border = set(np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))) - {0}
    return n - len(border)


# ----------------------------------------------------------------------------------------------------------- designed masks
def serpentine(H, W):
    """One-pixel path through every row: even rows full, odd rows one pixel joining alternately at the right and left end."""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 1
    for y in range(1, H, 2):
        m[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    return m


def comb(H, W):
    """Teeth on the even columns joined only by the bottom row."""
    m = np.zeros((H, W), np.uint8)
    m[:, 0::2] = 1
    m[-1] = 1
    return m


def spiral(n, closed):
    """Square spiral wall of width 1; the background between its turns is one corridor that leaves at (1, 0) -- or is shut there."""
    m = np.zeros((n, n), np.uint8)
    y, x, d = 0, 0, 0
    steps = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    lengths = [n - 1, n - 1, n - 1] + [L for L in range(n - 3, 0, -2) for _ in range(2)]
    m[0, 0] = 1
    for L in lengths:
        dy, dx = steps[d]
        for _ in range(L):
            y, x = y + dy, x + dx
            m[y, x] = 1
        d = (d + 1) % 4
    if closed:
        m[1, 0] = 1
    return m


def diagonal_holes(H, W):
    """Holes whose only contact with the outside background is a diagonal one: one inside, one at the image corner."""
    m = np.zeros((H, W), np.uint8)
    m[5:8, 5:8] = 1
    m[6, 6] = 0          # the hole
    m[7, 7] = 0          # its diagonal neighbour belongs to the outside
    m[0, 1] = m[1, 0] = m[1, 1] = m[1, 2] = m[2, 1] = 1
    m[1, 1] = 0          # hole at (1, 1); (0, 0) is outside background touching it diagonally
    m[0, 2] = m[2, 0] = 1
    return m


def nested(n, rings):
    """Concentric square rings of width 1 two pixels apart: ring, hole, ring, hole, ..."""
    m = np.zeros((n, n), np.uint8)
    for r in range(rings):
        a, b = 1 + 2 * r, n - 2 - 2 * r
        m[a, a:b + 1] = m[b, a:b + 1] = m[a:b + 1, a] = m[a:b + 1, b] = 1
    return m


def dots(H, W):
    """Singletons on the (even, even) lattice: background stays 4-connected, nothing is filled."""
    m = np.zeros((H, W), np.uint8)
    m[0::2, 0::2] = 1
    return m


def blob_of_area(H, W, a, width):
    """One component of exactly `a` pixels: rows of `width` from (1, 1), the last row partial."""
    m = np.zeros((H, W), np.uint8)
    flat = np.zeros(((a + width - 1) // width) * width, np.uint8)
    flat[:a] = 1
    rows = flat.reshape(-1, width)
    m[1:1 + len(rows), 1:1 + width] = rows
    return m


def runs(B, H, W, seed):
    """Horizontal runs of length 63, 64, 65 starting at flat offsets 0, 1, 63 of a 64-pixel chunk of the flattened batch, on most
    rows; pixels set at row ends / row starts and at the last / first pixel of consecutive images (same chunk, never joined)."""
    rng = np.random.default_rng(seed)
    m = np.zeros((B, H, W), np.uint8)
    HW = H * W
    for b in range(B):
        for y in range(H):
            if y % 3 == 2:
                continue
            g = b * HW + y * W
            L = int(rng.choice([63, 64, 65]))
            x = (int(rng.choice([0, 1, 63])) - g) % 64
            x += 64 * int(rng.integers(0, max(1, (W - L - x) // 64 + 1)))
            m[b, y, x:min(W, x + L)] = 1
            if rng.random() < 0.5:
                m[b, y, W - 1] = 1
                if y + 1 < H:
                    m[b, y + 1, 0] = 1
        m[b, 0, 0] = m[b, H - 1, W - 1] = 1
    return m


def blobs(B, H, W, seed, cell=8, noise=0.02):
    """Random blobs of ~cell pixels with salt-and-pepper noise: opening removes the noise and keeps most blobs."""
    rng = np.random.default_rng(seed)
    lo = rng.random((B, H // cell + 2, W // cell + 2)) > 0.55
    m = np.kron(lo, np.ones((cell, cell), bool))[:, :H, :W]
    return (m ^ (rng.random((B, H, W)) < noise)).astype(np.uint8)


def smooth_logits(B, h, w, seed, sigma=1.5, bias=-0.3):
    rng = np.random.default_rng(seed)
    f = ndi.gaussian_filter(rng.standard_normal((B, h, w)), (0, sigma, sigma), mode='wrap') * 3 * sigma + bias
    return f.astype(np.float32)


# ----------------------------------------------------------------------------------------------------------- host tests
def test_mask_reference_equals_oracle_off_the_band():
    from oracle import model as O
    for seed, (h, w, H, W) in enumerate([(16, 16, 64, 64), (24, 20, 96, 80), (9, 13, 33, 50), (32, 32, 128, 128)]):
        pred = smooth_logits(2, h, w, seed)
        blur, band = blur_ref64(pred, H, W)
        amb = np.abs(blur) <= band
        assert amb.sum() == 0, (seed, int(amb.sum()))
        ref = np.stack([open_ref(m) for m in blur > 0])
        orc = O.semantic_binary_mask(torch.from_numpy(pred)[:, None], (H, W)).numpy().astype(bool)
        assert ref.any() and (ref == orc).all(), seed


@pytest.mark.parametrize('name, m, comps, n_holes, comps_filled', [
    ('serpentine', serpentine(64, 70), 1, 0, 1),
    ('comb', comb(40, 65), 1, 0, 1),
    ('spiral_open', spiral(31, False), 1, 0, 1),
    ('spiral_closed', spiral(31, True), 1, 1, 1),
    ('diagonal', diagonal_holes(12, 12), 3, 2, 2),
    ('nested', nested(21, 4), 4, 4, 1),
    ('dots', dots(64, 128), 32 * 64, 0, 32 * 64),
])
def test_designed_masks_have_the_claimed_topology(name, m, comps, n_holes, comps_filled):
    assert ndi.label(m)[1] == comps, name
    assert holes(m) == n_holes, name
    assert ndi.label(ndi.binary_fill_holes(m))[1] == comps_filled, name


def test_oracle_area_rule_keeps_floor_quarter(monkeypatch):
    """min_area < a < H*W/4 in true division: at 31 x 31 (HW % 4 == 1) an area of floor(961/4) = 240 is kept, 241 is not."""
    from oracle import model as O
    for a, kept in ((240, True), (241, False), (239, True), (10, False), (11, True)):
        m = blob_of_area(31, 31, a, 16)
        monkeypatch.setattr(O, 'semantic_binary_mask', lambda pred, hw, m=m: torch.from_numpy(m[None].astype(np.float32)))
        got = O.cc_proposals(torch.zeros(1, 1, 8, 8), (31, 31))[0]
        assert (len(got) == 1) == kept, a
        assert cc_ref(m[None], False, 10, 16)[0]['n'] == int(kept), a


def test_runs_cross_chunks_rows_and_images():
    """The runs generator does what the GPU test relies on: W not a multiple of 64, HW % 64 != 0, and run starts at each chunk offset."""
    m = runs(16, 37, 90, 0)
    assert 90 % 64 and (37 * 90) % 64
    flat = m.reshape(-1)
    starts = np.nonzero(flat[1:] & ~flat[:-1])[0] + 1
    assert {0, 1, 63} <= set((starts % 64).tolist())


# ----------------------------------------------------------------------------------------------------------- GPU tests
@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    e = Engine(weights.bench_state_dict(0), device=0, max_batch=1, tile=(64, 64))
    yield e
    e.close()


def _run(eng, mask, open, min_area=10, cap=CC_LIST_CAP):
    r = eng.op_cc_proposals(torch.from_numpy(np.ascontiguousarray(mask)).cuda(), open=open, min_area=min_area, cap=cap)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def _check(got, mask, open, min_area=10, cap=CC_LIST_CAP, tag=''):
    """Exact agreement with scipy: opened and filled masks, label image, per-root statistics, boxes, counts, overflow."""
    ref = cc_ref(mask, open, min_area, cap)
    B, H, W = mask.shape
    n_over = 0
    for b, r in enumerate(ref):
        t = f'{tag} image {b} ({H}x{W})'
        assert (got['opened'][b] == r['opened']).all(), f'{t}: opened mask differs'
        assert (got['filled'][b] == r['filled']).all(), f'{t}: filled mask differs in {int((got["filled"][b] != r["filled"]).sum())} px'
        bad = got['labels'][b] != r['labels']
        assert not bad.any(), f'{t}: {int(bad.sum())} labels differ, first at {np.argwhere(bad)[0].tolist()}'
        st = got['stats'][b]
        assert (st[r['roots']] == r['stats']).all(), f'{t}: root statistics differ'
        nonroot = np.ones(H * W, bool)
        nonroot[r['roots']] = False
        assert (st[nonroot, 0] == 0).all(), f'{t}: area at a non-root pixel'
        n_over += r['n'] > cap
        assert got['counts'][b] == min(r['n'], cap), f'{t}: count {got["counts"][b]} != min({r["n"]}, {cap})'
        if r['n'] <= CC_LIST_CAP:
            k = min(r['n'], cap)
            assert (got['boxes'][b, :k] == r['boxes'][:k]).all(), f'{t}: boxes differ'
    assert got['overflow'] == n_over, (tag, got['overflow'], n_over)
    return ref


def _engine_hw(tile, sf=2):
    """(h, w, H, W) as the engine relates them: img_shape = tile * scale, the network input padded to 32, logits at stride 4."""
    H, W = int(tile[0] * sf), int(tile[1] * sf)
    return -(-H // 32) * 8, -(-W // 32) * 8, H, W


MASK_SHAPES = [(1,) + _engine_hw((t, t)) for t in (64, 96, 256)] + [
    (2,) + _engine_hw((100, 100)),                # tile not a multiple of 32
    (2,) + _engine_hw((64, 64), 4),               # scale factor 4 (a 20x slide)
    (2,) + _engine_hw((251, 253), 1),             # odd valid sizes at scale factor 1
    (16,) + _engine_hw((255, 256)[::-1], 1),      # B = 16
    (2, 8, 256, 3, 1024), (3, 8, 8, 4, 31), (2, 8, 9, 31, 33), (2, 9, 16, 33, 63), (1, 16, 16, 63, 64), (2, 16, 17, 64, 65),
    (1, 17, 64, 65, 255), (1, 64, 64, 255, 256), (1, 64, 250, 256, 1000), (1, 250, 8, 1000, 3), (1, 256, 8, 1024, 4),
    (1, 256, 256, 1024, 1024), (2, 1, 7, 33, 65), (2, 40, 1, 160, 31),
]


@pytest.mark.gpu
def test_cc_mask_vs_fp64(eng):
    for i, (B, h, w, H, W) in enumerate(MASK_SHAPES):
        pred = smooth_logits(B, h, w, 100 + i, sigma=1.0, bias=0.0)
        got = eng.op_cc_mask(torch.from_numpy(pred).cuda(), H, W).cpu().numpy().astype(bool)
        blur, band = blur_ref64(pred, H, W)
        amb = np.abs(blur) <= band
        bad = (got != (blur > 0)) & ~amb
        flips = int(((got != (blur > 0)) & amb).sum())
        print(f'cc_mask B={B} {h}x{w} -> {H}x{W}: {int(amb.sum())} ambiguous px of {amb.size}, {flips} of them flipped')
        assert not bad.any(), f'{H}x{W}: {int(bad.sum())} px differ outside the band, first at {np.argwhere(bad)[0].tolist()}'


@pytest.mark.gpu
@pytest.mark.parametrize('name, mask, kw', [
    ('serpentine_1024', serpentine(1024, 1024)[None], {}),
    ('comb', np.stack([comb(40, 65), comb(40, 65)[:, ::-1]]), {}),
    ('comb_strip', np.stack([comb(70, 128), comb(70, 128)[:, ::-1]]), {}),
    ('spiral', np.stack([np.pad(spiral(61, c), ((3, 6), (2, 27))) for c in (False, True)]), {}),
    ('spiral_border', np.stack([spiral(63, False), spiral(63, True)]), {}),
    ('diagonal', np.stack([diagonal_holes(12, 12), diagonal_holes(12, 12)[::-1, ::-1].copy()]), dict(min_area=0)),
    ('nested', np.stack([nested(21, 4), nested(21, 1)]), {}),
    ('runs_90', runs(16, 37, 90, 1), dict(min_area=0)),
    ('runs_200', runs(16, 33, 200, 2), dict(min_area=0)),
    ('runs_1000', runs(2, 17, 1000, 3), dict(min_area=0)),
    ('dots_strip', dots(64, 128)[None], dict(min_area=0)),
    ('dots_strip_bars', np.stack([dots(64, 128) | (np.arange(128) == 127)[None, :], dots(64, 128) | (np.arange(64) == 63)[:, None]]).astype(np.uint8),
     dict(min_area=0)),
    ('dots_atomic', dots(64, 65)[None], dict(min_area=0)),
    ('dots_over_cap', dots(64, 64)[None], dict(min_area=0, cap=512)),
    ('dots_over_list', dots(1024, 64)[None], dict(min_area=0)),
    ('zeros_ones', np.stack([np.zeros((33, 65), np.uint8), np.ones((33, 65), np.uint8)]), {}),
    ('zeros_ones_strip', np.stack([np.zeros((33, 64), np.uint8), np.ones((33, 64), np.uint8)]), {}),
    ('min_area', np.stack([blob_of_area(31, 64, a, 5) for a in (9, 10, 11, 12)]), {}),
    ('quarter_31x31', np.stack([blob_of_area(31, 31, a, 16) for a in (239, 240, 241)]), {}),
    ('quarter_33x31', np.stack([blob_of_area(33, 31, a, 17) for a in (254, 255, 256)]), {}),
    ('quarter_3x3', np.stack([blob_of_area(5, 3, a, 1) for a in (2, 3, 4)]), dict(min_area=0)),
    ('noise_90', (np.random.default_rng(5).random((4, 50, 90)) < 0.5).astype(np.uint8), dict(min_area=0)),
    ('noise_64', (np.random.default_rng(6).random((4, 96, 64)) < 0.45).astype(np.uint8), dict(min_area=0)),
])
def test_cc_from_mask_vs_scipy(eng, name, mask, kw):
    got = _run(eng, mask, False, **kw)
    ref = _check(got, mask, False, tag=name, **kw)
    print(name, 'components', [len(r['roots']) for r in ref], 'boxes', got['counts'].tolist(), 'overflow', got['overflow'])


@pytest.mark.gpu
@pytest.mark.parametrize('B, H, W', [(4, 40, 64), (2, 70, 128), (1, 256, 1024), (4, 37, 63), (4, 41, 65), (8, 90, 90), (1, 129, 1000)])
def test_cc_open_vs_scipy(eng, B, H, W):
    mask = blobs(B, H, W, H * W)
    got = _run(eng, mask, True)
    ref = _check(got, mask, True, tag='open')
    print(f'open {B}x{H}x{W}: boxes', [r['n'] for r in ref])


def _chain(eng, pred, H, W):
    m = eng.op_cc_mask(torch.from_numpy(pred).cuda(), H, W)
    return m.cpu().numpy(), _run(eng, m.cpu().numpy(), True)


@pytest.mark.gpu
@pytest.mark.parametrize('B, tile, sf', [(2, (64, 64), 2), (2, (100, 100), 2), (1, (256, 256), 2), (2, (64, 64), 4), (2, (251, 253), 1),
                                        (1, (31, 31), 1)])
def test_cc_chain_vs_scipy_and_oracle(eng, B, tile, sf):
    from oracle import model as O
    h, w, H, W = _engine_hw(tile, sf)
    pred = smooth_logits(B, h, w, h * w + B)
    mask, got = _chain(eng, pred, H, W)
    _check(got, mask, True, tag='chain')
    blur, band = blur_ref64(pred, H, W)
    amb = int((np.abs(blur) <= band).sum())
    print(f'chain {tile} x{sf}: {amb} ambiguous px, boxes {got["counts"].tolist()}')
    if amb == 0:
        orc = O.cc_proposals(torch.from_numpy(pred)[:, None], (H, W))
        for b in range(B):
            n = int(got['counts'][b])
            assert n == len(orc[b]) and (got['boxes'][b, :n] == orc[b].numpy()[:, :4]).all(), (tile, b)


@pytest.mark.gpu
def test_cc_batch_independence_and_determinism(eng):
    h, w, H, W = _engine_hw((100, 100))
    pred = smooth_logits(16, h, w, 7)
    _, a = _chain(eng, pred, H, W)
    for k in (0, 5, 15):
        _, s = _chain(eng, pred[k:k + 1], H, W)
        for key in ('opened', 'filled', 'labels', 'stats', 'boxes', 'counts'):
            assert np.array_equal(a[key][k], s[key][0]), (k, key)
    _, again = _chain(eng, pred, H, W)
    for key in ('opened', 'filled', 'labels', 'stats', 'boxes', 'counts', 'overflow'):
        assert np.array_equal(a[key], again[key]), key


def _engine_cc_vs_scipy(e, tiles):
    """The engine's cc_props / cc_counts / cc_labels equal scipy run on its own cc_mask buffer (the filled mask, [B][Hv*Wv] packed)."""
    from nuhtc_amd import hip
    B = len(tiles)
    e.infer_async(e.to_device(tiles), hip.CH_SWAP)
    e.check()
    H, W = int(round(e.image_hw[0] * e.cfg.scale_factor)), int(round(e.image_hw[1] * e.cfg.scale_factor))
    filled = e.buffer('cc_mask').reshape(-1)[:B * H * W].reshape(B, H, W).cpu().numpy()
    labels = e.buffer('cc_labels').reshape(-1)[:B * H * W].reshape(B, H, W).cpu().numpy()
    counts = e.buffer('cc_counts')[:B].cpu().numpy()
    props = e.buffer('cc_props')[:B].cpu().numpy()
    ref = cc_ref(filled, False, 10, e.cfg.max_cc_proposals)
    for b, r in enumerate(ref):
        assert (r['filled'] == filled[b]).all(), b
        assert (labels[b] == r['labels']).all(), b
        assert counts[b] == r['n'] and (props[b, :r['n']] == r['boxes']).all(), (b, counts[b], r['n'])
    return counts


@pytest.mark.gpu
def test_engine_cc_at_production_shape(hip_device):
    from nuhtc_amd import synth, weights
    from nuhtc_amd.engine import Engine
    sd = weights.bench_state_dict(0)
    tiles = synth.nuclei_tiles(16, 256, start=0)
    e = Engine(sd, device=0, max_batch=16)
    counts = _engine_cc_vs_scipy(e, tiles)
    e.close()
    print('production shape: cc proposals per tile', counts.tolist())
    # an odd valid size at scale factor 1: Hv * Wv = 251 * 253, HW % 4 == 3
    e = Engine(sd, device=0, max_batch=2, tile=(251, 253), scale_factor=1.0)
    counts = _engine_cc_vs_scipy(e, np.ascontiguousarray(tiles[:2, :251, :253]))
    e.close()
    print('251x253 x1: cc proposals per tile', counts.tolist())
