"""The attention half of a Swin block -- LN1, the QKV front that fills the window image, the shifted-window attention kernels and the
window geometry the engine builds for them -- op by op, against a float64 restatement of mmdet's SwinBlock -> ShiftWindowMSA ->
WindowMSA up to the attention output before `proj` (mmdet/models/backbones/swin.py:79-117, 178-252, 356-363).

Engine.op_window_msa (nuhtc_op_window_msa) builds the stage geometry with the code nuhtc_finalize uses (window maps, compact order,
padding rows, the split pipe's padbits and bias row, the packed shift mask and mask_any) for any B x H x W, packs the weights as the
engine packs them and runs the engine's own attention front (engine.hip run_attn_front): on the split pipe the fused LN1 + QKV kernel
(C = 96) or ln_stats + the A_LN linear (C > 96) and window_attn_split_kernel, on the fp32 pipe layernorm_windows + the linear and
window_attn_mfma_kernel.  These tests reach what the end-to-end tests cannot: errors confined to a few windows, one head, the padded keys,
key 48 or the shift regions.

Error bound per output element (i, c) of a window and head:
    |got - ref| <= EPS * ( sum_j p_ij V_jc + sum_j p_ij A_ij |v_jc - o_ic| )
V (and the Q / K magnitudes) are the linear's magnitudes |LN(x)| |W|^T + |b| with |LN(x)| taken as |x_hat| |gamma| + |beta|;
A_ij = scale sum_d |q_id| |k_jd| + |bias_ij| over the keys in the query's own shift region (masked keys weigh <= e^-90 and are left out of
A).  The first term holds the linear and P.V, the second the scores' error carried through the softmax.  The observed maxima are printed
per class and pipe (run with -s)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

# 4e-6 to start with; 8e-6 holds the index probes, whose largest observed err / mag is 5.3e-6 on the split pipe: the fast exp's error
# grows with |s_ij - max_k s_ik| (30 there, for keys whose own A_ij is 0), which A_ij does not carry
EPS = 8e-6
WS = 7
SCALE = 32 ** -0.5
SENTINEL = 0x7fc0dead                  # a quiet NaN with a payload: rows that must not be written keep it bit for bit
PIPES = ('split', 'fp32')
CS = (96, 192, 384, 768)


# ----------------------------------------------------------------------------------------------------------- references
def rel_index():
    """[49 query][49 key] -> row of the relative-position bias table (swin.py:54-66: (dy + 6) * 13 + (dx + 6), dy = yq - yk)."""
    yx = torch.stack(torch.meshgrid(torch.arange(WS), torch.arange(WS), indexing='ij')).flatten(1)     # (2, 49)
    d = yx[:, :, None] - yx[:, None, :] + WS - 1
    return d[0] * (2 * WS - 1) + d[1]


def regions(Hp, Wp):
    """Shift-mask region id of every position of the padded grid (swin.py:197-211): slices (0, -7), (-7, -3), (-3, None) per axis."""
    def r(n):
        t = torch.zeros(n, dtype=torch.long)
        t[n - WS:n - 3] = 1
        t[n - 3:] = 2
        return t
    return r(Hp)[:, None] * 3 + r(Wp)[None, :]


def _windows(t, Hp, Wp):
    """(B, Hp, Wp, ...) -> (B * nW, 49, ...), windows row-major, tokens row-major in the window."""
    B, rest = t.shape[0], t.shape[3:]
    t = t.reshape(B, Hp // WS, WS, Wp // WS, WS, *rest).permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest)))
    return t.reshape(B * (Hp // WS) * (Wp // WS), WS * WS, *rest)


def _unwindows(t, B, Hp, Wp):
    rest = t.shape[2:]
    t = t.reshape(B, Hp // WS, Wp // WS, WS, WS, *rest).permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest)))
    return t.reshape(B, Hp, Wp, *rest)


def ref_wmsa(x, g, b, w, bias, table, shifted, mask_pad=False):
    """float64 attention output before proj of x (B, H, W, C) and its bound magnitude, both (B*H*W, C) in token order.
    mask_pad: also mask the padded keys (NOT what mmdet does: the padded tokens are keys with k = b_k, v = b_v after F.pad)."""
    d = lambda t: torch.as_tensor(t).detach().cpu().double()
    x, g, b, w, bias, table = d(x), d(g), d(b), d(w), d(bias), d(table)
    B, H, W, C = x.shape
    nH = C // 32
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    xh = (x - mu) / torch.sqrt(var + 1e-5)
    ln, lnm = xh * g + b, xh.abs() * g.abs() + b.abs()
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    pad = lambda t: F.pad(t, (0, 0, 0, Wp - W, 0, Hp - H))
    ln, lnm = pad(ln), pad(lnm)
    valid = F.pad(torch.ones(B, H, W), (0, Wp - W, 0, Hp - H))
    ids = regions(Hp, Wp)
    if shifted:
        ln, lnm, valid = (torch.roll(t, (-3, -3), (1, 2)) for t in (ln, lnm, valid))
    lw, lmw, vw = _windows(ln, Hp, Wp), _windows(lnm, Hp, Wp), _windows(valid, Hp, Wp)
    nW = (Hp // WS) * (Wp // WS)
    relb = table[rel_index().reshape(-1)].reshape(WS * WS, WS * WS, nH).permute(2, 0, 1)       # (nH, q, k)
    same = (_windows(ids[None, ..., None], Hp, Wp)[..., 0][:, :, None] == _windows(ids[None, ..., None], Hp, Wp)[..., 0][:, None, :])
    if not shifted:
        same = torch.ones_like(same)
    maskv = torch.where(same, 0.0, -100.0).double()                                                # (nW, q, k)
    chunk = max(1, 288 // nH)           # windows per step: the |v_j - o_i| tensor stays below 200 MB
    out, mag = torch.empty(lw.shape[0], WS * WS, C, dtype=torch.float64), torch.empty(lw.shape[0], WS * WS, C, dtype=torch.float64)
    for w0 in range(0, lw.shape[0], chunk):
        sl = slice(w0, min(w0 + chunk, lw.shape[0]))
        n = sl.stop - sl.start
        qkv = (lw[sl] @ w.T + bias).reshape(n, 49, 3, nH, 32).permute(2, 0, 3, 1, 4)              # (3, n, nH, 49, 32)
        qkvm = (lmw[sl] @ w.abs().T + bias.abs()).reshape(n, 49, 3, nH, 32).permute(2, 0, 3, 1, 4)
        widx = torch.arange(sl.start, sl.stop) % nW
        s = SCALE * qkv[0] @ qkv[1].transpose(-1, -2) + relb
        s = s + maskv[widx][:, None]
        if mask_pad:
            s = s.masked_fill(vw[sl][:, None, None, :] == 0, -math.inf)
        p = s.softmax(-1)
        o = p @ qkv[2]
        A = (SCALE * qkvm[0] @ qkvm[1].transpose(-1, -2) + relb.abs()) * same[widx][:, None]
        m = p @ qkvm[2] + torch.einsum('nhij,nhijc->nhic', p * A, (qkv[2][:, :, None] - o[:, :, :, None]).abs())
        out[sl] = o.transpose(1, 2).reshape(n, 49, C)
        mag[sl] = m.transpose(1, 2).reshape(n, 49, C)
    res = []
    for t in (out, mag):
        t = _unwindows(t, B, Hp, Wp)
        if shifted:
            t = torch.roll(t, (3, 3), (1, 2))
        res.append(t[:, :H, :W].reshape(B * H * W, C))
    return res[0], res[1]


def compact_tokens(B, H, W, shifted):
    """Token of every compact row (the non-padding rows of the window image in window order), restated from swin.py's pad / roll /
    partition: what the engine calls ctok."""
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    ys, xs = torch.arange(Hp), torch.arange(Wp)
    if shifted:
        ys, xs = (ys + 3) % Hp, (xs + 3) % Wp             # rolled[ys] = padded[(ys + 3) % Hp]
    yy, xx = ys[:, None].expand(Hp, Wp), xs[None, :].expand(Hp, Wp)
    tok = torch.where((yy < H) & (xx < W), yy * W + xx, torch.full_like(yy, -1))
    tok = torch.stack([torch.where(tok >= 0, tok + bi * H * W, tok) for bi in range(B)])
    tok = _windows(tok[..., None], Hp, Wp).reshape(-1)
    return tok[tok >= 0]


def weights(gen, C, bias_scale=0.5):
    """LN1 gamma / beta, qkv weight (rows ~ N(0, 1 / C): q, k, v ~ N(0, 1)), qkv bias and a relative-position bias table."""
    return dict(g=1.0 + 0.2 * torch.randn(C, generator=gen), b=0.2 * torch.randn(C, generator=gen),
                w=torch.randn(3 * C, C, generator=gen) / math.sqrt(C), bias=bias_scale * torch.randn(3 * C, generator=gen),
                table=torch.randn(169, C // 32, generator=gen))


OBSERVED = {}
SQERR = {}


def _within(tag, pipe, got, ref, mag, bad=None):
    """got (any device, (rows, C)) vs the fp64 reference within EPS * mag; `bad` (bool, (rows, 1) or (rows, C)) masks out the elements a
    non-finite input may reach.  Records the largest err / mag and the squared errors per C for the rms comparison of the pipes."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (tag, pipe, got.shape, ref.shape)
    ok = torch.ones_like(got, dtype=torch.bool) if bad is None else ~bad.expand_as(got)
    assert torch.isfinite(got[ok]).all(), f'{tag} [{pipe}]: {int((~torch.isfinite(got[ok])).sum())} non-finite outputs'
    err = (got - ref).abs()[ok]
    m = mag[ok]
    over = err > EPS * m
    rel = float((err / m.clamp_min(1e-300)).max()) if err.numel() else 0.0
    key = (tag.split(' ')[0], pipe)
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), rel)
    print(f'wmsa {tag} [{pipe}]: max err/mag {rel:.3e}')
    assert not over.any(), f'{tag} [{pipe}]: {int(over.sum())}/{over.numel()} outside {EPS:g} * mag (max err/mag {rel:.3e})'
    return rel


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)


# ----------------------------------------------------------------------------------------------------------- GPU fixtures
@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights as W
    from nuhtc_amd.engine import Engine
    return Engine(W.seeded_state_dict(0), device=0, max_batch=1, tile=(64, 64))


def _run(eng, x, wt, shifted, pipe, order='token'):
    """op_window_msa into a sentinel-filled output (a row left unwritten fails the finiteness check)."""
    B, H, W, C = x.shape
    out = sentinel(B * H * W, C)
    return eng.op_window_msa(x, wt['g'], wt['b'], wt['w'], wt['bias'], wt['table'], shifted, pipe=pipe, order=order, out=out)


def _check(eng, tag, x, wt, shifted, pipes=PIPES, bad=None):
    """Both pipes against one reference; the squared errors go to SQERR[(C, pipe)]."""
    ref, mag = ref_wmsa(x, wt['g'], wt['b'], wt['w'], wt['bias'], wt['table'], shifted)
    xd = x.cuda()
    outs = {}
    for pipe in pipes:
        got = _run(eng, xd, wt, shifted, pipe)
        _within(tag, pipe, got, ref, mag, bad)
        d = (got.detach().cpu().double() - ref)
        d = d[torch.isfinite(d)]
        k = (x.shape[-1], pipe)
        s, n = SQERR.get(k, (0.0, 0))
        SQERR[k] = (s + float((d ** 2).sum()), n + d.numel())
        outs[pipe] = got
    return ref, mag, outs


# ----------------------------------------------------------------------------------------------------------- geometry
# production grids of stage s (C = 96 << s): 256-pixel tiles at scale factor 2 and 4, and the grids that need no padding
PROD = {96: [(128, 128), (256, 256), (56, 56)], 192: [(64, 64), (128, 128), (28, 28)], 384: [(32, 32), (64, 64), (14, 14)],
        768: [(16, 16), (32, 32), (7, 7)]}
EDGE = (1, 2, 3, 6, 7, 8, 13, 20)      # every residue mod 7 on each axis


def _sweep_cases(C):
    cases = [(1, H, W) for H, W in PROD[C]]
    cases += [(1, H, EDGE[(i + 3) % len(EDGE)]) for i, H in enumerate(EDGE)]       # each residue on each axis, mixed pairs
    cases += [(1, 14, 13), (1, 13, 21), (1, 7, 20)]                                # padding on one axis only
    cases += [(3, 1, 1), (3, 7, 20), (3, 15, 15)]                                   # B*nW*nH not a multiple of 4: the pair >= nPairs tail
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize('C', CS)
def test_geometry_sweep_vs_fp64(eng, C):
    """Production grids of every stage, grids with every residue mod 7 on each axis, padding on one axis only and batches whose
    (window, head) pair count leaves a partial workgroup; both pipes, both shift states."""
    gen = torch.Generator().manual_seed(C)
    wt = weights(gen, C)
    for B, H, W in _sweep_cases(C):
        if C * B * H * W > 96 * 256 * 256:
            continue
        x = torch.randn(B, H, W, C, generator=gen)
        nW = -(-H // WS) * -(-W // WS)
        if B == 3 and C < 384:         # (12 and 24 heads fill whole workgroups of 4 pairs)
            assert (B * nW * (C // 32)) % 4, (B, H, W, C)
        for shifted in (0, 1):
            _check(eng, f'sweep C{C} B{B} {H}x{W} sh{shifted}', x, wt, shifted)


@pytest.mark.gpu
def test_split_rms_within_fp32_rms():
    """The split pipe is fp32 arithmetic: over the geometry sweep its rms error stays within 1.5x the fp32 pipe's on the same operands."""
    for C in CS:
        if (C, 'split') not in SQERR or (C, 'fp32') not in SQERR:
            pytest.fail(f'no sweep data for C = {C} (run the module, not this test alone)')
        rs = math.sqrt(SQERR[(C, 'split')][0] / SQERR[(C, 'split')][1])
        rf = math.sqrt(SQERR[(C, 'fp32')][0] / SQERR[(C, 'fp32')][1])
        print(f'rms error C{C}: split {rs:.3e}  fp32 {rf:.3e}  ratio {rs / rf:.3f}')
        assert rs <= 1.5 * rf, (C, rs, rf)


# ----------------------------------------------------------------------------------------------------------- index probes
def probe_weights(gen, C, offsets):
    """q = k = 0, v = LN(x) (v rows of qkv.weight the identity, zero bias), and per head a table that is 0 except +30 at one relative
    offset: the scores are the bias (+ shift mask) alone, and a query whose offset key is in its window and region takes that key's LN
    vector (the other 48 keys weigh <= 48 e^-30 together)."""
    nH = C // 32
    wt = weights(gen, C)
    w = torch.zeros(3 * C, C)
    w[2 * C:] = torch.eye(C)
    table = torch.zeros(169, nH)
    for h, o in enumerate(offsets):
        table[o, h] = 30.0
    return dict(g=wt['g'], b=wt['b'], w=w, bias=torch.zeros(3 * C), table=table)


def probe_plan(C, launches):
    """Offsets of the heads of each launch: every one of the 169 relative offsets once over the launches, a different one per head."""
    nH = C // 32
    return [[(L * nH + h) * 37 % 169 for h in range(nH)] for L in range(launches)]


@pytest.mark.gpu
def test_index_probes_pin_bias_heads_and_mask(eng):
    """With scores = relative-position bias (+ shift mask) of one +30 offset per head, the output of a query is one token's LN vector:
    pins the bias indexing, the head offset, the per-lane pack, both query and key tiles (keys 31 / 32) and the key-48 path; with the
    shift on, the mask regions and mask_any.  Over the launches every offset is reached.  C = 768 (24 heads) covers the 169 offsets
    in 8 launches, the other widths check their head strides."""
    gen = torch.Generator().manual_seed(3)
    plans = [(768, p) for p in probe_plan(768, 8)] + [(C, p) for C in (96, 192, 384) for p in probe_plan(C, 1)]
    assert set(o for C, p in plans if C == 768 for o in p) == set(range(169))
    for C, offs in plans:
        x = torch.randn(1, 14, 20, C, generator=gen)
        wt = probe_weights(gen, C, offs)
        for shifted in (0, 1):
            _check(eng, f'probe C{C} offs{offs[0]} sh{shifted}', x, wt, shifted)


# ----------------------------------------------------------------------------------------------------------- padded keys
@pytest.mark.gpu
@pytest.mark.parametrize('C', (96, 384))
def test_padded_keys_carry_the_qkv_bias(eng, C):
    """Padded tokens are keys with k = b_k, v = b_v (mmdet masks only the shift regions): with a qkv bias as large as W LN(x) they carry
    real weight.  The result matches the reference and differs, by more than 20x the bound, from one that masks them (the case bites)."""
    gen = torch.Generator().manual_seed(4 + C)
    wt = weights(gen, C, bias_scale=1.0)
    for B, H, W in [(2, 9, 12), (1, 16, 16), (1, 4, 3)]:
        x = torch.randn(B, H, W, C, generator=gen)
        for shifted in (0, 1):
            ref, mag, outs = _check(eng, f'padkeys C{C} {H}x{W} sh{shifted}', x, wt, shifted)
            alt, _ = ref_wmsa(x, wt['g'], wt['b'], wt['w'], wt['bias'], wt['table'], shifted, mask_pad=True)
            assert float(((alt - ref).abs() / mag).max()) > 20 * EPS, (C, H, W, shifted)


# ----------------------------------------------------------------------------------------------------------- hard operands
def _hard_cases(gen, C):
    base = weights(gen, C)
    x = torch.randn(2, 9, 15, C, generator=gen)
    sat = dict(base, w=base['w'].clone())
    sat['w'][:2 * C] *= 32.0                      # q, k ~ N(0, 32^2): scores ~ N(0, 1000^2), softmax saturates to one key
    flat = dict(base, w=base['w'].clone(), table=torch.zeros(169, C // 32), bias=base['bias'].clone())
    flat['w'][:C] = 0.0
    flat['bias'][:C] = 0.0                        # q = 0, table 0: every score equal, uniform weights (per shift region)
    big = dict(base, table=50.0 * torch.randn(169, C // 32, generator=gen))
    return [('saturated', x, sat), ('uniform', x, flat), ('offset50', 50.0 + x, base), ('table50', x, big)]


@pytest.mark.gpu
@pytest.mark.parametrize('C', (96, 192, 768))
def test_hard_operand_classes_vs_fp64(eng, C):
    """Scores of +-1e3 (max subtraction), all scores equal, tokens with a common offset of 50 sigma (through LN), a bias table of
    magnitude 50."""
    gen = torch.Generator().manual_seed(5 + C)
    for label, x, wt in _hard_cases(gen, C):
        for shifted in (0, 1):
            _check(eng, f'{label} C{C} sh{shifted}', x, wt, shifted)


# ----------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.gpu
@pytest.mark.parametrize('C', (96, 384))
def test_nonfinite_token_stays_in_its_windows(eng, C):
    """A NaN or Inf in one token reaches only the windows that hold it in that shift state, in its own image; every other output
    matches the reference."""
    gen = torch.Generator().manual_seed(6 + C)
    wt = weights(gen, C)
    B, H, W = 2, 13, 16
    for val, (bi, y, xx) in [(float('nan'), (1, 5, 9)), (float('inf'), (0, 12, 15)), (-float('inf'), (1, 0, 2))]:
        x = torch.randn(B, H, W, C, generator=gen)
        x[bi, y, xx, 7] = val
        for shifted in (0, 1):
            # the tokens of the windows (of this shift state) that hold the token: the outputs it may reach
            Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
            t_of_row = _windows(_token_grid(B, H, W, shifted, Hp, Wp)[..., None], Hp, Wp).reshape(-1, WS * WS)
            hit = (t_of_row == bi * H * W + y * W + xx).any(1)
            reach = t_of_row[hit]
            bad = torch.zeros(B * H * W, 1, dtype=torch.bool)
            bad[reach[reach >= 0]] = True
            ref, mag = ref_wmsa(x.nan_to_num(0.0, 0.0, 0.0), wt['g'], wt['b'], wt['w'], wt['bias'], wt['table'], shifted)
            for pipe in PIPES:
                got = _run(eng, x.cuda(), wt, shifted, pipe)
                _within(f'nonfinite C{C} {val} sh{shifted}', pipe, got, ref, mag, bad)
                assert not torch.isfinite(got.cpu()[bad[:, 0]]).all(), 'the non-finite token reached no output'


def _token_grid(B, H, W, shifted, Hp, Wp):
    """(B, Hp, Wp) token index of every position of the (rolled) padded grid, -1 for padding."""
    ys, xs = torch.arange(Hp), torch.arange(Wp)
    if shifted:
        ys, xs = (ys + 3) % Hp, (xs + 3) % Wp
    yy, xx = ys[:, None].expand(Hp, Wp), xs[None, :].expand(Hp, Wp)
    tok = torch.where((yy < H) & (xx < W), yy * W + xx, torch.full_like(yy, -1))
    return torch.stack([torch.where(tok >= 0, tok + bi * H * W, tok) for bi in range(B)])


# ----------------------------------------------------------------------------------------------------------- sentinel, order
@pytest.mark.gpu
@pytest.mark.parametrize('C', (96, 768))
def test_rows_written_and_orders_agree(eng, C):
    """Into a sentinel-filled buffer with spare rows: compact order writes exactly the B*H*W rows [0, B*H*W), token order writes every
    token, and the two are bitwise equal after permuting with the restated compact -> token map."""
    gen = torch.Generator().manual_seed(7 + C)
    wt = weights(gen, C)
    for B, H, W in [(2, 9, 12), (1, 7, 7), (3, 3, 11)]:
        x = torch.randn(B, H, W, C, generator=gen).cuda()
        T = B * H * W
        for shifted in (0, 1):
            for pipe in PIPES:
                outs = {}
                for order in ('token', 'compact'):
                    buf = sentinel(T + 5, C)
                    eng.op_window_msa(x, wt['g'], wt['b'], wt['w'], wt['bias'], wt['table'], shifted, pipe=pipe, order=order, out=buf[:T])
                    assert bool((_bits(buf[T:]) == SENTINEL).all()), (order, 'wrote behind its rows')
                    assert not bool((_bits(buf[:T]) == SENTINEL).any(dim=1).any()), (order, 'left a row unwritten')
                    outs[order] = buf[:T]
                tok = compact_tokens(B, H, W, shifted).cuda()
                assert torch.equal(torch.sort(tok).values, torch.arange(T, device='cuda'))
                assert _same_bits(outs['token'][tok], outs['compact']), (C, B, H, W, shifted, pipe)


# ----------------------------------------------------------------------------------------------------------- batch, determinism
@pytest.mark.gpu
@pytest.mark.parametrize('C', (96, 384))
def test_batch_independence_and_determinism(eng, C):
    """Image b of a B = 3 launch is bitwise the image launched alone (the bias row sits behind the window image of B images, the padbits
    are per window of the image); two launches are bitwise equal."""
    gen = torch.Generator().manual_seed(8 + C)
    wt = weights(gen, C)
    H, W = 10, 13
    x = torch.randn(3, H, W, C, generator=gen).cuda()
    for shifted in (0, 1):
        for pipe in PIPES:
            all3 = _run(eng, x, wt, shifted, pipe)
            assert _same_bits(all3, _run(eng, x, wt, shifted, pipe)), (pipe, shifted, 'not deterministic')
            for bi in range(3):
                one = _run(eng, x[bi:bi + 1].contiguous(), wt, shifted, pipe)
                assert _same_bits(one, all3[bi * H * W:(bi + 1) * H * W]), (pipe, shifted, bi)


# ----------------------------------------------------------------------------------------------------------- the engine's path
@pytest.mark.gpu
def test_op_is_the_engines_path(hip_device):
    """For every block b >= 1 of every stage, the op on tok_s{s}b{b-1} with that block's weights reproduces the engine's attention
    output att_s{s}b{b}: bitwise where both compute the LN statistics the same way (stage 1 on the split pipe, every stage on the fp32
    pipe), within the bound where the engine takes them from the previous GEMM's epilogue (stages 2-4 on the split pipe)."""
    from nuhtc_amd import synth
    from nuhtc_amd import weights as Wt
    from nuhtc_amd.engine import Engine
    sd = Wt.bench_state_dict(0)
    tiles = synth.nuclei_tiles(2, 64, start=0)
    B = len(tiles)
    depths = (2, 2, 6, 2)
    for pipe, mp in (('split', 0), ('fp32', 1)):
        e = Engine(sd, device=0, max_batch=B, tile=(64, 64), matrix_pipe=mp)
        e.enable_token_dump()
        e(tiles)
        for s in range(4):
            C = 96 << s
            H = W = 32 >> s
            for b in range(1, depths[s]):
                p = f'backbone.stages.{s}.blocks.{b}.'
                wt = dict(g=sd[p + 'norm1.weight'], b=sd[p + 'norm1.bias'], w=sd[p + 'attn.w_msa.qkv.weight'],
                          bias=sd[p + 'attn.w_msa.qkv.bias'], table=sd[p + 'attn.w_msa.relative_position_bias_table'])
                x = e.buffer(f'tok_s{s}b{b - 1}')[:B].reshape(B, H, W, C).contiguous()
                att = e.buffer(f'att_s{s}b{b}')[:B].reshape(B * H * W, C)
                order = 'token' if (pipe == 'split' and s == 0) else 'compact'
                got = _run(e, x, wt, b & 1, pipe, order)
                if pipe == 'fp32' or s == 0:
                    assert _same_bits(got, att), (pipe, s, b)
                else:
                    ref, mag = ref_wmsa(x, wt['g'], wt['b'], wt['w'], wt['bias'], wt['table'], b & 1)
                    tok = compact_tokens(B, H, W, b & 1)
                    _within(f'engine s{s}b{b}', pipe, att.cpu()[torch.argsort(tok)], ref, mag)
                    _within(f'engine-op s{s}b{b}', pipe, got.cpu()[torch.argsort(tok)], ref, mag)
        e.close()
        del e


# ----------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_refusals_leave_the_engine_usable(eng):
    """Unsupported C, null pointers, bad enums and sizes whose window image overflows 32-bit offsets are refused with NUHTC_E_INVALID
    (no launch), and the next correct call gives the same bits as before."""
    from nuhtc_amd import hip
    gen = torch.Generator().manual_seed(9)
    wt = weights(gen, 192)
    x = torch.randn(1, 9, 9, 192, generator=gen).cuda()
    good = _run(eng, x, wt, 1, 'split')
    arrs = {k: np.ascontiguousarray(v.numpy(), dtype=np.float32) for k, v in wt.items()}
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = sentinel(81, 192)
    base = dict(x=x.data_ptr(), out=out.data_ptr(), ln_g=vp(arrs['g']), ln_b=vp(arrs['b']), qkv_w=vp(arrs['w']), qkv_b=vp(arrs['bias']),
                rel_table=vp(arrs['table']), B=1, H=9, W=9, C=192, shifted=1, pipe=hip.PIPE_BF16_SPLIT, out_order=hip.ORDER_TOKEN)
    bad = [dict(C=128), dict(C=32), dict(C=0), dict(x=None), dict(out=None), dict(ln_g=None), dict(ln_b=None), dict(qkv_w=None),
           dict(qkv_b=None), dict(rel_table=None), dict(pipe=2), dict(out_order=2), dict(shifted=2), dict(B=0), dict(H=0), dict(W=-1),
           dict(B=1 << 20, H=1 << 10, W=1 << 10), dict(B=3, H=4096, W=4096), dict(B=1, H=70000, W=70000)]
    for kw in bad:
        a = hip.WmsaArgs(**dict(base, **kw))
        assert eng.lib.nuhtc_op_window_msa(eng.h, ctypes.byref(a), eng._stream()) == hip.E_INVALID, kw
        assert bool((_bits(out) == SENTINEL).all()), kw
        assert _same_bits(_run(eng, x, wt, 1, 'split'), good), kw


@pytest.mark.gpu
def test_print_observed_maxima():
    """Summary of the largest err / mag seen per class and pipe in this module (run with -s)."""
    for (tag, pipe), rel in sorted(OBSERVED.items()):
        print(f'max err/mag {rel:.3e}  [{pipe}]  {tag}')


# ----------------------------------------------------------------------------------------------------------- host-only
def test_reference_is_mmdet_window_attention():
    """ref_wmsa with proj applied equals the oracle's ShiftWindowMSA (oracle/model.py window_attention) in float64, including grids
    below one window, both residue axes, and both shift states."""
    from oracle import model as O
    gen = torch.Generator().manual_seed(10)
    C = 192
    wt = weights(gen, C)
    pw, pb = torch.randn(C, C, generator=gen) / math.sqrt(C), torch.randn(C, generator=gen)
    sd = {'a.qkv.weight': wt['w'].double(), 'a.qkv.bias': wt['bias'].double(), 'a.relative_position_bias_table': wt['table'].double(),
          'a.proj.weight': pw.double(), 'a.proj.bias': pb.double()}
    for B, H, W in [(1, 3, 5), (2, 6, 6), (1, 7, 7), (1, 9, 14), (2, 14, 9), (1, 13, 20)]:
        x = torch.randn(B, H, W, C, generator=gen).double()
        h = F.layer_norm(x, (C,), wt['g'].double(), wt['b'].double(), 1e-5).reshape(B, H * W, C)
        for shifted in (0, 1):
            want = O.window_attention(sd, 'a.', h, H, W, C // 32, bool(shifted)).reshape(B * H * W, C)
            got, mag = ref_wmsa(x, wt['g'], wt['b'], wt['w'], wt['bias'], wt['table'], shifted)
            assert torch.allclose(got @ pw.double().T + pb.double(), want, rtol=1e-10, atol=1e-10), (B, H, W, shifted)
            assert (got.abs() <= mag * (1 + 1e-12) + 1e-12).all()


def _naive(x, g, b, w, bias, table, shifted):
    """Per-window loop straight from swin.py: LN, F.pad, roll, for each window and head softmax(s q k^T + B + M) v, scatter back."""
    x = x.double()
    B, H, W, C = x.shape
    nH = C // 32
    ln = F.layer_norm(x, (C,), g.double(), b.double(), 1e-5)
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    P = torch.zeros(B, Hp, Wp, C, dtype=torch.float64)
    P[:, :H, :W] = ln
    sy = sx = 3 if shifted else 0
    ids = regions(Hp, Wp)
    out = torch.zeros(B, Hp, Wp, C, dtype=torch.float64)
    for bi in range(B):
        for wy in range(0, Hp, WS):
            for wx in range(0, Wp, WS):
                pos = [((wy + i // WS + sy) % Hp, (wx + i % WS + sx) % Wp) for i in range(WS * WS)]
                t = torch.stack([P[bi, y, xx] for y, xx in pos])
                qkv = t @ w.double().T + bias.double()
                for h in range(nH):
                    q, k, v = (qkv[:, j * C + 32 * h: j * C + 32 * h + 32] for j in range(3))
                    s = SCALE * q @ k.T
                    for i in range(WS * WS):
                        for j in range(WS * WS):
                            dy = i // WS - j // WS
                            dx = i % WS - j % WS
                            s[i, j] += table[(dy + 6) * 13 + dx + 6, h].double()
                            ri, rj = ids[wy + i // WS, wx + i % WS], ids[wy + j // WS, wx + j % WS]
                            if shifted and ri != rj:
                                s[i, j] -= 100.0
                    o = s.softmax(-1) @ v
                    for i, (y, xx) in enumerate(pos):
                        out[bi, y, xx, 32 * h:32 * h + 32] = o[i]
    return out[:, :H, :W].reshape(B * H * W, C)


def test_reference_vs_naive_window_loop():
    gen = torch.Generator().manual_seed(11)
    C = 64
    wt = weights(gen, C)
    for B, H, W in [(1, 8, 10), (2, 3, 9)]:
        x = torch.randn(B, H, W, C, generator=gen)
        for shifted in (0, 1):
            got, _ = ref_wmsa(x, wt['g'], wt['b'], wt['w'], wt['bias'], wt['table'], shifted)
            want = _naive(x, wt['g'], wt['b'], wt['w'], wt['bias'], wt['table'], shifted)
            assert torch.allclose(got, want, rtol=1e-10, atol=1e-10), (B, H, W, shifted)


def test_compact_order_and_probe_plan():
    """compact_tokens is a permutation of the tokens; the probe plan reaches every offset with C = 768, every key (31, 32, 48
    included) is some query's +30 key, and a probe's reference is sharp: most queries put > 1 - 1e-9 on one key."""
    for B, H, W in [(1, 1, 1), (2, 9, 12), (1, 14, 14), (3, 20, 6)]:
        for shifted in (0, 1):
            tok = compact_tokens(B, H, W, shifted)
            assert torch.equal(torch.sort(tok).values, torch.arange(B * H * W))
    offs = set(o for p in probe_plan(768, 8) for o in p)
    assert offs == set(range(169))
    rel = rel_index()
    keys = set(int(j) for o in offs for j in torch.nonzero(rel == o)[:, 1])
    assert {31, 32, 48} <= keys and len(keys) == 49
    assert {int(i) for o in offs for i in torch.nonzero(rel == o)[:, 0]} == set(range(49))
    gen = torch.Generator().manual_seed(12)
    C = 96
    wt = probe_weights(gen, C, probe_plan(C, 1)[0])
    x = torch.randn(1, 14, 20, C, generator=gen)
    ref, _ = ref_wmsa(x, wt['g'], wt['b'], wt['w'], wt['bias'], wt['table'], 0)
    ln = F.layer_norm(x.double(), (C,), wt['g'].double(), wt['b'].double(), 1e-5).reshape(-1, C)
    # a query whose +30 key is a real token of its window takes that token's LN vector: count those (query, head) pairs and the hits
    Hp, Wp = 14, 21
    t = _windows(_token_grid(1, 14, 20, 0, Hp, Wp)[..., None], Hp, Wp).reshape(-1, WS * WS)
    want = hits = 0
    for h, o in enumerate(probe_plan(C, 1)[0]):
        i, j = torch.nonzero(rel == o, as_tuple=True)
        want += int(((t[:, i] >= 0) & (t[:, j] >= 0)).sum())
        d = torch.cdist(ref[:, 32 * h:32 * h + 32], ln[:, 32 * h:32 * h + 32], compute_mode='donot_use_mm_for_euclid_dist')
        hits += int((d.min(1).values < 1e-9).sum())
    assert want > 0 and hits >= want, (hits, want)
