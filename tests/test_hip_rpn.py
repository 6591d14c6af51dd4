"""The RPN half of proposal generation, op by op, on designed inputs: rpn_level_kernel (sigmoid, radix select, LDS sort, anchor decode,
clamp, min-size filter), the two NMS routes launch_nms_levels / launch_nms with the level as id (csrc/proposals.hip) and build_rois_kernel
(csrc/roi.hip).  Engine.op_rpn_select / op_nms_levels / op_build_rois (nuhtc_op_*) fill the parameter blocks run_roi_path fills and call
the same launch functions (test_ops_are_the_engines_rpn_path shows it bit for bit).  The host-only checks of the references and of the
designed inputs are in tests/test_rpn_reference.py (this file is marked gpu as a whole).

Why the selection is compared exactly.  Objectness logits are drawn from the grid j / 64, |x| <= 8.  Equal logits give bit-equal scores
on both sides.  Two distinct grid values differ by at least 1 / 64 in x, hence by s (1 - s) / 64 in the sigmoid s; relative to the
spacing of fp32 numbers at s that is smallest at x = +8, where s (1 - s) / 64 = 5.2e-6 against 2^-24 = 6.0e-8: about 80 units (for
x < 0 the relative step (1 - s) / 64 is above 2^-7).  The kernel's 1 / (1 + expf(-x)) is within 4 u of the true value (expf within 2 u,
as tests/test_hip_dettail.py assumes, one for the add, one for the division), so neither side can reorder two grid values or split a
tie: the selected index set and its (score descending, index ascending) order are fully determined, and the tests demand them exactly --
the share of cases they may leave out is zero.  The reference orders by the float32 image of the float64 sigmoid, which keeps both
properties.  Plateau cases use constant maps and logits 18, 20, 30: there expf(-x) < 2^-25, so 1 + expf(-x) and the float32 image of the
float64 sigmoid are both exactly 1.0.

The op returns boxes and scores, not indices: a row is identified by its box, so the inputs are checked (on the CPU too) to have
neighbours in the reference order that differ by far more than the bound wherever their scores tie.

Bounds (u = 2^-24): anchors are built from correctly rounded float32 steps (sqrt, reciprocal, products, sums) in numpy and are exact on
both sides; boxes are held to BOX_C u geom of tests/test_hip_dettail.py (stds 1), and exactly where the float64 value lies beyond a clip
limit by more than that bound (both sides then clip); scores to 4 u relative.  A min-size decision may differ only where the float64
width or height is within the box bound (plus the rounding of the subtraction) of min_size: the designed inputs have no such row, which
is asserted, so counts are compared exactly.

The NMS kernels promise the reference's float32 steps (-ffp-contract=off), so they are compared bit for bit with
oracle.ops_np.batched_nms (mmcv's offset trick restated in float32, pinned by tests/test_oracle_ops.py): kept sources, order, rows and
counts, on both routes.  The smallest |IoU - thr| over the pairs of a case (float64) is printed, not asserted."""
import functools

import numpy as np
import pytest
import torch

from test_hip_dettail import BOX_C, MAX_RATIO, SENTINEL, U, ref_delta2bbox

pytestmark = pytest.mark.gpu

SCORE_C = 4                      # 1 / (1 + expf(-x)): expf 2 u, add 1, division 1
SAT = (18.0, 20.0, 30.0)         # fp32 sigmoid == 1.0 exactly
OBSERVED = {}


def _obs(key, v):
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), float(v))


# ================================================================================================================ selection reference
def anchors_f32(level, py, px, a):
    """AnchorGenerator(scales [4], ratios (.5, 1, 2), centre offset 0) for stride 4 << level, in the kernel's float32 steps."""
    f = np.float32
    stride = f(4 << level)
    hr = np.sqrt(np.asarray([0.5, 1.0, 2.0], f))
    wr = f(1.0) / hr
    wsz, hsz = (stride * wr * f(4.0))[a], (stride * hr * f(4.0))[a]
    sx, sy = px.astype(f) * stride, py.astype(f) * stride
    out = np.stack([f(-0.5) * wsz + sx, f(-0.5) * hsz + sy, f(0.5) * wsz + sx, f(0.5) * hsz + sy], 1)
    assert out.dtype == np.float32
    return out


def ref_level(m, level, k, img_hw, min_size):
    """One (image, level): m (h, w, 32) float32 -> the selected anchors in order, their float64 boxes, bounds, scores and the min-size verdict."""
    h, w = m.shape[:2]
    flat = m.reshape(h * w, 32)
    x = flat[:, :3].reshape(-1).astype(np.float64)
    s64 = 1.0 / (1.0 + np.exp(-x))
    s32 = s64.astype(np.float32)
    n = h * w * 3
    order = np.argsort(-s32, kind='stable')[:k] if n > k else np.arange(n)      # n <= nms_pre: no sort (rpn_head.py:167)
    pix, a = order // 3, order % 3
    anch = anchors_f32(level, pix // w, pix % w, a)
    d = flat[:, 3:15].reshape(h * w, 3, 4)[pix, a]
    o, t = ref_delta2bbox(anch, d, (1.0, 1.0, 1.0, 1.0), img_hw[1], img_hw[0])
    bound = BOX_C * U * t['geom']
    raw = np.stack([t['gx'] - t['gw'] * 0.5, t['gy'] - t['gh'] * 0.5, t['gx'] + t['gw'] * 0.5, t['gy'] + t['gh'] * 0.5], 1)
    lim = np.asarray([img_hw[1], img_hw[0], img_hw[1], img_hw[0]], np.float64)
    bound = np.where((raw < -bound) | (raw > lim + bound), 0.0, bound)          # beyond a clip limit by more than the bound: exact on both sides
    ms = float(np.float32(min_size))
    wd, ht = o[:, 2] - o[:, 0], o[:, 3] - o[:, 1]
    bw, bh = bound[:, 0] + bound[:, 2], bound[:, 1] + bound[:, 3]
    band = ((bw > 0) & (np.abs(wd - ms) <= bw + U * wd)) | ((bh > 0) & (np.abs(ht - ms) <= bh + U * ht))
    return dict(order=order, boxes=o, bound=bound, geom=t['geom'], scores=s64[order], s32=s32[order], valid=(wd > ms) & (ht > ms), band=band)


def rows_identify_anchors(r):
    """Neighbours of the reference order whose scores tie have boxes further apart than four bounds: a row names its anchor."""
    tie = r['s32'][1:] == r['s32'][:-1]
    far = (np.abs(r['boxes'][1:] - r['boxes'][:-1]) > 4 * (r['bound'][1:] + r['bound'][:-1]) + 1e-3).any(1)
    both = r['valid'][1:] & r['valid'][:-1]
    return bool((far | ~tie | ~both).all())


# ================================================================================================================ designed selection inputs
def grid_logits(rng, n, lo=-8.0, hi=8.0):
    return (rng.integers(int(lo * 64), int(hi * 64) + 1, n) / 64.0).astype(np.float32)


def pattern_logits(rng, kind, n, k):
    if kind == 'random':
        return grid_logits(rng, n)
    if kind == 'few':                                   # eight values: rank k falls inside a tie
        return rng.choice(grid_logits(rng, 8), n).astype(np.float32)
    if kind == 'const':
        return np.full(n, 0.25, np.float32)
    if kind.startswith('sat'):                          # 'sat5000': that many saturated scores, wider than the sort image
        p = int(kind[3:])
        x = grid_logits(rng, n)
        x[rng.permutation(n)[:p]] = rng.choice(np.asarray(SAT, np.float32), p)
        return x
    if kind.startswith('ge'):                           # 'ge4096': keys >= T number exactly that, rank k inside the tie at -1.0
        ge, top = int(kind[2:]), 2000
        assert top < k < ge <= n
        x = np.concatenate([grid_logits(rng, top, 0.5, 8.0), np.full(ge - top, -1.0, np.float32), grid_logits(rng, n - ge, -8.0, -1.5)])
        return x[rng.permutation(n)]
    raise KeyError(kind)


def level_map(rng, h, w, kind, k, tame=False):
    n = h * w * 3
    m = rng.standard_normal((h, w, 32)).astype(np.float32)           # columns 15.. are never read: anything
    m[..., :3] = pattern_logits(rng, kind, n, k).reshape(h, w, 3)
    d = np.empty((h, w, 3, 4), np.float32)
    r = 0.1 if tame else 0.5
    d[..., :2] = rng.uniform(-r, r, (h, w, 3, 2))
    d[..., 2:] = rng.uniform(-0.5 if tame else -1.0, 1.0, (h, w, 3, 2))
    m[..., 3:15] = d.reshape(h, w, 12)
    return m


# name -> nms_pre, image size, min_size, the four level sizes, the logit pattern per image and level
SELECT_CASES = {
    # in-register route at its last size 49152, scratch-row route at 129 x 128 x 3, a tie across rank k, n < k
    'routes_k1000': dict(k=1000, img=(600, 700), min_size=10.0, dims=[(128, 128), (129, 128), (20, 50), (2, 3)], kinds=[['random', 'random', 'few', 'random']]),
    # plateau branch on the scratch-row route (constant, saturated) and in registers; n == k + 2 beside it
    'plateau_k1000': dict(k=1000, img=(600, 700), min_size=0.0, dims=[(129, 128), (128, 128), (1, 334), (1, 1)],
                          kinds=[['const', 'sat5000', 'random', 'random'], ['sat6000', 'few', 'few', 'const']]),
    # n == k, n == k + 3, n < k, n == 3: the unsorted branch emits in index order
    'unsorted_k300': dict(k=300, img=(90, 100), min_size=6.0, dims=[(10, 10), (1, 101), (9, 11), (1, 1)], kinds=[['random', 'random', 'few', 'random']]),
    # n == k + 1 (sorted, one dropped), n < k, n == k + 1 with ties, n < k
    'unsorted_k299': dict(k=299, img=(90, 100), min_size=6.0, dims=[(10, 10), (33, 3), (1, 100), (2, 2)], kinds=[['random', 'random', 'few', 'const']]),
    # (k - need) + s_eq == 4096 (usual branch, full sort image) against 4097 (plateau branch), a constant map, a saturated plateau; B = 2
    'edge4096_k3000': dict(k=3000, img=(200, 180), min_size=4.0, dims=[(40, 40)] * 4,
                           kinds=[['ge4096', 'ge4097', 'const', 'sat4500'], ['random', 'few', 'ge4097', 'ge4096']]),
    # nms_pre = 4096 and every selected box valid: the slot is full
    'full_k4096': dict(k=4096, img=(400, 400), min_size=0.0, dims=[(40, 40), (37, 37), (32, 43), (8, 8)], kinds=[['random', 'few', 'sat4100', 'random']], tame=True),
}


@functools.lru_cache(maxsize=None)
def select_case(name):
    """-> (spec, maps: four arrays (B, h, w, 32), ref[b][l])"""
    c = SELECT_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    maps = [np.stack([level_map(rng, *c['dims'][l], kinds[l], c['k'], c.get('tame', False)) for kinds in c['kinds']]) for l in range(4)]
    ref = [[ref_level(maps[l][b], l, c['k'], c['img'], c['min_size']) for l in range(4)] for b in range(len(c['kinds']))]
    return c, maps, ref


def select_branch(kind_n_k):
    """What rpn_level_kernel does for a level of n anchors whose keys >= T number `ge`: (route, branch)."""
    n, k, ge = kind_n_k
    route = 'unsorted' if n <= k else ('registers' if n <= 48 * 1024 else 'scratch')
    return route, (None if n <= k else ('usual' if ge <= 4096 else 'plateau'))


def keys_ge_T(m, k):
    """Number of keys >= the rank-k key of one level map (float32 image of the float64 sigmoid: same ties as the kernel's keys)."""
    x = m[..., :3].reshape(-1).astype(np.float64)
    s = (1.0 / (1.0 + np.exp(-x))).astype(np.float32)
    if len(s) <= k:
        return len(s)
    T = np.sort(s)[::-1][k - 1]
    return int((s >= T).sum())


# ---- placed exact cases: zero deltas on level 2 (ratio-1 anchors are 64 x 64, exact), clamp rows on level 1
PLACED_IMG = (112, 120)


@functools.lru_cache(maxsize=None)
def placed_maps():
    rng = np.random.default_rng(77)
    maps = []
    for l, (h, w) in enumerate([(4, 4), (6, 6), (8, 8), (2, 2)]):
        m = np.zeros((1, h, w, 32), np.float32)
        m[..., :3] = grid_logits(rng, h * w * 3).reshape(1, h, w, 3)
        maps.append(m)
    d = maps[1][0, :, :, 3:15].reshape(6, 6, 3, 4)
    d[..., 2] = np.where(np.arange(36).reshape(6, 6, 1) % 2 == 0, 10.0, -10.0)      # dw, dh beyond +-MAX_RATIO, both signs
    d[..., 3] = -d[..., 2]
    maps[1][0, :, :, 3:15] = d.reshape(6, 6, 12)
    return maps


# ================================================================================================================ NMS reference and inputs
def ref_nms(boxes, scores, counts, thr, max_keep):
    """oracle.ops_np.batched_nms on the group-major candidates of every image -> per image (dets (K, 5) float32, src (K,) flat index)."""
    from oracle import ops_np
    B, G, slot = scores.shape
    out = []
    for b in range(B):
        bx = np.concatenate([boxes[b, g, :counts[b, g]] for g in range(G)])
        sc = np.concatenate([scores[b, g, :counts[b, g]] for g in range(G)])
        ids = np.concatenate([np.full(counts[b, g], g) for g in range(G)])
        src = np.concatenate([(b * G + g) * slot + np.arange(counts[b, g]) for g in range(G)])
        dets, keep = ops_np.batched_nms(bx, sc, ids, thr)
        out.append((dets[:max_keep].astype(np.float32), src[keep][:max_keep].astype(np.int64)))
    return out


def min_iou_gap(boxes, counts, thr):
    """Smallest |IoU - thr| over the pairs of one group (float64, boxes without the offset)."""
    gap = np.inf
    B, G = counts.shape
    for b in range(B):
        for g in range(G):
            x = boxes[b, g, :counts[b, g]].astype(np.float64)
            if len(x) < 2:
                continue
            iw = np.clip(np.minimum(x[:, None, 2], x[None, :, 2]) - np.maximum(x[:, None, 0], x[None, :, 0]), 0, None)
            ih = np.clip(np.minimum(x[:, None, 3], x[None, :, 3]) - np.maximum(x[:, None, 1], x[None, :, 1]), 0, None)
            ar = (x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])
            with np.errstate(all='ignore'):
                iou = iw * ih / (ar[:, None] + ar[None, :] - iw * ih)
            iou = iou[np.triu_indices(len(x), 1)]
            iou = iou[np.isfinite(iou)]
            if len(iou):
                gap = min(gap, float(np.abs(iou - float(np.float32(thr))).min()))
    return gap


def group_boxes(rng, kind, n):
    if kind == 'spread':                               # moderate overlap
        xy, wh = rng.uniform(0, 300, (n, 2)), rng.uniform(8, 60, (n, 2))
    elif kind == 'clusters':                           # heavy overlap: removal words travel across chunks
        c = rng.uniform(40, 400, (max(n // 60, 2), 2))
        xy, wh = c[rng.integers(0, len(c), n)] + rng.uniform(-3, 3, (n, 2)), 40 + rng.uniform(-3, 3, (n, 2))
    elif kind == 'separate':                           # nothing overlaps: every row survives
        i = np.arange(n)
        xy, wh = np.stack([(i % 20) * 25.0, (i // 20) * 25.0], 1) + rng.uniform(0, 2, (n, 2)), rng.uniform(10, 20, (n, 2))
    else:
        raise KeyError(kind)
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def nms_inputs(counts, kinds, slot, seed, score_levels=16):
    """counts (B, G), kinds[g] -> boxes (B, G, slot, 4), scores (B, G, slot); scores on the grid j / score_levels, so ties inside and across
    groups are common; slots from the count on hold what would win the sort and raise the offset if they were read."""
    counts = np.asarray(counts, np.int32)
    B, G = counts.shape
    rng = np.random.default_rng(seed)
    boxes = np.full((B, G, slot, 4), 3.0e38, np.float32)
    scores = np.full((B, G, slot), 2.0, np.float32)
    for b in range(B):
        for g in range(G):
            n = int(counts[b, g])
            boxes[b, g, :n] = group_boxes(rng, kinds[g], n)
            scores[b, g, :n] = rng.integers(1, score_levels, n) / np.float32(score_levels)
    return boxes, scores, counts


NMS_CASES = {
    # empty groups, group 0 among them
    'empty_groups': dict(counts=[[0, 5, 0, 70]], kinds=['spread'] * 4, slot=128, max_keep=100),
    'all_empty': dict(counts=[[0, 0, 0, 0]], kinds=['spread'] * 4, slot=64, max_keep=10),
    # one row, one short of a chunk, a chunk, a chunk and one; a second image with other counts
    'chunk_edges_b2': dict(counts=[[1, 63, 64, 65], [70, 0, 5, 128]], kinds=['clusters', 'spread', 'clusters', 'spread'], slot=128, max_keep=256),
    'full_slot': dict(counts=[[128, 128, 128, 128]], kinds=['clusters', 'spread', 'clusters', 'separate'], slot=128, max_keep=512),
    # group 0 reaches max_keep at row 36 of its second chunk (words 2 and 3 of its keepbits must be zeroed), the others still have
    # survivors: 190 in all against max_keep = 100, the global cut falls inside a tie
    'group_break_and_cut': dict(counts=[[200, 50, 30, 10]], kinds=['separate'] * 4, slot=200, max_keep=100, score_levels=8),
    # clusters of ~60 boxes over five chunks
    'clusters': dict(counts=[[300, 130, 0, 64]], kinds=['clusters'] * 4, slot=320, max_keep=50),
    'one_group': dict(counts=[[150]], kinds=['clusters'], slot=150, max_keep=2048, score_levels=64),
}


@functools.lru_cache(maxsize=None)
def nms_case(name):
    c = NMS_CASES[name]
    boxes, scores, counts = nms_inputs(c['counts'], c['kinds'], c['slot'], sum(map(ord, name)), c.get('score_levels', 16))
    return boxes, scores, counts, 0.7, c['max_keep'], ref_nms(boxes, scores, counts, 0.7, c['max_keep'])


def placed_iou_case():
    """Small-integer boxes in group 0 and group 3 (offset 3 * 301: still integers, every step exact): 70 / 100 is not > 0.7f, 71 / 100 is.
    -> boxes, scores, counts, expected kept (group, index) in output order."""
    slot = 8
    boxes = np.full((1, 4, slot, 4), 3.0e38, np.float32)
    scores = np.full((1, 4, slot), 2.0, np.float32)
    rows = [([0, 0, 100, 100], 0.9), ([0, 0, 100, 70], 0.8), ([200, 0, 300, 100], 0.9), ([200, 0, 300, 71], 0.8)]
    for g in (0, 3):
        for i, (bx, s) in enumerate(rows):
            boxes[0, g, i], scores[0, g, i] = bx, s
    counts = np.asarray([[4, 0, 0, 4]], np.int32)
    # equal scores across groups: group-major position decides
    return boxes, scores, counts, [(0, 0), (0, 2), (3, 0), (3, 2), (0, 1), (3, 1)]


# ================================================================================================================ chain inputs
CHAIN = dict(k=300, img=(64, 64), min_size=4.0, dims=[(16, 16), (8, 8), (4, 4), (2, 2)], iou=0.7, max_keep=100, B=2, seed=9)


def chain_pairs_clear(ref_b, thr):
    """The chain runs NMS on float32 boxes that differ from side to side.  With every coordinate of a pair within d of the float64 one
    (d = the larger of the two rows' box bounds) and S the longest side involved: the intersection's sides move by at most 2 d each, so
    the intersection by 4 d S and each area likewise, the union by 12 d S, and IoU = I / Un by at most 4 d S / Un + I 12 d S / Un^2 <=
    16 d S / Un (second order in d / S ~ 1e-6 left to the 17).  -> the smallest |IoU - thr| - 17 d S / Un over the pairs of one level:
    positive means that no decision of the chain depends on which side's boxes it sees."""
    worst = np.inf
    for r in ref_b:
        x, d1 = r['boxes'][r['valid']], r['bound'][r['valid']].max(1, initial=0.0)
        if len(x) < 2:
            continue
        iw = np.clip(np.minimum(x[:, None, 2], x[None, :, 2]) - np.maximum(x[:, None, 0], x[None, :, 0]), 0, None)
        ih = np.clip(np.minimum(x[:, None, 3], x[None, :, 3]) - np.maximum(x[:, None, 1], x[None, :, 1]), 0, None)
        side = np.maximum(x[:, 2] - x[:, 0], x[:, 3] - x[:, 1])
        ar = (x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])
        un = ar[:, None] + ar[None, :] - iw * ih
        slack = 17 * np.maximum(d1[:, None], d1[None, :]) * np.maximum(side[:, None], side[None, :]) / un
        m = np.abs(iw * ih / un - float(np.float32(thr))) - slack
        worst = min(worst, float(m[np.triu_indices(len(x), 1)].min()))
    return worst


@functools.lru_cache(maxsize=None)
def chain_case():
    c = CHAIN
    rng = np.random.default_rng(c['seed'])
    maps = [np.stack([level_map(rng, *c['dims'][l], 'random', c['k']) for _ in range(c['B'])]) for l in range(4)]
    ref = [[ref_level(maps[l][b], l, c['k'], c['img'], c['min_size']) for l in range(4)] for b in range(c['B'])]
    return c, maps, ref


def chain_candidates(ref_b, slot):
    """The float64 reference's valid rows of one image as grouped float32 candidates."""
    boxes = np.zeros((1, 4, slot, 4), np.float32)
    scores = np.zeros((1, 4, slot), np.float32)
    counts = np.zeros((1, 4), np.int32)
    for l, r in enumerate(ref_b):
        v = r['valid']
        n = int(v.sum())
        boxes[0, l, :n], scores[0, l, :n], counts[0, l] = r['boxes'][v], r['scores'][v], n
    return boxes, scores, counts


def oracle_proposals(maps, c):
    from oracle import model as O
    cls = [torch.from_numpy(np.ascontiguousarray(m[..., :3])).permute(0, 3, 1, 2) for m in maps]
    reg = [torch.from_numpy(np.ascontiguousarray(m[..., 3:15])).permute(0, 3, 1, 2) for m in maps]
    return [p.numpy() for p in O.rpn_proposals(cls, reg, c['img'], nms_pre=c['k'], max_per_img=c['max_keep'], iou=c['iou'], min_size=c['min_size'])]


def chain_row_bounds(ref_b, src, slot):
    """Box bound of the rows `src` (flat index into the (1, 4, slot) candidates of chain_candidates)."""
    g, i = src // slot, src % slot
    return np.stack([ref_b[gg]['bound'][ref_b[gg]['valid']][ii] for gg, ii in zip(g, i)]) if len(src) else np.zeros((0, 4))


# ================================================================================================================ GPU helpers
@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    return Engine(weights.seeded_state_dict(0), device=0, max_batch=1, tile=(64, 64))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinel(*shape, dtype=torch.float32):
    t = torch.full(shape, SENTINEL, dtype=torch.int32, device='cuda')
    return t.view(torch.float32) if dtype == torch.float32 else t


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _keeps_sentinel(t):
    return bool((_bits(t) == SENTINEL).all())


def run_select(eng, maps, k, img, min_size):
    B = maps[0].shape[0]
    cb, cs, cc = eng.op_rpn_select([dev(m) for m in maps], k, img, min_size, cand_boxes=sentinel(B, 4, k, 4), cand_scores=sentinel(B, 4, k),
                                   cand_count=sentinel(B, 4, dtype=torch.int32))
    return cb, cs, cc


def check_level(tag, r, gb, gs, cnt):
    """One (image, level) of the op's output against ref_level's verdict: count and order exact, boxes and scores inside their bounds."""
    assert not r['band'].any(), f'{tag}: the designed input has a min-size decision inside its band'
    assert rows_identify_anchors(r), tag
    v = r['valid']
    assert cnt == int(v.sum()), f'{tag}: {cnt} rows, reference {int(v.sum())}'
    assert _keeps_sentinel(gb[cnt:]) and _keeps_sentinel(gs[cnt:]), f'{tag}: rows behind the count were written'
    if cnt == 0:
        return
    b, s = gb[:cnt].cpu().numpy().astype(np.float64), gs[:cnt].cpu().numpy().astype(np.float64)
    eb, es = np.abs(b - r['boxes'][v]), np.abs(s - r['scores'][v])
    _obs('box error / (u geom), bound %d' % BOX_C, (eb / (U * r['geom'][v])).max())
    _obs('score error / (u score), bound %d' % SCORE_C, (es / (U * r['scores'][v])).max())
    bad = np.nonzero((eb > r['bound'][v]).any(1) | (es > SCORE_C * U * r['scores'][v]))[0]
    assert len(bad) == 0, f'{tag}: row {bad[0]} of {cnt}: got {b[bad[0]]} {s[bad[0]]}, reference {r["boxes"][v][bad[0]]} {r["scores"][v][bad[0]]}'


# ================================================================================================================ selection
@pytest.mark.parametrize('name', list(SELECT_CASES))
def test_rpn_select_vs_fp64(eng, name):
    """Every (image, level) of the case: the selected anchors in (score descending, index ascending) order -- index order when the level has
    no more than nms_pre -- decoded, clipped and filtered, against the float64 reference; slots behind cand_count keep the sentinel."""
    c, maps, ref = select_case(name)
    cb, cs, cc = run_select(eng, maps, c['k'], c['img'], c['min_size'])
    cc = cc.cpu().numpy()
    seen = set()
    for b in range(len(ref)):
        for l in range(4):
            n = maps[l].shape[1] * maps[l].shape[2] * 3
            seen.add(select_branch((n, c['k'], keys_ge_T(maps[l][b], c['k']))))
            check_level(f'{name} image {b} level {l} (n = {n})', ref[b][l], cb[b, l], cs[b, l], int(cc[b, l]))
    print(f'{name}: counts {cc.tolist()}, paths {sorted(seen, key=str)}')
    want = {'routes_k1000': {('registers', 'usual'), ('scratch', 'usual'), ('unsorted', None)},
            'plateau_k1000': {('scratch', 'plateau'), ('registers', 'plateau'), ('registers', 'usual')},
            'edge4096_k3000': {('registers', 'usual'), ('registers', 'plateau')}}.get(name, set())
    assert want <= seen, f'{name}: the case no longer reaches {want - seen}'
    if name == 'full_k4096':
        assert int(cc[0, 0]) == 4096


def test_rpn_select_same_image_twice_and_apart(eng):
    """The same image at batch positions 0 and 1 gives the same bits at both (the scratch-row route keeps a key row per image), and a batch of two
    different images gives each the bits it gets alone."""
    c, maps, ref = select_case('routes_k1000')
    one = run_select(eng, maps, c['k'], c['img'], c['min_size'])
    two = run_select(eng, [np.concatenate([m, m]) for m in maps], c['k'], c['img'], c['min_size'])
    for t1, t2 in zip(one, two):
        assert torch.equal(_bits(t2[0]), _bits(t2[1])) and torch.equal(_bits(t2[0]), _bits(t1[0]))
    c, maps, ref = select_case('edge4096_k3000')
    both = run_select(eng, maps, c['k'], c['img'], c['min_size'])
    for b in range(2):
        alone = run_select(eng, [m[b:b + 1] for m in maps], c['k'], c['img'], c['min_size'])
        for t1, t2 in zip(alone, both):
            assert torch.equal(_bits(t1[0]), _bits(t2[b])), b


def test_rpn_select_placed_decisions(eng):
    """Zero deltas on an 8 x 8 level 2: the 16 ratio-1 anchors that cross no border are exactly 64 x 64.  min_size = 64 drops them (64 > 64 is
    false) and one fp32 step below keeps exactly them, bit-exact; anchors over a border clip to exactly 0 / img_w / img_h; dw, dh = +-10 clamp."""
    maps = placed_maps()
    k, img = 400, PLACED_IMG
    below = float(np.nextafter(np.float32(64.0), np.float32(0.0)))
    _, _, c64 = run_select(eng, maps, k, img, 64.0)
    assert int(c64[0, 2]) == 0
    cb, cs, cc = run_select(eng, maps, k, img, below)
    exp = np.asarray([[px * 16 - 32, py * 16 - 32, px * 16 + 32, py * 16 + 32] for py in range(2, 6) for px in range(2, 6)], np.float32)
    # interior ratio-1 anchors: x in [0, 120] needs 2 <= px <= 5 (px = 6 reaches 128), y in [0, 112] needs 2 <= py <= 5
    assert int(cc[0, 2]) == len(exp) and np.array_equal(cb[0, 2, :len(exp)].cpu().numpy(), exp)
    # min_size 0: every anchor with a positive clipped size; checked against the reference (exact where clipped), and the placed values
    cb, cs, cc = run_select(eng, maps, k, img, 0.0)
    for l in range(4):
        check_level(f'placed level {l}', ref_level(maps[l][0], l, k, img, 0.0), cb[0, l], cs[0, l], int(cc[0, l]))
    got = cb[0, 2, :int(cc[0, 2])].cpu().numpy()
    assert (got[:, 0] == 0).any() and (got[:, 1] == 0).any() and (got[:, 2] == img[1]).any() and (got[:, 3] == img[0]).any()
    assert got.min() >= 0 and got[:, [0, 2]].max() <= img[1] and got[:, [1, 3]].max() <= img[0]
    # the clamp (level 1, dw = -dh = +-10): check_level above holds the rows to the clamped reference; the narrow side, where the image does
    # not clip it, is e^-MAX_RATIO = 0.016 of an anchor side of at least 22.6, not e^-10 = 4.5e-5 of it
    r = ref_level(maps[1][0], 1, k, img, 0.0)
    g1 = cb[0, 1, :int(cc[0, 1])].cpu().numpy().astype(np.float64)
    bd = r['bound'][r['valid']]
    seen = 0
    for lo, hi in ((0, 2), (1, 3)):
        side = g1[:, hi] - g1[:, lo]
        rows = (bd[:, lo] > 0) & (bd[:, hi] > 0) & (side < 5.0)
        seen += int(rows.sum())
        assert (side[rows] > 0.015 * 22.0).all() and (side[rows] < 0.017 * 46.0).all()
    assert seen > 10


def test_rpn_select_refuses_4097(eng):
    from nuhtc_amd.engine import HipError
    c, maps, ref = select_case('unsorted_k300')
    good = run_select(eng, maps, c['k'], c['img'], c['min_size'])
    with pytest.raises(HipError, match='error -1'):
        run_select(eng, maps, 4097, c['img'], c['min_size'])
    again = run_select(eng, maps, c['k'], c['img'], c['min_size'])
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(good, again))


# ================================================================================================================ NMS
def run_nms(eng, boxes, scores, counts, thr, max_keep, route):
    B = scores.shape[0]
    dets, src, cnt = eng.op_nms_levels(dev(boxes), dev(scores), counts, thr, max_keep, route=route, dets=sentinel(B, max_keep, 5),
                                       src=sentinel(B, max_keep, dtype=torch.int32))
    return dets, src, cnt


def check_nms(tag, got, ref):
    dets, src, cnt = got
    for b, (rd, rs) in enumerate(ref):
        n = int(cnt[b])
        assert n == len(rs), f'{tag} image {b}: {n} kept, reference {len(rs)}'
        assert np.array_equal(src[b, :n].cpu().numpy(), rs), f'{tag} image {b}: kept sources or their order differ'
        assert np.array_equal(dets[b, :n].cpu().numpy().view(np.int32), rd.view(np.int32)), f'{tag} image {b}: rows differ'
        assert _keeps_sentinel(dets[b, n:]) and _keeps_sentinel(src[b, n:]), f'{tag} image {b}: rows behind the count were written'


@pytest.mark.parametrize('name', list(NMS_CASES))
def test_nms_levels_vs_batched_nms(eng, name):
    """Both routes against oracle.ops_np.batched_nms, bit for bit, and against each other; all scratch of the op starts as 0xFF bytes."""
    boxes, scores, counts, thr, max_keep, ref = nms_case(name)
    lv = run_nms(eng, boxes, scores, counts, thr, max_keep, 0)
    pl = run_nms(eng, boxes, scores, counts, thr, max_keep, 1)
    check_nms(name + ' level-wise', lv, ref)
    check_nms(name + ' plain', pl, ref)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(lv, pl))
    print(f'{name}: kept {lv[2].tolist()} of {counts.tolist()}, smallest |IoU - thr| {min_iou_gap(boxes, counts, thr):.3e}')
    if name == 'group_break_and_cut':
        # the case is what it says: group 0 alone has more than max_keep survivors, and the cut falls inside a tie
        rd, rs = ref_nms(boxes, scores, counts, thr, 10 ** 6)[0]
        assert (rs < 200).sum() > max_keep and len(rs) > max_keep and rd[max_keep - 1, 4] == rd[max_keep, 4]


def test_nms_placed_iou_pairs(eng):
    boxes, scores, counts, exp = placed_iou_case()
    want = np.asarray([g * boxes.shape[2] + i for g, i in exp])
    for route in (0, 1):
        dets, src, cnt = run_nms(eng, boxes, scores, counts, 0.7, 16, route)
        assert int(cnt[0]) == len(want) and np.array_equal(src[0, :len(want)].cpu().numpy(), want), route
    check_nms('placed', run_nms(eng, boxes, scores, counts, 0.7, 16, 0), ref_nms(boxes, scores, counts, 0.7, 16))


def test_nms_levels_refusals(eng):
    """What launch_nms_levels / launch_nms refuse reaches the caller as NUHTC_E_INVALID, and the op works afterwards."""
    from nuhtc_amd.engine import HipError
    boxes, scores, counts, thr, max_keep, ref = nms_case('empty_groups')
    with pytest.raises(HipError, match='error -1'):                       # n_groups * max_keep > 8192
        eng.op_nms_levels(dev(boxes), dev(scores), counts, thr, 2049, route=0)
    big_b, big_s = torch.zeros(1, 5, 4096, 4, device='cuda'), torch.zeros(1, 5, 4096, device='cuda')
    for route in (0, 1):                                                  # sorted-list capacity 20736: beyond both routes' limits
        with pytest.raises(HipError, match='error -1'):
            eng.op_nms_levels(big_b, big_s, np.zeros((1, 5), np.int32), thr, 100, route=route)
    with pytest.raises(HipError, match='error -1'):                       # a count beyond the slot
        eng.op_nms_levels(dev(boxes), dev(scores), counts + 200, thr, max_keep)
    check_nms('after refusals', run_nms(eng, boxes, scores, counts, thr, max_keep, 0), ref)


# ================================================================================================================ chain and engine identity
def test_chain_vs_oracle_rpn_proposals(eng):
    """op_rpn_select then op_nms_levels on grid-logit maps against oracle.model.rpn_proposals: count and order exact, boxes within the bound."""
    c, maps, ref = chain_case()
    want = oracle_proposals(maps, c)
    cb, cs, cc = run_select(eng, maps, c['k'], c['img'], c['min_size'])
    dets, src, cnt = eng.op_nms_levels(cb, cs, cc, c['iou'], c['max_keep'])
    for b in range(c['B']):
        n = int(cnt[b])
        assert n == len(want[b]) and n > 10, (b, n, len(want[b]))
        s = src[b, :n].cpu().numpy() - b * 4 * c['k']
        bound = chain_row_bounds(ref[b], s, c['k'])
        got = dets[b, :n].cpu().numpy().astype(np.float64)
        assert (np.abs(got[:, :4] - want[b][:, :4]) <= bound).all(), b
        assert (np.abs(got[:, 4] - want[b][:, 4]) <= 2 * SCORE_C * U * got[:, 4]).all(), b      # two float32 sigmoids
    print(f'chain: proposals {cnt.tolist()} of candidates {cc.tolist()}')


def test_ops_are_the_engines_rpn_path(hip_device):
    """One engine on two synthetic tiles with the token dump on: its rpn0..3 maps through op_rpn_select and op_nms_levels give the engine's
    rpn_cand_boxes / rpn_cand_scores / rpn_cand_count and rpn_props / rpn_counts bit for bit; op_build_rois on its proposals gives its rois."""
    from nuhtc_amd import synth, weights
    from nuhtc_amd.engine import Engine
    B = 2
    e = Engine(weights.bench_state_dict(3), device=0, max_batch=B, tile=(256, 256))
    e.enable_token_dump()
    e.infer_async(e.to_device(synth.nuclei_tiles(B, 256, start=3)))
    e.check()
    cfg = e.cfg
    sf = float(cfg.scale_factor)
    img = (int(256 * sf + 0.5), int(256 * sf + 0.5))
    k, K = cfg.rpn_nms_pre, cfg.rpn_max_per_img
    cb, cs, cc = e.op_rpn_select([e.buffer(f'rpn{l}')[:B] for l in range(4)], k, img, float(cfg.rpn_min_bbox_size), cand_boxes=sentinel(B, 4, k, 4),
                                 cand_scores=sentinel(B, 4, k), cand_count=sentinel(B, 4, dtype=torch.int32))
    ecc = e.buffer('rpn_cand_count')[:B]
    assert torch.equal(cc, ecc) and int(cc.sum()) > 0
    eb, es = e.buffer('rpn_cand_boxes'), e.buffer('rpn_cand_scores')
    for b in range(B):
        for l in range(4):
            n = int(cc[b, l])
            assert torch.equal(_bits(cb[b, l, :n]), _bits(eb[b, l, :n])) and torch.equal(_bits(cs[b, l, :n]), _bits(es[b, l, :n])), (b, l)
    ecnt, eprops = e.buffer('rpn_counts')[:B], e.buffer('rpn_props')
    for route in (0, 1):
        dets, src, cnt = e.op_nms_levels(cb, cs, cc, float(cfg.rpn_nms_iou), K, route=route)
        assert torch.equal(cnt, ecnt) and int(cnt.sum()) > 0
        for b in range(B):
            assert torch.equal(_bits(dets[b, :int(cnt[b])]), _bits(eprops[b, :int(cnt[b])])), (route, b)
    use_cc = bool(cfg.watershed_proposal) and cfg.max_cc_proposals > 0
    r = e.op_build_rois(eprops[:B], ecnt, cc_boxes=e.buffer('cc_props')[:B] if use_cc else None, cc_counts=e.buffer('cc_counts')[:B] if use_cc else None)
    T = int(e.buffer('roi_total').item())
    assert int(r['total'].item()) == T and T > 0
    assert torch.equal(r['roi_off'], e.buffer('roi_off')[:B]) and torch.equal(r['roi_cnt'], e.buffer('roi_counts')[:B])
    assert torch.equal(_bits(r['rois'][:T]), _bits(e.buffer('rois_stage0')[:T]))
    print(f'engine path: candidates {cc.tolist()}, proposals {ecnt.tolist()}, {T} RoIs')
    e.close()


# ================================================================================================================ build_rois
def build_rois_inputs():
    rng = np.random.default_rng(11)
    cc = rng.uniform(0, 100, (3, 5, 4)).astype(np.float32)
    rp = rng.uniform(0, 100, (3, 7, 5)).astype(np.float32)
    return cc, np.asarray([2, 0, 5], np.int32), rp, np.asarray([3, 7, 0], np.int32)


def ref_build_rois(cc, ncc, rp, nrp):
    rows, off, cnt = [], [], []
    for b in range(len(nrp)):
        off.append(len(rows))
        if cc is not None:
            rows += [[b, *cc[b, j]] for j in range(ncc[b])]
        rows += [[b, *rp[b, j, :4]] for j in range(nrp[b])]
        cnt.append(len(rows) - off[-1])
    return np.asarray(rows, np.float32).reshape(-1, 5), off, cnt


@pytest.mark.parametrize('mode', ['cc+rpn', 'rpn only', 'no rows', 'fixed'])
def test_build_rois(eng, mode):
    """cc rows first, then the RPN rows, per image; zero counts on either side; cc disabled; fixed lists; offsets and total for B = 3; the image
    index in column 0; rows behind total untouched.  All exact."""
    cc, ncc, rp, nrp = build_rois_inputs()
    rois = sentinel(40, 5)
    if mode == 'fixed':
        fx = rp[:, :4, :4].copy()
        r = eng.op_build_rois(fixed=dev(fx), rois=rois)
        want, off, cnt = ref_build_rois(None, None, np.concatenate([fx, fx[..., :1]], 2), [4, 4, 4])
    else:
        if mode == 'no rows':
            ncc, nrp = np.zeros(3, np.int32), np.zeros(3, np.int32)
        use = mode != 'rpn only'
        r = eng.op_build_rois(dev(rp), nrp, cc_boxes=dev(cc) if use else None, cc_counts=ncc if use else None, rois=rois)
        want, off, cnt = ref_build_rois(cc if use else None, ncc, rp, nrp)
    T = len(want)
    assert int(r['total'].item()) == T and r['roi_off'].tolist() == off and r['roi_cnt'].tolist() == cnt
    assert np.array_equal(rois[:T].cpu().numpy().view(np.int32), want.view(np.int32)) and _keeps_sentinel(rois[T:])


def test_build_rois_refuses_overflow(eng):
    from nuhtc_amd.engine import HipError
    cc, ncc, rp, nrp = build_rois_inputs()
    with pytest.raises(HipError, match='error -1'):
        eng.op_build_rois(dev(rp), nrp + 5, rois=sentinel(40, 5))
    with pytest.raises(HipError, match='error -1'):
        eng.op_build_rois(dev(rp), nrp, cc_boxes=dev(cc), cc_counts=ncc, rois=sentinel(16, 5))      # 17 rows


def test_print_observed_maxima():
    """Largest errors seen in this module beside their derived bounds (run with -s)."""
    for key, v in sorted(OBSERVED.items()):
        print(f'max {v:.3f}  {key}')
