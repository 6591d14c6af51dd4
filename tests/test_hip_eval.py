"""The device evaluation path (csrc/eval.hip) against the host functions of nuhtc_amd.evaluation, which tests/test_evaluation.py pins to
the reference's own metric code: op by op on designed inputs (exact integers), then end to end through Engine.eval_async / eval_read and
tools/eval_pannuke.py --eval-on gpu (integers exact, floats 1e-12 relative: the same float64 arithmetic on the same integer tables)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nuhtc_amd import evaluation as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
CFG = os.path.join(ROOT, 'configs/nuhtc/htc_lite_swin_pannuke_infer.py')
sys.path.insert(0, os.path.join(ROOT, 'tools'))
SIZES = [(64, 64), (64, 96)]          # two and three mask words per row
C = 3


@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    return Engine(weights.bench_state_dict(0, obj_bias=0.0), device=0, max_batch=3, tile=(64, 64))


def pack(masks):
    """(..., H, W) bool -> (..., H, W // 32) int32 words, pixel x in bit x & 31 of word x >> 5."""
    b = np.packbits(np.ascontiguousarray(masks).astype(bool), axis=-1, bitorder='little')
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int32)).cuda()


def dev(a, dtype=torch.int32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), bool)
    m[y0:y1, x0:x1] = True
    return m


def select_case(H, W):
    m = np.zeros((12, H, W), bool)
    m[0, 2, 0:10] = True                                    # A1: 10 px, touches column 0
    m[1, 2, 9] = True
    m[1, 3, 9:19] = True                                    # B1: 11 px; inter 1, union 20 with A1: IoU exactly 0.05
    m[2, 6, 26:46] = True                                   # C: 20 px across the word boundary
    m[3, 6, 44:46] = True
    m[3, 7, 27:46] = True                                   # D: 21 px; inter 2, union 39 with C: just over 0.05
    m[4] = rect(H, W, 50, 55, 2, 8)                         # below fg_thr, on top of ...
    m[5] = rect(H, W, 50, 55, 2, 8)                         # ... the one whose score equals fg_thr
    m[6] = rect(H, W, 20, 30, 30, 40)                       # X
    m[7] = rect(H, W, 20, 30, 35, 45)                       # Y: killed by X
    m[8] = rect(H, W, 20, 30, 42, 52)                       # Z: overlaps Y only, survives
    m[9] = rect(H, W, 40, 46, W - 5, W)                     # touches column W - 1
    m[10] = rect(H, W, 58, 64, 30, 36)
    m[11] = rect(H, W, 12, 16, 50, 56)
    fg = np.float32(0.1)
    scores = np.array([0.9, 0.8, 0.7, 0.95, 0.05, fg, 0.6, 0.55, 0.5, 0.3, 0.85, 0.2], np.float32)
    return m, scores, float(fg)


@pytest.mark.parametrize('H,W', SIZES)
def test_select_matches_mask_nms(eng, H, W):
    m, scores, fg = select_case(H, W)
    K = 16
    masks = np.zeros((2, K, H, W), bool)
    masks[0, :12] = m
    masks[1, :12] = m                                       # (tile 1 holds the same words but counts 0 detections)
    sc = np.zeros((2, K), np.float32)
    sc[:, :12] = scores
    labels = np.arange(2 * K).reshape(2, K) % C
    sel, nsel, sl = eng.op_eval_select(dev(sc, torch.float32), [12, 0], pack(masks), fg, 0.05, labels=dev(labels))
    idx = np.nonzero(scores >= np.float32(fg))[0]
    _, order = E.mask_nms(m[idx], scores[idx], thr=0.05)
    want = idx[order]
    assert {0, 1, 3, 5, 6, 8} <= set(want) and not {2, 4, 7} & set(want)          # the designed decisions, as numpy makes them
    nsel, sel = nsel.cpu().numpy(), sel.cpu().numpy()
    assert nsel.tolist() == [len(want), 0]
    assert sel[0, :len(want)].tolist() == want.tolist() and (sel[0, len(want):] == -1).all() and (sel[1] == -1).all()
    assert sl.cpu().numpy()[0, :len(want)].tolist() == labels[0, want].tolist()


def test_select_ties_go_to_descending_slot(eng):
    """Equal scores: numpy's default argsort leaves their order open; the kernel's documented rule is the order of a STABLE ascending
    argsort, reversed -- descending slot.  Reference: that argsort and the greedy loop of mask_nms on pairwise_inter_union."""
    H, W, K = 64, 64, 8
    m = np.stack([rect(H, W, 2, 8, 2 + 9 * j, 8 + 9 * j) for j in range(6)])      # non-overlapping ...
    m[4] = m[1]                                                                      # ... except slot 4, a copy of slot 1 with the same score
    scores = np.array([0.4, 0.7, 0.4, 0.9, 0.7, 0.4], np.float32)
    masks = np.zeros((1, K, H, W), bool)
    masks[0, :6] = m
    sc = np.zeros((1, K), np.float32)
    sc[0, :6] = scores
    sel, nsel, _ = eng.op_eval_select(dev(sc, torch.float32), [6], pack(masks), 0.1, 0.05)
    order = np.argsort(scores, kind='stable')[::-1]
    inter, union = E.pairwise_inter_union(m[order], m[order])
    iou = inter / np.maximum(union, 1.0)
    keep = np.ones(6, bool)
    for i in range(6):
        if keep[i]:
            keep[i + 1:] &= ~(iou[i, i + 1:] > 0.05)
    want = order[keep]
    assert want.tolist() == [3, 4, 5, 2, 0]                 # of the twins 4 and 1, the higher slot is visited first and removes the other
    assert int(nsel[0]) == 5 and sel.cpu().numpy()[0, :5].tolist() == want.tolist()


def pairs_case(H, W):
    gt = np.zeros((H, W, C + 1), np.int32)
    gt[1:7, 28:37, 0] = 3                                   # crosses the word boundary
    gt[10:16, 0:5, 0] = 9                                   # touches column 0
    gt[12:21, 2:9, 1] = 1                                   # overlaps the instance above, in another channel
    gt[40:46, W - 6:W, 2] = 5                               # touches column W - 1
    gt[55:61, 20:26, 2] = 7                                 # no prediction on it
    pm = np.stack([rect(H, W, 2, 9, 30, 41), rect(H, W, 11, 19, 0, 7), rect(H, W, 41, 48, W - 4, W),
                   rect(H, W, 30, 34, 50, 56)])             # the last one: no ground truth under it
    return gt, pm


@pytest.mark.parametrize('H,W', SIZES)
def test_pairs_match_pairwise_inter_union(eng, H, W):
    from test_pannuke import gt_instances
    gt, pm = pairs_case(H, W)
    tm, tl = gt_instances(gt, C)
    maps, labels, n_t = E.gt_rows(gt, C)
    assert n_t == 5 and labels.tolist() == tl.tolist()
    K, slots = 8, [5, 2, 7, 0]
    masks = np.zeros((3, K, H, W), bool)
    masks[:, slots] = pm
    sel = np.full((3, K), -1)
    sel[:, :4] = slots
    gtm = np.stack([maps, np.zeros_like(maps), maps])       # tile 1: n_t = 0; tile 2: n_p = 0
    args = (pack(masks), dev(sel), dev([4, 4, 0]), dev(gtm))
    inter, union = E.pairwise_inter_union(tm, pm)
    nnz = int((inter > 0).sum())
    assert nnz == 4 and (inter[:, 3] == 0).all() and (inter[4] == 0).all() and inter[1, 1] > 0 and inter[2, 1] > 0
    r = eng.op_eval_pairs(*args, t_cap=8, cap=32)
    assert (r['n'], r['overflow'], r['bad']) == (nnz, False, False)
    tr = r['trips'][:nnz].cpu().numpy()
    assert (tr[:, 0] == 0).all()                            # nothing from the tile without ground truth nor the one without predictions
    got = E.dense_pairs(n_t, 4, tr[:, 1], tr[:, 2], tr[:, 3])
    at, ap = r['area_t'].cpu().numpy(), r['area_p'].cpu().numpy()
    assert np.array_equal(got, inter)
    assert np.array_equal(at[0, :n_t][:, None] + ap[0, :4][None, :] - got, union)
    assert at[0, n_t:].sum() == 0 and (at[1] == 0).all() and np.array_equal(at[2], at[0])
    assert np.array_equal(ap[1, :4], ap[0, :4]) and (ap[2] == 0).all() and (ap[:, 4:] == 0).all()
    # one entry short: flagged, counted in full, nothing written behind the capacity
    r = eng.op_eval_pairs(*args, t_cap=8, cap=nnz - 1)
    assert r['overflow'] and r['n'] == nnz and (r['guard'].cpu().numpy() == -7).all()
    want = {(t, p, int(inter[t, p])) for t, p in zip(*np.nonzero(inter))}
    assert {tuple(x[1:]) for x in r['trips'].cpu().numpy().tolist()} <= want
    # a value the row tables cannot hold is reported, not used as an index
    assert eng.op_eval_pairs(*args, t_cap=4, cap=32)['bad']


@pytest.mark.parametrize('H,W', SIZES)
@pytest.mark.parametrize('fmt', ['pannuke', 'conic'])
def test_render_matches_convert_format(eng, H, W, fmt):
    pm = np.stack([rect(H, W, 2, 20, 20, 40), rect(H, W, 10, 30, 30, 50), rect(H, W, 15, 25, 25, 45), rect(H, W, 50, 60, 0, 10),
                   rect(H, W, 28, 36, W - 9, W)])
    labels = np.array([0, 2, 0, 2, 0])                      # class 1 has no instance; overlaps within and across classes
    K, slots = 8, [6, 1, 3, 0, 4]
    masks = np.zeros((2, K, H, W), bool)
    masks[:, slots] = pm
    lab = np.full((2, K), 1)
    lab[:, slots] = labels
    sel = np.full((2, K), -1)
    sel[:, :5] = slots
    out = eng.op_eval_render(pack(masks), dev(sel), dev([5, 0]), dev(lab), C, fmt).cpu().numpy()
    assert np.array_equal(out[0], E.convert_format(pm, labels, H, W, C, fmt))
    assert np.array_equal(out[1], E.convert_format(np.zeros((0, H, W)), [], H, W, C, fmt)) and not out[1].any()


def test_joint_tables_give_pannuke_stats(eng):
    pk = np.load(os.path.join(G, 'eval_pannuke.npz'))
    true, pred, types = pk['true'], pk['pred'], list(pk['types'])
    N = len(true)
    r = eng.op_eval_joint(dev(true), dev(pred), 5, cap=4096)
    assert not r['overflow'] and not r['bad']
    jt = r['joint'][:r['n']].cpu().numpy()
    tables = [[tuple(jt[(jt[:, 0] == i) & (jt[:, 1] == k)][:, j] for j in (2, 3, 4)) for k in range(6)] for i in range(N)]
    for i in range(N):
        for k, (t, p, n) in enumerate(tables[i]):
            assert n.sum() == 64 * 64
            wt, wp, wn = E.joint_tables(true[i], pred[i], 5)[k]
            o = np.lexsort((p, t))
            assert np.array_equal(t[o], wt) and np.array_equal(p[o], wp) and np.array_equal(n[o], wn)
    res, ref = E.pannuke_stats_tables(tables, types, num_classes=5), E.pannuke_stats(true, pred, types, num_classes=5)
    np.testing.assert_allclose(res['class_pq'], pk['class_pq'], rtol=1e-12, equal_nan=True)
    for name, m, b in zip(pk['tissue_names'], pk['tissue_mpq'], pk['tissue_bpq']):
        np.testing.assert_allclose(res['tissue_mpq'][str(name)], m, rtol=1e-12, equal_nan=True)
        np.testing.assert_allclose(res['tissue_bpq'][str(name)], b, rtol=1e-12, equal_nan=True)
    for name in E.PANNUKE_TISSUES:                          # NaN positions included
        np.testing.assert_allclose(res['tissue_mpq'][name], ref['tissue_mpq'][name], rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose([res['mPQ'], res['bPQ']], [ref['mPQ'], ref['bPQ']], rtol=1e-12, equal_nan=True)
    short = eng.op_eval_joint(dev(true), dev(pred), 5, cap=r['n'] - 1)
    assert short['overflow'] and short['n'] == r['n'] and (short['guard'].cpu().numpy() == -7).all()


def host_score(results, gts, nc, H, W, fg_thr=0.1, thr=0.05):
    """The host path of tools/test_pannuke.py on Engine.results."""
    from nuhtc_amd.apis import concat_results
    from test_pannuke import gt_instances
    out = dict(preds=[], stats=[], mpq=[], cm=np.zeros((nc + 1, nc + 1)))
    for res, gt in zip(results, gts):
        boxes, labels, pm = concat_results(res)
        s = boxes[:, 4] >= fg_thr
        boxes, labels, pm = boxes[s], labels[s], (pm[s] if len(pm) else np.zeros((0, H, W), bool))
        if len(pm):
            pm, keep = E.mask_nms(pm, boxes[:, 4], thr=thr)
            labels = labels[keep]
        out['preds'].append(E.convert_format(pm, labels, H, W, nc, 'pannuke'))
        if gt is not None:
            tm, tl = gt_instances(gt, nc)
            out['stats'].append(E.stat_calc(tm, pm))
            out['mpq'].append(E.multi_stat_calc(tm, pm, tl, labels, nc))
            E.update_confusion_matrix(out['cm'], tm, pm, tl, labels)
    return out


@pytest.fixture(scope='module')
def fold(hip_device):
    """Three synthetic nuclei tiles and a ground truth made from the detections of a second seed's weights."""
    from nuhtc_amd import synth, weights
    from nuhtc_amd.engine import Engine
    tiles = synth.nuclei_tiles(3, 64, start=40)
    other = Engine(weights.bench_state_dict(1, obj_bias=0.0), device=0, max_batch=3, tile=(64, 64))
    gts = np.array(host_score(other(tiles, 1), [None] * 3, 5, 64, 64)['preds'])
    other.close()
    assert gts[..., :5].max() > 0
    return tiles, gts


def test_eval_async_matches_the_host_path(eng, fold):
    tiles, gts = fold
    B, nc = len(tiles), 5
    eng.infer_async(eng.to_device(tiles), 1)
    want = host_score(eng.results(B), gts, nc, 64, 64)
    rows = [E.gt_rows(g, nc) for g in gts]
    eng.eval_async(B, dev(np.stack([r[0] for r in rows])), t_cap=max(r[2] for r in rows) + 1)
    eng.check()
    r = eng.eval_read()
    assert not r['overflow'] and r['nsel'].sum() > 0
    cm = np.zeros((nc + 1, nc + 1))
    for k in range(B):
        assert np.array_equal(r['maps'][k], want['preds'][k])
        _, tl, n_t = rows[k]
        inter = E.dense_pairs(n_t, len(r['labels'][k]), *r['pairs'][k])
        at, ap = r['area_t'][k, :n_t], r['area_p'][k]
        got, ref = E.stat_calc_tables(inter, at, ap), want['stats'][k]
        assert (got is None) == (ref is None)
        for key in (ref or {}):
            if key in ('tp', 'fp', 'fn'):
                assert got[key] == ref[key]
            else:
                assert got[key] == pytest.approx(ref[key], rel=1e-12, nan_ok=True)
        np.testing.assert_allclose(np.array(E.multi_stat_calc_tables(inter, at, ap, tl, r['labels'][k], nc), float),
                                   np.array(want['mpq'][k], float), rtol=1e-12, equal_nan=True)
        E.update_confusion_matrix_tables(cm, inter, at, ap, tl, r['labels'][k])
    assert np.array_equal(cm, want['cm'])
    types = ['Breast', 'Colon', 'Breast']
    res = E.pannuke_stats_tables(r['joint'], types, num_classes=nc)
    ref = E.pannuke_stats(gts, np.array(want['preds']), types, num_classes=nc)
    np.testing.assert_allclose(res['class_pq'], ref['class_pq'], rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose([res['mPQ'], res['bPQ']], [ref['mPQ'], ref['bPQ']], rtol=1e-12, equal_nan=True)


def same_outputs(h, g):
    ph, pg = np.load(h / 'preds_pannuke.npy'), np.load(g / 'preds_pannuke.npy')
    assert ph.dtype == pg.dtype and np.array_equal(ph, pg) and ph[..., :5].max() > 0
    assert np.array_equal(np.load(h / 'confusion_matrix.npy'), np.load(g / 'confusion_matrix.npy'))
    sh, sg = json.load(open(h / 'summary.json')), json.load(open(g / 'summary.json'))
    assert sh.keys() == sg.keys() and 'bPQ' in sh and 'aji' in sh
    for k in sh:
        assert sg[k] == pytest.approx(sh[k], rel=1e-12, nan_ok=True), k
    for name in ('class_stats.csv', 'tissue_stats.csv'):
        rh, rg = [list(__import__('csv').reader(open(d / name))) for d in (h, g)]
        assert [x[:2] for x in rh] == [x[:2] for x in rg]
        np.testing.assert_allclose([[float(v) for v in x[2:]] for x in rg[1:]], [[float(v) for v in x[2:]] for x in rh[1:]], rtol=1e-12, equal_nan=True)


def test_tool_writes_the_same_files_on_both_paths(hip_device, fold, tmp_path, capfd):
    """tools/test_pannuke.py (the host path, a process of its own) against tools/eval_pannuke.py --eval-on gpu, once with the default
    capacities -- every batch must come from the device tables -- and once with a joint capacity of one entry, where every batch must
    fall back to its masks and still write the same files."""
    import eval_pannuke
    from nuhtc_amd import weights
    tiles, gts = fold
    np.save(tmp_path / 'images.npy', tiles[..., ::-1])      # (the tool reverses the channels again: the network sees `tiles`)
    np.save(tmp_path / 'masks.npy', gts)
    np.save(tmp_path / 'types.npy', np.array(['Breast', 'Colon', 'Breast']))
    ck = tmp_path / 'w.pth'
    torch.save(dict(state_dict=weights.bench_state_dict(0, obj_bias=0.0)), ck)
    common = lambda out: [CFG, str(ck), '--images', str(tmp_path / 'images.npy'), '--masks', str(tmp_path / 'masks.npy'), '--types',
                          str(tmp_path / 'types.npy'), '--out', str(tmp_path / out), '--batch', '2']
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tools/test_pannuke.py')] + common('host'), stdout=subprocess.DEVNULL)
    capfd.readouterr()
    eval_pannuke.main(common('gpu') + ['--eval-on', 'gpu'])
    assert '2 of 2 batches scored from device tables, 0 through their masks' in capfd.readouterr().err
    same_outputs(tmp_path / 'host', tmp_path / 'gpu')
    eval_pannuke.main(common('fallback') + ['--eval-on', 'gpu', '--joint-cap', '1'])
    assert '0 of 2 batches scored from device tables, 2 through their masks' in capfd.readouterr().err
    same_outputs(tmp_path / 'host', tmp_path / 'fallback')


def test_tool_host_mode_is_the_host_tool(monkeypatch):
    """--eval-on host (and no --eval-on at all) hands the other arguments to tools/test_pannuke.py's main unchanged."""
    import eval_pannuke
    seen = []
    monkeypatch.setattr(eval_pannuke.host_tool, 'main', lambda: seen.append(list(sys.argv[1:])))
    eval_pannuke.main(['cfg', 'ck', '--images', 'x.npy', '--eval-on', 'host', '--batch', '4'])
    eval_pannuke.main(['cfg', 'ck', '--images', 'x.npy'])
    assert seen == [['cfg', 'ck', '--images', 'x.npy', '--batch', '4'], ['cfg', 'ck', '--images', 'x.npy']]
