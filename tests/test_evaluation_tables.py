"""The table-driven twins of nuhtc_amd.evaluation (stat_calc_tables, multi_stat_calc_tables, update_confusion_matrix_tables,
pannuke_stats_tables, gt_rows) against the mask-based functions and the golden vectors of the reference's own metric code.
The tables are built here with plain numpy popcounts, independently of evaluation.pair_tables / joint_tables (which are checked too).
Tolerance: counts and pairings exact; floats 1e-12 relative, the bound tests/test_evaluation.py uses (float64 sums of at most a few
hundred ratios in [0, 1], in a possibly different order)."""
import os
import sys

import numpy as np
import pytest

from nuhtc_amd import evaluation as E

G = os.path.join(os.path.dirname(__file__), 'golden')
sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'tools'))


@pytest.fixture(scope='module')
def ml():
    return np.load(os.path.join(G, 'eval_masklist.npz'))


@pytest.fixture(scope='module')
def pk():
    return np.load(os.path.join(G, 'eval_pannuke.npz'))


def popcount_tables(t, p):
    """inter (n_t, n_p), area_t, area_p by bit counting on packed rows."""
    flat = lambda m: np.asarray(m).reshape(len(m), int(np.prod(np.shape(m)[1:]))).astype(bool)
    tb, pb = np.packbits(flat(t), axis=1), np.packbits(flat(p), axis=1)
    pop = np.array([bin(i).count('1') for i in range(256)])
    inter = pop[tb[:, None, :] & pb[None, :, :]].sum(-1) if len(t) and len(p) else np.zeros((len(t), len(p)), int)
    return inter, pop[tb].sum(-1) if len(t) else np.zeros(0, int), pop[pb].sum(-1) if len(p) else np.zeros(0, int)


def same_stats(a, b):
    if a is None or b is None:
        assert a is None and b is None
        return
    assert a.keys() == b.keys()
    for k in a:
        if k in ('tp', 'fp', 'fn'):
            assert a[k] == b[k], k
        else:
            assert a[k] == pytest.approx(b[k], rel=1e-12, nan_ok=True), k


def test_stat_calc_tables_match_masks_and_fixture(ml):
    for i in range(int(ml['n_img'])):
        t, p = ml[f'true{i}'], ml[f'pred{i}']
        inter, at, ap = popcount_tables(t, p)
        assert np.array_equal(inter, ml[f'inter{i}']) and np.array_equal(at[:, None] + ap[None, :] - inter, ml[f'union{i}'])
        s = E.stat_calc_tables(inter, at, ap)
        same_stats(s, E.stat_calc(t, p))
        assert s['aji'] == pytest.approx(float(ml[f'aji{i}']), rel=1e-12)
        assert s['aji_plus'] == pytest.approx(float(ml[f'aji_plus{i}']), rel=1e-12)
        assert [s['dq'], s['sq'], s['pq']] == pytest.approx(list(ml[f'pq{i}']), rel=1e-12)
        assert [s['tp'], s['fp'], s['fn']] == list(ml[f'pq_counts{i}'])
        assert s['dice'] == pytest.approx(float(ml[f'dice{i}']), rel=1e-12)
        same_stats(E.stat_calc_tables(inter, at, ap, match_iou=0.6), E.stat_calc(t, p, match_iou=0.6))


def test_empty_sides():
    m = np.zeros((2, 8, 8), np.uint8)
    m[0, :3, :3] = 1
    m[1, 5:, 5:] = 1
    none = np.zeros((0, 8, 8), np.uint8)
    for t, p in ((none, none), (none, m), (m, none), (m, m)):
        inter, at, ap = popcount_tables(t, p)
        same_stats(E.stat_calc_tables(inter, at, ap), E.stat_calc(t, p))
        tl, pl = np.arange(len(t)) % 2, np.arange(len(p)) % 2
        got = E.multi_stat_calc_tables(inter, at, ap, tl, pl, 3)
        want = E.multi_stat_calc(t, p, tl, pl, 3)
        np.testing.assert_allclose(np.array(got, float), np.array(want, float), rtol=1e-12, equal_nan=True)
        assert np.isnan(got[2][0])                 # class 2 is absent on both sides: a NaN row
        cm = E.update_confusion_matrix_tables(np.zeros((4, 4)), inter, at, ap, tl, pl)
        assert np.array_equal(cm, E.update_confusion_matrix(np.zeros((4, 4)), t, p, tl, pl))
    assert E.stat_calc_tables(np.zeros((0, 0)), [], []) is None
    assert E.stat_calc_tables(np.zeros((0, 2)), [], [9, 9])['fp'] == 2 and E.stat_calc_tables(np.zeros((2, 0)), [9, 9], [])['fn'] == 2


def test_multiclass_and_confusion_tables(ml):
    rng = np.random.default_rng(3)
    for i in range(int(ml['n_img'])):
        t, p = ml[f'true{i}'], ml[f'pred{i}']
        tl, pl = rng.integers(0, 3, len(t)), rng.integers(0, 3, len(p))
        inter, at, ap = popcount_tables(t, p)
        got = E.multi_stat_calc_tables(inter, at, ap, tl, pl, 4)
        want = E.multi_stat_calc(t, p, tl, pl, 4)
        for g, w in zip(got, want):
            assert [g[0], g[1], g[2]] == pytest.approx([w[0], w[1], w[2]], nan_ok=True, abs=0)
            assert g[3] == pytest.approx(w[3], rel=1e-12, nan_ok=True)
        for thr in (0.5, 0.3):
            cm = E.update_confusion_matrix_tables(np.zeros((5, 5)), inter, at, ap, tl, pl, thr)
            assert np.array_equal(cm, E.update_confusion_matrix(np.zeros((5, 5)), t, p, tl, pl, thr))


def numpy_joint(t, p):
    """Rows (true id, pred id, pixels) of the joint histogram of two label maps, (0, 0) included."""
    t, p = t.ravel().astype(np.int64), p.ravel().astype(np.int64)
    rows = {}
    for a, b in zip(t.tolist(), p.tolist()):
        rows[(a, b)] = rows.get((a, b), 0) + 1
    k = sorted(rows)
    return np.array([a for a, _ in k]), np.array([b for _, b in k]), np.array([rows[x] for x in k])


def test_pannuke_stats_tables(pk):
    true, pred, types = pk['true'], pk['pred'], list(pk['types'])
    tables = []
    for i in range(len(true)):
        tab = [numpy_joint(true[i, :, :, c], pred[i, :, :, c]) for c in range(5)]
        tab.append(numpy_joint(E.binarize(true[i, :, :, :5]), E.binarize(pred[i, :, :, :5])))
        tables.append(tab)
        for c in range(5):
            want = pk['mpq_all'][i, c]
            assert E.pq_from_joint(*tab[c]) == pytest.approx(want, rel=1e-12, nan_ok=True)
        assert E.pq_from_joint(*tab[5]) == pytest.approx(pk['bpq_all'][i, 0], rel=1e-12, nan_ok=True)
    for tabs in (tables, [E.joint_tables(true[i], pred[i], 5) for i in range(len(true))]):
        res = E.pannuke_stats_tables(tabs, types, num_classes=5)
        ref = E.pannuke_stats(true, pred, types, num_classes=5)
        np.testing.assert_allclose(res['class_pq'], pk['class_pq'], rtol=1e-12, equal_nan=True)
        np.testing.assert_allclose(res['class_pq'], ref['class_pq'], rtol=1e-12, equal_nan=True)
        for n, m, b in zip(pk['tissue_names'], pk['tissue_mpq'], pk['tissue_bpq']):
            np.testing.assert_allclose(res['tissue_mpq'][str(n)], m, rtol=1e-12, equal_nan=True)
            np.testing.assert_allclose(res['tissue_bpq'][str(n)], b, rtol=1e-12, equal_nan=True)
        for k in ('mPQ', 'bPQ'):
            np.testing.assert_allclose(res[k], ref[k], rtol=1e-12, equal_nan=True)
        assert np.isnan(res['class_pq']).tolist() == np.isnan(pk['class_pq']).tolist()


def test_joint_tables_keep_the_binarised_partition(pk):
    true, pred = pk['true'], pk['pred']
    for i in range(len(true)):
        t, p, n = E.joint_tables(true[i], pred[i], 5)[5]
        tb, pb = E.binarize(true[i, :, :, :5]), E.remap_label(E.binarize(pred[i, :, :, :5]))
        rt, rp, rn = numpy_joint(tb, pb)
        # same partition, ids in the same order: ranking the ids gives binarize's contiguous numbers
        assert np.array_equal(np.searchsorted(np.unique(t), t), rt) and np.array_equal(np.searchsorted(np.unique(p), p), rp)
        assert np.array_equal(n, rn)


def test_gt_rows_matches_gt_instances(pk):
    from test_pannuke import gt_instances
    masks = [pk['true'][i] for i in range(len(pk['true']))]
    masks.append(np.zeros((64, 64, 6), np.int32))                       # no instance at all
    m = np.zeros((64, 64, 6), np.int32)
    m[2:9, 2:9, 0] = 7
    m[5:12, 5:12, 3] = 7                                                  # same id in two channels, overlapping pixels
    m[30:33, 30:33, 0] = 2
    masks.append(m)
    for mask in masks:
        tm, tl = gt_instances(mask, 5)
        maps, labels, n_t = E.gt_rows(mask, 5)
        assert maps.dtype == np.int32 and maps.shape == (64, 64, 5) and n_t == len(tm)
        assert np.array_equal(labels, tl)
        for r in range(n_t):
            assert np.array_equal(maps[:, :, tl[r]] == r + 1, tm[r])
        assert set(np.unique(maps)) <= set(range(n_t + 1))
        # pair tables from the row maps: overlapping GT instances of different channels count in both rows
        pm = np.zeros((2, 64, 64), bool)
        pm[0, 4:10, 4:10] = True
        pm[1, 40:44, 40:44] = True
        inter, at, ap = E.pair_tables(maps, n_t, pm)
        pi, pat, pap = popcount_tables(tm, pm)
        assert np.array_equal(inter, pi) and np.array_equal(at, pat) and np.array_equal(ap, pap)
    assert E.gt_rows(masks[-1])[2] == 3 and E.gt_rows(masks[-1])[1].tolist() == [0, 0, 3]
