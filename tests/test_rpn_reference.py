"""Host-only checks of what tests/test_hip_rpn.py compares the RPN kernels with: its float64 selection reference against
oracle.model.rpn_proposals, the properties its designed inputs claim, and the placed IoU pairs in float32."""
import numpy as np

import test_hip_rpn as R
from test_hip_dettail import U


def test_selection_reference_and_batched_nms_vs_oracle():
    """On random grid-logit maps the float64 selection followed by ops_np.batched_nms gives oracle.model.rpn_proposals: the same count and
    order, boxes within the bound, scores within 4 u; no pair of one level is so close to the IoU threshold that the two sides' boxes could
    decide it differently (chain_pairs_clear)."""
    c, maps, ref = R.chain_case()
    want = R.oracle_proposals(maps, c)
    for b in range(c['B']):
        boxes, scores, counts = R.chain_candidates(ref[b], c['k'])
        assert not any(r['band'].any() for r in ref[b]) and all(R.rows_identify_anchors(r) for r in ref[b])
        assert R.chain_pairs_clear(ref[b], c['iou']) > 0
        dets, src = R.ref_nms(boxes, scores, counts, c['iou'], c['max_keep'])[0]
        assert len(dets) == len(want[b]) > 10
        bound = R.chain_row_bounds(ref[b], src, c['k'])
        assert (np.abs(dets[:, :4].astype(np.float64) - want[b][:, :4]) <= bound + U * np.abs(want[b][:, :4])).all()      # + the float32 image of the reference
        assert (np.abs(dets[:, 4].astype(np.float64) - want[b][:, 4]) <= (R.SCORE_C + 1) * U * dets[:, 4]).all()


def test_designed_selection_inputs():
    """No min-size decision of the designed cases lies inside its band, tied neighbours are told apart by their boxes, and every case
    reaches the kernel paths it is there for."""
    seen = set()
    for name in R.SELECT_CASES:
        c, maps, ref = R.select_case(name)
        for b in range(len(ref)):
            for l in range(4):
                tag = (name, b, l)
                assert int(ref[b][l]['band'].sum()) == 0, tag
                assert R.rows_identify_anchors(ref[b][l]), tag
                n = maps[l].shape[1] * maps[l].shape[2] * 3
                ge = R.keys_ge_T(maps[l][b], c['k'])
                seen.add((n, c['k'], ge, *R.select_branch((n, c['k'], ge))))
    paths = {s[3:] for s in seen}
    assert paths == {('unsorted', None), ('registers', 'usual'), ('registers', 'plateau'), ('scratch', 'usual'), ('scratch', 'plateau')}
    sizes = {(s[0], s[1]) for s in seen}
    assert {(49152, 1000), (129 * 128 * 3, 1000), (300, 300), (300, 299), (297, 300)} <= sizes
    assert {(4800, 3000, 4096), (4800, 3000, 4097)} <= {s[:3] for s in seen}
    c, maps, ref = R.select_case('full_k4096')
    assert int(ref[0][0]['valid'].sum()) == 4096
    c, maps, ref = R.select_case('routes_k1000')                      # a tie across rank k: the first dropped anchor ties with the last kept
    x = maps[2][0][..., :3].reshape(-1)
    order = np.argsort(-x, kind='stable')
    assert x[order[c['k'] - 1]] == x[order[c['k']]]
    # the placed maps: exact ratio-1 anchors on level 2, nothing in a band at min_size 0
    pm = R.placed_maps()
    a = R.anchors_f32(2, np.asarray([2]), np.asarray([2]), np.asarray([1]))
    assert a.tolist() == [[0.0, 0.0, 64.0, 64.0]]
    for l in range(4):
        r = R.ref_level(pm[l][0], l, 400, R.PLACED_IMG, 0.0)
        assert not r['band'].any() and R.rows_identify_anchors(r), l


def test_placed_iou_pairs_in_float32():
    """[0,0,100,100] against [0,0,100,70] is 0.7f, not above it; the 71-row box is; group 3's offset keeps every step exact."""
    f = np.float32
    boxes, scores, counts, exp = R.placed_iou_case()
    off = f(3) * (boxes[0, :, :4][[0, 3]].max() + f(1))
    assert off == 903.0
    for o in (f(0), off):
        b = boxes[0, 0, :4] + o
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        assert area.tolist() == [10000.0, 7000.0, 10000.0, 7100.0]
        iou70 = f(7000) / (area[0] + area[1] - f(7000))
        iou71 = f(7100) / (area[2] + area[3] - f(7100))
        assert iou70 == f(0.7) and not iou70 > f(0.7) and iou71 > f(0.7)
    ref = R.ref_nms(boxes, scores, counts, 0.7, 16)[0][1]
    assert ref.tolist() == [g * boxes.shape[2] + i for g, i in exp]


def test_nms_cases_are_what_they_say():
    for name in R.NMS_CASES:
        boxes, scores, counts, thr, max_keep, ref = R.nms_case(name)
        assert len(ref) == len(counts)
    boxes, scores, counts, thr, max_keep, ref = R.nms_case('group_break_and_cut')
    rd, rs = R.ref_nms(boxes, scores, counts, thr, 10 ** 6)[0]
    assert (rs < 200).sum() > max_keep and rd[max_keep - 1, 4] == rd[max_keep, 4]
    boxes, scores, counts, thr, max_keep, ref = R.nms_case('clusters')
    assert len(R.ref_nms(boxes, scores, counts, thr, 10 ** 6)[0][1]) < counts.sum() // 4          # most rows are suppressed
