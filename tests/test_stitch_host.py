"""The crop-based host route of the stitched-tile evaluation (nuhtc_amd/stitch.py) against the pinned mask functions of
nuhtc_amd.evaluation run on full frames: every candidate pasted into a frame of the image, then mask_nms, stat_calc, multi_stat_calc,
update_confusion_matrix and convert_format.  Everything compared is an integer, or a float computed by the same host functions from
identical integer tables: exact equality throughout."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stitch_cases as SC  # noqa: E402
from nuhtc_amd import cocomask  # noqa: E402
from nuhtc_amd import evaluation as E  # noqa: E402
from nuhtc_amd import stitch as S  # noqa: E402


@pytest.fixture(scope='module')
def case():
    tiles, gt = SC.designed()
    c = tiles.candidates()
    return tiles, gt, c, SC.full_frame_reference(c, gt), S.score_image_host(c, gt, SC.H, SC.W, SC.THR, want_maps=True)


def same_stats(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], k


def test_grid_is_the_references():
    g = S.tile_grid(1000, 1000)
    assert len(g) == 81 and g[80]['ox'] == g[80]['oy'] == 744 and g[9]['first_col'] and g[8]['last_col'] and g[8]['first_row'] and g[72]['last_row']
    assert [t['loc'] for t in g] == list(range(81)) and (g[10]['ox'], g[10]['oy']) == (93, 93)
    assert len(SC.GRID) == 12 and (SC.GRID[5]['ox'], SC.GRID[5]['oy']) == (29, 29)
    for bad in [(1000, 1001, 256, 93), (200, 1000, 256, 93), (1000, 1000, 250, 93)]:
        with pytest.raises(ValueError):
            S.tile_grid(*bad)


def test_kept_indices_match_mask_nms_on_full_frames(case):
    tiles, gt, c, ref, got = case
    assert len(c) > 40 and len(np.unique(c.score)) == len(c)        # distinct scores: numpy's default argsort decides nothing here
    assert 5 < len(ref['kept']) < len(c)
    assert got['kept'].tolist() == ref['kept'].tolist()
    assert got['labels'].tolist() == ref['labels'].tolist()


def test_statistics_and_confusion_matrix_match(case):
    tiles, gt, c, ref, got = case
    gt_map, gt_labels, n_t = gt
    same_stats(E.stat_calc_tables(got['inter'], got['area_t'], got['area_p']), ref['stat'])
    assert ref['stat']['tp'] >= 3 and ref['stat']['fn'] >= 1 and ref['stat']['fp'] >= 1
    multi = E.multi_stat_calc_tables(got['inter'], got['area_t'], got['area_p'], gt_labels, got['labels'], SC.C)
    assert np.array_equal(np.array(multi, dtype=float), np.array(ref['multi'], dtype=float), equal_nan=True)
    cm = E.update_confusion_matrix_tables(np.zeros((SC.C + 1, SC.C + 1)), got['inter'], got['area_t'], got['area_p'], gt_labels, got['labels'])
    assert np.array_equal(cm, ref['cm'])
    fs = S.FoldScores(SC.C)
    fs.add('img', got['inter'], got['area_t'], got['area_p'], gt_labels, got['labels'])
    assert np.array_equal(fs.cm, ref['cm']) and fs.summary()['pq'] == ref['stat']['pq']
    assert fs.summary()['multi_pq+'] == float(E.aggregate_mpq([ref['multi']])['multi_pq+'])


def test_maps_match_convert_format(case):
    tiles, gt, c, ref, got = case
    assert np.array_equal(got['inst_map'], ref['maps'][:, :, 0]) and np.array_equal(got['type_map'], ref['maps'][:, :, 1])
    # the two planes are independent maxima: somewhere a pixel takes its id from one mask and its type from another
    inst, typ = got['inst_map'], got['type_map']
    assert ((inst > 0) & (typ != got['labels'][np.maximum(inst, 1) - 1] + 1)).any()


def test_edge_rule_on_inner_and_outer_tiles():
    inner, first, last = SC.GRID[5], SC.GRID[0], SC.GRID[11]
    T = SC.TILE
    up = np.nextafter(np.float32(T - 4), np.float32(1e9))
    bx = np.array([[3.99, 10, 20, 20, 0.9], [4.0, 10, 20, 20, 0.9], [10, 10, T - 4, 20, 0.9], [10, 10, up, 20, 0.9],
                   [10, 3.99, 20, 20, 0.9], [10, 4.0, 20, 20, 0.9], [10, 10, 20, T - 4, 0.9], [10, 10, 20, up, 0.9]], np.float32)
    assert S.select_tile(bx, inner, T, SC.FG, 4).tolist() == [False, True, True, False, False, True, True, False]
    assert S.select_tile(bx, first, T, SC.FG, 4).tolist() == [True, True, True, False, True, True, True, False]       # first column and row
    assert S.select_tile(bx, last, T, SC.FG, 4).tolist() == [False, True, True, True, False, True, True, True]        # last column and row
    # the float box decides, not the mask: a mask reaching the tile edge under a box that keeps its distance stays
    t = SC.Tiles()
    t.add(5, SC.tile_mask(rects=[(0, 64, 0, 64)]), 0.9, 0, box=(4, 4, 60, 60))
    t.add(5, SC.tile_mask(rects=[(20, 30, 20, 30)]), 0.9, 0, box=(3, 20, 30, 30))
    c = t.candidates()
    assert len(c) == 1 and c.box[0].tolist() == [29, 29, 93, 93]


def test_score_filter_equal_to_threshold_and_nan(case):
    tiles, gt, c, ref, got = case
    bx = tiles.boxes[5, :tiles.counts[5]]
    sel = S.select_tile(bx, SC.GRID[5], SC.TILE, SC.FG, SC.OFFSET)
    fg = np.float32(SC.FG)
    assert sel[bx[:, 4] == fg].all() and (bx[:, 4] == fg).sum() == 1
    assert not sel[np.isnan(bx[:, 4])].any() and np.isnan(bx[:, 4]).sum() == 1
    assert not sel[bx[:, 4] < fg].any() and (bx[:, 4] < fg).sum() == 1


def find(c, score):
    i = np.nonzero(c.score == np.float32(score))[0]
    assert len(i) == 1
    return int(i[0])


def test_nms_threshold_two_and_three_in_a_hundred(case):
    tiles, gt, c, ref, got = case
    a, b, cc, d = (find(c, s) for s in (0.99, 0.98, 0.97, 0.96))
    assert (S.crop_inter(c, a, b), c.area[a] + c.area[b] - 2) == (2, 100) and (S.crop_inter(c, cc, d), c.area[cc] + c.area[d] - 3) == (3, 100)
    kept = set(got['kept'].tolist())
    assert {a, b, cc} <= kept and d not in kept
    # a and b come from different tiles whose offsets differ by 29 pixels: their crops meet at unaligned bit positions
    assert c.box[a][0] % 32 != c.box[b][0] % 32


def test_suppression_chain_and_empty_mask(case):
    tiles, gt, c, ref, got = case
    x, y, z, e = (find(c, s) for s in (0.95, 0.94, 0.93, 0.91))
    kept = got['kept'].tolist()
    assert x in kept and y not in kept and z in kept and S.crop_inter(c, y, z) > 0 and S.crop_inter(c, x, z) == 0
    assert c.area[e] == 0 and c.box[e].tolist() == [0, 0, 0, 0] and e in kept
    q = kept.index(e)
    assert got['inter'][:, q].sum() == 0 and got['area_p'][q] == 0


def test_equal_scores_across_tiles_go_to_the_higher_candidate():
    """Equal scores: descending candidate index, the order of a stable ascending argsort reversed (the convention of the evaluation's
    device mask-NMS, tests/test_hip_eval.py).  Reference: that argsort and the greedy loop of mask_nms on pairwise_inter_union."""
    t = SC.Tiles()
    f = SC.frame_rect(40, 50, 40, 52)
    for loc in (0, 1, 4, 5):          # the same object at the same score from four tiles
        g = SC.GRID[loc]
        t.add(loc, f[g['oy']:g['oy'] + SC.TILE, g['ox']:g['ox'] + SC.TILE], 0.5, loc % SC.C)
    t.add(0, SC.tile_mask(rects=[(5, 9, 5, 9)]), 0.5, 0)
    t.add(5, SC.tile_mask(rects=[(30, 34, 30, 34)]), 0.7, 1)
    c = t.candidates()
    frames = np.stack([c.frame(i, SC.H, SC.W) for i in range(len(c))])
    order = np.argsort(c.score, kind='stable')[::-1]
    inter, union = E.pairwise_inter_union(frames[order], frames[order])
    iou = inter / np.maximum(union, 1.0)
    keep = np.ones(len(c), bool)
    for i in range(len(c)):
        if keep[i]:
            keep[i + 1:] &= ~(iou[i, i + 1:] > SC.THR)
    want = order[keep]
    assert want.tolist() == [5, 4, 1]          # of the four twins (0, 2, 3, 4) the one of the last tile is visited first
    assert S.mask_nms_crops(c, SC.THR).tolist() == want.tolist()


def test_ground_truth_rows_absent_id_and_type_remap(case):
    tiles, gt, c, ref, got = case
    gt_map, labels, n_t = gt
    assert n_t == 9 and labels.tolist() == [0, 1, 2, 2, 3, 3, 3, 0, 1]
    assert S.remap_types([[1], [2], [3], [4], [5], [6], [7]]).tolist() == [0, 1, 2, 2, 3, 3, 3]
    assert got['area_t'][3] == 0 and got['inter'][3].sum() == 0          # id 4 occurs nowhere: a row of area 0 ...
    tm = np.stack([gt_map == i + 1 for i in range(n_t)])
    assert ref['stat']['fn'] == E.stat_calc(np.delete(tm, 3, 0), ref['frames'][ref['kept']])['fn'] + 1      # ... that counts as a false negative
    with pytest.raises(ValueError):
        S.gt_from_mat(gt_map, np.arange(8))


def test_mat_writer_and_loader_round_trip(tmp_path, case):
    sio = pytest.importorskip('scipy.io')
    Image = pytest.importorskip('PIL.Image')
    tiles, gt, c, ref, got = case
    gt_map = gt[0]
    os.makedirs(tmp_path / 'Images')
    os.makedirs(tmp_path / 'Labels')
    rgb = np.random.RandomState(0).randint(0, 255, (SC.H, SC.W, 3)).astype(np.uint8)
    for name in ('b_2', 'a_1'):
        Image.fromarray(rgb).save(tmp_path / 'Images' / f'{name}.png')
        sio.savemat(tmp_path / 'Labels' / f'{name}.mat', {'inst_map': gt_map.astype(float), 'inst_type': np.array([[1, 2, 3, 4, 5, 6, 7, 1, 2]]).T.astype(float)})
    names, images, gts = S.load_fold(str(tmp_path))
    assert names == ['a_1', 'b_2'] and np.array_equal(images['a_1'], rgb)
    assert np.array_equal(gts['b_2'][0], gt_map) and gts['b_2'][1].tolist() == gt[1].tolist() and gts['b_2'][2] == 9
    mat = S.pred_mat(got['inst_map'], got['labels'], got['box'])
    sio.savemat(tmp_path / 'out.mat', mat)
    back = sio.loadmat(tmp_path / 'out.mat')
    n = len(got['kept'])
    assert np.array_equal(back['inst_map'], ref['maps'][:, :, 0])
    assert back['inst_type'].shape == (n, 1) and back['inst_type'][:, 0].tolist() == (ref['labels'] + 1).tolist()
    assert back['inst_uid'].shape == (n, 1) and back['inst_uid'][:, 0].tolist() == list(range(1, n + 1))
    assert back['inst_centroid'].shape == (n, 2)


def test_centroids_are_tobbox_of_the_full_frame_rle(case):
    tiles, gt, c, ref, got = case
    bb = np.array([cocomask.to_bbox(cocomask.encode(ref['frames'][i])) for i in got['kept']])
    want = np.stack([bb[:, 0] + bb[:, 2] / 2, bb[:, 1] + bb[:, 3] / 2], 1)
    assert np.array_equal(S.centroids(got['box']), want)
    # a run that spans two columns: the mask touches the bottom of column x and the top of column x + 1
    h, w = 20, 12
    m = np.zeros((h, w), bool)
    m[h - 1, 4] = m[0, 5] = True
    m[7, 5] = True
    cnd = S.Candidates()
    cnd.add(m, 0, 0, 0.5, 0)
    cnd.freeze()
    x, y, bw, bh = cocomask.to_bbox(cocomask.encode(m))
    assert (y, bh) == (0.0, float(h)) and cnd.box[0].tolist() == [4, 0, 6, h]
    assert S.centroids(cnd.box).tolist() == [[x + bw / 2, y + bh / 2]]
