"""CPU tests of the per-nucleus embeddings: nuhtc_amd.nucfeat.pool_reference (the float64 restatement the GPU tests compare against) on cases
worked out by hand, and the path of the embedding rows through wsi.pack_records -> gather -> wsi.merge_gathered."""
import numpy as np
import pytest

from nuhtc_amd import nucfeat

STRIDES = (4, 8, 16, 32)


@pytest.fixture(scope='module')
def maps():
    rng = np.random.default_rng(11)
    return [rng.standard_normal((64 // s, 64 // s, 64)) for s in STRIDES]


def _mask(pixels=(), block=None):
    m = np.zeros((64, 64), bool)
    for y, x in pixels:
        m[y, x] = True
    if block is not None:
        y0, y1, x0, x1 = block
        m[y0:y1, x0:x1] = True
    return m


def test_one_pixel_is_its_cell_at_every_level(maps):
    got = nucfeat.pool_reference(maps, STRIDES, _mask([(5, 9)]))
    want = np.concatenate([maps[0][1, 2], maps[1][0, 1], maps[2][0, 0], maps[3][0, 0]])
    assert got.dtype == np.float64 and got.shape == (256,) and np.array_equal(got, want)


def test_a_block_on_one_cell_is_that_cell(maps):
    got = nucfeat.pool_reference(maps, STRIDES, _mask(block=(8, 12, 12, 16)))            # rows 8..11, columns 12..15: level-0 cell (2, 3)
    want = np.concatenate([maps[0][2, 3], maps[1][1, 1], maps[2][0, 0], maps[3][0, 0]])
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)
    w = nucfeat.cell_weights(_mask(block=(8, 12, 12, 16)), 4, (16, 16))
    assert w.sum() == 16 and w[2, 3] == 16


def test_a_block_over_four_cells_weighs_each_once(maps):
    m = _mask(block=(3, 5, 3, 5))                                                         # pixels (3..4, 3..4): cells (0,0) (0,1) (1,0) (1,1)
    w = nucfeat.cell_weights(m, 4, (16, 16))
    assert w[:2, :2].tolist() == [[1, 1], [1, 1]] and w.sum() == 4
    got = nucfeat.pool_reference(maps, STRIDES, m)
    want0 = (maps[0][0, 0] + maps[0][0, 1] + maps[0][1, 0] + maps[0][1, 1]) / 4
    np.testing.assert_allclose(got[:64], want0, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(got[64:], np.concatenate([maps[1][0, 0], maps[2][0, 0], maps[3][0, 0]]), rtol=1e-13, atol=1e-15)


def test_a_full_mask_is_the_mean_of_every_level(maps):
    got = nucfeat.pool_reference(maps, STRIDES, np.ones((64, 64), bool))
    want = np.concatenate([m.mean(axis=(0, 1)) for m in maps])
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)


def test_unequal_weights_and_the_empty_mask(maps):
    m = _mask(block=(0, 4, 2, 6))                                                         # 8 pixels in cell (0, 0), 8 in cell (0, 1)
    m[0, 2] = False                                                                       # 7 and 8
    got = nucfeat.pool_reference(maps, STRIDES, m)
    np.testing.assert_allclose(got[:64], (7 * maps[0][0, 0] + 8 * maps[0][0, 1]) / 15, rtol=1e-13, atol=1e-15)
    assert not nucfeat.pool_reference(maps, STRIDES, np.zeros((64, 64), bool)).any()
    assert not nucfeat.pool_bound(maps, STRIDES, np.zeros((64, 64), bool)).any()
    b = nucfeat.pool_bound(maps, STRIDES, m)
    np.testing.assert_allclose(b[:64], (2 + 3) * 2.0 ** -24 * (7 * np.abs(maps[0][0, 0]) + 8 * np.abs(maps[0][0, 1])) / 15, rtol=1e-13)
    np.testing.assert_allclose(b[192:], (1 + 3) * 2.0 ** -24 * np.abs(maps[3][0, 0]), rtol=1e-13)


def test_mask_words_round_trip_and_padding_bits():
    rng = np.random.default_rng(3)
    m = rng.random((2, 3, 48, 80)) < 0.4
    w = nucfeat.pack_mask_words(m)
    assert w.shape == (2, 3, 48, 3) and w.dtype == np.int32
    assert np.array_equal(nucfeat.unpack_mask_words(w, 80), m)
    assert not nucfeat.unpack_mask_words(w)[..., 80:].any()
    assert w.view(np.uint32)[0, 0, 0, 1] == sum(1 << (x - 32) for x in range(32, 64) if m[0, 0, 0, x])


def _host_merge(boxes, scores, areas, bits, off, overlap_threshold=0.05, device=0, overlap='polygon'):
    """Stand-in for wsi.merge_overlap_packed (nuhtc_merge_overlap needs a GPU): greedy suppression by mask IoU in descending score."""
    from nuhtc_amd import wsi
    pm = wsi.PackedMasks(np.asarray(boxes, np.int32), np.asarray(areas, np.int32), np.asarray(bits, np.uint32), np.asarray(off, np.int64))
    canvas = []
    for crop, x0, y0 in pm:
        c = np.zeros((200, 200), bool)
        c[y0:y0 + crop.shape[0], x0:x0 + crop.shape[1]] = crop
        canvas.append(c)
    alive = np.ones(len(canvas), bool)
    for i in np.argsort(-np.asarray(scores), kind='stable'):
        if not alive[i]:
            continue
        for j in range(len(canvas)):
            if j != i and alive[j] and scores[j] <= scores[i]:
                inter = (canvas[i] & canvas[j]).sum()
                if inter / max((canvas[i] | canvas[j]).sum(), 1) > overlap_threshold:
                    alive[j] = False
    return np.flatnonzero(alive).astype(np.int64)


def test_embedding_rows_follow_their_records_through_pack_and_merge(monkeypatch):
    """Two ranks' records, every embedding row filled with the record's own number: after pack_records (with a `keep` that drops a
    record), the gather and merge_gathered, the surviving rows are exactly the survivors' numbers."""
    from nuhtc_amd import wsi
    sq = lambda n: np.ones((n, n), bool)
    ring = lambda x, y, n: np.array([[x, y], [x + n - 1, y], [x + n - 1, y + n - 1], [x, y + n - 1], [x, y]], np.int64)

    def records(items, first):
        rec = dict(tile=[], box=[], score=[], label=[], mask=[], ring=[], feat=[])
        for k, (x, y, n, score) in enumerate(items):
            rec['tile'].append(k); rec['box'].append(np.array([x, y, x + n, y + n], np.float64)); rec['score'].append(score); rec['label'].append(k % 3)
            rec['mask'].append((sq(n), x, y)); rec['ring'].append(ring(x, y, n))
            rec['feat'].append(np.full(256, first + k, np.float32))
        return rec
    # rank 0: records 0..2 (record 1 is dropped by `keep`); rank 1: records 10..12; 10 duplicates 0 with a lower score, 2 duplicates 12
    r0 = records([(10, 10, 12, 0.9), (60, 60, 8, 0.95), (100, 20, 10, 0.5)], 0)
    r1 = records([(11, 11, 12, 0.8), (150, 150, 9, 0.7), (101, 21, 10, 0.6)], 10)
    p0, p1 = wsi.pack_records(r0, [0, 2]), wsi.pack_records(r1)
    assert len(p0) == 6 and tuple(p0[5].shape) == (2, 256) and p0[5].dtype.is_floating_point and tuple(p1[5].shape) == (3, 256)
    assert p0[5][:, 0].tolist() == [0, 2]
    no_feat = dict(r0)
    del no_feat['feat']
    assert len(wsi.pack_records(no_feat, [0, 2])) == 5                                   # records without embeddings: the five parts as before
    for a, b in zip(wsi.pack_records(no_feat, [0, 2]), p0):
        assert a.shape == b.shape and bool((a == b).all())
    gathered = [p0, p1]
    every = wsi.gathered_features(gathered)
    assert every[:, 0].tolist() == [0, 2, 10, 11, 12] and (every == every[:, :1]).all()
    monkeypatch.setattr(wsi, 'merge_overlap_packed', _host_merge)
    kept = wsi.merge_gathered(gathered, 0.05)
    assert kept.tolist() == [0, 3, 4]                                                     # 0 beats 10, 12 beats 2, 11 stands alone
    rows = wsi.gathered_features(gathered, kept)
    assert rows.shape == (3, 256) and rows[:, 0].tolist() == [0, 11, 12] and (rows == rows[:, :1]).all()


def test_npz_table_round_trip(tmp_path):
    f = np.arange(3 * 256, dtype=np.float32).reshape(3, 256)
    p = nucfeat.write_npz(str(tmp_path / 's_nuclei_feat.npz'), [0, 2, 5], f, [1, 0, 4], [0.9, 0.8, 0.7])
    z = nucfeat.read_npz(p)
    assert z['nuclei_id'].dtype == np.int64 and z['nuclei_id'].tolist() == [0, 2, 5] and z['features'].dtype == np.float32
    assert np.array_equal(z['features'], f) and z['label'].tolist() == [1, 0, 4] and z['score'].tolist() == [0.9, 0.8, 0.7]
    with pytest.raises(ValueError):
        nucfeat.write_npz(str(tmp_path / 'bad.npz'), [0, 1], f, [1, 0, 4], [0.9, 0.8, 0.7])


def test_the_flag_is_listed_with_the_tools_own(tmp_path):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('tool_infer_wsi_nf', os.path.join(root, 'tools', 'infer_wsi.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(['src', 'cfg', 'ck', '--save_dir', 'o'])
    assert a.nuclei_feat is False
    assert tool.parse_args(['src', 'cfg', 'ck', '--save_dir', 'o', '--nuclei-feat']).nuclei_feat is True
    src = open(os.path.join(root, 'tools', 'infer_wsi.py')).read()
    assert src.index('# ---- not in the reference') < src.index("'--nuclei-feat'")
