"""The numpy references of tests/export_cases.py against arrays worked out by hand, and the designed cases against the properties their
names promise: tests/test_hip_export.py compares the export, crop and contour kernels of csrc/contour.hip with these references on these
cases, so an edit that drops an edge from the case set has to fail here, on the CPU."""
import numpy as np

import export_cases as EC

M = EC.MARK
M16, M32, M64 = -0x5A5B, -0x5A5A5A5B, -0x5A5A5A5A5A5A5A5B          # 0xA5 bytes read as int16 / int32 / int64
MU32 = 0xA5A5A5A5


def test_marked_buffers_hold_the_mark_byte_in_every_type():
    assert EC.marked(3, np.int16).tolist() == [M16] * 3 and EC.marked((2, 2), np.int32).tolist() == [[M32] * 2] * 2
    assert EC.marked(1, np.int64).tolist() == [M64] and EC.marked(2, np.uint32).tolist() == [MU32] * 2
    assert EC.marked((0, 4), np.int32).shape == (0, 4)


def test_pack_layout_and_round_trip():
    m = np.zeros((1, 2, 96), bool)
    m[0, 0, [0, 31, 32]] = True
    m[0, 1, [63, 64, 95]] = True
    assert EC.pack(m).tolist() == [[0x80000001, 1, 0, 0, 0x80000000, 0x80000001]]
    for H, W in EC.FRAMES:
        masks = np.stack(list(EC.crop_cases(H, W).values()))
        words = EC.pack(masks)
        assert words.dtype == np.uint32 and words.shape == (len(masks), H * W // 32)
        assert np.array_equal(EC.unpack(words, H, W), masks)
    rng = np.random.default_rng(0)
    w = rng.integers(0, 1 << 32, (5, 65 * 3), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(EC.pack(EC.unpack(w, 65, 96)), w)


# ----------------------------------------------------------------------------- reference_export by hand
def _tiny():
    """B = 2 tiles of K = 3 slots, 2 words per mask, ccap = 2."""
    boxes = np.arange(30, dtype=np.int32).reshape(6, 5) + 100
    boxes[4, 0] = np.int32(-0x80000000)                    # -0.0
    labels = np.array([10, 11, 12, 13, 14, 15], np.int32)
    counts = np.array([2, 3], np.int32)
    keep = np.array([1, 0, 1, 0, 1, 1], np.uint8)          # slot 2 of tile 0 is past counts[0]
    words = np.arange(12, dtype=np.uint32).reshape(6, 2) + 1000
    cn = np.array([2, 2, 2, 2, -1, 1], np.int32)
    xy = (np.arange(24, dtype=np.int16).reshape(6, 2, 2) + 1)
    return boxes, labels, counts, keep, words, cn, xy


def test_reference_export_by_hand():
    boxes, labels, counts, keep, words, cn, xy = _tiny()
    r = EC.reference_export(boxes, labels, counts, keep, words, cn, xy, B=2, K=3, cap=4, ccap=2)
    assert r['n'].tolist() == [3, 0]
    assert r['idx'].tolist() == [0, 4, 5, M64] and r['idx'].dtype == np.int64
    assert r['labels'].tolist() == [10, 14, 15, M32] and r['cn'].tolist() == [2, -1, 1, M32]
    assert r['boxes'].tolist() == [[100, 101, 102, 103, 104], [-0x80000000, 121, 122, 123, 124], [125, 126, 127, 128, 129], [M32] * 5]
    assert r['words'].tolist() == [[1000, 1001], [1008, 1009], [1010, 1011], [MU32] * 2]
    assert r['xy'].tolist() == [[[1, 2], [3, 4]], [[M16] * 2] * 2, [[21, 22], [M16] * 2], [[M16] * 2] * 2]      # cn = -1: no vertex; cn = 1: one
    # float32 input gives the same bit patterns
    rf = EC.reference_export(boxes.view(np.float32), labels, counts, keep, words, cn, xy, B=2, K=3, cap=4, ccap=2)
    assert all(np.array_equal(r[k], rf[k]) for k in r)


def test_reference_export_cap_below_n_and_fewer_tiles():
    boxes, labels, counts, keep, words, cn, xy = _tiny()
    r = EC.reference_export(boxes, labels, counts, keep, words, cn, xy, B=2, K=3, cap=2, ccap=2)
    assert r['n'].tolist() == [3, 0] and r['idx'].tolist() == [0, 4] and r['labels'].tolist() == [10, 14]          # the true count, the first cap rows
    assert r['words'].tolist() == [[1000, 1001], [1008, 1009]]
    r = EC.reference_export(boxes, labels, counts, keep, words, cn, xy, B=1, K=3, cap=2, ccap=2)                # tile 1 is not named
    assert r['n'].tolist() == [1, 0] and r['idx'].tolist() == [0, M64]


def test_reference_export_without_contour_inputs():
    boxes, labels, counts, keep, words, cn, xy = _tiny()
    r = EC.reference_export(boxes, labels, counts, keep, words, None, None, B=2, K=3, cap=3, ccap=2)
    assert r['cn'].tolist() == [0, 0, 0] and (r['xy'] == M16).all()
    r = EC.reference_export(boxes, labels, counts, keep, words, None, xy, B=2, K=3, cap=3, ccap=2)                # no lengths: ccap vertices each
    assert r['cn'].tolist() == [0, 0, 0] and r['xy'].tolist() == [xy[0].tolist(), xy[4].tolist(), xy[5].tolist()]
    cn[0] = 7                                                                                                  # a length past the capacity
    r = EC.reference_export(boxes, labels, counts, keep, words, cn, xy, B=2, K=3, cap=3, ccap=2)
    assert r['cn'].tolist() == [7, -1, 1] and r['xy'][0].tolist() == xy[0].tolist()


# ----------------------------------------------------------------------------- reference_crops by hand
def _frame(*pixels, H=4, W=96):
    m = np.zeros((H, W), bool)
    for y, x in pixels:
        m[y, x] = True
    return m


def test_reference_crops_by_hand():
    masks = np.stack([_frame((2, 70)),                                   # single pixel
                      _frame((1, 31), (1, 32), (2, 32)),                 # x0 = 31, x1 = 33: one word wide across the 31 | 32 seam
                      _frame(),                                          # empty
                      _frame((0, 0), (3, 40))])                          # two words wide
    r = EC.reference_crops(masks, n=4, cap=4, pool_cap=100, pool_len=12)
    assert r['box'].tolist() == [[70, 2, 71, 3], [31, 1, 33, 3], [0, 0, 0, 0], [0, 0, 41, 4]]
    assert r['area'].tolist() == [1, 3, 0, 2] and r['off'].tolist() == [0, 1, 3, 3, 11]
    assert r['pool'].tolist() == [1, 0b11, 0b10, 1, 0, 0, 0, 0, 0, 0, 1 << 8, MU32]
    assert r['written'].tolist() == [True, True, False, True]
    # one word short: the last crop stays out whole, the total is still the need
    r = EC.reference_crops(masks, n=4, cap=4, pool_cap=10, pool_len=12)
    assert r['off'].tolist() == [0, 1, 3, 3, 11] and r['pool'].tolist() == [1, 0b11, 0b10] + [MU32] * 9 and r['written'].tolist() == [True, True, False, False]
    # n below cap: the rows from n on are zero and take no words; n above cap is clamped; n = 0 leaves the pool alone
    r = EC.reference_crops(masks, n=1, cap=4, pool_cap=100, pool_len=3)
    assert r['box'].tolist() == [[70, 2, 71, 3]] + [[0] * 4] * 3 and r['area'].tolist() == [1, 0, 0, 0] and r['off'].tolist() == [0, 1, 1, 1, 1]
    assert r['pool'].tolist() == [1, MU32, MU32]
    r = EC.reference_crops(masks, n=9, cap=2, pool_cap=100, pool_len=4)
    assert r['box'].tolist() == [[70, 2, 71, 3], [31, 1, 33, 3]] and r['off'].tolist() == [0, 1, 3] and r['pool'].tolist() == [1, 3, 2, MU32]
    r = EC.reference_crops(masks, n=0, cap=4, pool_cap=100, pool_len=2)
    assert not r['box'].any() and not r['area'].any() and not r['off'].any() and r['pool'].tolist() == [MU32] * 2


# ----------------------------------------------------------------------------- the edges the device tests rely on
def _geometry(m, W):
    """x0, cw, wpr and the source words the first crop word reads."""
    ys, xs = np.nonzero(m)
    x0, x1 = int(xs.min()), int(xs.max()) + 1
    return x0, (x1 - x0 + 31) // 32, W // 32, x1


def test_crop_cases_hold_the_edges():
    for H, W in EC.FRAMES:
        cases = EC.crop_cases(H, W)
        names = list(cases)
        nonempty = {k: _geometry(m, W) for k, m in cases.items() if m.any()}
        assert [k for k in names if k not in nonempty] == ['empty_first', 'empty', 'empty_last']
        assert any(x0 & 31 == 31 for x0, cw, wpr, x1 in nonempty.values())                                      # sh == 31
        assert any(cw == 1 and (x0 >> 5) != ((x1 - 1) >> 5) for x0, cw, wpr, x1 in nonempty.values())           # one word wide over two source words
        assert any((x0 >> 5) + cw == wpr for x0, cw, wpr, x1 in nonempty.values())                              # the last crop word is the row's last word
        assert any((x0 >> 5) + cw == wpr and x0 & 31 for x0, cw, wpr, x1 in nonempty.values())                  # ... shifted: the guard on word + 1
        i = names.index('empty')
        assert 0 < i < len(names) - 1 and cases[names[i - 1]].any() and cases[names[i + 1]].any()               # empty strictly between non-empty
        for x0, x1 in EC.X_RANGES:
            ys, xs = np.nonzero(cases[f'x{x0}_{x1}'])
            assert (xs.min(), xs.max() + 1) == (x0, x1) and ys.max() - ys.min() >= 5
        for x in (31, 32, 63, 64, 95):
            assert cases[f'pixel_x{x}'].sum() == 1 and cases[f'pixel_x{x}'][:, x].any()
        corners = {(int(np.nonzero(cases[k])[0][0]), int(np.nonzero(cases[k])[1][0])) for k in ('pixel_top_left', 'pixel_top_right', 'pixel_bottom_left', 'pixel_bottom_right')}
        assert all(cases[k].sum() == 1 for k in names if k.startswith('pixel_'))
        assert corners == {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
        assert cases['full_frame'].all() and cases['full_row'].sum() == W and cases['full_column'].sum() == H
        assert cases['last_row'][H - 1].any() and not cases['last_row'][:H - 1].any()
        assert sum(k.startswith('blob_') for k in names) == EC.N_BLOBS >= 12
        ys, xs = np.nonzero(cases['two_blobs'])
        assert (xs.min(), ys.min(), xs.max(), ys.max()) == (2, 3, 92, H - 3) and not cases['two_blobs'][20:30].any()
        # a crop that ends in the last word of the frame's last row, shifted, followed by a mask whose first word is set: reading one
        # word past the row would pick up the next mask's pixels
        for k in ('pixel_bottom_right', 'tail_bottom'):
            x0, cw, wpr, x1 = nonempty[k]
            nxt = cases[names[names.index(k) + 1]]
            assert cases[k][H - 1].any() and x0 & 31 and (x0 >> 5) + cw == wpr and nxt[0, :32 - (x0 & 31)].any()
        assert len(names) % 5 != 0          # detection_set(masks='designed') walks the cases in steps of 5
        assert len(np.unique(EC.pack(np.stack(list(cases.values()))), axis=0)) == len(names) - 2        # all different but the three empty ones


def test_detection_sets_reach_both_sides_of_1024():
    sizes = {g: v['max_batch'] * v['K'] for g, v in EC.GEOMETRY.items()}
    assert any(s < 1024 for s in sizes.values())
    assert any(s > 1024 and s % 1024 != 0 for s in sizes.values())
    assert sizes == dict(small64=800, big65=1203, big64=1203)
    assert {v['frame'] for v in EC.GEOMETRY.values()} == set(EC.FRAMES)
    for g, v in EC.GEOMETRY.items():
        H, W = v['frame']
        assert (H * W // 32) % 4 == (0 if H == 64 else 3)          # 16-byte copies at 64 rows, dword copies at 65
        per = -(-sizes[g] // 1024)          # rows per thread of the scan kernels
        if sizes[g] > 1024:                 # several rows per thread, a thread with fewer rows than the others, threads that start past the end
            assert per >= 2 and sizes[g] % per != 0 and 1023 * per > sizes[g]
        else:
            assert per == 1
    # on a big engine the set that names fewer tiles is below 1024 rows: both sides at both frames
    for g in ('big65', 'big64'):
        assert EC.detection_set(g, 'past_B')['B'] * 401 < 1024 < EC.detection_set(g, 'all')['B'] * 401


def test_detection_sets_have_the_properties_of_their_names():
    for g, v in EC.GEOMETRY.items():
        K, Bm = v['K'], v['max_batch']
        n = {}
        for p in EC.PATTERNS:
            s = EC.detection_set(g, p)
            kept = EC.kept_slots(s)
            n[p] = len(kept)
            want = EC.reference_export(s['boxes'], s['labels'], s['counts'], s['keep'], s['masks_words'], s['contour_n'], s['contour_xy'], s['B'], K,
                                       cap=len(kept) + 1, ccap=EC.CCAP)
            assert want['n'][0] == len(kept) and np.array_equal(want['idx'][:-1], kept) and want['idx'][-1] == M64, (g, p)
            assert len(np.unique(s['masks_words'], axis=0)) == Bm * K and s['keep'].dtype == np.uint8 and s['counts'].dtype == np.int32
        assert n['none'] == 0 and n['last_only'] == 1 and EC.kept_slots(EC.detection_set(g, 'last_only')).tolist() == [Bm * K - 1]
        s = EC.detection_set(g, 'all')
        assert n['all'] == s['counts'].sum() and 0 < n['all'] < Bm * K
        s = EC.detection_set(g, 'alternating')
        assert (EC.kept_slots(s) % 2 == 1).all() and n['alternating'] > 100
        s = EC.detection_set(g, 'beyond_counts')
        assert s['keep'].all() and (s['counts'] < K).all() and n['beyond_counts'] == s['counts'].sum()
        s = EC.detection_set(g, 'empty_tile_between')
        assert s['counts'][0] > 0 and s['counts'][1] == 0 and s['counts'][2] > 0 and s['keep'][K:2 * K].all()
        assert not ((EC.kept_slots(s) >= K) & (EC.kept_slots(s) < 2 * K)).any() and (EC.kept_slots(s) >= 2 * K).any()
        s = EC.detection_set(g, 'counts_full')
        assert (s['counts'] == K).all() and n['counts_full'] == s['keep'].sum()
        s = EC.detection_set(g, 'past_B')
        assert 0 < s['B'] < Bm and s['keep'][s['B'] * K:].all() and (s['counts'][s['B']:] == K).all() and EC.kept_slots(s).max() < s['B'] * K
        # contour lengths: every designed value among the kept rows; special float values among the boxes
        s = EC.detection_set(g, 'alternating')
        assert set(s['contour_n'][EC.kept_slots(s)].tolist()) >= {EC.CCAP, 1, 0, -1, EC.CCAP + 3} and EC.CCAP > 64
        b = s['boxes'][EC.kept_slots(s)].view(np.uint32)
        for pattern in (0x80000000, 0x7F800000, 0x7FC12345, 0x7F812345):
            assert (b == pattern).any(), hex(pattern)
        d = EC.detection_set(g, 'alternating', masks='designed')
        assert d['masks_words'].shape == s['masks_words'].shape and (d['masks_words'][:-1] != d['masks_words'][1:]).any(1).all()


def test_contour_shapes_at_65_by_96():
    from oracle import contour as OC
    shapes = EC.contour_shapes()
    assert all(m.shape == (65, 96) and m.any() for m in shapes.values()) and sum(k.startswith('fragments_') for k in shapes) == 10
    s = shapes['serpentine']
    full, _ = OC.find_contours_tree(s, simple=False)
    ring, _ = OC.find_contours_tree(s, simple=True)
    assert len(full) == 1 and len(ring) == 1                       # one component, no hole
    border = len({tuple(p) for p in full[0].tolist()})
    assert border == int(s.sum()) > 2048 and len(ring[0]) < 1024, (border, len(ring[0]))
    print('serpentine:', border, 'border pixels,', len(ring[0]), 'vertices')
    # the words a blob occupies: the staged rectangle of the kernel
    wcols = lambda m: sorted(set((np.nonzero(m)[1] >> 5).tolist()))
    assert wcols(shapes['last_word_column_only']) == [2] and wcols(shapes['seam_31_32']) == [0, 1] and wcols(shapes['seam_63_64']) == [1, 2]
    assert shapes['touches_right_and_bottom'][64, 95] and shapes['right_edge_blob_and_bottom_edge_blob'][:, 95].any()
    assert shapes['right_edge_blob_and_bottom_edge_blob'][64].any()
    for name, n_top in (('hole_across_seam', 1), ('island_in_hole', 1), ('island_in_hole_and_later_blob', 2)):
        c, hier = OC.find_contours_tree(shapes[name])
        assert (hier[:, 3] == -1).sum() == n_top and (hier[:, 3] >= 0).any(), name
    c, hier = OC.find_contours_tree(shapes['island_in_hole_and_later_blob'])
    assert c[0][:, 0].min() >= 64                                  # [0][0] is the blob found last, in the last word column
    h = shapes['hole_across_seam']
    assert h[20, 25] and not h[20, 31] and not h[20, 32] and h[20, 40]
    assert sum(len(OC.find_contours_tree(shapes[f'fragments_{k}'])[0]) > 1 for k in range(10)) >= 5          # really fragmented
