"""The cross-tile merge kernels (csrc/merge.hip: nuhtc_merge_overlap) pair by pair against exact overlap ratios, on the designed
crops of tests/merge_cases.py: a sweep of the threshold over every reference value pins the device's double `inter / uni` of
every pair bit for bit (no tolerance anywhere); then how far one round launch propagates along a chain, translation of the
grid origin, a crop at the LDS bound of merge_prepare_kernel, and ties."""
import time

import numpy as np
import pytest

import merge_cases as MC

pytestmark = pytest.mark.gpu
MODES = ('polygon', 'mask')
N_CHAIN = 20000


@pytest.fixture(scope='module')
def packed(hip_device):
    """The placed set, packed once: (boxes, scores, areas, bits, off)."""
    from nuhtc_amd import wsi
    masks, scores = MC.placed()
    boxes, areas, bits, off = wsi.pack_masks(masks)
    return boxes, np.asarray(scores, np.float32), areas, bits, off


def run(packed, thr, mode, shift=(0, 0)):
    """-> bool [detections]: kept by the device."""
    from nuhtc_amd import wsi
    boxes, scores, areas, bits, off = packed
    keep = np.zeros(len(scores), bool)
    keep[wsi.merge_overlap_packed(boxes + np.array(shift * 2, np.int32), scores, areas, bits, off, thr, overlap=mode)] = True
    return keep


def expected(r, thr):
    """The higher-scored member of every pair is kept, the lower-scored one exactly when not r > thr."""
    sw = np.array([p[4] for p in MC.pairs()])
    keep = np.ones((len(r), 2), bool)
    keep[np.arange(len(r)), np.where(sw, 0, 1)] = ~(r > thr)
    return keep.reshape(-1)


@pytest.mark.parametrize('mode', MODES)
def test_threshold_sweep_pins_every_pair_ratio(packed, mode):
    """For every distinct reference value v: at thr = v exactly the pairs with r > v lose their lower-scored member, and one
    ulp below v those with r == v lose it too -- so the device's double of every pair IS the reference's."""
    _, _, r = MC.reference(mode)
    values = sorted(set(r.tolist()))
    assert values[0] == 0.0 and values[-1] == 1.0
    thrs = [t for v in values for t in ((v, float(np.nextafter(v, -np.inf))) if v > 0 else (v,))]
    t0 = time.time()
    bad = {}
    for thr in thrs:
        diff = np.nonzero(run(packed, thr, mode) != expected(r, thr))[0]
        for d in diff:
            bad.setdefault(int(d) // 2, []).append((thr, 'A' if d % 2 == 0 else 'B'))
    print(f'{mode}: {len(thrs)} calls on {2 * len(r)} detections in {time.time() - t0:.2f} s')
    msg = [f'{MC.describe(k, mode)}; wrong keep bit of member {v[0][1]} at thr {v[0][0]!r} (and {len(v) - 1} more thresholds)'
           for k, v in sorted(bad.items())]
    assert not bad, f'{len(bad)} pairs differ:\n' + '\n'.join(msg[:20])


@pytest.mark.parametrize('mode', MODES)
def test_keep_set_does_not_depend_on_the_grid_origin(packed, mode):
    """Negative coordinates and slide-scale offsets: the same keep set as in place, which is the reference's."""
    _, _, r = MC.reference(mode)
    want = expected(r, 0.05)
    assert 0 < want.sum() - len(r) < len(r)                    # some lower-scored members go, some stay
    for shift in ((0, 0), (-1000, -1000), (180000, 90000)):
        got = run(packed, 0.05, mode, shift)
        diff = np.nonzero(got != want)[0]
        assert len(diff) == 0, (shift, [MC.describe(int(d) // 2, mode) for d in diff[:10]])


@pytest.fixture(scope='module')
def chain():
    """20000 solid 8 x 8 crops on one row at a 4-px pitch: neighbours overlap (IoU 1/3 as pixel sets, 21/77 as polygons),
    second neighbours share a box edge at most.  -> (boxes, areas, bits, off), packed as wsi.pack_masks does."""
    n = N_CHAIN
    x = 4 * np.arange(n, dtype=np.int32)
    boxes = np.stack([x, np.zeros(n, np.int32), x + 8, np.full(n, 8, np.int32)], 1)
    return boxes, np.full(n, 64, np.int32), np.full(8 * n, 0xff, np.uint32), 8 * np.arange(n, dtype=np.int64)


def chain_ranks(order):
    n = N_CHAIN
    if order == 'descending':              # the higher-priority neighbour has the lower index
        return np.arange(n)
    if order == 'ascending':               # ... the higher index: the same wave or a later block of merge_round_kernel
        return n - 1 - np.arange(n)
    return np.random.default_rng(3).permutation(n)


@pytest.fixture(scope='module')
def chain_random_expectation():
    from oracle.merge import merge_overlap
    crop = np.ones((8, 8), bool)
    rank = chain_ranks('random')
    keep = np.zeros(N_CHAIN, bool)
    keep[merge_overlap(dict(score=(1.0 - rank / 32768.0).tolist(), mask=[(crop, 4 * i, 0) for i in range(N_CHAIN)]), 0.05)] = True
    return keep


@pytest.mark.parametrize('order', ('descending', 'ascending', 'random'))
def test_long_chain_is_decided_to_the_end(hip_device, chain, chain_random_expectation, order):
    """Along a chain the decision of one detection waits for that of its neighbour, 20000 levels deep when the priorities are
    monotonic, in either index order (the lanes of a wave read before any of them writes: one level per launch).  Every detection is
    decided whatever the number of round launches that takes; the kept ones are ranks 0, 2, 4, ...  (A cap of 16384 launches used
    to end the rounds there and drop the 1807 kept detections beyond level 16385 without an error.)"""
    from nuhtc_amd import wsi
    boxes, areas, bits, off = chain
    rank = chain_ranks(order)
    scores = (1.0 - rank / 32768.0).astype(np.float32)          # exact in float32: every score is different
    assert len(np.unique(scores)) == N_CHAIN
    want = chain_random_expectation if order == 'random' else rank % 2 == 0
    if order == 'random':
        assert want[rank == 0].all() and 0.4 * N_CHAIN < want.sum() < 0.5 * N_CHAIN
    for mode in MODES:
        t0 = time.time()
        keep = np.zeros(N_CHAIN, bool)
        keep[wsi.merge_overlap_packed(boxes, scores, areas, bits, off, 0.05, overlap=mode)] = True
        print(f'{order} {mode}: {time.time() - t0:.2f} s')
        diff = np.nonzero(keep != want)[0]
        assert len(diff) == 0, (order, mode, len(diff), 'first at index', int(diff[0]), 'rank', int(rank[diff[0]]), 'kept', int(keep.sum()), 'of', int(want.sum()))


def test_crop_at_the_lds_bound(hip_device):
    """195 x 960 is 5850 words, the largest h x wpr whose seven bit images fit the 160 KB of merge_prepare_kernel; the copy is
    shifted down by 97 rows: IoU 97 / 291 as polygons.  One row more is refused."""
    from nuhtc_amd import wsi
    from oracle.merge_poly import merge_overlap_masks
    m = np.ones((195, 960), bool)
    masks, scores = [(m, 10, 20), (m, 10, 117)], [0.9, 0.8]
    packed = wsi.pack_masks(masks)
    assert 7 * 4 * 195 * 30 <= 160 * 1024 < 7 * 4 * 196 * 30
    for thr, want in ((0.3, [0]), (0.4, [0, 1])):
        assert merge_overlap_masks(masks, scores, thr).tolist() == want
        assert wsi.merge_overlap_packed(packed[0], scores, *packed[1:], thr, overlap='polygon').tolist() == want, thr
    with pytest.raises(RuntimeError):
        wsi.merge_overlap(dict(score=[0.9], mask=[(np.ones((196, 960), bool), 10, 20)]), 0.3, overlap='polygon')


@pytest.mark.parametrize('mode', MODES)
def test_ties_and_the_strict_comparison_across_words(hip_device, mode):
    """Two identical 9 x 65 crops (three words per row) with equal scores: IoU exactly 1.0, the lower index wins."""
    from nuhtc_amd import wsi
    m = np.ones((9, 65), bool)
    rec = dict(score=[0.5, 0.5], mask=[(m, 70, 40), (m, 70, 40)])
    assert wsi.merge_overlap(rec, 1.0, overlap=mode).tolist() == [0, 1]
    assert wsi.merge_overlap(rec, float(np.nextafter(1.0, 0.0)), overlap=mode).tolist() == [0]
