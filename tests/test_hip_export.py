"""The producers of everything the slide loop takes off the device, op by op on designed inputs (tests/export_cases.py, checked on the CPU
by tests/test_export_cases.py): nuhtc_export_kept (export_scan_kernel, export_copy_kernel), nuhtc_export_crops (crop_bounds_kernel,
crop_scan_kernel, crop_write_kernel) and nuhtc_mask_contours at a frame of three words per row, all in csrc/contour.hip.

Every output buffer holds a mark byte before a call and is one row longer than the call is told, and every comparison is equality of the
whole buffer with the numpy reference: what had to be written is there, and nothing else was touched.  Integer work and bit copies on
both sides: there is no tolerance anywhere."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from nuhtc_amd import hip
import export_cases as EC

pytestmark = pytest.mark.gpu
GUARD = 1                          # rows past `cap` in every output buffer: they must keep the mark
BIG = ('big65', 'big64')
ALL = tuple(EC.GEOMETRY)


@pytest.fixture(scope='module')
def engines(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    sd = weights.bench_state_dict(0, obj_bias=0.0)
    return {g: Engine(sd, device=0, max_batch=v['max_batch'], tile=v['frame'], max_per_img=v['K']) for g, v in EC.GEOMETRY.items()}


def up(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def same(got, want, what):
    """The first len(want) rows are the reference, bit for bit; the guard rows behind them still hold the mark."""
    got = got.view(want.dtype) if got.dtype != want.dtype else got
    assert got.shape[1:] == want.shape[1:] and len(got) >= len(want), what
    diff = np.flatnonzero((got[:len(want)] != want).reshape(len(want), int(np.prod(want.shape[1:]))).any(1))
    assert not len(diff), (what, 'first differing rows', diff[:8].tolist(), 'of', len(want))
    assert (got[len(want):] == EC.marked(1, want.dtype)[0]).all(), (what, 'written past the capacity')


# ----------------------------------------------------------------------------- nuhtc_export_kept
EXPORT_FIELDS = dict(n=((2,), np.int32), idx=((), np.int64), boxes=((5,), np.int32), labels=((), np.int32), cn=((), np.int32),
                     xy=((EC.CCAP, 2), np.int16), words=(None, np.uint32))


def export_outputs(cap, words, dev):
    shapes = {k: ((2 + 2 * GUARD,) if k == 'n' else (cap + GUARD,) + (tail if tail is not None else (words,))) for k, (tail, dt) in EXPORT_FIELDS.items()}
    return {k: up(EC.marked(shapes[k], EXPORT_FIELDS[k][1]), dev) for k in EXPORT_FIELDS}


def run_export(eng, s, cap, contours='both', B=None, null=(), out=None, sync=True):
    """One nuhtc_export_kept call on detection set `s` with marked outputs -> (return code, name -> numpy buffer incl. guard rows, device
    outputs).  contours: 'both', 'xy_only' (NULL contour_n) or 'none'; null: names of pointers passed as NULL."""
    dev = eng.device
    H, W = s['frame']
    t = {k: up(s[k], dev) for k in ('boxes', 'labels', 'counts', 'keep', 'masks_words', 'contour_n', 'contour_xy')}
    dets = hip.Dets(t['boxes'].data_ptr(), t['labels'].data_ptr(), t['counts'].data_ptr(), None if 'masks' in null else t['masks_words'].data_ptr(), None,
                    None if 'keep' in null else t['keep'].data_ptr())
    o = out or export_outputs(max(cap, 1), H * W // 32, dev)
    rc = eng.lib.nuhtc_export_kept(eng.h, ctypes.byref(dets), s['B'] if B is None else B, vp(t['contour_n']) if contours == 'both' else None,
                                   vp(t['contour_xy']) if contours != 'none' else None, EC.CCAP, cap, vp(o['n']), vp(o['idx']), vp(o['boxes']), vp(o['labels']),
                                   vp(o['cn']), None if 'xy_dev' in null else vp(o['xy']), vp(o['words']), eng._stream())
    if not sync:
        return rc, None, (o, t)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}, (o, t)


def want_export(s, cap, contours='both'):
    return EC.reference_export(s['boxes'], s['labels'], s['counts'], s['keep'], s['masks_words'], s['contour_n'] if contours == 'both' else None,
                               s['contour_xy'] if contours != 'none' else None, s['B'], s['K'], cap, EC.CCAP)


def check_export(eng, s, cap, contours='both', what=''):
    rc, got, _ = run_export(eng, s, cap, contours)
    assert rc == 0, (what, eng.lib.nuhtc_last_error(eng.h))
    want = want_export(s, cap, contours)
    for k in EXPORT_FIELDS:
        same(got[k], want[k], (what, cap, contours, k))
    return int(want['n'][0])


@pytest.mark.parametrize('geometry', ALL)
def test_export_kept_keep_patterns(engines, geometry):
    """Every designed keep pattern with room to spare: the rows, their order and nothing else.  On both frames (16-byte and dword mask
    copies) and with B * K on both sides of 1024 (one row per scan thread; two, with a ragged end)."""
    seen = {}
    for pattern in EC.PATTERNS:
        s = EC.detection_set(geometry, pattern)
        seen[pattern] = (check_export(engines[geometry], s, len(EC.kept_slots(s)) + 3, what=(geometry, pattern)), s['B'] * s['K'])
    print(geometry, seen)
    assert seen['none'][0] == 0 and seen['last_only'][0] == 1 and all(v[0] > 1 for k, v in seen.items() if k not in ('none', 'last_only'))
    if geometry in BIG:
        assert seen['past_B'][1] < 1024 < seen['all'][1] and seen['all'][1] % 1024 != 0


@pytest.mark.parametrize('geometry', ALL)
def test_export_kept_capacities(engines, geometry):
    """cap > n, == n, == n - 1 and 1: n[0] is the true count whatever the capacity, the first cap rows are written, the row at `cap` is not."""
    for pattern in ('alternating', 'beyond_counts'):
        s = EC.detection_set(geometry, pattern)
        n = len(EC.kept_slots(s))
        for cap in (n + 5, n, n - 1, 1):
            assert check_export(engines[geometry], s, cap, what=(geometry, pattern)) == n


@pytest.mark.parametrize('geometry', ('small64', 'big65'))
def test_export_kept_contour_inputs(engines, geometry):
    """Contour lengths of ccap, 1, 0, -1 and past ccap among the kept rows (export_cases.CONTOUR_N; checked on the CPU): the row holds
    min(max(cn, 0), ccap) vertices and the mark behind them.  Without lengths every row gets ccap vertices and cn = 0; without both, cn = 0 and
    no vertex is written."""
    s = EC.detection_set(geometry, 'alternating')
    n = len(EC.kept_slots(s))
    for contours in ('both', 'xy_only', 'none'):
        for cap in (n + 2, n - 1):
            check_export(engines[geometry], s, cap, contours, what=geometry)


@pytest.mark.parametrize('geometry', ('small64', 'big65'))
def test_export_kept_twice_is_bitwise_equal(engines, geometry):
    s = EC.detection_set(geometry, 'counts_full')
    cap = len(EC.kept_slots(s)) - 4
    a, b = run_export(engines[geometry], s, cap)[1], run_export(engines[geometry], s, cap)[1]
    assert all(np.array_equal(a[k], b[k]) for k in EXPORT_FIELDS)


def test_export_kept_refusals(engines):
    eng = engines['small64']
    s = EC.detection_set('small64', 'alternating')
    calls = dict(cap_0=dict(cap=0), B_0=dict(cap=8, B=0), B_past_max_batch=dict(cap=8, B=s['max_batch'] + 1), null_keep=dict(cap=8, null=('keep',)),
                 null_masks=dict(cap=8, null=('masks',)), contour_xy_without_xy_dev=dict(cap=8, null=('xy_dev',)))
    for name, kw in calls.items():
        rc, got, _ = run_export(eng, s, **kw)
        assert rc == hip.E_INVALID, (name, rc)
        for k, (tail, dt) in EXPORT_FIELDS.items():
            assert (got[k].view(np.uint8) == EC.MARK).all(), (name, k)
    rc, got, _ = run_export(eng, s, cap=8, contours='none', null=('xy_dev',))          # no contour input: xy_dev is not needed
    assert rc == 0 and got['n'][:2].tolist() == [len(EC.kept_slots(s)), 0]


# ----------------------------------------------------------------------------- nuhtc_export_crops
def run_crops(eng, words, n, cap, pool_cap, pool_len, null=()):
    """One nuhtc_export_crops call on `words` (numpy uint32 (cap, H * W // 32), or a device tensor) with marked outputs -> (return code,
    box, area, off, pool as numpy with guard rows)."""
    dev = eng.device
    w = words if isinstance(words, torch.Tensor) else up(words, dev)
    n_dev = n if isinstance(n, torch.Tensor) else torch.tensor([n, EC.MARK], dtype=torch.int32, device=dev)
    o = dict(box=up(EC.marked((cap + GUARD, 4), np.int32), dev), area=up(EC.marked(cap + GUARD, np.int32), dev), off=up(EC.marked(cap + 1 + GUARD, np.int32), dev),
             pool=up(EC.marked(pool_len, np.uint32), dev))
    arg = lambda k, t: None if k in null else vp(t)
    rc = eng.lib.nuhtc_export_crops(eng.h, arg('words', w), arg('n', n_dev), cap, arg('box', o['box']), arg('area', o['area']), arg('off', o['off']),
                                    arg('pool', o['pool']), pool_cap, eng._stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def check_crops(eng, masks, words, n, cap, pool_cap, pool_len, what):
    rc, got = run_crops(eng, words, n, cap, pool_cap, pool_len)
    assert rc == 0, (what, eng.lib.nuhtc_last_error(eng.h))
    want = EC.reference_crops(masks, int(n[0]) if isinstance(n, torch.Tensor) else n, cap, pool_cap, pool_len)
    for k in ('box', 'area', 'off'):
        same(got[k], want[k], (what, k))
    bad = np.flatnonzero(got['pool'].view(np.uint32) != want['pool'])          # bits past a crop's width are zero, words past the total keep the mark
    assert not len(bad), (what, 'pool words', bad[:8].tolist(), 'total', int(want['off'][cap]), 'pool_cap', pool_cap)
    return want


@functools.lru_cache(maxsize=None)
def designed(H, W):
    masks = np.stack(list(EC.crop_cases(H, W).values()))
    return masks, EC.pack(masks), int(sum(EC.crop_words_per_mask(m) for m in masks))


@pytest.mark.parametrize('geometry', ('small64', 'big65'))
def test_export_crops_designed_masks(engines, geometry):
    """All designed masks of the frame in one call, then *n_dev below, at and above cap and zero."""
    eng = engines[geometry]
    masks, words, total = designed(*EC.GEOMETRY[geometry]['frame'])
    cap = len(masks)
    want = check_crops(eng, masks, words, cap, cap, total + 7, total + 64, (geometry, 'n == cap'))
    assert want['off'][cap] == total and want['written'].sum() == cap - 3
    check_crops(eng, masks, words, cap - 5, cap, total + 7, total + 64, (geometry, 'n < cap'))
    check_crops(eng, masks, words, cap + 9, cap, total + 7, total + 64, (geometry, 'n > cap'))          # clamped
    check_crops(eng, masks[:cap - 4], words[:cap - 4], cap + 9, cap - 4, total, total + 64, (geometry, 'n > cap, fewer rows'))
    zero = check_crops(eng, masks, words, 0, cap, total + 7, total + 64, (geometry, 'n == 0'))
    assert not zero['off'].any()
    check_crops(eng, masks, words, cap, cap, total, total + 64, (geometry, 'pool_cap == total'))          # exactly enough


@pytest.mark.parametrize('geometry', ('small64', 'big65'))
def test_export_crops_pool_overflow(engines, geometry):
    """A pool one word short of the need, and one that ends one word before the end of a middle crop: the crops that fit are exact, the
    others and every word at or past pool_cap keep the mark (the buffer is longer than pool_cap), off[cap] is the full need."""
    eng = engines[geometry]
    masks, words, total = designed(*EC.GEOMETRY[geometry]['frame'])
    cap, names = len(masks), list(EC.crop_cases(*EC.GEOMETRY[geometry]['frame']))
    full = EC.reference_crops(masks, cap, cap, total, total)
    mid = names.index('x0_33')
    for pool_cap in (total - 1, int(full['off'][mid + 1]) - 1):
        want = check_crops(eng, masks, words, cap, cap, pool_cap, total + 64, (geometry, pool_cap))
        k, nonempty = int(want['written'].sum()), int((want['area'] > 0).sum())
        print(geometry, 'pool_cap', pool_cap, 'of', total, ':', k, 'of', nonempty, 'crops written')
        assert 0 < k < nonempty <= cap and want['off'][cap] == total and (want['pool'][pool_cap:] == EC.marked(1, np.uint32)[0]).all()
    assert not want['written'][mid] and want['written'][:mid].sum() == k


@pytest.mark.parametrize('geometry', BIG)
def test_export_crops_cap_above_1024(engines, geometry):
    """cap = 1203: crop_scan_kernel sums two rows per thread, one in thread 601, none in the threads past it."""
    eng = engines[geometry]
    H, W = EC.GEOMETRY[geometry]['frame']
    words = EC.detection_set(geometry, 'all', masks='designed')['masks_words']
    masks = EC.unpack(words, H, W)
    cap = len(words)
    assert cap > 1024 and cap % 1024 != 0 and cap == EC.GEOMETRY[geometry]['max_batch'] * EC.GEOMETRY[geometry]['K']
    total = int(sum(EC.crop_words_per_mask(m) for m in masks))
    check_crops(eng, masks, words, cap, cap, total + 5, total + 64, (geometry, 'n == cap'))
    check_crops(eng, masks, words, 1100, cap, total // 2, total + 64, (geometry, 'n < cap, half a pool'))


def test_export_crops_refusals(engines):
    eng = engines['small64']
    masks, words, total = designed(64, 96)
    cap = len(masks)
    max_cap = EC.GEOMETRY['small64']['max_batch'] * EC.GEOMETRY['small64']['K']
    big = np.zeros((max_cap + 1, words.shape[1]), np.uint32)
    calls = dict(cap_past_the_engine=dict(words=big, cap=max_cap + 1, pool_cap=64), pool_cap_0=dict(words=words, cap=cap, pool_cap=0),
                 cap_0=dict(words=words, cap=0, pool_cap=64))
    calls.update({f'null_{k}': dict(words=words, cap=cap, pool_cap=total, null=(k,)) for k in ('words', 'n', 'box', 'area', 'off', 'pool')})
    for name, kw in calls.items():
        rc, got = run_crops(eng, kw['words'], kw['cap'], kw['cap'], kw['pool_cap'], total + 64, null=kw.get('null', ()))
        assert rc == hip.E_INVALID, (name, rc)
        assert all((v.view(np.uint8) == EC.MARK).all() for v in got.values()), name
    rc, got = run_crops(eng, big[:max_cap], max_cap, max_cap, 64, 64)          # the engine's whole capacity is taken
    assert rc == 0 and not got['off'][:max_cap + 1].any()


# ----------------------------------------------------------------------------- the two in a row
@pytest.mark.parametrize('geometry', ('small64', 'big65'))
def test_export_then_crops_with_n_read_on_the_device(engines, geometry):
    """nuhtc_export_kept with cap < n, then nuhtc_export_crops behind it on the same stream taking the count from n_dev[0] (above cap: clamped):
    the crops are those of the first cap kept masks."""
    eng = engines[geometry]
    H, W = EC.GEOMETRY[geometry]['frame']
    s = EC.detection_set(geometry, 'alternating', masks='designed')
    kept = EC.kept_slots(s)
    cap = len(kept) - 7
    rc, _, (o, inputs) = run_export(eng, s, cap, sync=False)
    assert rc == 0
    masks = EC.unpack(s['masks_words'][kept[:cap]], H, W)
    total = int(sum(EC.crop_words_per_mask(m) for m in masks))
    rc, got = run_crops(eng, o['words'], o['n'], cap, total, total + 64)
    assert rc == 0 and o['n'][:2].tolist() == [len(kept), 0]
    want = EC.reference_crops(masks, len(kept), cap, total, total + 64)
    for k in ('box', 'area', 'off'):
        same(got[k], want[k], (geometry, k))
    assert np.array_equal(got['pool'].view(np.uint32), want['pool']) and want['off'][cap] == total
    exported = want_export(s, cap)
    for k in EXPORT_FIELDS:
        same(o[k].cpu().numpy(), exported[k], (geometry, k))


def test_engine_export_matches_numpy_crops(engines):
    """One real inference through Engine.export_async on 64 x 96 tiles: idx lists the kept slots in (tile, slot) order, every crop is the
    numpy crop of its row of eng.masks, and the capacity flag n[1] of an inference that did not overflow is zero -- also in a designed
    export on the same engine afterwards."""
    from nuhtc_amd import synth
    eng = engines['small64']
    H, W = 64, 96
    K = eng.cfg.max_per_img
    tiles = np.ascontiguousarray(np.stack([synth.nuclei_tile(60 + k, 128) for k in range(4)])[:, :H, :W])
    with torch.cuda.stream(eng.stream):
        B = eng.infer_async(eng.to_device(tiles), hip.CH_SWAP)
        eng.export_async(B)
        eng.stream.synchronize()
        g = eng.export_read()
        counts, keep = eng.counts[:B].cpu().numpy(), eng.keep[:B].cpu().numpy()
        words = eng.masks[:B].cpu().numpy().view(np.uint32).reshape(B * K, -1)
    slots = np.flatnonzero((np.arange(K)[None] < counts[:, None]) & (keep != 0))
    n = g['n']
    print('kept', n, 'of', int(counts.sum()), 'detections on', B, 'tiles of 64 x 96')
    assert n == len(slots) > 0 and np.array_equal(g['tile'] * K + g['slot'], slots)
    masks = EC.unpack(words[slots], H, W)
    want = EC.reference_crops(masks, n, n, g['pool'], g['pool'])
    assert g['crop_total'] == want['off'][n] <= g['pool'] and want['written'].sum() == n          # no kept mask is empty
    assert np.array_equal(g['crop_box'], want['box']) and np.array_equal(g['crop_area'], want['area']) and np.array_equal(g['crop_off'], want['off'][:n])
    assert np.array_equal(g['crop_words'][:g['crop_total']], want['pool'][:g['crop_total']])
    s = EC.detection_set('small64', 'empty_tile_between')
    check_export(eng, s, len(EC.kept_slots(s)), what='after an inference')


# ----------------------------------------------------------------------------- contours at 65 x 96
def test_device_contours_at_65_by_96(engines):
    """nuhtc_mask_contours against oracle/contour.py, vertex for vertex, at three words per row and H != W: blobs across both word seams,
    on the right and bottom edges, in the last word column only, a hole and an island across a seam, fragmented blobs, and a serpentine
    one pixel wide with 3200 border pixels and 162 vertices: the kernel has no limit on the border's length, only on the vertices."""
    from oracle import contour as OC
    eng = engines['big65']
    H, W = 65, 96
    shapes = EC.contour_shapes(H, W)
    names = list(shapes)
    rings = [OC.find_contours_tree(m)[0][0] for m in shapes.values()]
    i = names.index('serpentine')
    border = len({tuple(p) for p in OC.find_contours_tree(shapes['serpentine'], simple=False)[0][0].tolist()})
    assert border > 2048 and len(rings[i]) < 1024
    eng.masks.zero_()
    eng.masks[0, :len(names)] = up(EC.pack(np.stack(list(shapes.values()))).reshape(len(names), H, W // 32), eng.device)
    eng.counts.zero_()
    eng.counts[0] = len(names)
    for cap in (1024, 100):
        eng.contours_async(1, cap, kept_only=False)
        torch.cuda.synchronize()
        n = eng.contour_n[0].cpu().numpy()
        xy = eng.contour_xy[0, :len(names)].cpu().numpy()
        assert not n[len(names):].any()                     # slots past counts[0] are not traced
        for k, ring in enumerate(rings):
            if len(ring) > cap:
                assert n[k] == -1, (names[k], cap, n[k], len(ring))
            else:
                assert n[k] == len(ring) and np.array_equal(xy[k, :n[k]], ring), (names[k], cap, n[k], len(ring))
        # the serpentine: a ring at cap = 1024 whatever its border length, -1 only when the vertices do not fit
        assert n[i] == (len(rings[i]) if cap == 1024 else -1)
        assert (n == -1).sum() == sum(len(r) > cap for r in rings) and ((n[:len(names)] > 0).all() if cap == 1024 else (n == -1).any())
