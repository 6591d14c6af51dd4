"""The device route of the stitched-tile evaluation (csrc/stitch.hip: nuhtc_op_stitch_gather / _pairs / _render, and the image-level
mask-NMS through nuhtc_merge_overlap) against the host route of nuhtc_amd/stitch.py, which tests/test_stitch_host.py pins to the mask
functions of nuhtc_amd.evaluation on full frames.  Integers, and floats computed by the same host functions from identical integer
tables: exact equality.  Then tools/eval_consep.py end to end, --eval-on gpu against --eval-on host."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stitch_cases as SC  # noqa: E402
from nuhtc_amd import evaluation as E  # noqa: E402
from nuhtc_amd import stitch as S  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs/nuhtc/htc_lite_swin_consep_infer.py')
sys.path.insert(0, os.path.join(ROOT, 'tools'))


@pytest.fixture(scope='module')
def eng(hip_device):
    from nuhtc_amd import weights
    from nuhtc_amd.engine import Engine
    return Engine(weights.bench_state_dict(0, obj_bias=0.0), device=0, max_batch=3, tile=(64, 64))


def pack(masks):
    """(..., H, W) bool -> (..., H, W // 32) int32 words, pixel x in bit x & 31 of word x >> 5."""
    b = np.packbits(np.ascontiguousarray(masks).astype(bool), axis=-1, bitorder='little')
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int32)).cuda()


def second_image():
    """Equal scores across tiles, and little else."""
    t = SC.Tiles()
    f = SC.frame_rect(40, 50, 40, 52)
    for loc in (0, 1, 4, 5):
        g = SC.GRID[loc]
        t.add(loc, f[g['oy']:g['oy'] + SC.TILE, g['ox']:g['ox'] + SC.TILE], 0.5, loc % SC.C)
    t.add(0, SC.tile_mask(rects=[(5, 9, 5, 9)]), 0.5, 0)
    t.add(5, SC.tile_mask(rects=[(30, 34, 30, 34)]), 0.7, 1)
    inst = np.zeros((SC.H, SC.W), np.int32)
    inst[40:50, 41:52] = 1
    inst[5:9, 5:9] = 2
    return t, S.gt_from_mat(inst, np.array([2, 5]))


def gather(eng, store, images, batch=8):
    """Tiles of all `images` (Tiles objects) in image, row-major tile order, `batch` at a time: a batch may hold tiles of two images."""
    items = [(i, t) for i, tl in enumerate(images) for t in tl.grid]
    for i0 in range(0, len(items), batch):
        part = items[i0:i0 + batch]
        f = lambda name: np.stack([getattr(images[i], name)[t['loc']] for i, t in part])
        meta = np.array([S.tile_meta(i, t) for i, t in part], np.int32)
        eng.op_stitch_gather(torch.from_numpy(f('boxes')).cuda(), torch.from_numpy(f('labels')).cuda(), torch.from_numpy(f('counts')).cuda(), pack(f('masks')),
                             torch.from_numpy(meta).cuda(), SC.C, store, SC.FG, SC.OFFSET)


def crops_of(store, image, rec):
    pool = store['pool'][image * store['pool_cap']:(image + 1) * store['pool_cap']].cpu().numpy().view(np.uint32)
    out = []
    for (x0, y0, x1, y1), off in zip(rec['box'], rec['off']):
        h, w = y1 - y0, x1 - x0
        wpr = (w + 31) // 32
        words = pool[off:off + h * wpr].reshape(h, wpr)
        out.append(np.unpackbits(words.view(np.uint8), axis=-1, bitorder='little').astype(bool)[:, :w] if h else np.zeros((0, 0), bool))
    return out


@pytest.fixture(scope='module')
def scored(eng):
    """Both designed images through gather (default-sized store), NMS, pairs and render, beside the host route."""
    images = [SC.designed(), second_image()]
    store = eng.stitch_store(2, cand_cap=len(SC.GRID) * SC.K, pool_cap=1 << 14, slots=8 * SC.K)
    gather(eng, store, [im[0] for im in images])
    out = []
    for i, (tiles, gt) in enumerate(images):
        c = tiles.candidates()
        host = S.score_image_host(c, gt, SC.H, SC.W, SC.THR, want_maps=True)
        rec = eng.stitch_read(store, i)
        kept = eng.stitch_nms(store, i, rec, SC.THR, SC.H, SC.W)
        gtd = torch.from_numpy(gt[0]).cuda()
        pairs = eng.stitch_pairs(store, i, rec, kept, gtd, gt[2], 4096)
        maps = eng.stitch_render(store, i, rec, kept, SC.H, SC.W)
        out.append(dict(c=c, gt=gt, host=host, rec=rec, kept=kept, pairs=pairs, maps=maps, store=store))
    return out


@pytest.mark.parametrize('i', [0, 1])
def test_gather_builds_the_host_routes_candidates(scored, i):
    s = scored[i]
    c, rec = s['c'], s['rec']
    assert rec['n'] == len(c) and rec['need'][0] == len(c) and not rec['overflow']          # default capacities: no fallback
    assert np.array_equal(rec['box'], c.box) and np.array_equal(rec['area'], c.area) and np.array_equal(rec['label'], c.label)
    assert np.array_equal(rec['score'], c.score)
    got = crops_of(s['store'], i, rec)
    assert all(np.array_equal(g, w) for g, w in zip(got, c.crops))
    assert rec['need'][1] == sum(m.shape[0] * ((m.shape[1] + 31) // 32) for m in c.crops)
    if i == 0:
        # crops that start at every kind of bit offset of a tile row, some running over a word boundary of the tile; bit 31 of the last word
        offs = {(int(b[0]) - 29 * k) % 32 for b in c.box for k in range(4)}
        assert len(offs) > 8
        last = [j for j in range(len(c)) if c.box[j].tolist() == [87 + 31, 58 + 62, 151, 122]]
        assert len(last) == 1 and got[last[0]][1, 32] and got[last[0]][0, 32] and got[last[0]][1, 0]


@pytest.mark.parametrize('i', [0, 1])
def test_image_level_nms_matches_the_host_route(scored, i):
    s = scored[i]
    assert s['kept'].tolist() == s['host']['kept'].tolist()
    if i == 1:
        assert s['kept'].tolist() == [5, 4, 1]          # equal scores: the higher candidate index is visited first


@pytest.mark.parametrize('i', [0, 1])
def test_pairs_and_statistics_match_the_host_route(scored, i):
    s = scored[i]
    gt_map, gt_labels, n_t = s['gt']
    p, host = s['pairs'], s['host']
    assert not p['overflow'] and p['n'] == int((host['inter'] > 0).sum())
    inter = E.dense_pairs(n_t, len(s['kept']), *p['pairs'])
    assert np.array_equal(inter, host['inter']) and np.array_equal(p['area_t'][:n_t], host['area_t'])
    area_p = s['rec']['area'][s['kept']].astype(np.float64)
    assert np.array_equal(area_p, host['area_p'])
    got, ref = E.stat_calc_tables(inter, p['area_t'][:n_t], area_p), E.stat_calc_tables(host['inter'], host['area_t'], host['area_p'])
    assert got == ref


@pytest.mark.parametrize('i', [0, 1])
def test_render_matches_the_host_route(scored, i):
    s = scored[i]
    inst, typ = (m.cpu().numpy() for m in s['maps'])
    assert np.array_equal(inst, s['host']['inst_map']) and np.array_equal(typ, s['host']['type_map']) and inst.max() == len(s['kept'])


def test_checkerboard_of_ground_truth_ids_raises_the_partner_counter(eng):
    t = SC.Tiles(grid=S.tile_grid(64, 64, 64, 29))
    t.add(0, SC.tile_mask(rects=[(10, 26, 30, 46)]), 0.9, 0)          # 256 px over ...
    inst = np.zeros((64, 64), np.int32)
    yy, xx = np.mgrid[10:26, 30:46]
    on = (yy + xx) % 2 == 0
    inst[yy[on], xx[on]] = np.arange(1, on.sum() + 1)                 # ... 128 one-pixel instances: more than the 64 a wave's table holds
    store = eng.stitch_store(1, cand_cap=8, pool_cap=256, slots=SC.K)
    gather(eng, store, [t])
    rec = eng.stitch_read(store, 0)
    assert rec['n'] == 1 and not rec['overflow']
    r = eng.stitch_pairs(store, 0, rec, np.array([0]), torch.from_numpy(inst).cuda(), 128, 1024)
    assert r['partners'] and r['overflow']
    inst[inst > 60] = 0                                               # 60 partners fit
    r = eng.stitch_pairs(store, 0, rec, np.array([0]), torch.from_numpy(inst).cuda(), 128, 1024)
    assert not r['overflow'] and r['n'] == 60 and sorted(r['pairs'][0].tolist()) == list(range(60)) and (r['pairs'][2] == 1).all()


def test_capacities_one_below_the_need_are_reported_and_respected(eng, scored):
    tiles, gt = SC.designed()
    rec0, c = scored[0]['rec'], scored[0]['c']
    need_c, need_w = rec0['need']
    G = 64
    for cand_cap, pool_cap, flag in [(need_c - 1, need_w, 1), (need_c, need_w - 1, 2), (need_c, need_w, 0)]:
        store = eng.stitch_store(1, cand_cap=cand_cap, pool_cap=pool_cap, slots=8 * SC.K, guard=G)
        gather(eng, store, [tiles])
        cnt = store['counters'].cpu().numpy()
        assert cnt[:2].tolist() == [need_c, need_w] and cnt[2] == flag and cnt[3] == 0          # the need is counted past the capacity
        for k, per in (('box', 4), ('area', 1), ('score', 1), ('label', 1), ('key', 1), ('off', 1)):
            assert (store[k][cand_cap * per:].cpu().numpy() == -7).all(), k          # nothing at or past the capacity
        assert (store['pool'][pool_cap:].cpu().numpy() == -7).all() and (store['work'][8 * SC.K * 8:].cpu().numpy() == -7).all()
        if flag:
            with torch.cuda.device(0):
                rec = eng.stitch_read(store, 0)
            assert rec['overflow']
        else:
            assert not eng.stitch_read(store, 0)['overflow']
    s = scored[0]
    need = s['pairs']['n']
    r = eng.stitch_pairs(s['store'], 0, s['rec'], s['kept'], torch.from_numpy(gt[0]).cuda(), gt[2], need - 1, guard=8)
    assert r['overflow'] and r['n'] == need and (r['guard'].cpu().numpy() == -7).all()
    r = eng.stitch_pairs(s['store'], 0, s['rec'], s['kept'], torch.from_numpy(gt[0]).cuda(), gt[2], need, guard=8)
    assert not r['overflow'] and (r['guard'].cpu().numpy() == -7).all()


def test_out_of_range_values_are_reported(eng, scored):
    from nuhtc_amd.engine import HipError
    s = scored[0]
    gt_map = s['gt'][0].copy()
    gt_map[50, 20] = s['gt'][2] + 1          # a ground-truth value past t_cap, under a kept prediction
    with pytest.raises(HipError):
        eng.stitch_pairs(s['store'], 0, s['rec'], s['kept'], torch.from_numpy(gt_map).cuda(), s['gt'][2], 4096)
    bad = dict(s['rec'], dev=np.full_like(s['rec']['dev'], 10 ** 6))          # candidate numbers outside the store
    with pytest.raises(HipError):
        eng.stitch_render(s['store'], 0, bad, s['kept'], SC.H, SC.W)


MIN_CANDIDATES, MIN_REMOVED = 20, 3


def test_tool_writes_the_same_files_on_both_routes(hip_device, tmp_path, capfd):
    """tools/eval_consep.py on one synthetic 349 x 349 image (a 2 x 2 grid of 256-pixel tiles at stride 93), seeded synthetic weights:
    --eval-on gpu and --eval-on host must write identical files, with no fallback.  The image must yield at least MIN_CANDIDATES
    candidates of which the cross-tile NMS removes at least MIN_REMOVED (printed below)."""
    sio = pytest.importorskip('scipy.io')
    Image = pytest.importorskip('PIL.Image')
    import eval_consep
    from nuhtc_amd import synth, weights
    rgb = synth.nuclei_canvas(2, step=93, size=256)
    rgb = np.asarray(rgb[0] if isinstance(rgb, tuple) else rgb)[:349, :349, :3].astype(np.uint8)
    assert rgb.shape == (349, 349, 3)
    os.makedirs(tmp_path / 'fold' / 'Images')
    os.makedirs(tmp_path / 'fold' / 'Labels')
    Image.fromarray(rgb).save(tmp_path / 'fold' / 'Images' / 'img_1.png')
    inst = np.zeros((349, 349), np.int32)
    rng = np.random.RandomState(3)
    for k in range(40):
        y, x = rng.randint(0, 330, 2)
        inst[y:y + rng.randint(8, 18), x:x + rng.randint(8, 18)] = k + 1
    sio.savemat(tmp_path / 'fold' / 'Labels' / 'img_1.mat', {'inst_map': inst, 'inst_type': rng.randint(1, 8, (40, 1))})
    ck = tmp_path / 'w.pth'
    torch.save(dict(state_dict=weights.bench_state_dict(0, num_classes=4, obj_bias=0.0)), ck)
    common = lambda out: [CFG, str(ck), '--data', str(tmp_path / 'fold'), '--out', str(tmp_path / out), '--batch', '3', '--save']
    eval_consep.main(common('host'))
    capfd.readouterr()
    eval_consep.main(common('gpu') + ['--eval-on', 'gpu'])
    assert '1 of 1 images scored from device tables, 0 through their masks' in capfd.readouterr().err
    h, g = tmp_path / 'host', tmp_path / 'gpu'
    sh, sg = json.load(open(h / 'summary.json')), json.load(open(g / 'summary.json'))
    assert sh.keys() == sg.keys() and 'aji' in sh and 'multi_pq+' in sh
    for k in sh:
        assert sh[k] == sg[k] or (sh[k] != sh[k] and sg[k] != sg[k]), k
    assert np.array_equal(np.load(h / 'confusion_matrix.npy'), np.load(g / 'confusion_matrix.npy'))
    mh, mg = sio.loadmat(h / 'img_1.mat'), sio.loadmat(g / 'img_1.mat')
    for k in ('inst_map', 'inst_type', 'inst_centroid', 'inst_uid'):
        assert np.array_equal(mh[k], mg[k]), k
    n_kept = int(mh['inst_map'].max())
    cm = np.load(h / 'confusion_matrix.npy')
    print(f'end to end: {n_kept} predictions kept, confusion matrix sum {cm.sum()}')
    # how much the cross-tile NMS had to do: candidates from the host route
    a = eval_consep.parse_args(common('x'))
    from nuhtc_amd import hip
    from nuhtc_amd.apis import init_detector
    model = init_detector(a.config, a.checkpoint, max_batch=3)
    c = eval_consep.host_image(model.engine((256, 256)), rgb, S.tile_grid(349, 349), a, hip)
    print(f'end to end: {len(c)} candidates, {len(c) - n_kept} removed by the image-level mask-NMS')
    assert len(c) >= MIN_CANDIDATES and len(c) - n_kept >= MIN_REMOVED
