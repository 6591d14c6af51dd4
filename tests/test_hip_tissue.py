"""The device route of tissue segmentation and tile selection (csrc/tissue.hip: nuhtc_tissue_mask, nuhtc_points_polygon_test,
nuhtc_grid_in_contour) against the host functions of nuhtc_amd/tissue.py: stage by stage, then through segment_tissue / contour_coords /
seg_and_patch / tools/infer_wsi.py --seg-on gpu.  Integer work on both sides: every comparison is exact equality."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nuhtc_amd import hip
from nuhtc_amd import tissue as T
import tissue_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, 'configs/nuhtc/htc_lite_swin_pannuke_infer.py')
TILE_W, TILE_H = 64, 32            # TM_TW x TM_TH of csrc/tissue.hip
STAGES = ('sat', 'med', 'hist', 'binary')


def check_mask(img, **kw):
    got, want = T.tissue_mask_device(img, device=0, planes=True, **kw), TC.host_planes(img, **kw)
    for k in STAGES:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, img.shape, kw)
    assert got['thr'] == want['thr']
    assert np.array_equal(T.tissue_mask_device(img, device=0, **kw), want['binary'])          # the route without the optional planes
    return want


# ----------------------------------------------------------------------------- mask op
SHAPES = [(1, 1), (1, 9), (9, 1), (3, 3), (17, 33), (65, 67), (130, 257),
          (TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (2 * TILE_H, 2 * TILE_W + 1)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_mask_stages_over_shapes(hip_device, shape):
    for name in ('noisy', 'random'):
        img = TC.image_kinds(*shape, seed=shape[1])[name]
        check_mask(img)
        check_mask(img, mthresh=9, close=5, sthresh=20)
        check_mask(img, mthresh=15, close=16, sthresh=12)


@pytest.mark.parametrize('mthresh', [1, 3, 5, 7, 9, 11, 13, 15])
def test_mask_median_sizes(hip_device, mthresh):
    kinds = TC.image_kinds(65, 67, seed=mthresh)
    for name in ('noisy', 'checker', 'random', 'one_bright'):
        check_mask(kinds[name], mthresh=mthresh)
    check_mask(TC.image_kinds(3, 3, seed=1)['random'], mthresh=mthresh)


@pytest.mark.parametrize('close', [0, 1, 2, 3, 4, 5, 8, 15, 16])
def test_mask_close_sizes(hip_device, close):
    kinds = TC.image_kinds(65, 67, seed=close)
    for name in ('noisy', 'checker', 'borders'):
        for mthresh in (7, 1):
            w = check_mask(kinds[name], close=close, mthresh=mthresh)
    assert 0 < np.count_nonzero(w['binary']) < w['binary'].size        # (the frame and its bar stay apart: their gaps are 16 wide)
    check_mask(TC.image_kinds(5, 4, seed=2)['borders'], close=close, mthresh=1)


@pytest.mark.parametrize('sthresh', [0, 8, 254])
@pytest.mark.parametrize('sthresh_up', [255, 128])
def test_mask_thresholds(hip_device, sthresh, sthresh_up):
    for name in ('random', 'noisy'):
        w = check_mask(TC.image_kinds(17, 33, seed=3)[name], sthresh=sthresh, sthresh_up=sthresh_up)
        assert set(np.unique(w['binary'])) <= {0, sthresh_up}
    check_mask(TC.image_kinds(17, 33, seed=3)['random'], sthresh=sthresh, sthresh_up=sthresh_up, mthresh=1, close=0)


@pytest.mark.parametrize('kind', sorted(TC.image_kinds(2, 2)))
def test_mask_image_kinds(hip_device, kind):
    for shape in ((65, 67), (3, 3), (33, 130)):
        img = TC.image_kinds(*shape, seed=7)[kind]
        for close in (4, 5):
            check_mask(img, close=close)
    assert img.shape[2] == (4 if kind == 'four_channel' else 3)


def test_mask_saturation_table_and_strided_input(hip_device):
    v, d = np.mgrid[0:256, 0:256]
    img = np.stack([v, np.maximum(v - d, 0), np.maximum(v - d // 2, 0)], 2).astype(np.uint8)          # every (v, v - min) pair
    w = check_mask(img, mthresh=1, close=0)
    assert w['sat'][0, 0] == 0 and w['sat'][255, 255] == 255
    big = TC.image_kinds(70, 140, seed=9)['four_channel']
    check_mask(big[::2, ::2])                                                                          # a strided view, as image[::scale, ::scale]


def test_mask_otsu_end_to_end(hip_device):
    rng = np.random.default_rng(4)
    H, W = 70, 90
    tissue = np.zeros((H, W), bool)
    tissue[10:50, 15:70] = True
    img = np.where(tissue[..., None], np.array([200, 120, 180]), np.array([225, 215, 222])).astype(np.uint8)
    img -= rng.integers(0, 12, img.shape, dtype=np.uint8)
    w = check_mask(img, use_otsu=True)
    assert 8 < w['thr'] < 100 and 0 < np.count_nonzero(w['binary']) < H * W
    check_mask(img, use_otsu=True, mthresh=3, close=2)
    check_mask(np.full((9, 9, 3), 77, np.uint8), use_otsu=True)


# ----------------------------------------------------------------------------- polygon op
SMALL, LARGE = TC.small_contours(), TC.large_contours()


@pytest.mark.parametrize('name', sorted(SMALL))
def test_polygon_small_contours_against_both_host_functions(hip_device, name):
    c = SMALL[name]
    pts = TC.probe_points(c)
    got = T.points_polygon_test_device(c, pts, device=0)
    assert got.dtype == np.int64 and np.array_equal(got, T.points_polygon_test_int(c, pts)) and np.array_equal(got, T.points_polygon_test(c, pts))
    assert 0 in got and -1 in got and (len(c) < 3 or 1 in got)


@pytest.mark.parametrize('name', sorted(LARGE))
def test_polygon_large_contours(hip_device, name):
    c = LARGE[name]
    pts = TC.probe_points(c)
    got = T.points_polygon_test_device(c, pts, device=0)
    assert np.array_equal(got, T.points_polygon_test_int(c, pts))
    assert {-1, 0, 1} <= set(got.tolist())


def test_polygon_edge_rules_and_random(hip_device):
    sq = SMALL['square']
    f = lambda *p: T.points_polygon_test_device(sq, np.array(p).reshape(-1, 2), device=0).tolist()
    assert f((4, 3), (8, 3), (4, 0), (8, 6), (9, 3), (-1, 3)) == [1, 0, 0, 0, -1, -1]
    assert f((12, 0), (-4, 6), (8, 9), (-3, 0), (-3, 6)) == [-1] * 5              # on the line of an edge past its end; a ray through vertices
    rng = np.random.default_rng(11)
    for k in range(12):
        n = int(rng.integers(1, 60))
        scale, off = int(rng.choice([1, 16, 4096])), int(rng.choice([0, -77, TC.BIG]))
        c = rng.integers(0, 12, (n, 2)) * scale + off
        pts = np.concatenate([rng.integers(-2, 14, (700, 2)) * scale + off + rng.integers(-1, 2, (700, 2)), TC.probe_points(c, n_random=20, seed=k)], 0)
        got = T.points_polygon_test_device(c, pts, device=0)
        assert np.array_equal(got, T.points_polygon_test_int(c, pts)) and np.array_equal(got, T.points_polygon_test(c, pts))


# ----------------------------------------------------------------------------- grid op
def traced(mask, scale, shift=(0, 0)):
    return (T._trace_all(mask) * scale + np.array(shift)).astype(np.int32)


@pytest.fixture(scope='module')
def grid_case():
    """A tissue contour in level-0 pixels (scale 16, as segment_tissue leaves it) and nine hole contours inside it."""
    yy, xx = np.mgrid[0:100, 0:140]
    blob = ((yy - 50) / 44.0) ** 2 + ((xx - 70) / 62.0) ** 2 <= 1
    blob[20:30, 0:40] = False                                              # a notch: concave
    cont = traced(blob, 16)
    holes = []
    for k in range(9):
        cy, cx = 32 + 18 * (k // 3), 40 + 28 * (k % 3)
        holes.append(traced(((yy - cy) / (4.0 + k)) ** 2 + ((xx - cx) / (6.0 + k)) ** 2 <= 1, 16))
    return cont, holes, (140 * 16, 100 * 16)


@pytest.mark.parametrize('fn', ['basic', 'center', 'four_pt', 'four_pt_hard'])
@pytest.mark.parametrize('n_holes', [0, 1, 9])
def test_grid_equals_host_contour_coords(hip_device, grid_case, fn, n_holes):
    cont, holes, wh = grid_case
    n_cases = 0
    for pad in (True, False):
        for step in (192, 256):
            for patch in (256, 255):
                want = T.contour_coords(cont, holes[:n_holes], wh, patch, step, fn, pad)
                got = T.contour_coords(cont, holes[:n_holes], wh, patch, step, fn, pad, device=0)
                assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (pad, step, patch)
                n_cases += len(want) > 4
    assert n_cases == 8
    if n_holes == 9 and fn == 'four_pt':                                   # the holes remove tiles, and a half-integer centre decides some
        assert len(T.contour_coords(cont, [], wh, 256, 64, fn)) > len(T.contour_coords(cont, holes, wh, 256, 64, fn, device=0))


def test_grid_shapes_cuts_and_the_more_than_one_rule(hip_device, grid_case):
    cont, holes, wh = grid_case
    x0, y0, w, h = T.bounding_rect(cont)
    same = lambda *a, **k: np.array_equal(T.contour_coords(*a, device=0, **k), T.contour_coords(*a, **k))
    cuts = [dict(top_left=(x0 + 300, y0 + 200)), dict(bot_right=(x0 + 900, y0 + 700)), dict(top_left=(x0 + 300, y0 + 200), bot_right=(x0 + 1100, y0 + 900)),
            dict(top_left=(x0 + 500, y0 + 500), bot_right=(x0 + 400, y0 + 900)),                       # empty cut
            dict(top_left=(x0 + 100, y0 + 600), bot_right=(x0 + w, y0 + 700)),                         # one row
            dict(top_left=(x0 + 700, y0), bot_right=(x0 + 800, y0 + h)),                               # one column
            dict(top_left=(x0 + 700, y0 + 600), bot_right=(x0 + 800, y0 + 700))]                       # one cell
    shapes = []
    for cut in cuts:
        for fn in ('four_pt', 'four_pt_hard', 'center'):
            assert same(cont, holes[:2], wh, 256, 192, fn, **cut), (cut, fn)
        shapes.append(len(T.contour_coords(cont, holes[:2], wh, 256, 192, 'four_pt', **cut)))
    assert shapes[3] == 0 and shapes[6] == 0 and min(shapes[:3] + shapes[4:6]) > 1              # one cell passes alone: the `> 1` rule drops it
    grid = lambda c, start, n, fn='four_pt', patch=256: T.grid_in_contour_device(c, [], start, n, 192, patch, fn, device=0)
    assert grid(cont, (x0 + 700, y0 + 600), (1, 1)).tolist() == [True]
    # a contour whose grid yields exactly one tile and one that yields none, whole call
    small = np.array([[1000, 1000], [1100, 1000], [1100, 1100], [1000, 1100]], np.int32)
    assert len(T.contour_coords(small, [], wh, 256, 192, 'four_pt')) == 0 and same(small, [], wh, 256, 192, 'four_pt')
    assert grid(small, (1000, 1000), (1, 1)).tolist() == [True] and grid(small, (1000, 1000), (1, 1), 'four_pt_hard').tolist() == [False]
    assert same(small, [], wh, 256, 192, 'four_pt_hard') and same(small, [], wh, 64, 50, 'four_pt') and len(T.contour_coords(small, [], wh, 64, 50, 'four_pt', device=0)) > 1
    # no contour: only the holes decide; the order is meshgrid(indexing='ij')
    assert same(None, holes, wh, 256, 192, 'four_pt') and same(None, [], wh, 255, 256, 'center')
    k = T.grid_in_contour_device(small, [], (900, 900), (3, 2), 100, 2, 'basic', device=0).reshape(3, 2)
    assert k.tolist() == [[False, False], [False, True], [False, True]]


# ----------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def slide():
    return TC.blob_slide()


def test_tissue_tile_coords_on_the_device_equals_the_host(hip_device, slide):
    for kw in (dict(), dict(contour_fn='four_pt_hard', use_padding=False), dict(seg_params=dict(T.SEG_PARAMS, use_otsu=True))):
        want = T.tissue_tile_coords(slide, 256, 192, scale=16, filter_params=TC.FILTER, **kw)
        got = T.tissue_tile_coords(slide, 256, 192, scale=16, filter_params=TC.FILTER, device=0, **kw)
        assert np.array_equal(got[0], want[0]) and got[0].dtype == np.int64 and len(want[0]) > 30
        assert len(got[1]) == len(want[1]) == 2 and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
        assert sorted(len(h) for h in want[2]) == [0, 1] and all(np.array_equal(a, b) for p, q in zip(got[2], want[2]) for a, b in zip(p, q))
    got = T.tissue_tile_coords(slide, 256, 192, scale=16, filter_params=TC.FILTER, device=torch.device('cuda:0'))
    assert np.array_equal(got[0], T.tissue_tile_coords(slide, 256, 192, scale=16, filter_params=TC.FILTER)[0])


def test_seg_and_patch_on_the_gpu_writes_the_same_files(hip_device, slide, tmp_path):
    from nuhtc_amd import slides
    src = tmp_path / 'wsi'
    src.mkdir()
    np.save(src / 'a.npy', slide)
    np.save(src / 'b.npy', slide[::-1, ::-1].copy())
    seg, flt, vis, pat = slides.default_parameters()
    flt = dict(flt, **TC.FILTER)
    for where in ('host', 'gpu'):
        out = tmp_path / where
        dirs = dict(source=str(src), save_dir=str(out), patch_save_dir=str(out / 'patches'), mask_save_dir=str(out / 'masks'), stitch_save_dir=str(out / 'stitches'))
        for k, v in dirs.items():
            if k != 'source':
                os.makedirs(v)
        slides.seg_and_patch(**dirs, seg_params=seg, filter_params=flt, vis_params=vis, patch_params=pat, patch_size=256, step_size=192, seg=True,
                             patch=True, seg_downsample=16, log=lambda *a: None, seg_on=where, device=0)
    read = lambda where, name: open(tmp_path / where / name, 'rb').read()
    assert read('gpu', 'process_list_autogen.csv') == read('host', 'process_list_autogen.csv')
    for sid in ('a', 'b'):
        g, h = np.load(tmp_path / 'gpu' / 'patches' / f'{sid}.npz'), np.load(tmp_path / 'host' / 'patches' / f'{sid}.npz')
        assert sorted(g.files) == sorted(h.files) and all(np.array_equal(g[k], h[k]) for k in h.files) and len(h['coords']) > 30
        assert read('gpu', f'masks/{sid}.png') == read('host', f'masks/{sid}.png')


def test_infer_wsi_seg_on_gpu_writes_the_same_geojson(hip_device, tmp_path):
    from nuhtc_amd import synth, weights
    H, W = 768, 1024
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    blob = ((yy - 380) / 300.0) ** 2 + ((xx - 500) / 420.0) ** 2 <= 1
    tex = np.concatenate([np.concatenate([synth.nuclei_tile(40 + 4 * r + c, 256) for c in range(W // 256)], 1) for r in range(H // 256)], 0)
    img = np.full((H, W, 3), 235, np.uint8)
    img[blob] = tex[blob]
    np.save(tmp_path / 'slide.npy', img)
    ck = tmp_path / 'w.pth'
    torch.save(dict(state_dict=weights.bench_state_dict(0, obj_bias=0.0)), ck)
    docs = {}
    for where in ('host', 'gpu'):
        cmd = ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'tools/infer_wsi.py'), str(tmp_path / 'slide.npy'), CFG, str(ck), '--seg', '--patch',
               '--patch_size', '128', '--step_size', '96', '--batch_size', '16', '--seg_downsample', '4', '--save_dir', str(tmp_path / where), '--seg-on', where]
        log = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
        assert '1 contour(s), ' in log
        docs[where] = open(tmp_path / where / 'nuclei/slide/slide.geojson', 'rb').read()
        assert np.array_equal(np.load(tmp_path / where / 'patches/slide.npz')['coords'], np.load(tmp_path / 'host/patches/slide.npz')['coords'])
    assert docs['gpu'] == docs['host'] and len(json.loads(docs['host'])) > 20


# ----------------------------------------------------------------------------- refusals
def test_refusals_return_negative_codes_and_write_nothing(hip_device):
    lib = hip.load()
    dev = torch.device('cuda:0')
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    H, W = 20, 30
    img = torch.from_numpy(TC.noisy_tissue(H, W)).to(dev)
    fill = lambda n, dt=torch.uint8: torch.full((n,), 7, dtype=dt, device=dev)
    outs = [fill(H * W), fill(H * W), fill(H * W), fill(256, torch.int64)]
    mask = lambda im=img, h=H, w=W, stage=0, mthresh=7, close=4, up=255, o=outs: lib.nuhtc_tissue_mask(
        0, vp(im), h, w, w * 3, 3, stage, mthresh, 8, up, close, vp(o[0]), vp(o[1]), vp(o[2]), vp(o[3]), stream)
    bad = [mask(mthresh=4), mask(mthresh=17), mask(mthresh=0), mask(mthresh=-1), mask(close=17), mask(close=-1), mask(im=None), mask(h=0), mask(w=-3),
           mask(stage=3), mask(up=-1), mask(o=[None] + outs[1:]), mask(o=outs[:3] + [None]), mask(stage=2, o=outs[:2] + [None, outs[3]]),
           lib.nuhtc_tissue_mask(0, vp(img), H, W, W * 3 - 1, 3, 0, 7, 8, 255, 4, vp(outs[0]), None, None, vp(outs[3]), stream),
           lib.nuhtc_tissue_mask(0, vp(img), H, W, W * 3, 2, 0, 7, 8, 255, 4, vp(outs[0]), None, None, vp(outs[3]), stream)]
    assert all(rc < 0 for rc in bad), bad
    assert all(bool((o == 7).all()) for o in outs)
    assert mask() == 0 and not bool((outs[0] == 7).all())

    cont = torch.tensor([[0, 0], [8, 0], [8, 6], [0, 6]], dtype=torch.int32, device=dev)
    pts = torch.tensor([[4, 3], [9, 9]], dtype=torch.int32, device=dev)
    res = torch.full((2,), 7, dtype=torch.int8, device=dev)
    pip = lambda c=cont, nv=4, p=pts, n=2, r=res: lib.nuhtc_points_polygon_test(0, vp(c), nv, vp(p), n, vp(r), stream)
    bad = [pip(nv=0), pip(nv=-1), pip(c=None), pip(n=-1), pip(p=None), pip(r=None)]
    assert all(rc < 0 for rc in bad) and res.tolist() == [7, 7]
    assert pip(n=0) == 0 and res.tolist() == [7, 7] and pip() == 0 and res.tolist() == [1, -1]

    keep = fill(12)
    offs = (ctypes.c_int32 * 8)(1, 1, 3, 3, 3, 1, 1, 3)
    pool = torch.tensor([[2, 2], [6, 2], [6, 5], [2, 5], [1, 1], [3, 1], [3, 3]], dtype=torch.int32, device=dev)
    I64 = lambda *v: (ctypes.c_int64 * len(v))(*v)

    def grid(nx=4, ny=3, step=2, n_off=4, c=cont, nv=4, h=pool, n_pool=7, hole_off=I64(0, 4, 7), n_holes=2, start=0, o=offs, k=keep):
        return lib.nuhtc_grid_in_contour(0, start, start, nx, ny, step, o, n_off, 0, vp(c), nv, vp(h), n_pool, hole_off, n_holes, 2, 2, vp(k), stream)
    bad = [grid(nx=-1), grid(ny=-2), grid(step=0), grid(n_off=0), grid(n_off=5), grid(o=None), grid(nv=-1), grid(c=None), grid(nv=0), grid(k=None),
           grid(hole_off=I64(0, 4, 8)), grid(hole_off=I64(0, 9, 7)), grid(hole_off=I64(1, 4, 7)), grid(hole_off=I64(0, 4, 4)), grid(hole_off=I64(0, 5, 4)),
           grid(hole_off=I64(0, -1, 7)), grid(n_pool=6), grid(h=None), grid(hole_off=None), grid(n_holes=-1), grid(nx=1 << 16, ny=1 << 16),
           grid(start=(1 << 30) + 1), grid(nx=1 << 20, ny=1, step=1 << 11)]
    assert all(rc < 0 for rc in bad), bad
    assert bool((keep == 7).all())
    assert grid(nx=0) == 0 and bool((keep == 7).all())
    assert grid() == 0 and set(keep.tolist()) <= {0, 1}
    want = T.in_contour(cont.cpu().numpy(), np.stack(np.meshgrid(np.arange(0, 8, 2), np.arange(0, 6, 2), indexing='ij'), -1).reshape(-1, 2), 4, 'four_pt')
    want &= ~T.in_holes([pool[:4].cpu().numpy(), pool[4:].cpu().numpy()], np.stack(np.meshgrid(np.arange(0, 8, 2), np.arange(0, 6, 2), indexing='ij'), -1).reshape(-1, 2), 4)
    assert keep.bool().tolist() == want.tolist()
