"""Host side of the device route of tissue segmentation (nuhtc_amd/tissue.py): the exact-integer restatement of pointPolygonTest that the
kernel of csrc/tissue.hip computes equals the float host function, Otsu on a histogram equals Otsu on the image, and `device=None` is the
code path the functions had before the keyword existed.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

from nuhtc_amd import tissue as T
import tissue_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTOURS = {**TC.small_contours(), **TC.large_contours()}


@pytest.mark.parametrize('name', sorted(CONTOURS))
def test_integer_polygon_test_equals_the_float_host_function_on_designed_points(name):
    c = CONTOURS[name]
    pts = TC.probe_points(c)
    got, want = T.points_polygon_test_int(c, pts), T.points_polygon_test(c, pts)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert (want[:min(len(c), 200)] == 0).all()                     # the vertices lead the list


def test_designed_points_hit_every_answer_and_the_edge_rules():
    sq = TC.small_contours()['square']                               # (0,0) (8,0) (8,6) (0,6)
    f = lambda *p: int(T.points_polygon_test_int(sq, [p])[0])
    assert (f(4, 3), f(8, 3), f(4, 0), f(8, 6), f(9, 3), f(-1, 3)) == (1, 0, 0, 0, -1, -1)
    assert f(12, 0) == -1 and f(-4, 6) == -1 and f(8, 9) == -1      # on the line of an edge, past its end: not on it
    assert f(-3, 0) == -1 and f(-3, 6) == -1 and f(3, 6) == 0       # a ray through two vertices
    u = TC.small_contours()['concave_u']
    g = lambda *p: int(T.points_polygon_test_int(u, [p])[0])
    assert (g(6, 4), g(2, 4), g(10, 4), g(6, 10), g(6, 8), g(6, 0)) == (-1, 1, 1, 1, 0, -1)
    assert T.points_polygon_test_int(np.zeros((0, 2)), [(1, 1)])[0] == -1
    one = TC.small_contours()['one']
    assert T.points_polygon_test_int(one, [(4, 6), (4, 7)]).tolist() == [0, -1]
    for name, c in TC.small_contours().items():
        r = T.points_polygon_test_int(c, TC.probe_points(c))
        assert 0 in r and -1 in r and (len(c) < 3 or 1 in r), name


def test_integer_polygon_test_equals_the_float_host_function_on_random_input():
    rng = np.random.default_rng(5)
    for k in range(60):
        n = int(rng.integers(1, 40))
        scale = int(rng.choice([1, 2, 16, 256, 4096]))
        off = int(rng.choice([0, -77, TC.BIG]))
        c = rng.integers(0, 12, (n, 2)) * scale + off
        pts = np.concatenate([rng.integers(-2, 14, (200, 2)) * scale + off + rng.integers(-1, 2, (200, 2)), TC.probe_points(c, n_random=20, seed=k)], 0)
        assert np.array_equal(T.points_polygon_test_int(c, pts), T.points_polygon_test(c, pts)), k


def test_otsu_on_a_histogram_equals_otsu_on_the_image():
    rng = np.random.default_rng(1)
    bimodal = np.clip(np.where(rng.random((60, 80)) < 0.4, rng.normal(40, 12, (60, 80)), rng.normal(170, 25, (60, 80))), 0, 255).astype(np.uint8)
    two = np.where(rng.random((30, 30)) < 0.3, 20, 180).astype(np.uint8)
    for im in (bimodal, np.full((9, 9), 77, np.uint8), two, np.zeros((4, 4), np.uint8), rng.integers(0, 256, (50, 50), dtype=np.uint8)):
        assert T.otsu_threshold_hist(np.bincount(im.reshape(-1), minlength=256)) == T.otsu_threshold(im)
    assert 40 < T.otsu_threshold_hist(np.bincount(bimodal.reshape(-1), minlength=256)) < 170


def test_device_none_is_the_host_route():
    img = TC.blob_slide(1024, 1536)
    for kw in (dict(scale=8, filter_params=TC.FILTER), dict(scale=8, filter_params=TC.FILTER, use_otsu=True, mthresh=5, close=3)):
        a, b = T.segment_tissue(img, **kw), T.segment_tissue(img, device=None, **kw)
        assert len(a[0]) == len(b[0]) >= 2 and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
        assert [len(h) for h in a[1]] == [len(h) for h in b[1]] and all(np.array_equal(x, y) for p, q in zip(a[1], b[1]) for x, y in zip(p, q))
    conts, holes = a
    assert sum(len(h) for h in holes) >= 1
    for c, h in zip(conts, holes):
        for fn in ('basic', 'center', 'four_pt', 'four_pt_hard'):
            want = T.contour_coords(c, h, (1536, 1024), 255, 96, fn)
            assert np.array_equal(T.contour_coords(c, h, (1536, 1024), 255, 96, fn, device=None), want) and len(want) > 1
    x, y = T.tissue_tile_coords(img, 128, 96, scale=8, filter_params=TC.FILTER), T.tissue_tile_coords(img, 128, 96, scale=8, filter_params=TC.FILTER, device=None)
    assert np.array_equal(x[0], y[0]) and len(x[0]) > 20


def test_cli_has_seg_on_with_the_host_default():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import infer_wsi
    base = ['src', 'cfg.py', 'w.pth', '--save_dir', 'out']
    assert infer_wsi.parse_args(base).seg_on == 'host'
    assert infer_wsi.parse_args(base + ['--seg-on', 'gpu']).seg_on == 'gpu'
    with pytest.raises(SystemExit):
        infer_wsi.parse_args(base + ['--seg-on', 'tpu'])


def test_seg_on_is_validated_and_gpu_without_a_gpu_is_an_error(tmp_path):
    import torch
    from nuhtc_amd import slides
    with pytest.raises(ValueError):
        slides.seg_and_patch(str(tmp_path), str(tmp_path), str(tmp_path), str(tmp_path), str(tmp_path), seg_on='cpu')
    if not torch.cuda.is_available():                               # no fallback: the device route refuses, it does not run the host code
        with pytest.raises(RuntimeError, match='needs a GPU'):
            T.segment_tissue(TC.blob_slide(256, 256), scale=8, device=0)
        with pytest.raises(RuntimeError, match='needs a GPU'):
            T.contour_coords(np.array([[0, 0], [900, 0], [900, 900]]), [], (1000, 1000), device=0)
