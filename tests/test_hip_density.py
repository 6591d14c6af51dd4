"""GPU tests of the density rasters (csrc/celldensity.hip, nuhtc_cell_density): count and weight must EQUAL
nuhtc_amd.density.density_reference, the brute-force int64 restatement of the definition -- same dtype and shape, no tolerance, nothing
left out.  Sites outside the points' box on all four sides (as they are, mirrored, at the far corners of the coordinate range), windows
that are no multiple of a tile, the inclusive radius and the weight-0 ring, 64-bit sums and a cell fuller than a staging chunk, labels
out of range, pitch against reach, other windows, a binning over two scan chunks, random sets (repeatable, independent of the row order),
the edge sizes, the refused arguments, and tools/infer_wsi.py --nuclei-density end to end.  The designed sets of tests/density_cases.py
reach both kernels (staged through LDS, and every site on its own); which one ran is read from the library's profile."""
import os

import numpy as np
import pytest
import torch

import density_cases as DC
import proximity_cases as PC
import points_util
from nuhtc_amd import cellgraph, cellpoints, hip
from nuhtc_amd import density as dn

pytestmark = pytest.mark.gpu
FAR = (((1 << 26) + 12345, -(1 << 26) - 321), (-(1 << 26) - 7, (1 << 26) + 50001))


def _equal(got, want, what):
    for name, g, w in zip(dn.INT_NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, f'{len(bad)} entries differ, first at {bad[0].tolist()}', int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


def _raw(case, win, fill=77, bounds=None, shape=None):
    """One call on buffers filled with `fill` (of the window's shape, or `shape` where the arguments describe none) -> (return code, count, weight)."""
    p, lab, C, h, s = case
    dev = torch.device('cuda', 0)
    p = np.ascontiguousarray(np.asarray(p, np.int32).reshape(-1, 2))
    out = dn.outputs(C, win, dev, fill=fill) if shape is None else dn.outputs(shape[0], (0, 0, shape[2], shape[1]), dev, fill=fill)
    rc = dn.call(torch.from_numpy(p).to(dev), torch.from_numpy(np.ascontiguousarray(lab, np.int32)).to(dev), C, h, s, win, *out, bounds=bounds)
    torch.cuda.synchronize()
    return rc, out[0].cpu().numpy(), out[1].cpu().numpy()


def _device(case, win=None):
    win = DC.default_window(case) if win is None else win
    rc, count, weight = _raw(case, win)
    assert rc == hip.OK, rc
    return count, weight


def _check(case, what, win=None):
    win = DC.default_window(case) if win is None else win
    got = _device(case, win)
    _equal(got, dn.density_reference(*case, win), what)
    return got


# ---- 1: sites outside the box on all four sides
@pytest.mark.parametrize('s', [4, 1])
def test_sites_outside_the_box_on_all_four_sides(hip_device, s):
    case = DC.patch(s)
    win = DC.default_window(case)
    x_min, y_min, x_max, y_max = cellpoints.bounds_of(case[0])
    assert win[0] * s < x_min and win[1] * s < y_min and (win[0] + win[2] - 1) * s > x_max and (win[1] + win[3] - 1) * s > y_max
    got = _check(case, f'patch, s {s}')
    assert got[0][:, 0, :].any() or got[0][:, :, 0].any() or got[0][:, -1, :].any() or got[0][:, :, -1].any()
    _check(DC.mirror(case), f'patch mirrored, s {s}')
    for dx, dy in FAR:
        _check(DC.translate(case, dx, dy), f'patch moved by ({dx}, {dy}), s {s}')
        _check(DC.translate(DC.mirror(case), dx, dy), f'patch mirrored and moved by ({dx}, {dy}), s {s}')


def test_both_kernels_are_reached(hip_device):
    """The library's profile names the stage that ran: the tile kernel where 15 s <= 2 h + side, the site kernel elsewhere."""
    for case in (DC.patch(1), DC.patch(4), DC.crowded(8), DC.crowded(3), DC.lattice(1), DC.lattice(5), DC.coincident(2048), DC.coincident(16384)):
        hip.profile_enable(True)
        try:
            _device(case)
            tags = {tag for tag in hip.profile_read() if tag.startswith('cell_density')}
        finally:
            hip.profile_enable(False)
        assert tags == {'cell_density_bin', 'cell_density_tile' if DC.staged(case) else 'cell_density_site'}, (case[3:], tags)
    assert DC.staged(DC.patch(1)) and not DC.staged(DC.patch(4))


# ---- 2: tiles
@pytest.mark.parametrize('s, shape', [(1, (37, 21)), (1, (70, 50)), (5, (37, 21)), (5, (70, 50))])
def test_windows_that_are_no_multiple_of_a_tile(hip_device, s, shape):
    case = DC.lattice(s)
    full = DC.default_window(case)
    assert len(case[0]) == 1200 and (full[2] > shape[0] or s == 5)          # at pitch 5 the larger window reaches past the default one
    got = _check(case, f'lattice, s {s}, {shape}', (full[0] + 3, full[1] + 2) + shape)
    assert got[0].any()


# ---- 3: the inclusive radius and the weight-0 ring
def test_inclusive_radius_and_the_ring_at_exactly_h(hip_device):
    count, weight = _check(DC.three_four_five(), '3-4-5', (-5, -5, 11, 11))
    assert count[0, 9, 8] == 1 and weight[0, 9, 8] == 0 and count[0, 10, 8] == 0 and weight[0, 10, 8] == 0
    count, weight = _check(DC.pythagorean_ring(), 'ring', (-1, -1, 3, 3))
    assert count[:, 1, 1].tolist() == [6, 6] and weight[:, 1, 1].tolist() == [0, 0]
    count, weight = _check(DC.pythagorean_ring()[:3] + (25, 1), 'ring at pitch 1')
    win = DC.default_window(DC.pythagorean_ring()[:3] + (25, 1))
    assert count[:, -win[1], -win[0]].tolist() == [6, 6] and weight[:, -win[1], -win[0]].tolist() == [0, 0]


# ---- 4: 64-bit sums and a crowded cell
@pytest.mark.parametrize('s', [16384, 2048])
def test_1500_coincident_points_sum_in_64_bits(hip_device, s):
    case = DC.coincident(s)
    win = DC.default_window(case)
    count, weight = _check(case, f'coincident, s {s}')
    at = (0, -2 * 16384 // s - win[1], 3 * 16384 // s - win[0])
    assert count[at] == 1500 and weight[at] == 1500 * (1 << 28) > 1 << 32


@pytest.mark.parametrize('h', [8, 3])
def test_1500_points_on_nine_places_in_two_cells(hip_device, h):
    count, weight = _check(DC.crowded(h), f'crowded, h {h}')
    assert count.sum(0).max() == 1500 if h == 8 else count.sum(0).max() > 500


# ---- 5: labels
def test_labels_outside_the_classes_land_nowhere(hip_device):
    case = DC.labels_out_of_range()
    p, lab, C, h, s = case
    assert set(lab.tolist()) == {-1, 0, 1, 2, 3, 14}
    count, weight = _check(case, 'labels')
    keep = (lab >= 0) & (lab < C)
    one = _device((p[keep], np.zeros(keep.sum(), np.int32), 1, h, s), DC.default_window(case))
    assert np.array_equal(count.sum(0), one[0][0]) and np.array_equal(weight.sum(0), one[1][0]) and one[0].any()


# ---- 6: pitch against reach
@pytest.mark.parametrize('name', ['dense', 'sparse', 'unit'])
def test_pitch_against_reach(hip_device, name):
    case = DC.pitch_cases()[name]
    assert case[3:] == dict(dense=(3, 1), sparse=(7, 50), unit=(1, 1))[name]
    count, weight = _check(case, name)
    assert count.any()
    if name == 'unit':
        assert set(np.unique(weight).tolist()) <= set(range(0, 1 + int(count.max())))     # h = 1: a term is 1 (on the site) or 0 (beside it)


# ---- 7: other windows
@pytest.mark.parametrize('s', [4, 1])
def test_other_windows(hip_device, s):
    case = DC.patch(s)
    gx0, gy0, W, H = DC.default_window(case)
    full = _device(case)
    sub = _device(case, (gx0 + 5, gy0 + 3, W - 9, H - 7))
    _equal(sub, [a[:, 3:H - 4, 5:W - 4] for a in full], 'a sub-window')
    assert sub[0].any()
    got = _check(case, 'half off the points', (gx0 - W // 2, gy0 - H // 2, W, H))
    assert got[0].any() and not got[0][:, :H // 2 - 1].any()
    for win in ((gx0 + 10000, gy0 - 10000, 40, 23), (gx0 - 10000, gy0, 17, 18), (gx0, gy0 + 10000, 16, 16)):
        rc, count, weight = _raw(case, win)
        assert rc == hip.OK and not count.any() and not weight.any(), win                  # nowhere near: zeros, written over the fill
    _check(case, 'one site', (gx0 + W // 2, gy0 + H // 2, 1, 1))
    _check(case, 'one column', (gx0 + W // 2, gy0, 1, H))


# ---- 8: a binning over two scan chunks
def test_chain_of_20000_points_over_two_scan_chunks(hip_device):
    """The chain of tests/proximity_cases.py, 8 half pixels between neighbours on the line y = 11, with h = 8: 20 000 cells of side 8, more
    than one scan chunk of 16 384.  Pitch 18 puts one row of 8 890 sites on y = 18, 7 beside the line: a site sees the points at most 3
    along x from it."""
    p, lab = PC.chain('shuffled')[:2]
    case = (p, lab, 2, 8, 18)
    win = DC.default_window(case)
    assert win[3] == 1 and 8000 < win[2] * win[3] < 200000 and (p[:, 0].max() - p[:, 0].min()) // 8 + 1 > 16384
    count, weight = _check(case, 'chain')
    assert count.sum() > 2000


# ---- 9: random sets
@pytest.fixture(scope='module')
def large_references():
    out = {}
    for kind in ('uniform', 'clumps'):
        p, lab = DC.random_large(kind)
        for h, s in DC.LARGE_HS:
            out[(kind, h, s)] = dn.density_reference(p, lab, 5, h, s, DC.default_window((p, lab, 5, h, s)))
    return out


@pytest.mark.parametrize('kind', ['uniform', 'clumps'])
@pytest.mark.parametrize('h, s', DC.LARGE_HS)
def test_3000_random_points(hip_device, large_references, kind, h, s):
    p, lab = DC.random_large(kind)
    case = (p, lab, 5, h, s)
    a, b = _device(case), _device(case)
    _equal(a, large_references[(kind, h, s)], f'{kind}, h {h}, s {s}')
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    order = np.random.default_rng(4).permutation(len(p))
    _equal(_device((p[order], lab[order], 5, h, s)), a, 'permuted rows')
    built = dn.build(p, lab, 5, h / 2, s / 2)
    _equal(built[:2], a, 'build')
    assert built[2] == DC.default_window(case)


# ---- 10: edge sizes
def test_no_points_and_one_point(hip_device):
    rc, count, weight = _raw((np.zeros((0, 2)), np.zeros(0), 3, 8, 4), (-2, 5, 7, 3))
    assert rc == hip.OK and count.shape == (3, 3, 7) and not count.any() and not weight.any()       # zeros over the 77 fill
    got = dn.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, 4, 2)
    assert got[2] == (0, 0, 1, 1) and not got[0].any() and got[0].shape == (3, 1, 1)
    case = DC.single_point()
    win, count, weight = DC.single_point_expected()
    _equal(_device(case), (count, weight), 'one point')
    _check(DC.translate(case, 123457, -7891), 'one point off the lattice')


# ---- 11: refused arguments
P3 = (np.array([[0, 0], [3, 4], [6, 0]], np.int32), np.array([0, 1, 2], np.int32))
REFUSED = [(0, 5, 4, (0, 0, 3, 3)), (15, 5, 4, (0, 0, 3, 3)), (3, 0, 4, (0, 0, 3, 3)), (3, 16385, 4, (0, 0, 3, 3)), (3, 5, 0, (0, 0, 3, 3)),
           (3, 5, (1 << 20) + 1, (0, 0, 3, 3)), (3, 5, 4, (0, 0, 0, 3)), (3, 5, 4, (0, 0, 3, 0)), (1, 5, 4, (0, 0, (1 << 24) + 1, 1)),
           (1, 5, 4, (0, 0, 1 << 12, (1 << 12) + 1)), (3, 5, 1 << 20, (256, 0, 1, 1)), (3, 5, 1 << 20, (0, -256, 1, 1)),
           (3, 5, 1 << 20, (254, 0, 3, 1)), (3, 5, 4, (0, (1 << 26) - 2, 2, 3))]


@pytest.mark.parametrize('C, h, s, win', REFUSED)
def test_arguments_out_of_range_are_refused_before_anything_runs(hip_device, C, h, s, win):
    rc, count, weight = _raw(P3 + (C, h, s), win, shape=(3, 3, 3))
    assert rc == hip.E_INVALID and (count == 77).all() and (weight == 77).all()
    with pytest.raises(ValueError):
        dn.check_args(C, h, s, win)


def test_the_last_accepted_site_and_points_outside_the_box(hip_device):
    rc, count, weight = _raw(P3 + (3, 5, 1 << 20), (253, -255, 3, 2))                              # the sites next to +-2**28: accepted, zeros
    assert rc == hip.OK and not count.any() and not weight.any()
    far = (np.array([[0, 0], [1 << 27, 4], [6, 0]], np.int32), P3[1])
    rc, count, weight = _raw(far + (3, 5, 4), (0, 0, 3, 3))                                        # a point at 2**27
    assert rc == hip.E_INVALID and (count == 77).all() and (weight == 77).all()
    out = (np.array([[0, 0], [3, 4], [600, 0]], np.int32), P3[1])
    rc, count, weight = _raw(out + (3, 5, 4), (0, 0, 3, 3), bounds=(0, 0, 10, 10))                 # refused by the binning, outputs untouched
    assert rc == hip.E_INVALID and (count == 77).all() and (weight == 77).all()
    rc, count, weight = _raw(out + (3, 5, 4), (0, 0, 3, 3), bounds=(0, 0, 10, -1))                 # an empty box
    assert rc == hip.E_INVALID and (count == 77).all() and (weight == 77).all()
    rc, count, weight = _raw(out + (3, 5, 4), (0, 0, 3, 3))                                        # (the same points with their own box are fine)
    assert rc == hip.OK
    _equal((count, weight), dn.density_reference(*out, 3, 5, 4, (0, 0, 3, 3)), 'own box')
    assert count[0, 0, 0] == 1 and weight[0, 0, 0] == 25 and count[1, 1, 1] == 1 and weight[1, 1, 1] == 24
    with pytest.raises(ValueError, match='coarsen the pitch'):
        dn.build(np.array([[0, 0], [40000, 40000]], np.int32), [0, 1], 3, 4, 0.5)                  # 80 017 x 80 017 sites
    with pytest.raises(ValueError):
        dn.build(np.array([[0, 0], [1 << 27, 4]], np.int32), [0, 1], 3, 2.5, 2)


# ---- 12: the tool
_run = points_util.run_tool


def test_cli_nuclei_density(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-graph --nuclei-density on the synthetic .npy slide of tests/test_hip_clusters.py, with --merge on one
    rank and on two (three runs of the tool): the folder gains exactly the one file, every other file is the same bytes as without the
    flag, the rows are those of <id>_nuclei_graph.npz, the integers equal density_reference on the file's own xy and label, and every
    derived key equals `derive` of them."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-graph')
    flags = ['--nuclei-density', '--density-bandwidth', '20', '--density-pitch', '7.5']
    files = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d)))}
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    _run(base + flags + ['--save_dir', str(tmp_path / 'merge'), '--merge'], env)
    said = _run(base + flags + ['--save_dir', str(tmp_path / 'two'), '--merge', '--gpus', '2'], two)
    assert 'density' in said and 's1_nuclei_density.npz' in said and 'sites' in said and 'peak' in said
    for run, ref in (('merge', 'merge0'), ('two', 'merge0')):
        with_flag, without = files(run), files(ref)
        assert sorted(with_flag) == sorted(list(without) + ['s1_nuclei_density.npz']), run
        for f in without:
            assert with_flag[f] == without[f], (run, f)
        g = cellgraph.read_npz(str(folder(run) / 's1_nuclei_graph.npz'))
        z = dn.read_npz(str(folder(run) / 's1_nuclei_density.npz'))
        assert tuple(z) == dn.NPZ_KEYS
        n = len(g['nuclei_id'])
        assert n > 10 and np.array_equal(z['nuclei_id'], g['nuclei_id']) and np.array_equal(z['xy'], g['xy']) and np.array_equal(z['label'], g['label'])
        assert float(z['bandwidth_px']) == 20.0 and float(z['pitch_px']) == 7.5
        pts = np.rint(2 * z['xy']).astype(np.int32)
        win = dn.window(cellpoints.bounds_of(pts), 40, 15)
        assert z['window'].tolist() == list(win) and z['origin_px'].tolist() == [win[0] * 7.5, win[1] * 7.5]
        want = dn.density_reference(pts, z['label'], 5, 40, 15, win)
        _equal([z[name] for name in dn.INT_NAMES], want, run)
        d = dn.derive(want[0], want[1], 40)
        for key in dn.DERIVED_KEYS:
            assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype, (run, key)
        print(f"{run}: {n} nuclei, window {win}, class totals {z['class_total'].tolist()}")
        assert int(z['class_total'].sum()) >= n
    zm, zt = dn.read_npz(str(folder('merge') / 's1_nuclei_density.npz')), dn.read_npz(str(folder('two') / 's1_nuclei_density.npz'))
    for key in dn.NPZ_KEYS:
        assert np.array_equal(zm[key], zt[key]), key
