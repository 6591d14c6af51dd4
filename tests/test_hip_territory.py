"""GPU tests of the nucleus territories (csrc/cellterritory.hip, nuhtc_cell_territory): owner, nearest_d2 and every tally must EQUAL
nuhtc_amd.territory.territory_reference, the brute-force int64 restatement of the definition -- same dtype and shape, no tolerance, nothing
left out.  The designed cases of tests/test_territory_host.py (the tie, the inclusive reach, points on sites), sites outside the points'
box on all four sides (as they are, mirrored, at the far corners of the coordinate range), windows that are no multiple of a tile,
sub-windows, a window of many tiles in x, an argmin across staging chunks, labels out of range, a binning over two scan chunks, random sets
full of ties (repeatable, independent of the row order), the edge sizes, the refused arguments, the profile tags, and tools/infer_wsi.py
--nuclei-territory end to end.  The cases lie on both sides of the rule that picks the owner kernel (site_route_staged)."""
import os

import numpy as np
import pytest
import torch

import proximity_cases as PC
import points_util
import territory_cases as TC
from nuhtc_amd import cellgraph, cellpoints, hip
from nuhtc_amd import territory as tr

pytestmark = pytest.mark.gpu
FAR = (((1 << 26) + 12345, -(1 << 26) - 321), (-(1 << 26) - 7, (1 << 26) + 50001))
FILL = 77


def _raw(case, win, bounds=None, shape=None):
    """One call on buffers filled with 77 (of the case's shapes, or of shape = (n, C, H, W) where the arguments describe none) -> (return
    code, the eight outputs in the reference's form)."""
    p, lab, C, r, s = case
    dev = torch.device('cuda', 0)
    p = np.ascontiguousarray(np.asarray(p, np.int32).reshape(-1, 2))
    n, Cs, H, W = (len(p), C, win[3], win[2]) if shape is None else shape
    out = tr.outputs(n, Cs, (0, 0, W, H), dev, fill=FILL)
    rc = tr.call(torch.from_numpy(p).to(dev), torch.from_numpy(np.ascontiguousarray(lab, np.int32)).to(dev), C, r, s, win, *out, bounds=bounds)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in out]
    return rc, got


def _untouched(got):
    return all((g == FILL).all() for g in got)


def _shaped(got):
    """The device's arrays as the reference returns them: open as uint8, free_sites 0-d."""
    return tuple(got[:4]) + (got[4].astype(np.uint8),) + tuple(got[5:7]) + (got[7].reshape(()),)


def _device(case, win=None):
    win = TC.default_window(case) if win is None else win
    rc, got = _raw(case, win)
    assert rc == hip.OK, rc
    return _shaped(got)


def _check(case, what, win=None):
    win = TC.default_window(case) if win is None else win
    got = _device(case, win)
    TC.equal(got, tr.territory_reference(*case, win), what)
    return got


# ---- 1: the designed cases
def test_tie_reach_and_points_on_sites(hip_device):
    for swapped in (False, True):
        case = TC.bisector(swapped)
        win = TC.default_window(case)
        owner = _check(case, f'bisector, swapped {swapped}')[0]
        assert (owner[:, 1 - win[0]][owner[:, 1 - win[0]] >= 0] == 0).all()                # the column x = 4: the smaller row, whichever point it is
    owner, nearest = _check(TC.three_four_five(), '3-4-5', (-5, -5, 11, 11))[:2]
    assert owner[9, 8] == 0 and nearest[9, 8] == 25 and owner[10, 8] == -1 and nearest[10, 8] == -1
    for k, s, m, classes in ((3, 2, 5, 2), (5, 1, 7, 2), (3, 7, 4, 1)):
        case = TC.on_sites(k, s, m, classes)
        got = _check(case, f'on sites {k} {s} {m}', TC.on_sites_window(k, m))
        y, x = np.divmod(np.arange(m * m), m)
        rim = (x == 0) | (x == m - 1) | (y == 0) | (y == m - 1)
        assert (got[2][~rim] == k * k).all() and not got[4][~rim].any() and got[4][rim].all() and int(got[7]) == 0
        _check(case, f'on sites {k} {s} {m}, default window')


# ---- 2: sites outside the box on all four sides
@pytest.mark.parametrize('s', [4, 1])
def test_sites_outside_the_box_on_all_four_sides(hip_device, s):
    case = TC.patch(s)
    win = TC.default_window(case)
    x_min, y_min, x_max, y_max = cellpoints.bounds_of(case[0])
    assert win[0] * s < x_min and win[1] * s < y_min and (win[0] + win[2] - 1) * s > x_max and (win[1] + win[3] - 1) * s > y_max
    got = _check(case, f'patch, s {s}')
    owner = got[0]
    assert (owner[0] >= 0).any() or (owner[-1] >= 0).any() or (owner[:, 0] >= 0).any() or (owner[:, -1] >= 0).any()
    _check(TC.mirror(case), f'patch mirrored, s {s}')
    for dx, dy in FAR:
        _check(TC.translate(case, dx, dy), f'patch moved by ({dx}, {dy}), s {s}')
        _check(TC.translate(TC.mirror(case), dx, dy), f'patch mirrored and moved by ({dx}, {dy}), s {s}')
    assert TC.staged(TC.patch(1)) and not TC.staged(TC.patch(4))                           # one case on each side of the rule


# ---- 3: tiles and windows
@pytest.mark.parametrize('s, shape', [(1, (37, 21)), (1, (70, 50)), (5, (37, 21)), (5, (70, 50))])
def test_windows_that_are_no_multiple_of_a_tile(hip_device, s, shape):
    case = TC.lattice(s)
    full = TC.default_window(case)
    got = _check(case, f'lattice, s {s}, {shape}', (full[0] + 3, full[1] + 2) + shape)
    assert (got[0] >= 0).any() and got[5].sum() > 0


@pytest.mark.parametrize('s', [4, 1])
def test_a_sub_window_is_a_slice_with_tallies_of_its_own(hip_device, s):
    case = TC.patch(s)
    gx0, gy0, W, H = TC.default_window(case)
    full = _device(case)
    sub_win = (gx0 + 5, gy0 + 3, W - 9, H - 7)
    sub = _check(case, 'a sub-window', sub_win)                                            # the tallies equal the reference ON the sub-window
    assert np.array_equal(sub[0], full[0][3:H - 4, 5:W - 4]) and np.array_equal(sub[1], full[1][3:H - 4, 5:W - 4])
    assert not np.array_equal(sub[2], full[2])                                             # a territory is counted as far as the window goes
    got = _check(case, 'half off the points', (gx0 - W // 2, gy0 - H // 2, W, H))
    assert (got[0] >= 0).any() and not (got[0][:H // 2 - 1] >= 0).any()
    for win in ((gx0 + 10000, gy0 - 10000, 40, 23), (gx0 - 10000, gy0, 17, 18), (gx0, gy0 + 10000, 16, 16)):
        got = _check(case, f'nowhere near: {win}', win)
        assert (got[0] == -1).all() and int(got[7]) == win[2] * win[3] and not got[2].any()
    _check(case, 'one site', (gx0 + W // 2, gy0 + H // 2, 1, 1))
    _check(case, 'one column', (gx0 + W // 2, gy0, 1, H))


def test_a_window_of_70000_by_3_sites(hip_device):
    p, lab, C, r, s = TC.patch(1)
    case = (np.concatenate([p, p + [69000, 0]]).astype(np.int32), np.concatenate([lab, lab]), C, r, s)     # a patch at either end of it
    got = _check(case, '70000 x 3', (-500, 30, 70000, 3))
    assert (got[0][:, :600] >= 0).any() and (got[0][:, 69400:] >= 40).any() and int(got[7]) > 200000


# ---- 4: the argmin across staging chunks
@pytest.mark.parametrize('s', [16384, 2048])
def test_1500_coincident_points_belong_to_the_smallest_row(hip_device, s):
    p, lab, C, r, _ = TC.coincident(s)
    lab = np.zeros(1500, np.int32)
    lab[:7] = 3                                                                           # rows 0 .. 6 do not compete: row 7 is the smallest that does
    case = (p, lab, 1, r, s)
    got = _check(case, f'coincident, s {s}')
    assert set(np.unique(got[0]).tolist()) <= {-1, 7} and got[2][7] == got[2].sum() > 0 and (got[1].max() <= 1 << 28)
    order = np.random.default_rng(3).permutation(1500)
    got = _check((p, lab[order], 1, r, s), f'coincident and permuted, s {s}')
    assert set(np.unique(got[0]).tolist()) <= {-1, int(np.flatnonzero(lab[order] == 0)[0])}


@pytest.mark.parametrize('r', [8, 3])
def test_1500_points_in_two_cells(hip_device, r):
    case = TC.crowded(r)
    got = _check(case, f'crowded, R {r}')
    p = case[0]
    first = sorted({int(np.flatnonzero((p == q).all(1))[0]) for q in np.unique(p, axis=0)})   # the smallest row of each of the nine places
    assert sorted(np.unique(got[0][got[0] >= 0]).tolist()) == first and len(first) == 9


# ---- 5: labels
def test_labels_out_of_range_neither_own_nor_block(hip_device):
    case = TC.labels_out_of_range()
    p, lab, C, r, s = case
    assert set(lab.tolist()) == {-1, 0, 1, 2, 3, 14}
    got = _check(case, 'labels')
    keep = np.flatnonzero((lab >= 0) & (lab < C))
    alone = _device((p[keep], lab[keep], C, r, s), TC.default_window(case))                # as if the others were absent
    assert np.array_equal(np.where(alone[0] >= 0, keep[np.maximum(alone[0], 0)], -1), got[0]) and np.array_equal(alone[1], got[1])
    assert not got[2][(lab < 0) | (lab >= C)].any() and np.array_equal(alone[5], got[5]) and (got[0] >= 0).any()


# ---- 6: a binning over two scan chunks
def test_chain_of_20000_points_over_two_scan_chunks(hip_device):
    """The chain of tests/proximity_cases.py, 8 half pixels between neighbours on the line y = 11, with R = 8: 20 000 cells of side 8, more
    than one scan chunk of 16 384.  Pitch 18 puts one row of 8 890 sites on y = 18, 7 beside the line."""
    p, lab = PC.chain('shuffled')[:2]
    case = (p, lab, 2, 8, 18)
    win = TC.default_window(case)
    assert win[3] == 1 and 8000 < win[2] < 200000 and (p[:, 0].max() - p[:, 0].min()) // 8 + 1 > 16384
    got = _check(case, 'chain')
    assert (got[0] >= 0).sum() > 2000


# ---- 7: random sets full of ties
@pytest.mark.parametrize('seed', [0, 1])
def test_random_sets_on_a_coarse_grid(hip_device, seed):
    case = TC.ties(seed)
    p, lab, C, r, s = case
    a, b = _device(case), _device(case)
    TC.equal(a, tr.territory_reference(*case, TC.default_window(case)), f'ties {seed}')
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert len(np.unique(p, axis=0)) < len(p) and (a[0] >= 0).any() and (a[0] == -1).any()
    order = np.random.default_rng(4).permutation(len(p))
    _check((p[order], lab[order], C, r, s), 'permuted rows')                               # the owners change with the rows: against the reference on them


@pytest.mark.parametrize('kind', ['uniform', 'clumps'])
@pytest.mark.parametrize('r, s', TC.LARGE_RS)
def test_3000_random_points(hip_device, kind, r, s):
    p, lab = TC.random_large(kind)
    case = (p, lab, 5, r, s)
    got = _check(case, f'{kind}, R {r}, s {s}')
    tallies, win, maps = tr.build(p, lab, 5, r / 2, s / 2, maps=True)
    TC.equal(tuple(maps) + tuple(tallies), got, 'build')
    assert win == TC.default_window(case) and tr.build(p, lab, 5, r / 2, s / 2)[2] is None
    assert TC.staged(case) == (15 * s <= 3 * r)


# ---- 8: edge sizes
def test_no_points_and_one_point(hip_device):
    rc, got = _raw((np.zeros((0, 2)), np.zeros(0), 3, 8, 4), (-2, 5, 7, 3))
    assert rc == hip.OK
    TC.equal(_shaped(got), tr.territory_reference(np.zeros((0, 2)), [], 3, 8, 4, (-2, 5, 7, 3)), 'no points')
    assert (got[0] == -1).all() and (got[1] == -1).all() and not got[5].any() and not got[6].any() and got[7].tolist() == [21]
    tallies, win, maps = tr.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, 4, 2, maps=True)
    assert win == (0, 0, 1, 1) and maps[0].tolist() == [[-1]] and int(tallies[5]) == 1 and tallies[0].shape == (0,)
    case = TC.single_point()
    win, count, weight = TC.single_point_expected()
    got = _check(case, 'one point', win)
    assert np.array_equal(got[0], count[0] - 1) and got[4].tolist() == [1]
    _check(TC.translate(case, 123457, -7891), 'one point off the lattice')


# ---- 9: refused arguments
P3 = (np.array([[0, 0], [3, 4], [6, 0]], np.int32), np.array([0, 1, 2], np.int32))
REFUSED = [(0, 5, 4, (0, 0, 3, 3)), (15, 5, 4, (0, 0, 3, 3)), (3, 0, 4, (0, 0, 3, 3)), (3, 16385, 4, (0, 0, 3, 3)), (3, 5, 0, (0, 0, 3, 3)),
           (3, 5, (1 << 20) + 1, (0, 0, 3, 3)), (3, 5, 4, (0, 0, 0, 3)), (3, 5, 4, (0, 0, 3, 0)), (1, 5, 4, (0, 0, (1 << 28) + 1, 1)),
           (1, 5, 4, (0, 0, 1 << 14, (1 << 14) + 1)), (3, 5, 1 << 20, (256, 0, 1, 1)), (3, 5, 1 << 20, (0, -256, 1, 1)),
           (3, 5, 1 << 20, (254, 0, 3, 1)), (3, 5, 4, (0, (1 << 26) - 2, 2, 3))]


@pytest.mark.parametrize('C, r, s, win', REFUSED)
def test_arguments_out_of_range_are_refused_before_anything_runs(hip_device, C, r, s, win):
    rc, got = _raw(P3 + (C, r, s), win, shape=(3, 3, 3, 3))
    assert rc == hip.E_INVALID and _untouched(got)
    with pytest.raises(ValueError):
        tr.check_args(C, r, s, win)


def test_the_last_accepted_site_and_points_outside_the_box(hip_device):
    rc, got = _raw(P3 + (3, 5, 1 << 20), (253, -255, 3, 2))                                # the sites next to +-2**28: accepted, nobody's
    assert rc == hip.OK and (got[0] == -1).all() and got[7].tolist() == [6] and not got[2].any()
    far = (np.array([[0, 0], [1 << 27, 4], [6, 0]], np.int32), P3[1])
    rc, got = _raw(far + (3, 5, 4), (0, 0, 3, 3))                                          # a point at 2**27
    assert rc == hip.E_INVALID and _untouched(got)
    out = (np.array([[0, 0], [3, 4], [600, 0]], np.int32), P3[1])
    rc, got = _raw(out + (3, 5, 4), (0, 0, 3, 3), bounds=(0, 0, 10, 10))                   # refused by the binning, outputs untouched
    assert rc == hip.E_INVALID and _untouched(got)
    rc, got = _raw(out + (3, 5, 4), (0, 0, 3, 3), bounds=(0, 0, 10, -1))                   # an empty box
    assert rc == hip.E_INVALID and _untouched(got)
    rc, got = _raw(out + (3, 5, 4), (0, 0, 3, 3))                                          # (the same points with their own box are fine)
    assert rc == hip.OK
    TC.equal(_shaped(got), tr.territory_reference(*out, 3, 5, 4, (0, 0, 3, 3)), 'own box')
    assert got[0].tolist() == [[0, 0, -1], [1, 1, 1], [1, 1, -1]]
    with pytest.raises(ValueError, match='coarsen the pitch'):
        tr.build(np.array([[0, 0], [40000, 40000]], np.int32), [0, 1], 3, 4, 0.5)          # 40 017 x 40 017 sites
    with pytest.raises(ValueError):
        tr.build(np.array([[0, 0], [1 << 27, 4]], np.int32), [0, 1], 3, 2.5, 2)


# ---- 10: the profile
def test_profile_tags_of_one_call(hip_device):
    for case in (TC.patch(1), TC.patch(4), TC.crowded(8), TC.crowded(3)):                  # both owner kernels: one tag for the stage
        hip.profile_enable(True)
        try:
            _device(case)
            tags = {tag for tag in hip.profile_read() if tag.startswith('cell_territory')}
        finally:
            hip.profile_enable(False)
        assert tags == {'cell_territory_bin', 'cell_territory_owner', 'cell_territory_tally'}, (case[3:], tags)


# ---- 11: the tool
_run = points_util.run_tool


def test_cli_nuclei_territory(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-graph --nuclei-territory on the synthetic .npy slide of tests/points_util.py, with --merge: without the
    flag, with it, and with --territory-maps on two ranks (three runs of the tool).  The folder gains exactly the one file, every other
    file is the same bytes as without the flag, the rows are those of <id>_nuclei_graph.npz, every integer equals territory_reference on
    the file's own xy and label, every derived key equals `derive` of them, and the closing clause ends with the file's name."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-graph')
    flags = ['--nuclei-territory', '--territory-reach', '20', '--territory-pitch', '2.5']
    files = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d)))}
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    said = {'merge': _run(base + flags + ['--save_dir', str(tmp_path / 'merge'), '--merge'], env),
            'maps': _run(base + flags + ['--territory-maps', '--save_dir', str(tmp_path / 'maps'), '--merge', '--gpus', '2'], two)}
    z = {}
    for run in ('merge', 'maps'):
        assert 'territories of' in said[run] and 'closed, median area' in said[run] and 'largest area share' in said[run]
        assert ' of the owned sites) in s1_nuclei_territory.npz' in said[run], said[run][-400:]
        with_flag, without = files(run), files('merge0')
        assert sorted(with_flag) == sorted(list(without) + ['s1_nuclei_territory.npz']), run
        for f in without:
            assert with_flag[f] == without[f], (run, f)
        g = cellgraph.read_npz(str(folder(run) / 's1_nuclei_graph.npz'))
        z[run] = tr.read_npz(str(folder(run) / 's1_nuclei_territory.npz'))
        assert tuple(z[run]) == tr.NPZ_KEYS + (tr.MAP_NAMES if run == 'maps' else ())
        n = len(g['nuclei_id'])
        assert n > 10 and all(np.array_equal(z[run][k], g[k]) for k in ('nuclei_id', 'xy', 'label'))
        assert float(z[run]['reach_px']) == 20.0 and float(z[run]['pitch_px']) == 2.5
        pts = np.rint(2 * z[run]['xy']).astype(np.int32)
        win = tr.window(cellpoints.bounds_of(pts), 40, 5)
        assert z[run]['window'].tolist() == list(win) and z[run]['origin_px'].tolist() == [win[0] * 2.5, win[1] * 2.5]
        want = tr.territory_reference(pts, z[run]['label'], 5, 40, 5, win)
        TC.equal([want[i] if name in tr.MAP_NAMES and run != 'maps' else z[run][name] for i, name in enumerate(TC.NAMES)], want, run)
        d = tr.derive(want[2], want[4], want[5], want[6], want[7], z[run]['label'], 5)
        for key in tr.DERIVED_KEYS:
            assert np.array_equal(z[run][key], d[key]) and z[run][key].dtype == d[key].dtype, (run, key)
        print(f"{run}: {n} nuclei, window {win}, class sites {z[run]['class_sites'].tolist()}, free {int(z[run]['free_sites'])}, closed {int(z[run]['closed'].sum())}")
        assert int(z[run]['class_sites'].sum()) > n
    for key in tr.NPZ_KEYS:
        assert np.array_equal(z['merge'][key], z['maps'][key]), key
