"""GPU tests of the alpha-shape outline (csrc/celloutline.hip, nuhtc_alpha_outline): ring_vertex, ring_start, ring_area2,
component_of_ring, component, component_label and the counts h, R, K must EQUAL nuhtc_amd.outline.outline_reference, the plain walk in
Python integers -- same dtype and shape, no tolerance, nothing left out.  The reference walks the alpha complex the device computed in
the same `build` (tests/test_hip_alpha.py holds that against its own restatement); the designed sets also go against the restatement's
complex.  A strip of 20 000 points that is ONE ring of 20 000 half-edges in three row orders (15 doubling rounds), a ring of 16 385
half-edges (one past a scan chunk), 5000 separate triangles (the numbering scans), the designed sets of tests/outline_cases.py as they
are and moved to a corner of the coordinate range, random sets full of ties twice for bitwise repeatability and with permuted rows, the
refused arguments with untouched outputs, the device region census on the written GeoJSON, the profile tags, and tools/infer_wsi.py
--nuclei-outline end to end on one and two ranks."""
import ctypes
import os

import numpy as np
import pytest
import torch

import outline_cases as OC
import points_util
from nuhtc_amd import alphacomplex as ax
from nuhtc_amd import cellgraph, hip, regions
from nuhtc_amd import outline as ol

pytestmark = pytest.mark.gpu
FILL = 77


def _build(case):
    """-> (the nine results of the device, the alpha complex the device walked)."""
    p, lab, C, r, by = case
    got = ol.build(p, lab, C, r / 2, by, with_alpha=True)
    return got[:9], got[9:]


def _against_own_complex(case, what):
    got, alpha = _build(case)
    OC.equal(got, OC.reference(case, alpha), what)
    return got, alpha


# ---- 1: long rings, a ring past a scan chunk, many rings
@pytest.mark.parametrize('order', ['ascending', 'descending', 'shuffled'])
def test_strip_of_20000_points_is_one_ring(hip_device, order):
    case = OC.strip(20000, order)
    got, alpha = _against_own_complex(case, f'strip, {order}')
    assert got[6:] == (20000, 1, 1) and got[1].tolist() == [0, 20000] and (got[4] == 0).all()
    assert int(got[2][0]) == 2 * 9999 * 10 * 8                                 # 19 998 triangles of base 10 and height 8
    assert ol.half_edges(*alpha[:3], 20000)[0].size == 20000 and (1 << 14) < 20000 <= (1 << 15)   # 15 doubling rounds


def test_ring_of_16385_half_edges(hip_device):
    got, _ = _against_own_complex(OC.strip(16385), 'strip of 16385')
    assert got[6:] == (16385, 1, 1)


def test_5000_separate_triangles(hip_device):
    case = OC.many_triangles(5000)
    got, _ = _against_own_complex(case, '5000 triangles')
    assert got[6:] == (15000, 5000, 5000) and (got[2] == 64).all() and np.array_equal(got[3], np.arange(5000)) and np.array_equal(got[4], np.arange(15000) // 3)
    by_class = case[:4] + (1,)
    got, _ = _against_own_complex(by_class, '5000 triangles by class')
    assert np.array_equal(got[5], np.arange(5000) % 3)


# ---- 2: the designed sets, against the restatement's complex, as they are and moved to the far corner of the coordinate range
@pytest.fixture(scope='module')
def small_references():
    return {name: OC.reference(case) for name, case in OC.small_cases().items()}


@pytest.mark.parametrize('name', sorted(OC.small_cases()))
def test_designed_sets_and_the_same_sets_translated(hip_device, small_references, name):
    case, want = OC.small_cases()[name], small_references[name]
    OC.equal(_build(case)[0], want, name)
    if len(case[0]):
        dx, dy = -(1 << 27) + 1 - int(case[0][:, 0].min()), (1 << 27) - 1 - int(case[0][:, 1].max())
        moved = (case[0] + np.array([dx, dy], np.int32),) + case[1:]
        OC.equal(_build(moved)[0], want, f'{name} moved by ({dx}, {dy})')
    if name in OC.SHAPES:
        assert (want[7], int((want[2] < 0).sum()), want[8]) == OC.SHAPES[name]
    if name in OC.HAND_WRITTEN:
        OC.equal(_build(case)[0], OC.HAND_WRITTEN[name], name + ' (hand-written)')


# ---- 3: random sets full of ties: twice, and with permuted rows
@pytest.mark.parametrize('by, r', [(0, 4), (1, 4), (0, 5), (1, 2)])
def test_coarse_lattice_twice_and_with_permuted_rows(hip_device, by, r):
    case = OC.coarse(by, 600, 41, r, seed=12 + r)
    a, alpha = _against_own_complex(case, f'coarse, by_class {by}, r {r}')
    b, _ = _build(case)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:6], b[:6])) and a[6:] == b[6:]
    OC.equal(a, OC.reference(case), f'coarse, by_class {by}, r {r} (the restatement\'s complex)')
    _against_own_complex(OC.permuted(case), f'coarse, by_class {by}, r {r}, permuted rows')
    rep = ol.representatives(len(case[0]), alpha[0], alpha[1])
    print(f'coarse by {by} r {r}: {a[6]} half-edges, {a[7]} rings, {int((a[2] < 0).sum())} holes, {a[8]} components, {int((rep != np.arange(len(rep))).sum())} rows set aside')


def test_3000_random_points_in_clumps(hip_device):
    rng = np.random.default_rng(2026)
    centres = rng.integers(40, 360, (12, 2))
    p = np.rint(centres[rng.integers(0, 12, 3000)] + rng.normal(0, 14, (3000, 2))).astype(np.int32)
    for by in (0, 1):
        got, _ = _against_own_complex((p, rng.integers(0, 3, 3000).astype(np.int32), 3, 6, by), f'clumps, by_class {by}')
        assert got[7] > 10
        print(f'clumps by {by}: {got[6]} half-edges, {got[7]} rings, {int((got[2] < 0).sum())} holes, {got[8]} components')


# ---- 4: refused arguments
def _raw(case, alpha, m=None, by=None, edit=None):
    """nuhtc_alpha_outline on tensors of the case and its complex, the outputs filled with FILL -> (rc, counts, outputs as numpy)."""
    dev = torch.device('cuda', 0)
    p, lab = torch.from_numpy(case[0]).to(dev), torch.from_numpy(case[1]).to(dev)
    e, d2, ap = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in alpha[:3])
    if edit:
        edit(p, e, d2, ap)
    out = ol.outputs(len(case[0]), len(alpha[0]), dev, fill=FILL)
    rc, h, R, K = ol.call(p, lab, case[4] if by is None else by, e, d2, ap, len(alpha[0]) if m is None else m, *out)
    torch.cuda.synchronize()
    return rc, (h, R, K), [o.cpu().numpy() for o in out]


def _untouched(arrays):
    return all((a == FILL).all() for a in arrays)


def test_refused_arguments_leave_the_outputs_untouched(hip_device):
    case = OC.annulus()
    alpha = ax.alpha_reference(*case)
    rc, counts, out = _raw(case, alpha)
    assert rc == hip.OK and counts == (20, 2, 1) and _untouched([out[0][20:], out[1][3:], out[2][2:], out[3][2:], out[5][1:]])
    for what, kw in (('m < 0', dict(m=-1)), ('m > 2**24', dict(m=(1 << 24) + 1)), ('by_class 2', dict(by=2))):
        rc, counts, out = _raw(case, alpha, **kw)
        assert rc == hip.E_INVALID and counts == (None, None, None) and _untouched(out), what
    m = len(alpha[0])

    def row_out_of_range(p, e, d2, ap): e[m // 2, 1] = len(case[0])
    def negative_row(p, e, d2, ap): e[3, 0] = -1
    def apex_out_of_range(p, e, d2, ap): ap[5, 0] = len(case[0])
    def apex_below(p, e, d2, ap): ap[5, 1] = -2
    def apex_on_the_wrong_side(p, e, d2, ap): ap[0] = ap[0].flip(0)
    def not_ascending(p, e, d2, ap): e[[4, 5]] = e[[5, 4]]
    def point_out_of_range(p, e, d2, ap): p[0, 0] = 1 << 27
    for edit in (row_out_of_range, negative_row, apex_out_of_range, apex_below, apex_on_the_wrong_side, not_ascending, point_out_of_range):
        rc, counts, out = _raw(case, alpha, edit=edit)
        assert rc == hip.E_INVALID and counts == (None, None, None) and _untouched(out), edit.__name__
    assert (alpha[2][0] >= 0).sum() == 1                                       # (edge 0 has one apex: flipped, it lies on the wrong side)


def test_null_pointers_are_refused(hip_device):
    case = OC.triangle()
    alpha = ax.alpha_reference(*case)
    dev = torch.device('cuda', 0)
    tensors = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (case[0], case[1]) + tuple(alpha[:3])]
    out = ol.outputs(3, 3, dev, fill=FILL)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    ptrs = [vp(t) for t in tensors] + [vp(t) for t in out]
    counts = (ctypes.c_int64 * 3)(-7, -7, -7)
    fn = hip.load().nuhtc_alpha_outline
    call = lambda q, c: fn(0, q[0], q[1], 3, 0, q[2], q[3], q[4], 3, q[5], q[6], q[7], q[8], q[9], q[10], c, None)
    for k in range(11):
        assert call(ptrs[:k] + [None] + ptrs[k + 1:], counts) == hip.E_INVALID, k
    assert call(ptrs, None) == hip.E_INVALID
    torch.cuda.synchronize()
    assert list(counts) == [-7, -7, -7] and all((t == FILL).all().item() for t in out)
    assert call(ptrs, counts) == hip.OK and list(counts) == [3, 1, 1]
    torch.cuda.synchronize()
    assert out[0].tolist() == [0, 1, 2] and out[1].tolist() == [0, 3, FILL, FILL] and out[2].tolist() == [64, FILL, FILL]


def test_no_points_and_no_edges(hip_device):
    got = ol.build(np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 3, 4)
    OC.equal(got, OC.reference(OC.small_cases()['none']), 'n = 0')
    got = ol.build(np.array([[0, 0], [900, 0], [0, 900]], np.int32), [0, 1, 2], 3, 4)
    assert got[4].tolist() == [-1, -1, -1] and got[1].tolist() == [0] and got[6:] == (0, 0, 0)
    with pytest.raises(ValueError):
        ol.build(np.array([[0, 0], [3, 4]], np.int32), [0, 1], 3, 256.5)


# ---- 5: the written GeoJSON through the device region census
@pytest.mark.parametrize('name', ['island', 'pinched', 'bow_tie', 'scattered', 'coarse_any'])
def test_the_written_geojson_through_the_region_census(hip_device, tmp_path, name):
    """Every row lies inside or on the boundary of some written polygon exactly when it is in a component (by_class 0: no row of another
    label can lie inside a triangle)."""
    case = OC.small_cases()[name]
    p, lab, C, r, by = case
    got, _ = _build(case)
    path = str(tmp_path / 's_nuclei_outline.npz')
    ol.write_npz(path, np.arange(len(p)), p / 2.0, lab, *got[:6], C, r / 2, by, min_nuclei=0)
    table = regions.read_geojson(ol.geojson_path(path))
    assert len(table.names) == got[8] and table.names.tolist() == [f'alpha-{k}' for k in range(got[8])] and table.skipped == 0
    region, depth, on, census = regions.build(p, lab, C, table.edges, table.edge_region, len(table.names))
    assert np.array_equal((depth > 0) | (on > 0), got[4] >= 0), name
    signed = np.zeros(got[8], np.int64)
    np.add.at(signed, got[3], got[2])
    assert np.array_equal(table.area2, signed)                                # the file states the area of the material


# ---- 6: the profile
def test_profile_tags_of_one_call(hip_device):
    hip.profile_enable(True)
    try:
        got, _ = _build(OC.annulus())
        tags = {tag for tag in hip.profile_read() if tag.startswith('cell_outline')}
    finally:
        hip.profile_enable(False)
    assert got[6:] == (20, 2, 1) and tags == {'cell_outline_mark', 'cell_outline_link', 'cell_outline_rank', 'cell_outline_place', 'cell_outline_components'}, tags


# ---- 7: the tool
_run = points_util.run_tool


def test_cli_nuclei_outline(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-graph --nuclei-outline on the synthetic .npy slide of tests/points_util.py, with --merge: without the flag,
    with it, and with it on two ranks (three runs of the tool).  The folder gains exactly the two files, every other file is the same bytes
    as without the flag, the rows are those of <id>_nuclei_graph.npz, every integer equals `build` and the walk on the restatement's complex
    of the file's own xy and label, every derived key equals `derive` of them, the GeoJSON holds the components of three nuclei or more,
    and the closing clause ends with the file's name."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-graph')
    flags = ['--nuclei-outline', '--outline-radius', '32', '--outline-by', 'any']
    files = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d)))}
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    said = {'one': _run(base + flags + ['--save_dir', str(tmp_path / 'one'), '--merge'], env),
            'two': _run(base + flags + ['--save_dir', str(tmp_path / 'two'), '--merge', '--gpus', '2'], two)}
    z = {}
    for run in ('one', 'two'):
        assert 'alpha-shape components in' in said[run] and 'in s1_nuclei_outline.npz' in said[run] and '(32 px radius, by any;' in said[run], said[run][-400:]
        with_flag, without = files(run), files('merge0')
        assert sorted(with_flag) == sorted(list(without) + ['s1_nuclei_outline.npz', 's1_nuclei_outline.geojson']), run
        for f in without:
            assert with_flag[f] == without[f], (run, f)
        g = cellgraph.read_npz(str(folder(run) / 's1_nuclei_graph.npz'))
        z[run] = ol.read_npz(str(folder(run) / 's1_nuclei_outline.npz'))
        assert tuple(z[run]) == ol.NPZ_KEYS
        n = len(g['nuclei_id'])
        assert n > 10 and all(np.array_equal(z[run][k], g[k]) for k in ('nuclei_id', 'xy', 'label'))
        assert float(z[run]['radius_px']) == 32.0 and int(z[run]['by_class']) == 0
        pts = np.rint(2 * z[run]['xy']).astype(np.int32)
        case = (pts, z[run]['label'].astype(np.int32), 5, 64, 0)
        want = OC.reference(case)
        OC.equal(ol.build(pts, z[run]['label'], 5, 32.0, 0), want, run + ': build')
        OC.equal([z[run][name] for name in ol.INT_NAMES] + [len(z[run]['ring_vertex']), int(z[run]['n_rings']), int(z[run]['n_components'])], want, run)
        d = ol.derive(*want[:6], pts, z[run]['label'], 5)
        for key in ol.DERIVED_KEYS:
            assert np.array_equal(z[run][key], d[key]) and z[run][key].dtype == d[key].dtype, (run, key)
        table = regions.read_geojson(str(folder(run) / 's1_nuclei_outline.geojson'))
        assert table.names.tolist() == [f'alpha-{k}' for k in range(want[8]) if d['n_nuclei'][k] >= 3]
        print(f"{run}: {n} nuclei, {want[6]} half-edges, {want[7]} rings, {want[8]} components")
        assert want[8] >= 1
    for key in ol.NPZ_KEYS:
        assert np.array_equal(z['one'][key], z['two'][key]), key
    assert open(folder('one') / 's1_nuclei_outline.geojson', 'rb').read() == open(folder('two') / 's1_nuclei_outline.geojson', 'rb').read()
