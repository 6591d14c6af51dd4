"""GPU tests of the margin bands (csrc/cellmargin.hip, nuhtc_cell_margin): band_census, census, band, band_region and band_inside must
EQUAL nuhtc_amd.margin.margin_reference, the brute-force restatement of the definition -- same dtype and shape, no tolerance, nothing left
out.  Every designed set of tests/margin_cases.py through `build`, each at three slab heights (1 and 16384 among them) with identical
outputs, two calls bitwise equal, permuted rows, the second-call path, the refused arguments with the outputs untouched, the census
against regions.build, and tools/infer_wsi.py --nuclei-margin end to end."""
import json
import os

import numpy as np
import pytest
import torch

import margin_cases as MC
import points_util
from nuhtc_amd import cellgraph, cellpoints, hip
from nuhtc_amd import margin as mg
from nuhtc_amd import regions as rg

pytestmark = pytest.mark.gpu
CASES = MC.all_cases()
SLABS = (1, 7, 16384)


def _equal(got, want, what):
    for name, g, w in zip(mg.INT_NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, f'{len(bad)} entries differ, first at {bad[0].tolist()}', int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


@pytest.fixture(scope='module')
def references():
    return {name: mg.margin_reference(*case) for name, case in CASES.items()}


def _raw(case, slab, slot_cap, fill=77, bounds=None, thresholds=None):
    """One call on buffers filled with `fill` -> (return code, M, the five outputs as numpy, whole buffers)."""
    p, lab, C, edges, er, G, thr = case
    dev = torch.device('cuda', 0)
    up = lambda a, rows: torch.from_numpy(np.ascontiguousarray(a) if len(a) else np.zeros(rows, a.dtype)).to(dev)[:len(a)]
    out = mg.outputs(len(p), G, C, len(thr), dev, fill=fill)
    rc, m = mg.call(up(p, (1, 2)), up(lab, 1), C, up(edges, (1, 4)), up(er, 1), G, thr if thresholds is None else thresholds, slab, slot_cap, *out, bounds=bounds)
    torch.cuda.synchronize()
    return rc, m, [t.cpu().numpy() for t in out]


# ---- 1: every designed set equals the restatement, at every slab height, twice
@pytest.mark.parametrize('name', sorted(CASES))
def test_every_case_equals_the_reference_at_three_slab_heights(hip_device, references, name):
    case, want = CASES[name], references[name]
    first = None
    for slab in SLABS:
        got = mg.build(*case, slab=slab, with_calls=True)
        assert got[5] == 1, (name, slab, 'the host states the records exactly: one call')
        _equal(got[:5], want, f'{name}, slab {slab}')
        again = mg.build(*case, slab=slab)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:5], again)), (name, slab, 'two calls differ')
        first = got if first is None else first
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:5], first[:5])), (name, slab, 'the outputs depend on the slab')
    _equal(mg.build(*case), want, f'{name}, the slab of choose_slab')
    if len(case[0]):
        shuffled, order = MC.permuted(case)
        got = mg.build(*shuffled)
        _equal(got, want[:2] + tuple(w[order] for w in want[2:]), f'{name}, permuted rows')


def test_the_designed_sets_reach_what_they_are_for(hip_device, references):
    p, lab, C, edges, er, G, thr = CASES['staging']
    bounds = cellpoints.bounds_of(p)
    assert mg.slots_needed(edges, bounds, 16384, thr) == len(edges) and (er == 0).sum() == 256       # one slab, every edge once: region 0 ends with the first pass
    assert len(edges) > 3 * 256 and len(p) > 2 * 256 and mg.slots_needed(edges, bounds, 1, thr) > 2 * 2001
    assert np.bincount(p[:, 1] - bounds[1]).max() >= 600                                           # a slab row fuller than a workgroup at slab 1
    bc, census, band, band_region, band_inside = references['staging']
    assert bc[0].any() and bc[1].any() and bc[:, 0].any() and bc[:, 1].any() and (band == len(thr)).any() and census[3].sum() == ((lab >= 0) & (lab < C)).sum()
    p, lab, C, edges, er, G, thr = CASES['empty_slab']
    rows = (p[:, 1] - p[:, 1].min()) // 7
    ylo, yhi = np.minimum(edges[:, 1], edges[:, 3]) - 20, np.maximum(edges[:, 1], edges[:, 3]) + 20
    bare = [r for r in np.unique(rows) if not ((yhi >= p[:, 1].min() + 7 * r) & (ylo <= p[:, 1].min() + 7 * r + 6)).any()]
    assert len(bare) >= 1                                                                          # slabs with points and no record
    bc = references['around_the_box'][0]
    assert bc[:4].any(axis=(1, 2, 3)).all() and not bc[4:8].any() and not bc[8].any() and references['around_the_box'][1][8].sum() == len(CASES['around_the_box'][0])
    assert len(CASES['pythagorean_5'][6]) == 32 and np.array_equal(references['pythagorean_169'][2], MC.pythagorean(MC.TRIPLES[1])[1])
    case = CASES['shared_edge']
    on = np.flatnonzero((case[0][:, 0] == 12) & (case[0][:, 1] >= 0) & (case[0][:, 1] < 8))
    got = [mg.build(case[0][on], case[1][on], 1, case[3][case[4] == g], np.zeros(4, np.int32), 1, case[6]) for g in (0, 1)]
    assert all((q[2] == 0).all() for q in got) and (got[0][4].astype(int) + got[1][4] == 1).all()    # band 0 of both, inside exactly one


def test_the_slab_walk_case_equals_the_reference(hip_device):
    """`margin_cases.slab_walk` at its one slab height: a first workgroup whose records lie in three slabs, the middle one without an edge
    record, a partial second workgroup, region changes at record 256 of a slab (between two staging passes) and inside its last, partial
    pass, and a region behind both that is kept for the parity and never near (tests/test_margin_host.py checks that layout).  Every
    output equals the restatement."""
    case = MC.slab_walk()
    got = mg.build(*case, slab=MC.SLAB_WALK_SLAB, with_calls=True)
    assert got[5] == 1
    _equal(got[:5], mg.margin_reference(*case), 'slab_walk')


def test_census_equals_the_region_census_of_the_device(hip_device):
    for name in ('staging', 'holes_and_nested', 'random_lattice_1', 'around_the_box'):
        case = CASES[name]
        assert np.array_equal(mg.build(*case)[1], rg.build(*case[:6])[3]), name


# ---- 2: the second call
def test_a_cap_below_the_records_writes_nothing_and_the_second_call_has_room(hip_device, references):
    case = CASES['staging']
    need = mg.slots_needed(case[3], cellpoints.bounds_of(case[0]), 7, case[6])
    for cap in (0, need - 1):
        rc, m, out = _raw(case, 7, cap)
        assert rc == hip.OK and m == need and all((a == 77).all() for a in out), cap               # M is reported, the outputs are untouched
    rc, m, out = _raw(case, 7, need)
    assert rc == hip.OK and m == need
    _equal(out, references['staging'], 'exactly enough room')
    _equal(_raw(case, 7, need + 1000)[2], references['staging'], 'more room than needed')
    got = mg.build(*case, slab=7, slot_cap=3, with_calls=True)
    assert got[5] == 2
    _equal(got[:5], references['staging'], 'build with too small a first cap')


# ---- 3: refused arguments, outputs untouched
def _refused(case, slab=4, cap=20000, bounds=None, thresholds=None):
    rc, m, out = _raw(case, slab, cap, bounds=bounds, thresholds=thresholds)
    assert rc == hip.E_INVALID and m is None and all((a == 77).all() for a in out)


def test_refused_arguments_leave_the_outputs_untouched(hip_device):
    p, lab, C, edges, er, G, thr = CASES['around_the_box']
    ok = (p, lab, C, edges, er, G, thr)
    far = edges.copy()
    far[5, 2] = 1 << 27
    _refused((p, lab, C, far, er, G, thr))                                                         # a vertex outside the range
    far[5, 2] = -(1 << 27)
    _refused((p, lab, C, far, er, G, thr))
    down = er.copy()
    down[6] = 0
    _refused((p, lab, C, edges, down, G, thr))                                                     # edge_region decreasing
    _refused((p, lab, C, edges, er, G - 1, thr))                                                   # a region outside 0 .. G - 1
    _refused((p, lab, C, edges, er - 1, G, thr))
    _refused((p, lab, C, edges, er, (1 << 16) + 1, thr))                                           # G above its limit
    _refused((p, lab, C, edges, er, 0, thr))
    _refused((p, lab, 0, edges, er, G, thr))
    _refused((p, lab, 15, edges, er, G, thr))
    for slab in (0, 16385):
        _refused(ok, slab=slab)
    _refused(ok, cap=-1)
    _refused(ok, cap=(1 << 28) + 1)
    _refused(ok, bounds=(0, 0, 10, 10))                                                            # a point outside the stated box
    _refused(ok, bounds=(0, 0, 10, -1))
    for row in ((5, 5, 20), (5, 4, 20), (0, 5, 20), (-1, 5, 20), (5, 10, 16385)):                  # not increasing, outside 1 .. 16384
        _refused(ok, thresholds=row)
    _refused((p, lab, C, edges, er, G, np.arange(1, 34, dtype=np.int32)))                          # B == 33
    _refused((p, lab, C, edges, er, G, np.zeros(0, np.int32)))                                     # B == 0
    _refused((np.zeros((0, 2), np.int32), np.zeros(0, np.int32), C, far, er, G, thr))              # no points: the edges are still checked
    rc, m, out = _raw(ok, 4, 20000)                                                                # (the same arguments as they are: fine)
    assert rc == hip.OK and m <= 20000
    for bad in ((p, lab, C, far, er, G, thr), (p, lab, C, edges, down, G, thr), (p, lab, C, edges, er, (1 << 16) + 1, thr), (p + (1 << 27), lab, C, edges, er, G, thr),
                (p, lab, C, edges, er, G, (5, 5)), (p, lab, C, edges, er, G, np.arange(1, 34))):
        with pytest.raises(ValueError):
            mg.build(*bad)


def test_no_points_and_no_regions_write_the_empty_answer_over_the_fill(hip_device):
    rc, m, out = _raw(CASES['no_regions'], 4, 0)
    assert rc == hip.OK and m == 0 and (out[2] == 4).all() and (out[3] == -1).all() and not out[4].any()
    rc, m, out = _raw(CASES['no_points'], 4, 0)
    assert rc == hip.OK and m == 0 and not out[0].any() and not out[1].any() and out[0].shape == (3, 2, 4, 2)
    got = mg.build(*CASES['neither'])
    assert [a.shape for a in got] == [(0, 2, 4, 2), (0, 2), (0,), (0,), (0,)]
    some = CASES['regimes']
    far = (some[0] + 4000,) + some[1:]                                                             # every edge left of and below the box, beyond R: no record
    rc, m, out = _raw(far, 4, 0)
    assert rc == hip.OK and m == 0 and (out[2] == 4).all() and not out[0].any() and not out[1].any()


# ---- 4: the tool
_run = points_util.run_tool
FEATURES = [dict(type='Feature', properties=dict(classification=dict(name='left')), geometry=dict(type='Polygon', coordinates=[
                [[0, 0], [160.5, 0], [160.5, 192], [0, 192], [0, 0]], [[40, 40], [90, 40], [90, 120], [40, 120], [40, 40]]])),
            dict(type='Feature', properties=dict(name='band'), geometry=dict(type='MultiPolygon', coordinates=[
                [[[100, 20], [300, 60], [280, 100], [100, 90], [100, 20]]], [[[200, 130], [320, 130], [320, 192], [200, 192], [200, 130]]]])),
            dict(type='Feature', properties={}, geometry=dict(type='Point', coordinates=[5, 5]))]


def test_cli_nuclei_margin(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-graph --nuclei-margin on the synthetic .npy slide of tests/points_util.py, with --merge: the folder gains
    exactly the one file, every other file is the same bytes as without the flag, the rows are those of <id>_nuclei_graph.npz, the
    integers equal margin_reference on the file's own xy, label, edges and thresholds, and every derived key equals `derive` of them.  A
    directory without the slide's file: no output, and a clause that says so."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-graph')
    (tmp_path / 'regions').mkdir()
    (tmp_path / 'regions' / 's1.geojson').write_text(json.dumps(dict(type='FeatureCollection', features=FEATURES)))
    (tmp_path / 'empty').mkdir()
    flags = ['--nuclei-margin', str(tmp_path / 'regions'), '--margin-step', '7.5', '--margin-bands', '6']
    files = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d)))}
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    said = _run(base + flags + ['--save_dir', str(tmp_path / 'merge'), '--merge'], env)
    assert 'regions of s1.geojson' in said and 's1_nuclei_margin.npz' in said and 'within 45 px' in said and '6 bands' in said
    table = rg.read_geojson(str(tmp_path / 'regions' / 's1.geojson'))
    with_flag, without = files('merge'), files('merge0')
    assert sorted(with_flag) == sorted(list(without) + ['s1_nuclei_margin.npz'])
    for f in without:
        assert with_flag[f] == without[f], f
    g = cellgraph.read_npz(str(folder('merge') / 's1_nuclei_graph.npz'))
    z = mg.read_npz(str(folder('merge') / 's1_nuclei_margin.npz'))
    assert tuple(z) == mg.NPZ_KEYS and z['names'].tolist() == ['left', 'band'] and z['thresholds'].tolist() == [15, 30, 45, 60, 75, 90]
    n = len(g['nuclei_id'])
    assert n > 10 and np.array_equal(z['nuclei_id'], g['nuclei_id']) and np.array_equal(z['xy'], g['xy']) and np.array_equal(z['label'], g['label'])
    assert np.array_equal(z['edges'], table.edges) and np.array_equal(z['edge_region'], table.edge_region) and np.array_equal(z['area2'], table.area2)
    pts = np.rint(2 * z['xy']).astype(np.int32)
    want = mg.margin_reference(pts, z['label'], 5, z['edges'], z['edge_region'], 2, z['thresholds'])
    _equal([z[name] for name in mg.INT_NAMES], want, 'merge')
    d = mg.derive(want[0], want[1], z['thresholds'])
    for key in mg.DERIVED_KEYS:
        assert np.array_equal(z[key], d[key]) and z[key].dtype == d[key].dtype, key
    print(f"{n} nuclei, {int((z['band'] < 6).sum())} within the last band, n_near {z['n_near'].tolist()}")
    assert 0 < int((z['band'] < 6).sum()) <= n and int(z['n_near'].sum()) > 0
    said = _run(base + ['--nuclei-margin', str(tmp_path / 'empty'), '--save_dir', str(tmp_path / 'none'), '--merge'], env)
    assert 'no s1.geojson' in said and 'no s1_nuclei_margin.npz' in said and files('none') == files('merge0')
