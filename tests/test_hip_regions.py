"""GPU tests of the region census (csrc/cellregion.hip, nuhtc_cell_regions): region, depth, on_boundary and census must EQUAL
nuhtc_amd.regions.regions_reference, the brute-force int64 restatement of the definition -- same dtype and shape, no tolerance, nothing
left out.  Every designed set of tests/regions_cases.py through `build`, each at three slab heights (1 and 16384 among them) with
identical outputs, two calls bitwise equal, permuted rows, the second-call path, the refused arguments with the outputs untouched, and
tools/infer_wsi.py --nuclei-regions end to end."""
import json
import os

import numpy as np
import pytest
import torch

import points_util
import regions_cases as RC
from nuhtc_amd import cellgraph, cellpoints, hip
from nuhtc_amd import regions as rg

pytestmark = pytest.mark.gpu
CASES = RC.all_cases()
SLABS = (1, 7, 16384)


def _equal(got, want, what):
    for name, g, w in zip(rg.INT_NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, f'{len(bad)} entries differ, first at {bad[0].tolist()}', int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


@pytest.fixture(scope='module')
def references():
    return {name: rg.regions_reference(*case) for name, case in CASES.items()}


def _raw(case, slab, slot_cap, fill=77, bounds=None):
    """One call on buffers filled with `fill` -> (return code, M, the four outputs as numpy, whole buffers)."""
    p, lab, C, edges, er, G = case
    dev = torch.device('cuda', 0)
    up = lambda a, rows: torch.from_numpy(np.ascontiguousarray(a) if len(a) else np.zeros(rows, a.dtype)).to(dev)[:len(a)]
    out = rg.outputs(len(p), G, C, dev, fill=fill)
    rc, m = rg.call(up(p, (1, 2)), up(lab, 1), C, up(edges, (1, 4)), up(er, 1), G, slab, slot_cap, *out, bounds=bounds)
    torch.cuda.synchronize()
    return rc, m, [t.cpu().numpy() for t in out]


# ---- 1: every designed set equals the restatement, at every slab height, twice
@pytest.mark.parametrize('name', sorted(CASES))
def test_every_case_equals_the_reference_at_three_slab_heights(hip_device, references, name):
    case, want = CASES[name], references[name]
    first = None
    for slab in SLABS:
        got = rg.build(*case, slab=slab, with_calls=True)
        assert got[4] == 1, (name, slab, 'the host states the records exactly: one call')
        _equal(got[:4], want, f'{name}, slab {slab}')
        again = rg.build(*case, slab=slab)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], again)), (name, slab, 'two calls differ')
        first = got if first is None else first
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], first[:4])), (name, slab, 'the outputs depend on the slab')
    _equal(rg.build(*case), want, f'{name}, the slab of choose_slab')
    if len(case[0]):
        shuffled, order = RC.permuted(case)
        got = rg.build(*shuffled)
        _equal(got, tuple(w[order] for w in want[:3]) + (want[3],), f'{name}, permuted rows')


def test_the_designed_sets_reach_what_they_are_for(hip_device):
    p, lab, C, edges, er, G = CASES['staging']
    bounds = cellpoints.bounds_of(p)
    assert rg.slots_needed(edges, bounds, 16384) > 600 and len(p) > 2 * 256                        # one slab: three staging passes, ten workgroups
    assert rg.slots_needed(edges, bounds, 1) > 4 * 2001                                            # the tall edges have a record in every slab
    assert np.bincount(p[:, 1] - bounds[1]).max() >= 1500                                          # a slab row fuller than a workgroup at slab 1
    region, depth, on, census = rg.build(*CASES['staging'])
    assert (region == 6).all() and census[6].sum() == (lab < 4).sum() and not census[2:6].any()   # region 6 holds the whole box, 2..5 nothing
    assert census[1].sum() >= 1500 and census[0].sum() > 0 and depth.max() >= 2                    # the coincident points lie in the star
    assert len(CASES['chain_shuffled'][0]) == 20000 and rg.choose_slab(cellpoints.bounds_of(CASES['chain_shuffled'][0])) == 1


def test_the_slab_walk_case_equals_the_reference(hip_device):
    """`regions_cases.slab_walk` at its one slab height: a first workgroup whose records lie in three slabs, the middle one without an edge
    record, a partial second workgroup, and region changes at record 256 of a slab (between two staging passes) and inside its last,
    partial pass (tests/test_regions_host.py checks that layout).  Every output equals the restatement."""
    case = RC.slab_walk()
    got = rg.build(*case, slab=RC.SLAB_WALK_SLAB, with_calls=True)
    assert got[4] == 1
    _equal(got[:4], rg.regions_reference(*case), 'slab_walk')


# ---- 2: the second call
def test_a_cap_below_the_records_writes_nothing_and_the_second_call_has_room(hip_device, references):
    case = CASES['staging']
    need = rg.slots_needed(case[3], cellpoints.bounds_of(case[0]), 7)
    for cap in (0, need - 1):
        rc, m, out = _raw(case, 7, cap)
        assert rc == hip.OK and m == need and all((a == 77).all() for a in out), cap               # M is reported, the outputs are untouched
    rc, m, out = _raw(case, 7, need)
    assert rc == hip.OK and m == need
    _equal(out, references['staging'], 'exactly enough room')
    _equal(_raw(case, 7, need + 1000)[2], references['staging'], 'more room than needed')
    got = rg.build(*case, slab=7, slot_cap=3, with_calls=True)
    assert got[4] == 2
    _equal(got[:4], references['staging'], 'build with too small a first cap')


# ---- 3: refused arguments, outputs untouched
def _refused(case, slab=4, cap=1000, bounds=None):
    rc, m, out = _raw(case, slab, cap, bounds=bounds)
    assert rc == hip.E_INVALID and m is None and all((a == 77).all() for a in out)


def test_refused_arguments_leave_the_outputs_untouched(hip_device):
    p, lab, C, edges, er, G = RC.overlap()
    far = edges.copy()
    far[5, 2] = 1 << 27
    _refused((p, lab, C, far, er, G))                                                              # a vertex outside the range
    far[5, 2] = -(1 << 27)
    _refused((p, lab, C, far, er, G))
    down = er.copy()
    down[6] = 0
    _refused((p, lab, C, edges, down, G))                                                          # edge_region decreasing
    _refused((p, lab, C, edges, er, G - 1))                                                        # a region outside 0 .. G - 1
    _refused((p, lab, C, edges, er - 1, G))
    _refused((p, lab, C, edges, er, (1 << 16) + 1))                                                # G above its limit
    _refused((p, lab, C, edges, er, 0))
    _refused((p, lab, 0, edges, er, G))
    _refused((p, lab, 15, edges, er, G))
    for slab in (0, 16385):
        _refused((p, lab, C, edges, er, G), slab=slab)
    _refused((p, lab, C, edges, er, G), cap=-1)
    _refused((p, lab, C, edges, er, G), cap=(1 << 28) + 1)
    _refused((p, lab, C, edges, er, G), bounds=(0, 0, 10, 10))                                     # a point outside the stated box
    _refused((p, lab, C, edges, er, G), bounds=(0, 0, 10, -1))
    _refused((np.zeros((0, 2), np.int32), np.zeros(0, np.int32), C, far, er, G))                   # no points: the edges are still checked
    rc, m, out = _raw((p, lab, C, edges, er, G), 4, 1000)                                          # (the same arguments as they are: fine)
    assert rc == hip.OK and m <= 1000
    for bad in ((p, lab, C, far, er, G), (p, lab, C, edges, down, G), (p, lab, C, edges, er, (1 << 16) + 1), (p + (1 << 27), lab, C, edges, er, G)):
        with pytest.raises(ValueError):
            rg.build(*bad)


def test_no_points_and_no_regions_write_the_empty_answer_over_the_fill(hip_device):
    some = RC.unit_rectangle()
    rc, m, out = _raw(CASES['no_regions'], 4, 0)
    assert rc == hip.OK and m == 0 and (out[0] == -1).all() and not out[1].any() and not out[2].any()
    rc, m, out = _raw(CASES['no_points'], 4, 0)
    assert rc == hip.OK and m == 0 and not out[3].any() and out[3].shape == (1, 2)
    got = rg.build(*CASES['neither'])
    assert [a.shape for a in got] == [(0,), (0,), (0,), (0, 2)]
    far = (some[0] + 4000,) + some[1:]                                                             # every edge left of and below the box: no record
    rc, m, out = _raw(far, 4, 0)
    assert rc == hip.OK and m == 0 and (out[0] == -1).all() and not out[3].any()


# ---- 4: the tool
_run = points_util.run_tool
FEATURES = [dict(type='Feature', properties=dict(classification=dict(name='left')), geometry=dict(type='Polygon', coordinates=[
                [[0, 0], [160.5, 0], [160.5, 192], [0, 192], [0, 0]], [[40, 40], [90, 40], [90, 120], [40, 120], [40, 40]]])),
            dict(type='Feature', properties=dict(name='band'), geometry=dict(type='MultiPolygon', coordinates=[
                [[[100, 20], [300, 60], [280, 100], [100, 90], [100, 20]]], [[[200, 130], [320, 130], [320, 192], [200, 192], [200, 130]]]])),
            dict(type='Feature', properties={}, geometry=dict(type='Point', coordinates=[5, 5]))]


def test_cli_nuclei_regions(hip_device, tmp_path):
    """tools/infer_wsi.py --nuclei-graph --nuclei-regions on the synthetic .npy slide of tests/points_util.py, with --merge on one rank and on
    two (three runs of the tool): the folder gains exactly the one file, every other file is the same bytes as without the flag, the rows
    are those of <id>_nuclei_graph.npz, the integers equal regions_reference on the file's own xy, label and edges, and every derived key
    equals `derive` of them.  A directory without the slide's file: no output, and a clause that says so."""
    base, env, two, folder = points_util.slide_runs(tmp_path, '--nuclei-graph')
    (tmp_path / 'regions').mkdir()
    (tmp_path / 'regions' / 's1.geojson').write_text(json.dumps(dict(type='FeatureCollection', features=FEATURES)))
    (tmp_path / 'empty').mkdir()
    flags = ['--nuclei-regions', str(tmp_path / 'regions'), '--regions-order', 'area']
    files = lambda d: {f: open(folder(d) / f, 'rb').read() for f in sorted(os.listdir(folder(d)))}
    _run(base + ['--save_dir', str(tmp_path / 'merge0'), '--merge'], env)
    _run(base + flags + ['--save_dir', str(tmp_path / 'merge'), '--merge'], env)
    said = _run(base + flags + ['--save_dir', str(tmp_path / 'two'), '--merge', '--gpus', '2'], two)
    assert 'regions of s1.geojson' in said and 's1_nuclei_regions.npz' in said and 'on a boundary' in said
    table = rg.read_geojson(str(tmp_path / 'regions' / 's1.geojson'), 'area')
    assert table.skipped == 1 and table.names.tolist() == ['left', 'band']
    for run, ref in (('merge', 'merge0'), ('two', 'merge0')):
        with_flag, without = files(run), files(ref)
        assert sorted(with_flag) == sorted(list(without) + ['s1_nuclei_regions.npz']), run
        for f in without:
            assert with_flag[f] == without[f], (run, f)
        g = cellgraph.read_npz(str(folder(run) / 's1_nuclei_graph.npz'))
        z = rg.read_npz(str(folder(run) / 's1_nuclei_regions.npz'))
        assert tuple(z) == rg.NPZ_KEYS and str(z['order']) == 'area' and z['names'].tolist() == ['left', 'band']
        n = len(g['nuclei_id'])
        assert n > 10 and np.array_equal(z['nuclei_id'], g['nuclei_id']) and np.array_equal(z['xy'], g['xy']) and np.array_equal(z['label'], g['label'])
        assert np.array_equal(z['edges'], table.edges) and np.array_equal(z['edge_region'], table.edge_region) and np.array_equal(z['area2'], table.area2)
        pts = np.rint(2 * z['xy']).astype(np.int32)
        want = rg.regions_reference(pts, z['label'], 5, z['edges'], z['edge_region'], 2)
        _equal([z[name] for name in rg.INT_NAMES], want, run)
        d = rg.derive(want[3], z['area2'], want[1], z['label'])
        for key in rg.DERIVED_KEYS:
            assert np.array_equal(z[key], d[key], equal_nan=True) and z[key].dtype == d[key].dtype, (run, key)
        print(f"{run}: {n} nuclei, {int(z['n_inside'])} inside, census {z['census'].tolist()}")
        assert 0 < int(z['n_inside']) < n and int(z['census'].sum()) >= int(z['n_inside'])
    zm, zt = rg.read_npz(str(folder('merge') / 's1_nuclei_regions.npz')), rg.read_npz(str(folder('two') / 's1_nuclei_regions.npz'))
    for key in rg.NPZ_KEYS:
        assert np.array_equal(zm[key], zt[key], equal_nan=zm[key].dtype.kind == 'f'), key
    said = _run(base + ['--nuclei-regions', str(tmp_path / 'empty'), '--save_dir', str(tmp_path / 'none'), '--merge'], env)
    assert 'no s1.geojson' in said and files('none') == files('merge0')
