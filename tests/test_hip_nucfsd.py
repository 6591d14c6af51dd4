"""GPU tests of the Fourier-descriptor integers (csrc/nucfsd.hip): the device produces integers only, so every check is EQUALITY with the
numpy restatement (nuhtc_amd.nucfsd.fsd_reference) -- nuhtc_op_ring_fsd on the designed rings of tests/nucfsd_cases.py in one batch and
one at a time, the smallest and the largest batch, the statuses, repeatability, refused arguments, the document route
(ringfeat.measure(fsd=True)) and tools/wsi_feat_extract.py --fsd end to end."""
import ctypes
import json
import os
import sqlite3
import subprocess
import sys

import numpy as np
import pytest
import torch

from nuhtc_amd import contours, hip, ringfeat
from nuhtc_amd import nucfsd as nf
from nuhtc_amd import nucgrad as ng
from nuhtc_amd import nucshape as ns

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucfsd_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'wsi_feat_extract.py')
CLASSES = ('T', 'I', 'C', 'D', 'E')
POISON = -7


def _call(dev, verts, ring_off, n=None, null=()):
    """nuhtc_op_ring_fsd on host arrays -> (rc, rows int32 (n, 644), status int32 (n,)); the outputs are poisoned first."""
    lib = hip.load()
    n = len(ring_off) - 1 if n is None else n
    v = torch.from_numpy(np.ascontiguousarray(np.asarray(verts, np.int32).reshape(-1, 2))).to(dev)
    if v.numel() == 0:
        v = torch.zeros(1, 2, dtype=torch.int32, device=dev)                # the entry wants a vertex array, even for empty rings only
    off = torch.from_numpy(np.ascontiguousarray(ring_off, np.int64)).to(dev)
    rows = torch.full((max(n, 1), nf.ROW), POISON, dtype=torch.int32, device=dev)
    status = torch.full((max(n, 1),), POISON, dtype=torch.int32, device=dev)
    ptr = {'verts': v, 'ring_off': off, 'rows': rows, 'status': status}
    arg = lambda k: None if k in null else ctypes.c_void_p(ptr[k].data_ptr())
    rc = lib.nuhtc_op_ring_fsd(0, arg('verts'), int(v.shape[0]) if 'nv' not in null else 0, arg('ring_off'), int(n), arg('rows'), arg('status'),
                               ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    return rc, rows.cpu().numpy(), status.cpu().numpy()


def _run(dev, rings):
    verts, off = ringfeat.pack_rings(rings)
    rc, rows, status = _call(dev, verts, off)
    assert rc == 0
    assert np.array_equal(rows[:, 0], status)
    return rows


@pytest.fixture(scope='module')
def designed():
    """names, rings and the restatement (n, 644) of the designed rings, computed once."""
    d = cases.designed()
    names, rings = list(d), list(d.values())
    assert names.index('empty') not in (0, len(names) - 1)                 # the empty ring sits in the middle of the batch
    want = np.stack([nf.fsd_reference(r) for r in rings])
    want.setflags(write=False)
    return names, rings, want


def test_designed_rings_in_one_batch_and_one_at_a_time(hip_device, designed):
    names, rings, want = designed
    got = _run(hip_device, rings)
    assert got.dtype == np.int32 and got.shape == want.shape
    for k, name in enumerate(names):
        assert np.array_equal(got[k], want[k]), (name, np.nonzero(got[k] != want[k])[0][:8])
        assert got[k, 0] == cases.STATUS.get(name, 0), name
        if got[k, 0]:
            assert not got[k, 1:].any(), name
    for k, name in enumerate(names):
        assert np.array_equal(_run(hip_device, [rings[k]])[0], want[k]), name
    c = cases.PELL                                                         # the exact decision on the device: not the edge float64 picks
    assert got[names.index('pell'), 4 + 5 * c['k'] + 3:4 + 5 * c['k'] + 5].tolist() != [c['a'], c['b']]


def test_statuses_of_bad_offsets(hip_device, designed):
    names, rings, want = designed
    sq, dia = rings[names.index('square of perimeter 128')], rings[names.index('diamond, A = 0')]
    verts = np.concatenate([sq, dia])                                       # nv = 8
    off = np.array([0, 4, 2, 4, 8, 9, 8, -1, 8], np.int64)                  # ok, decreasing, ok (two vertices), ok, past nv, decreasing, negative end, negative start
    rc, rows, status = _call(hip_device, verts, off)
    assert rc == 0
    assert np.array_equal(rows, nf.fsd_reference_batch(verts, off))
    assert status.tolist() == [0, 2, 0, 0, 2, 2, 2, 2]
    assert np.array_equal(rows[0], want[names.index('square of perimeter 128')]) and np.array_equal(rows[3], want[names.index('diamond, A = 0')])
    assert not rows[status == 2][:, 1:].any()


def test_smallest_and_largest_batch(hip_device):
    base = [cases.traced(cases.disc(r), (3 * r, 5 * r)) for r in range(2, 10)] + [cases.saw(n, seed=n) for n in (4, 5, 31, 300)]
    ref = [nf.fsd_reference(r) for r in base]
    got = _run(hip_device, [base[0]])
    assert got.shape == (1, nf.ROW) and np.array_equal(got[0], ref[0])
    pick = np.random.default_rng(4).integers(0, len(base), 4096)
    got = _run(hip_device, [base[i] for i in pick])
    assert got.shape == (4096, nf.ROW) and np.array_equal(got, np.stack(ref)[pick])


def test_repeatable_across_calls_and_batch_splits(hip_device, designed):
    names, rings, want = designed
    whole = _run(hip_device, rings)
    assert _run(hip_device, rings).tobytes() == whole.tobytes()
    cut = len(rings) // 3
    split = np.concatenate([_run(hip_device, rings[:cut]), _run(hip_device, rings[cut:])])
    assert split.tobytes() == whole.tobytes() == want.tobytes()
    assert _run(hip_device, rings[::-1])[::-1].tobytes() == whole.tobytes()


def test_invalid_arguments_are_refused_without_a_launch(hip_device):
    ring = cases.designed()['square of perimeter 128']
    verts, off = ringfeat.pack_rings([ring])
    for null in ('verts', 'ring_off', 'rows', 'status', 'nv'):
        rc, rows, status = _call(hip_device, verts, off, null=(null,))
        assert rc == hip.E_INVALID and (rows == POISON).all() and (status == POISON).all(), null
    for n in (0, -1, 4097):
        rc, rows, status = _call(hip_device, verts, np.zeros(2, np.int64), n=n)
        assert rc == hip.E_INVALID and (rows == POISON).all() and (status == POISON).all(), n
    rc, rows, _ = _call(hip_device, verts, off)
    assert rc == 0 and np.array_equal(rows[0], nf.fsd_reference(ring))


# ---------------------------------------------------------------------------------------------------------------- the document route
SLIDE_H, SLIDE_W = 300, 280


def _slide():
    return np.random.default_rng(29).integers(0, 256, (SLIDE_H, SLIDE_W, 3), dtype=np.uint8)


def _placed():
    """[(name, bool mask cropped to its rectangle, slide (x, y) of the rectangle)]: nuclei in the slide's corners, across the block
    boundary at 128, of every frame side, and one pixel (a ring of one vertex: status 1)."""
    sq = lambda h, w: np.ones((h, w), bool)
    crop = lambda m: m[np.ix_(m.any(1), m.any(0))]
    out = [('corner 0 0', crop(cases.disc(7)), (0, 0)), ('last corner', sq(3, 3), (SLIDE_W - 3, SLIDE_H - 3)), ('across the block corner', crop(cases.disc(7)), (121, 122)),
           ('clover', crop(cases.clover()), (40, 40)), ('side 33', sq(33, 20), (70, 200)), ('ellipse 45x25', crop(cases.ellipse(45, 25)), (150, 30)),
           ('ellipse 50x65', crop(cases.ellipse(50, 65)), (140, 160)), ('one pixel', sq(1, 1), (200, 10)), ('254 px', sq(6, 254), (10, 290))]
    for n, m, (x, y) in out:
        assert x + m.shape[1] <= SLIDE_W and y + m.shape[0] <= SLIDE_H, n
    return out


def _features(placed):
    return [contours.feature(contours.mask_to_ring(m, (x, y)), k % 5, 0.5 + k / 100.0, CLASSES) for k, (n, m, (x, y)) in enumerate(placed)]


def _want_rows(feats):
    """The restatement of the rings measure() parses out of the features."""
    return np.stack([nf.fsd_reference(r) for r in ringfeat.parse(feats)['rings']])


def test_measure_with_fsd_equals_the_restatement(hip_device):
    slide, placed = _slide(), _placed()
    feats = _features(placed)
    m = ringfeat.measure(slide, feats, device=0, block=128, fsd=True)
    plain = ringfeat.measure(slide, feats, device=0, block=128)
    n = len(placed)
    assert len(m['raw']) == n and m['fsd'].shape == (n, nf.ROW) and m['fsd'].dtype == np.int32 and sum(m['left_out'].values()) == 0
    assert set(m) == set(plain) | {'fsd'}
    for k in ('raw', 'hist', 'glcm', 'origin', 'nuclei_id', 'rect', 'score', 'label'):            # the other measurements: the same bytes
        assert m[k].dtype == plain[k].dtype and m[k].tobytes() == plain[k].tobytes(), k
    want = _want_rows(feats)
    for i, (name, _, _) in enumerate(placed):
        assert np.array_equal(m['fsd'][i], want[i]), name
    assert m['fsd'][:, 0].tolist() == [1 if name == 'one pixel' else 0 for name, _, _ in placed]     # a kept nucleus: status 0 or 1
    assert sorted(set(ringfeat.frame_sides(m['rect']).tolist())) == [32, 64, 128, 256]
    one = ringfeat.measure(slide, feats, device=0, block=2048, fsd=True)                        # the block size changes nothing
    assert one['fsd'].tobytes() == m['fsd'].tobytes()
    cols, val = ringfeat.table(m, fsd=True)
    assert cols == ringfeat.table_columns(fsd=True) and val.shape == (n, 61) and np.isfinite(val).all()
    assert np.array_equal(val[:, :55], ringfeat.table(plain)[1]) and np.array_equal(val[:, 55:], nf.derive(want)[1])
    every = ringfeat.measure(slide, feats, device=0, block=128, gradient=True, shape=True, fsd=True)
    cols, val2 = ringfeat.table(every, gradient=True, shape=True, fsd=True)
    assert cols == ringfeat.table_columns(gradient=True, shape=True, fsd=True) and val2.shape == (n, 77) and every['fsd'].tobytes() == m['fsd'].tobytes()
    assert np.array_equal(val2[:, 71:], val[:, 55:]) and np.array_equal(val2[:, :55], val[:, :55])
    assert cols[63:71] == ns.COLUMNS and cols[71:] == nf.COLUMNS


def _run_tool(cmd, limit=120):
    p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, TOOL] + cmd, cwd=ROOT, capture_output=True, text=True)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, p.returncode
    return p.stdout, p.stderr


def _rows(path):
    con = sqlite3.connect(path)
    try:
        return con.execute(f'SELECT * FROM {ringfeat.TABLE} ORDER BY rowid').fetchall()
    finally:
        con.close()


def test_tool_with_and_without_fsd(hip_device, tmp_path):
    slide, placed = _slide(), _placed()
    feats = _features(placed)
    data = tmp_path / 'wsi'
    data.mkdir()
    np.save(data / 's1.npy', slide)
    segs = {}
    for d in ('plain', 'fsd', 'every'):
        segs[d] = tmp_path / d
        (segs[d] / 's1').mkdir(parents=True)
        with open(segs[d] / 's1' / 's1_merged.geojson', 'w') as f:
            json.dump(feats[:5] if d == 'fsd' else feats, f)
    db = lambda d: str(segs[d] / 's1' / 'nuclei_feat.db')
    base = lambda d: [str(data), '--segdir', str(segs[d]), '--slide_ext', '.npy']
    flags = {'plain': [], 'fsd': ['--fsd'], 'every': ['--gradient', '--shape', '--fsd']}
    for d in segs:
        _, err = _run_tool(base(d) + flags[d])
        assert f's1: {5 if d == "fsd" else len(feats)} rows written, left out none' in err
    # resume: the --fsd table holds five of the nuclei; with the whole file the other four are measured and appended
    with open(segs['fsd'] / 's1' / 's1_merged.geojson', 'w') as f:
        json.dump(feats, f)
    out, err = _run_tool(base('fsd') + ['--fsd'])
    assert f's1: {len(feats) - 5} rows written' in err and f'skipped 5/{len(feats)} nuclei' in out
    assert ringfeat.missing_ids(db('fsd'), range(len(feats))) == []
    a, b, c = (ringfeat.read_db(db(d)) for d in ('plain', 'fsd', 'every'))
    assert a['columns'] == ringfeat.db_columns() and b['columns'] == ringfeat.db_columns(fsd=True) and c['columns'] == ringfeat.db_columns(gradient=True, shape=True, fsd=True)
    under = lambda cols: [x.replace('.', '_') for x in cols]
    assert [x for x, _ in b['columns'][56:62]] == under(nf.COLUMNS) == [x for x, _ in c['columns'][72:78]]
    assert [x for x, _ in c['columns'][56:64]] == under(ng.COLUMNS) and [x for x, _ in c['columns'][64:72]] == under(ns.COLUMNS)
    assert [x for x, _ in b['columns'][62:]] == [x for x, _ in a['columns'][56:]] == [x for x, _ in c['columns'][78:]] and b['columns'][62][0] == 'score'
    val = nf.derive(_want_rows(feats))[1]                                                       # derive of the restatement of the parsed rings
    for i, (ra, rb, rc) in enumerate(zip(_rows(db('plain')), _rows(db('fsd')), _rows(db('every')))):
        assert rb[:56] == ra[:56] and rb[62:] == ra[56:], i                                      # the common columns: equal bytes
        assert rc[:56] == ra[:56] and rc[78:] == ra[56:], i
        assert all(isinstance(v, float) and np.isfinite(v) for v in rb[56:62]) and list(rb[56:62]) == val[i].tolist() == list(rc[72:78]), i
    # --fsd onto the table written without it: skipped with the message, which names the file and the difference; the bytes unchanged
    before = {d: open(db(d), 'rb').read() for d in segs}
    out, err = _run_tool(base('plain') + ['--fsd'])
    assert 'skipped:s1' in out and db('plain') in out and 'Shape_FSD1' in out and db('plain') in err
    assert 'Shape_HuMoments1' in ringfeat.column_mismatch(db('fsd'), shape=True, fsd=True) and 'Shape_FSD1' in ringfeat.column_mismatch(db('fsd'))
    assert 'Shape_FSD1' in ringfeat.column_mismatch(db('every'), gradient=True, shape=True) and ringfeat.column_mismatch(db('every'), gradient=True, shape=True, fsd=True) is None
    assert {d: open(db(d), 'rb').read() for d in segs} == before
