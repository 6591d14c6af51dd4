"""Host side of the per-nucleus table from a written GeoJSON (nuhtc_amd/ringfeat.py, tools/wsi_feat_extract.py): parsing, frame sides,
the block walk, the SQLite file with its resume rule, and the tool's command line.  No GPU."""
import ast
import itertools
import json
import os
import sqlite3

import numpy as np
import pytest

from nuhtc_amd import nucmorph, nuctex, ringfeat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'wsi_feat_extract.py')


def _feat(ring, **props):
    return {'type': 'Feature', 'geometry': {'type': 'Polygon', 'coordinates': [ring]},
            'properties': dict({'label': 2, 'score': 0.75, 'classification': {'name': 'C', 'color': [0, 0, 255]}}, **props)}


def test_parse_rings_ids_and_what_is_left_out():
    sq = [[10, 20], [10, 23], [14, 23], [14, 20]]
    feats = [_feat(sq + sq[:1]),                                              # 0 closed
             _feat(sq, nuclei_id=41),                                         # 1 open, its own id
             _feat([[float(x), float(y)] for x, y in sq]),                    # 2 floats that are integers
             _feat([[10.5, 20.0], [10.0, 23.0], [14.0, 23.0]]),               # 3 not integers: left out
             _feat([[0, 0], [0, 255], [255, 255], [255, 0]]),                 # 4 side 256: kept
             _feat([[0, 0], [0, 255], [256, 255], [256, 0]]),                 # 5 side 257: left out
             {'type': 'Feature', 'geometry': {'type': 'Polygon', 'coordinates': []}, 'properties': {}},      # 6 no ring
             {'type': 'Feature', 'geometry': {'type': 'Point', 'coordinates': [1.5, 2.5]}, 'properties': {}},  # 7 no polygon: not counted
             _feat([[7, 9]], nuclei_id=3)]                                    # 8 a single vertex
    p = ringfeat.parse(feats)
    assert p['nuclei_id'].tolist() == [0, 41, 2, 4, 3]
    for k in range(3):
        assert p['rings'][k].dtype == np.int32 and p['rings'][k].tolist() == sq
    assert p['rect'].tolist() == [[10, 20, 14, 23]] * 3 + [[0, 0, 255, 255], [7, 9, 7, 9]]
    assert ringfeat.frame_sides(p['rect']).tolist() == [32, 32, 32, 256, 32]
    assert p['score'].tolist() == [0.75] * 5 and p['label'].tolist() == [2] * 5 and p['type'] == ['C'] * 5
    assert p['left_out'] == dict(non_integer=1, no_ring=1, too_large=1, off_slide=0, not_traced=0)
    assert set(p['left_out']) == set(ringfeat.REASONS)


def test_buckets():
    assert [ringfeat.bucket(s) for s in (1, 32, 33, 64, 65, 128, 129, 256)] == [32, 32, 64, 64, 128, 128, 256, 256]
    with pytest.raises(ValueError):
        ringfeat.bucket(257)


def test_block_assignment_corner_halo_and_slide_edge():
    H, W, B = 700, 900, 256
    rect = np.array([[255, 255, 300, 400],        # 0 corner = the last pixel of block (0, 0), the body in the halo
                     [256, 255, 300, 300],        # 1 one pixel on: block (1, 0)
                     [W - 1, H - 1, W - 1, H - 1],  # 2 the slide's last row and column
                     [W - 40, H - 30, W - 1, H - 1],  # 3 ends on them
                     [W - 40, 10, W, 20],         # 4 leaves the slide on the right
                     [-1, 5, 8, 9],               # 5 ... on the left
                     [0, 0, 0, 0]])               # 6 the first pixel
    blocks, off = ringfeat.block_plan(rect, (H, W), B)
    assert off.tolist() == [4, 5]
    owner = {}
    for x, y, w, h, idx in blocks:
        assert x % B == 0 and y % B == 0 and 0 < w <= B + 256 and 0 < h <= B + 256 and x + w <= W and y + h <= H
        assert w == min(B + 256, W - x) and h == min(B + 256, H - y)
        for i in idx.tolist():
            assert i not in owner
            owner[i] = (x, y)
            assert x <= rect[i, 0] < x + B and y <= rect[i, 1] < y + B            # the corner is in the block proper ...
            assert rect[i, 2] < x + w and rect[i, 3] < y + h                      # ... and the whole rectangle in what is read
    assert owner == {0: (0, 0), 6: (0, 0), 1: (256, 0), 2: (768, 512), 3: (768, 512)}
    assert [(b[0], b[1]) for b in blocks] == [(0, 0), (256, 0), (768, 512)]       # row-major, only blocks that own a nucleus
    # one block for the whole slide at the default size
    blocks, off = ringfeat.block_plan(rect, (H, W))
    assert len(blocks) == 1 and blocks[0][:4] == (0, 0, W, H) and sorted(blocks[0][4].tolist()) == [0, 1, 2, 3, 6]


def _rows(n, first_id=0):
    rng = np.random.default_rng(n)
    values = rng.random((n, 55))
    ids = np.arange(first_id, first_id + n)
    return values, rng.random(n), [f't{i}' for i in range(n)], np.arange(n) % 5, ids, np.stack([ids, ids + 1, ids + 9, ids + 12], 1)


def test_db_columns_types_and_resume(tmp_path):
    path = str(tmp_path / 'seg' / 's1' / ringfeat.DB_NAME)
    assert ringfeat.read_db(path) is None and ringfeat.missing_ids(path, [3, 1, 2]) == [3, 1, 2]
    v, score, kind, cls, ids, rect = _rows(3)
    assert ringfeat.write_db(path, v, score, kind, cls, ids, rect) == 3
    got = ringfeat.read_db(path)
    names = ['Label'] + [c.replace('.', '_') for c in nucmorph.COLUMNS + nuctex.COLUMNS] + ['score', 'type', 'class_id', 'nuclei_id', 'x_min', 'y_min', 'x_max', 'y_max']
    types = ['INTEGER'] + ['REAL'] * 55 + ['REAL', 'TEXT', 'INTEGER', 'INTEGER'] + ['INTEGER'] * 4
    assert got['columns'] == list(zip(names, types)) == ringfeat.db_columns()
    assert len(names) == 64 and names[1] == 'Size_Area' and names[30] == 'Haralick_ASM_Mean' and not any('.' in c for c in names)
    assert len(got['rows']) == 3
    for i, r in enumerate(got['rows']):
        assert r[0] == 1 and list(r[1:56]) == v[i].tolist() and r[56] == score[i] and r[57] == kind[i] and r[58] == cls[i] and r[59] == i
        assert list(r[60:]) == rect[i].tolist()
    con = sqlite3.connect(path)                                                # the storage classes, not only the declared types
    assert con.execute(f'SELECT typeof(Label), typeof(Size_Area), typeof(score), typeof(type), typeof(nuclei_id), typeof(x_max) FROM {ringfeat.TABLE}').fetchone() \
        == ('integer', 'real', 'real', 'text', 'integer', 'integer')
    con.close()
    # resume: all ids there -> nothing to do; some -> exactly the others, in the file's order
    assert ringfeat.missing_ids(path, [2, 0, 1]) == []
    assert ringfeat.missing_ids(path, [5, 0, 4, 2, 3]) == [5, 4, 3]
    # a 3-row table is far below 1 MB and survives a second run: the rows are appended to, never dropped
    assert os.path.getsize(path) < 1 << 20
    v2, score2, kind2, cls2, ids2, rect2 = _rows(2, first_id=3)
    ringfeat.write_db(path, v2, score2, kind2, cls2, ids2, rect2)
    again = ringfeat.read_db(path)
    assert again['rows'][:3] == got['rows'] and [r[59] for r in again['rows']] == [0, 1, 2, 3, 4]
    assert ringfeat.missing_ids(path, range(5)) == []
    with pytest.raises(ValueError):
        ringfeat.write_db(path, v, score[:2], kind, cls, ids, rect)


def test_tool_flags_and_defaults():
    """The flag set of the reference's tool and the three of our own, read off the tool's source."""
    want = [(('datadir',), {}),
            (('--segdir',), {}),
            (('--start',), dict(type='int', default=0)),
            (('--end',), dict(type='int', default=None)),
            (('--mag',), dict(type='int', default=40)),
            (('--reverse',), dict(action='store_true', default=False)),
            (('--bs_size',), dict(type='int', default=1024)),
            (('--num_workers',), dict(type='int', default=8)),
            (('--slide_ext',), dict(type='str', default='.svs')),
            (('--geojson',), dict(choices=('merged', 'plain'), default='merged')),
            (('--device',), dict(type='int', default=0))]
    tree = ast.parse(open(TOOL).read())
    got = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'add_argument':
            kw = {}
            for k in node.keywords:
                if k.arg != 'help':
                    kw[k.arg] = k.value.id if k.arg == 'type' else ast.literal_eval(k.value)
            got.append((tuple(ast.literal_eval(a) for a in node.args), kw))
    assert sorted(got, key=lambda g: g[0]) == sorted(want, key=lambda g: g[0])
    assert ast.get_docstring(tree) and '1 MB' in ast.get_docstring(tree) and 'traced rings' in ast.get_docstring(tree).lower()


def _tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location('tool_wsi_feat_extract', TOOL)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_slide_ids_follow_the_reference_slices(tmp_path):
    tool = _tool()
    for name in ('b.npy', 'a.svs', 'c.tif', 'd.npy'):
        (tmp_path / name).write_bytes(b'')
    d = str(tmp_path)
    assert tool.slide_ids(d) == ['a', 'b', 'c', 'd']
    assert tool.slide_ids(d, 1, 3) == ['b', 'c'] and tool.slide_ids(d, 1, None) == ['b', 'c', 'd'] and tool.slide_ids(d, 0, -1) == ['a', 'b', 'c']
    assert tool.slide_ids(d, 1, None, reverse=True) == ['c', 'b', 'a']           # reversed first, sliced after
    a = tool.parse_args(['data', '--segdir', 'seg'])
    assert (a.datadir, a.segdir, a.start, a.end, a.mag, a.reverse, a.bs_size, a.num_workers, a.slide_ext, a.geojson, a.device) \
        == ('data', 'seg', 0, None, 40, False, 1024, 8, '.svs', 'merged', 0)


def test_select_keeps_the_order_of_the_table_and_refuses_other_keywords(tmp_path):
    F = ringfeat.FAMILIES
    assert [f.keyword for f in F] == [None, None, 'gradient', 'shape', 'fsd'] and [f.columns for f in F[:2]] == [nucmorph.COLUMNS, nuctex.COLUMNS]
    assert ringfeat.select() == ringfeat.select(gradient=False, shape=False, fsd=False) == F[:2]
    assert ringfeat.select(fsd=True, shape=True, gradient=True) == ringfeat.select(gradient=True, shape=True, fsd=True) == F
    assert ringfeat.select(fsd=True, gradient=True) == ringfeat.select(gradient=True, shape=False, fsd=True) == F[:3] + F[4:]
    assert ringfeat.select(shape=True) == F[:2] + F[3:4]
    for call in (ringfeat.select, ringfeat.table_columns, ringfeat.db_columns, lambda **k: ringfeat.column_mismatch(str(tmp_path / 'no.db'), **k),
                 lambda **k: ringfeat.table({}, **k), lambda **k: ringfeat.write_db(str(tmp_path / 'no.db'), *_rows(2), **k),
                 lambda **k: ringfeat.measure(None, [], **k)):
        with pytest.raises(TypeError):
            call(cytoplasm=True)
        with pytest.raises(TypeError):
            call(gradient=True, Shape=True)
    assert not os.path.exists(str(tmp_path / 'no.db'))


def test_columns_and_help_of_every_selection_equal_the_recorded_ones(monkeypatch):
    """tests/golden/ringfeat_columns.json: table_columns, db_columns and the tool's --help as they were before the families became a table."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'ringfeat_columns.json')) as f:
        gold = json.load(f)
    assert sorted(gold['table']) == sorted(gold['db']) == sorted(''.join(b) for b in itertools.product('01', repeat=3))
    for g, s, f in itertools.product((False, True), repeat=3):
        key = ''.join('01'[v] for v in (g, s, f))
        assert list(ringfeat.table_columns(gradient=g, shape=s, fsd=f)) == gold['table'][key], key
        assert [list(c) for c in ringfeat.db_columns(gradient=g, shape=s, fsd=f)] == gold['db'][key], key
    monkeypatch.setenv('COLUMNS', str(gold['help_columns']))
    parser = _tool().build_parser()
    parser.prog = 'wsi_feat_extract.py'
    assert parser.format_help() == gold['help']


def test_nan_is_null_in_a_family_a_nucleus_can_lack_and_refused_elsewhere(tmp_path):
    assert [bool(f.lacking) for f in ringfeat.FAMILIES] == [False, False, True, False, False]
    n, every = 3, dict(gradient=True, shape=True, fsd=True)
    args = (np.linspace(0.5, 0.9, n), ['a', 'b', 'c'], [1, 2, 3], [7, 8, 9], np.arange(n * 4).reshape(n, 4))
    vals = np.arange(n * 77, dtype=np.float64).reshape(n, 77) + 0.5
    vals[1, 55:63] = np.nan                                                     # the eight gradient columns of one nucleus
    path = str(tmp_path / 'every.db')
    assert ringfeat.write_db(path, vals, *args, **every) == n
    rows = ringfeat.read_db(path)['rows']
    assert list(rows[1][56:64]) == [None] * 8 and list(rows[1][1:56]) == vals[1, :55].tolist() and list(rows[1][64:78]) == vals[1, 63:].tolist()
    assert [list(r[1:78]) for r in (rows[0], rows[2])] == vals[[0, 2]].tolist()
    before = open(path, 'rb').read()
    for col in (0, 28, 29, 54, 63, 70, 71, 76):                                 # first and last column of each of the other four families
        bad = vals.copy()
        bad[2, col] = np.nan
        with pytest.raises(ValueError):
            ringfeat.write_db(path, bad, *args, **every)
    with pytest.raises(ValueError):                                             # without the family that can be lacking: no NaN at all
        ringfeat.write_db(str(tmp_path / 'plain.db'), np.where(np.arange(55) == 7, np.nan, vals[:, :55]), *args)
    assert not os.path.exists(str(tmp_path / 'plain.db'))
    with pytest.raises(ValueError):                                             # a foreign column set
        ringfeat.write_db(path, vals[:, :55], *args)
    with pytest.raises(ValueError):
        ringfeat.write_db(path, vals[:, :63], *args, gradient=True)
    assert open(path, 'rb').read() == before
