"""CPU tests of tile feature extraction (tools/extract_features_nuhtc.py, nuhtc_amd.features, h5coords.write_features): the reference's
command line, the target-size rules, the Pillow resize, the save_hdf5 layout of the feature files, the CSV loop with its .pt auto-skip.
The device step is stubbed; tests/test_hip_features.py runs it on the GPU."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
TYPES = {'int': int, 'float': float, 'str': str}


def _tool():
    spec = importlib.util.spec_from_file_location('tool_extract_features_nuhtc', os.path.join(ROOT, 'tools', 'extract_features_nuhtc.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parser_declares_every_reference_argument():
    """tests/golden/cli_extract_features_args.json = oracle/ref_harness/make_cli_golden.py's parser_table of the reference's tool; the
    same checks as tests/test_cli_parity.py."""
    table = json.load(open(os.path.join(GOLD, 'cli_extract_features_args.json')))['tools/extract_features_nuhtc.py']
    parser = _tool().build_parser()
    assert parser.allow_abbrev is False
    by_flag = {}
    for a in parser._actions:
        for f in (a.option_strings or [a.dest]):
            by_flag[f] = a
    assert len(table) == 12
    for row in table:
        acts = {id(by_flag[f]): by_flag[f] for f in row['flags'] if f in by_flag}
        assert len(acts) == 1 and all(f in by_flag for f in row['flags']), row['flags']
        a = next(iter(acts.values()))
        if row['flags'][0].startswith('-'):
            assert sorted(a.option_strings) == sorted(row['flags']), row
        assert a.default == row.get('default', False if row.get('action') == 'store_true' else None), (row, a.default)
        if 'dest' in row:
            assert a.dest == row['dest']
        if 'type' in row:
            assert a.type is TYPES[row['type']], row
        if row.get('action') == 'store_true':
            assert a.nargs == 0 and a.const is True
        else:
            assert a.nargs is None
        assert bool(a.required) == bool(row.get('required', not row['flags'][0].startswith('-')))
    # the example command in the reference's header, token for token
    args = _tool().parse_args('--config m.py --checkpoint e.pth --data_h5_dir /d/FEAT --data_slide_dir /d/WSI --slide_ext .svs --csv_path /d/l.csv '
                              '--feat_dir /d/out --target_patch_size 256 --batch_size 16'.split())
    assert (args.batch_size, args.target_patch_size, args.custom_downsample, args.no_auto_skip, args.stain_norm, args.gpus) == (16, 256, 1, False, False, 1)


def test_stain_norm_is_refused_with_a_message():
    tool = _tool()
    args = tool.parse_args('--config m.py --data_h5_dir a --data_slide_dir b --csv_path c.csv --feat_dir d --stain_norm'.split())
    with pytest.raises(SystemExit, match='stain_norm'):
        tool.check_args(args)
    with pytest.raises(SystemExit, match='--stain_norm'):
        tool.main('--config m.py --data_h5_dir a --data_slide_dir b --csv_path c.csv --feat_dir d --stain_norm'.split())
    with pytest.raises(SystemExit, match='CSV path'):
        tool.check_args(tool.parse_args('--config m.py --feat_dir d'.split()))


def test_target_size_rules():
    from nuhtc_amd.features import target_size
    assert target_size(256, 1, -1) is None
    assert target_size(256, 2, -1) == (128, 128)
    assert target_size(256, 3, -1) == (85, 85)
    assert target_size(256, 2, 224) == (224, 224)          # target_patch_size wins
    assert target_size(512, 1, 100) == (100, 100)
    assert target_size(256, 0, 0) is None


def test_pillow_resize_path():
    from PIL import Image
    from nuhtc_amd.features import resize_tiles
    rng = np.random.default_rng(0)
    tiles = rng.integers(0, 256, (3, 64, 64, 3), dtype=np.uint8)
    assert resize_tiles(tiles, None) is tiles
    out = resize_tiles(tiles, (40, 40))
    assert out.shape == (3, 40, 40, 3) and out.dtype == np.uint8
    for t, o in zip(tiles, out):
        assert np.array_equal(o, np.asarray(Image.fromarray(t).resize((40, 40))))
        assert np.array_equal(o, np.asarray(Image.fromarray(t).resize((40, 40), Image.BICUBIC)))     # Pillow's default for RGB
    assert not np.array_equal(out[0], np.asarray(Image.fromarray(tiles[0]).resize((40, 40), Image.BILINEAR)))


def test_write_features_roundtrip(tmp_path):
    from nuhtc_amd import h5coords
    if not h5coords.available():
        pytest.skip('no HDF5 back end')
    rng = np.random.default_rng(1)
    f = rng.standard_normal((7, 256)).astype(np.float32)
    c = rng.integers(0, 10 ** 6, (7, 2))
    p = str(tmp_path / 's.h5')
    h5coords.write_features(p, f, c)
    r = h5coords.read_features(p)
    assert sorted(r['names']) == ['coords', 'features']
    assert r['features'].dtype == np.float32 and r['features'].shape == (7, 256) and np.array_equal(r['features'], f)
    assert r['coords'].dtype == np.int64 and r['coords'].shape == (7, 2) and np.array_equal(r['coords'], c)
    assert r['dtypes'] == {'features': np.dtype('float32'), 'coords': np.dtype('int64')}
    assert r['chunks'] == {'features': (1, 256), 'coords': (1, 2)}
    assert r['maxshape'] == {'features': (None, 256), 'coords': (None, 2)}
    assert r['attrs'] == {'features': {}, 'coords': {}}
    h5coords.write_features(p, np.zeros((0, 256), np.float32), np.zeros((0, 2), np.int64))      # an empty slide still gets its file
    r = h5coords.read_features(p)
    assert r['features'].shape == (0, 256) and r['coords'].shape == (0, 2)
    with pytest.raises(ValueError):
        h5coords.write_features(p, f[:3], c)


def _slide_dir(tmp_path, names, patch_level=0):
    from nuhtc_amd import slides
    h5dir, sdir = tmp_path / 'h5', tmp_path / 'wsi'
    (h5dir / 'patches').mkdir(parents=True)
    sdir.mkdir()
    rng = np.random.default_rng(2)
    for name in names:
        np.save(sdir / (name + '.npy'), rng.integers(0, 256, (200, 300, 3), dtype=np.uint8))
        c = np.array([[0, 0], [64, 0], [128, 64], [256, 150], [10, 20]], np.int64)
        slides.save_coords(slides.coords_path(str(h5dir / 'patches'), name), c, 64, patch_level, name)
    with open(tmp_path / 'list.csv', 'w') as f:
        f.write('slide_id,process\n' + ''.join(f'{n}.npy,1\n' for n in names))
    return h5dir, sdir


def test_csv_loop_and_pt_auto_skip(tmp_path):
    """The slide loop with a stubbed device step: one .h5 + .pt per CSV row, rows in coordinate order, a second run skips the slides
    whose .pt exists, --no_auto_skip redoes them, the host batch size and the number of ranks change nothing."""
    import torch
    from nuhtc_amd import h5coords
    tool = _tool()
    h5dir, sdir = _slide_dir(tmp_path, ['a', 'b'])
    seen = []

    def stub(bag, lo, hi):          # a row that identifies the tile: its origin and the mean of its pixels
        t = bag.read(lo, hi)
        seen.append((lo, hi))
        return np.concatenate([bag.coords[lo:hi].astype(np.float32), t.reshape(len(t), -1).mean(1, keepdims=True).astype(np.float32),
                               np.zeros((hi - lo, 253), np.float32)], 1)
    argv = f'--config m.py --data_h5_dir {h5dir} --data_slide_dir {sdir} --slide_ext .npy --csv_path {tmp_path / "list.csv"} --feat_dir {tmp_path / "out"}'
    args = tool.parse_args(argv.split())
    tool.check_args(args)
    assert tool.run(args, feat_fn=stub, log=lambda *a: None) == [('a', 'done'), ('b', 'done')]
    out = tmp_path / 'out'
    for name in 'ab':
        pt = torch.load(out / 'pt_files' / f'{name}.pt')
        assert pt.dtype == torch.float32 and tuple(pt.shape) == (5, 256)
        if h5coords.available():
            r = h5coords.read_features(str(out / 'h5_files' / f'{name}.h5'))
            assert np.array_equal(r['features'], pt.numpy())
            assert np.array_equal(r['coords'], [[0, 0], [64, 0], [128, 64], [256, 150], [10, 20]])
        assert np.array_equal(pt[:, :2].numpy(), [[0, 0], [64, 0], [128, 64], [256, 150], [10, 20]])
    assert tool.run(args, feat_fn=stub, log=lambda *a: None) == [('a', 'skipped'), ('b', 'skipped')]
    os.remove(out / 'pt_files' / 'b.pt')
    assert tool.run(args, feat_fn=stub, log=lambda *a: None) == [('a', 'skipped'), ('b', 'done')]
    before = torch.load(out / 'pt_files' / 'a.pt')
    args2 = tool.parse_args((argv + ' --no_auto_skip --batch_size 2').split())
    assert tool.run(args2, feat_fn=stub, log=lambda *a: None) == [('a', 'done'), ('b', 'done')]
    assert torch.equal(torch.load(out / 'pt_files' / 'a.pt'), before)
    # shards of two ranks (the gather itself is one process here): rank 1 computes [3, 5)
    from nuhtc_amd import features, slides, tilestore
    c, ps, _ = slides.load_coords(str(h5dir / 'patches'), 'a')
    bag = tilestore.TileBag(slides.open_array_slide(str(sdir / 'a.npy')), c, ps)
    seen.clear()
    assert features.slide_features(None, bag, rank=1, world=2, feat_fn=stub) is None and seen == [(3, 5)]


def test_missing_slide_is_reported_and_level_must_be_zero(tmp_path):
    tool = _tool()
    h5dir, sdir = _slide_dir(tmp_path, ['a', 'b'])
    os.remove(sdir / 'a.npy')
    logs = []
    args = tool.parse_args(f'--config m.py --data_h5_dir {h5dir} --data_slide_dir {sdir} --slide_ext .npy --csv_path {tmp_path / "list.csv"} '
                           f'--feat_dir {tmp_path / "out"}'.split())
    res = tool.run(args, feat_fn=lambda bag, lo, hi: np.zeros((hi - lo, 256), np.float32), log=lambda *a: logs.append(' '.join(map(str, a))))
    assert res == [('a', 'error'), ('b', 'done')] and any(l.startswith('ERROR: a.h5') for l in logs)
    h5dir, sdir = _slide_dir(tmp_path / 'l1', ['c'], patch_level=1)
    args = tool.parse_args(f'--config m.py --data_h5_dir {h5dir} --data_slide_dir {sdir} --slide_ext .npy --csv_path {tmp_path / "l1" / "list.csv"} '
                           f'--feat_dir {tmp_path / "out1"}'.split())
    with pytest.raises(SystemExit, match='patch_level 1'):
        tool.run(args, feat_fn=lambda bag, lo, hi: np.zeros((hi - lo, 256), np.float32), log=lambda *a: None)
