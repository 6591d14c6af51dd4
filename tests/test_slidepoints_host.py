"""The table of the per-slide point analyses (nuhtc_amd/slidepoints.py) against the command line of tools/infer_wsi.py, without a GPU: its
shape, and what `select` says of unusable arguments, of a missing GPU and of no flag at all."""
import importlib.util
import os
import sys

import pytest
import torch

from nuhtc_amd import slidepoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = ('graph', 'spatial', 'clusters', 'mst', 'proximity', 'density')
MODULES = ('cellgraph', 'spatial', 'clusters', 'mst', 'proximity', 'density')
BAD = {'graph': ['--graph-k', '33'], 'spatial': ['--spatial-bins', '33'], 'clusters': ['--cluster-min', '0'], 'mst': ['--mst-radius', '0.25'],
       'proximity': ['--proximity-radius', '9000'], 'density': ['--density-pitch', '0.25']}


@pytest.fixture(scope='module')
def tool():
    spec = importlib.util.spec_from_file_location('infer_wsi_for_slidepoints', os.path.join(ROOT, 'tools', 'infer_wsi.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(tool, *flags):
    return tool.parse_args(['slide.npy', 'config.py', 'weights.pth', *flags])


def test_table_shape(tool):
    assert tuple(a.cli for a in slidepoints.ANALYSES) == tuple('nuclei_' + w for w in WORDS)
    assert tuple(a.flag for a in slidepoints.ANALYSES) == tuple('--nuclei-' + w for w in WORDS)
    assert tuple(a.module for a in slidepoints.ANALYSES) == MODULES
    plain = _args(tool)
    for a in slidepoints.ANALYSES:
        assert getattr(plain, a.cli) is False, a.cli
        assert getattr(_args(tool, a.flag), a.cli) is True, a.flag
    suffixes = [a.suffix for a in slidepoints.ANALYSES]
    assert len(set(suffixes)) == len(suffixes) and all(s == f'_nuclei_{w}.npz' for s, w in zip(suffixes, WORDS))


@pytest.mark.parametrize('word', WORDS)
def test_bad_arguments_are_named_before_the_missing_gpu(tool, monkeypatch, word):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SystemExit) as bad:
        slidepoints.select(_args(tool, '--nuclei-' + word, *BAD[word]))
    text = str(bad.value)
    assert text.startswith(f'--nuclei-{word}: ') and 'no GPU' not in text, text
    with pytest.raises(SystemExit) as good:
        slidepoints.select(_args(tool, '--nuclei-' + word))
    assert str(good.value) == f'--nuclei-{word}: no GPU is visible (there is no fallback)'


def test_good_arguments_select_in_table_order(tool):
    flags = ['--nuclei-' + w for w in reversed(WORDS)] + ['--mst-by', 'class', '--cluster-radius', '12.5']
    chosen = slidepoints.select(_args(tool, *flags), need_gpu=False)
    assert [an.cli for an, _ in chosen] == ['nuclei_' + w for w in WORDS]
    params = {an.module: p for an, p in chosen}
    assert params['mst'] == (64.0, 1) and params['clusters'] == (12.5, 5, 0) and params['cellgraph'] == (64.0, 8)
    assert params['spatial'][0].tolist() == [16 * b for b in range(1, 33)] and params['density'] == (128.0, 64.0)


def test_no_flag_selects_nothing_and_imports_nothing(tool, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for name in MODULES:
        monkeypatch.delitem(sys.modules, 'nuhtc_amd.' + name, raising=False)
    assert slidepoints.select(_args(tool)) == ()
    assert not [name for name in MODULES if 'nuhtc_amd.' + name in sys.modules]
