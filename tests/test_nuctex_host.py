"""Host tests of the per-nucleus texture (nuhtc_amd/nuctex.py): the numpy restatement of the co-occurrence counts pinned to
scikit-image's greycomatrix on designed masks (tests/golden/nuctex_skimage.npz, written by tools/dev/make_texture_golden.py), derive()
against greycoprops of that fixture and against a second, plain-loop float64 restatement of all 13 formulas written here, the degenerate
rows, the triangle index, the row packing, the file and the tool's flag."""
import math
import os
import sys

import numpy as np
import pytest

from nuhtc_amd import nuctex as nt

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nuctex_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'nuctex_skimage.npz')
# Largest differences measured on the CPU when the tests were written, over every designed mask with pairs on the tiles named; each test
# asserts 16 times its figure (the same float64 formulas summed in another order).  Relative, except for the features of order 1 that
# come out of a cancellation (Correlation, IMC1, IMC2), which are held by their absolute difference.
MEASURED_SKIMAGE = {'ASM': 4.200e-16, 'Contrast': 3.557e-16, 'Correlation': 2.221e-16, 'IDM': 2.346e-16}   # against greycoprops (random and ramp tiles)
MEASURED_LOOP_REL = 3.776e-15   # ASM of 'touches four edges' on the random tile, offset (0, 1); against the plain loops, the ten relative features
MEASURED_LOOP_ABS = 2.601e-14   # IMC2 of 'full frame' on the random tile, offset (1, 0): 1 - exp(-2 (HXY2 - HXY)) with HXY2 - HXY = 0.026; Correlation, IMC1, IMC2
ABSOLUTE = ('Correlation', 'IMC1', 'IMC2')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def counted():
    """(tile name, mask name) -> T int64 (2, 136) of every designed mask on every tile."""
    tiles, masks = cases.tiles(cases.H_SMALL, cases.W_SMALL), cases.small_masks()
    return {(t, k): nt.glcm_reference(tile, m) for t, tile in tiles.items() for k, m in masks.items()}


def _per_offset(T):
    """The 13 features of each offset alone, (2, 13): derive() of a record whose two offsets hold the same counts has Mean = the value."""
    return np.stack([nt.derive(np.stack([T[o], T[o]]))[1][0, 0::2] for o in range(2)])


def test_fixture_holds_the_designed_masks_and_levels(golden):
    masks, tiles = cases.small_masks(), cases.tiles(cases.H_SMALL, cases.W_SMALL)
    assert golden['names'].tolist() == list(masks) and golden['tiles'].tolist() == list(cases.GOLDEN_TILES) and str(golden['skimage_version']).startswith('0.18')
    for i, m in enumerate(masks.values()):
        assert np.array_equal(np.unpackbits(golden['masks'][i], axis=-1, bitorder='little')[:, :cases.W_SMALL].astype(bool), m)
    for t in cases.GOLDEN_TILES:
        assert np.array_equal(golden[f'levels_{t}'], nt.levels(tiles[t]))
    # what the tiles were designed to hold: all 16 levels; ten adjacent ones; one level each
    assert np.unique(nt.levels(tiles['random'])).tolist() == list(range(16))
    assert np.unique(nt.levels(tiles['ramp'])).tolist() == list(range(10))
    assert all(len(np.unique(nt.levels(tiles[t]))) == 1 for t in ('zeros', 'full', 'planes'))


def test_counts_equal_skimage(golden, counted):
    for t, tname in enumerate(golden['tiles'].tolist()):
        for i, name in enumerate(golden['names'].tolist()):
            assert np.array_equal(nt.full_matrix(counted[tname, name]), golden['glcm'][t, i]), (tname, name)
    k = {n: i for i, n in enumerate(golden['names'].tolist())}
    assert golden['glcm'][:, k['full frame']].sum() == 2 * 2 * (64 * 39 + 63 * 40) and not golden['glcm'][:, k['checkerboard']].any()
    assert (golden['glcm'][:, k['1x2 pair']].sum((-1, -2)) == [2, 0]).all() and (golden['glcm'][:, k['2x1 pair']].sum((-1, -2)) == [0, 2]).all()
    # on the ramp every pair lies on the diagonal or next to it
    i, j = np.mgrid[0:16, 0:16]
    assert not golden['glcm'][1][..., np.abs(i - j) > 1].any() and golden['glcm'][1][..., np.abs(i - j) == 1].any()


def test_derive_against_greycoprops(golden, counted):
    """ASM, Contrast, Correlation and IDM of every offset with pairs against skimage's greycoprops ('ASM', 'contrast', 'correlation',
    'homogeneity') of the same normalised matrix.  Largest differences measured: MEASURED_SKIMAGE; asserted at 16 x."""
    ours = {'ASM': 0, 'Contrast': 1, 'Correlation': 2, 'IDM': 3}
    worst, used = {k: 0.0 for k in ours}, 0
    for t, tname in enumerate(golden['tiles'].tolist()):
        for i, name in enumerate(golden['names'].tolist()):
            f = _per_offset(counted[tname, name])
            for o in range(2):
                if not counted[tname, name][o].any():
                    assert not f[o].any() and not golden['props'][t, i, o].any()
                    continue
                used += 1
                for k, c in ours.items():
                    got, want = f[o, nt.NAMES.index(k)], golden['props'][t, i, o, c]
                    diff = abs(got - want) if k in ABSOLUTE else (abs(got - want) / abs(want) if got != want else 0.0)
                    worst[k] = max(worst[k], diff)
    print(f'{used} matrices; largest differences {worst}')
    assert used == 42                      # 2 tiles x the 21 (mask, offset) of the designed masks that hold a pair
    for k in ours:
        assert worst[k] <= 16 * MEASURED_SKIMAGE[k], (k, worst[k])


def _loops(G):
    """The 13 features of one symmetric matrix of counts in plain Python loops, float64, straight from the formulas (Haralick 1973;
    0-based levels, natural logarithm, 0 log 0 = 0, the degenerate cases of nuhtc_amd/nuctex.py)."""
    n = len(G)
    tot = float(sum(sum(int(v) for v in row) for row in G))
    if tot == 0:
        return [0.0] * 13
    p = [[int(G[i][j]) / tot for j in range(n)] for i in range(n)]
    xlogx = lambda v: v * math.log(v) if v > 0 else 0.0
    px = [sum(p[i]) for i in range(n)]
    py = [sum(p[i][j] for i in range(n)) for j in range(n)]
    mux, muy = sum(i * px[i] for i in range(n)), sum(j * py[j] for j in range(n))
    vx, vy = sum((i - mux) ** 2 * px[i] for i in range(n)), sum((j - muy) ** 2 * py[j] for j in range(n))
    asm = sum(v * v for row in p for v in row)
    contrast = sum((i - j) ** 2 * p[i][j] for i in range(n) for j in range(n))
    if sum(1 for v in px if v > 0) == 1:
        corr = 1.0
    else:
        corr = (sum(i * j * p[i][j] for i in range(n) for j in range(n)) - mux * muy) / math.sqrt(vx * vy)
    sos = sum((i - mux) ** 2 * p[i][j] for i in range(n) for j in range(n))
    idm = sum(p[i][j] / (1 + (i - j) ** 2) for i in range(n) for j in range(n))
    ps = [sum(p[i][k - i] for i in range(n) if 0 <= k - i < n) for k in range(2 * n - 1)]
    pd = [sum(p[i][j] for i in range(n) for j in range(n) if abs(i - j) == k) for k in range(n)]
    savg = sum(k * ps[k] for k in range(2 * n - 1))
    svar = sum((k - savg) ** 2 * ps[k] for k in range(2 * n - 1))
    sent = -sum(xlogx(v) for v in ps)
    ent = -sum(xlogx(v) for row in p for v in row)
    dmean = sum(k * pd[k] for k in range(n))
    dvar = sum((k - dmean) ** 2 * pd[k] for k in range(n))
    dent = -sum(xlogx(v) for v in pd)
    hx, hy = -sum(xlogx(v) for v in px), -sum(xlogx(v) for v in py)
    hxy1 = -sum(p[i][j] * math.log(px[i] * py[j]) for i in range(n) for j in range(n) if p[i][j] > 0)
    hxy2 = -sum(xlogx(px[i] * py[j]) for i in range(n) for j in range(n))
    imc1 = (ent - hxy1) / max(hx, hy) if max(hx, hy) > 0 else 0.0
    imc2 = math.sqrt(max(0.0, 1.0 - math.exp(-2.0 * (hxy2 - ent))))
    return [asm, contrast, corr, sos, idm, savg, svar, sent, ent, dvar, dent, imc1, imc2]


def test_derive_against_plain_loops(counted):
    """All 13 features of every offset of every designed mask on the random, ramp and planes tiles against _loops.  Largest relative
    difference over the ten features held relatively: MEASURED_LOOP_REL; largest absolute difference of Correlation, IMC1, IMC2:
    MEASURED_LOOP_ABS; each asserted at 16 x."""
    rel, ab, where = 0.0, 0.0, [None, None]
    for (tname, name), T in counted.items():
        if tname not in ('random', 'ramp', 'planes'):
            continue
        f, G = _per_offset(T), nt.full_matrix(T)
        for o in range(2):
            want = _loops(G[o].tolist())
            for k, nm_ in enumerate(nt.NAMES):
                got = f[o, k]
                if nm_ in ABSOLUTE:
                    if abs(got - want[k]) > ab:
                        ab, where[1] = abs(got - want[k]), (tname, name, o, nm_, got, want[k])
                elif got != want[k] and abs(got - want[k]) / abs(want[k]) > rel:
                    rel, where[0] = abs(got - want[k]) / abs(want[k]), (tname, name, o, nm_, got, want[k])
    print(f'largest relative difference {rel:.3e} at {where[0]}; largest absolute difference {ab:.3e} at {where[1]}')
    assert rel <= 16 * MEASURED_LOOP_REL, (rel, where[0])
    assert ab <= 16 * MEASURED_LOOP_ABS, (ab, where[1])


def test_mean_and_range_over_the_offsets(counted):
    T = counted['random', 'disc r=7']
    f = _per_offset(T)
    cols, val = nt.derive(T)
    assert cols == nt.COLUMNS and len(cols) == 26 and val.shape == (1, 26) and val.dtype == np.float64
    assert cols[:4] == ('Haralick.ASM.Mean', 'Haralick.ASM.Range', 'Haralick.Contrast.Mean', 'Haralick.Contrast.Range') and cols[-1] == 'Haralick.IMC2.Range'
    assert np.array_equal(val[0, 0::2], (f[0] + f[1]) / 2.0) and np.array_equal(val[0, 1::2], np.abs(f[0] - f[1]))
    many = nt.derive(np.stack([counted['random', k] for k in cases.small_masks()]))[1]
    assert np.array_equal(many[list(cases.small_masks()).index('disc r=7')], val[0])            # a row does not depend on its neighbours


def test_degenerate_rows_are_finite_and_defined(counted):
    for key, T in counted.items():
        val = nt.derive(T)[1]
        assert np.isfinite(val).all(), key
    col = {c: i for i, c in enumerate(nt.COLUMNS)}
    for name in ('empty', 'pixel', 'corner bottom right', 'checkerboard', 'diagonal line'):       # no 4-neighbour pair: a zero row
        assert not counted['random', name].any() and not nt.derive(counted['random', name])[1].any(), name
    # one offset without pairs: its 13 zeros enter Mean and Range
    T = counted['random', '1x2 pair']
    assert T[0].sum() == 1 and not T[1].any()
    f, val = _per_offset(T), nt.derive(T)[1][0]
    assert not f[1].any() and np.array_equal(val[0::2], f[0] / 2.0) and np.array_equal(val[1::2], np.abs(f[0]))
    # one level only (a constant tile): Correlation 1, ASM 1, IDM 1, IMC1 0 (HX = 0), IMC2 0, every entropy and variance 0
    val = nt.derive(counted['planes', 'disc r=7'])[1][0]
    want = {'ASM': 1, 'Contrast': 0, 'Correlation': 1, 'SumOfSquares': 0, 'IDM': 1, 'SumAverage': 14, 'SumVariance': 0, 'SumEntropy': 0, 'Entropy': 0,
            'DifferenceVariance': 0, 'DifferenceEntropy': 0, 'IMC1': 0, 'IMC2': 0}
    for k, w in want.items():
        assert val[col[f'Haralick.{k}.Mean']] == w and val[col[f'Haralick.{k}.Range']] == 0, k
    # a pair of two different levels: the two marginals are (1/2, 1/2), perfectly anti-correlated
    T = np.zeros((2, nt.CELLS), np.int64)
    T[:, nt.tri(3, 9)] = 1
    val = nt.derive(T)[1][0]
    assert val[col['Haralick.Correlation.Mean']] == -1 and val[col['Haralick.Contrast.Mean']] == 36 and val[col['Haralick.IMC2.Mean']] > 0.8


def test_triangle_index_and_matrix_sum(counted):
    cells = [nt.tri(a, b) for a in range(nt.L) for b in range(a, nt.L)]
    assert cells == list(range(nt.CELLS)) and nt.CELLS == 136                                   # a bijection, in row-major order
    a, b = np.triu_indices(nt.L)
    assert np.array_equal(nt.tri(a, b), np.arange(nt.CELLS))
    for key, T in counted.items():
        G = nt.full_matrix(T)
        m = cases.small_masks()[key[1]]
        pairs = np.array([(m[:, 1:] & m[:, :-1]).sum(), (m[1:] & m[:-1]).sum()])
        assert np.array_equal(G.sum((-1, -2)), 2 * pairs) and np.array_equal(T.sum(-1), pairs) and np.array_equal(G, np.swapaxes(G, -1, -2)), key


def test_rows_and_npz_round_trip(tmp_path, counted):
    glcm = np.stack([counted['random', k] for k in cases.small_masks()]).astype(np.int32)
    glcm[0, 1, 135] = 2 ** 31 - 1                                                               # the last count of a record, at the top of its range
    rows = nt.pack_rows(glcm)
    assert rows.shape == (len(glcm), nt.ROW) and rows.dtype == np.int64 and nt.ROW == 136
    back = nt.unpack_rows(rows)
    assert back.dtype == np.int32 and back.shape == glcm.shape and np.array_equal(back, glcm)
    assert nt.pack_rows(np.zeros((0, 2, 136), np.int32)).shape == (0, nt.ROW) and nt.unpack_rows(np.zeros((0, nt.ROW), np.int64)).shape == (0, 2, 136)
    glcm[0, 1, 135] = 0
    ids, label, score = np.arange(len(glcm))[::-1], np.arange(len(glcm)) % 5, np.linspace(0.1, 0.9, len(glcm))
    t = nt.read_npz(nt.write_npz(str(tmp_path / 't.npz'), ids, glcm, label, score))
    assert t['columns'].tolist() == list(nt.COLUMNS) and t['values'].dtype == np.float64 and t['values'].shape == (len(glcm), 26)
    assert np.array_equal(t['values'], nt.derive(glcm)[1]) and np.isfinite(t['values']).all()
    assert t['glcm'].dtype == np.int32 and np.array_equal(t['glcm'], glcm)
    assert np.array_equal(t['nuclei_id'], ids) and np.array_equal(t['label'], label) and np.array_equal(t['score'], score)
    with pytest.raises(ValueError):
        nt.write_npz(str(tmp_path / 'bad.npz'), ids[:-1], glcm, label, score)


def test_cli_flag():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import infer_wsi
    p = infer_wsi.build_parser()
    base = ['slide.npy', 'cfg.py', 'w.pth']
    assert p.parse_args(base).nuclei_texture is False
    a = p.parse_args(base + ['--nuclei-texture', '--nuclei-morph', '--nuclei-feat', '--merge'])
    assert a.nuclei_texture is True and a.nuclei_morph is True and a.nuclei_feat is True
