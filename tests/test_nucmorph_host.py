"""Host tests of the per-nucleus morphometry (nuhtc_amd/nucmorph.py): the numpy restatement and the float64 derivation pinned to
scikit-image's regionprops on designed masks (tests/golden/nucmorph_skimage.npz, written by tools/dev/make_morph_golden.py), the
histogram statistics against numpy on the expanded pixel list, the degenerate cases, the stain table, the file and the tool's flag."""
import math
import os
import sys

import numpy as np
import pytest

from nuhtc_amd import nucmorph as nm

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucmorph_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'nucmorph_skimage.npz')
# largest relative difference between derive() and skimage 0.18.3 over the float properties of the designed masks with lambda1 != lambda2
# and A > 2, measured when the fixture was made (Size.MinorAxisLength of 'two blobs'); the test asserts 16 times it (the same float64 formulas summed in another order)
MEASURED_REL = 1.456e-15
COL = {c: i for i, c in enumerate(nm.COLUMNS)}


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def measured(golden):
    """name -> (raw, values row) of every designed mask on a random tile."""
    out = {}
    for name, m in cases.all_masks().items():
        raw, hist = nm.morph_reference(cases.tiles(*m.shape)['random'], m)
        out[name] = (raw, nm.derive(raw, hist)[1][0])
    return out


def test_fixture_holds_the_designed_masks(golden):
    masks = cases.all_masks()
    assert golden['names'].tolist() == list(masks) and str(golden['skimage_version']).startswith('0.18')
    for i, m in enumerate(masks.values()):
        h, w = golden[f'shape_{i}']
        assert np.array_equal(np.unpackbits(golden[f'mask_{i}'], axis=-1, bitorder='little')[:, :w].astype(bool), m) and m.shape == (h, w)


def test_integers_against_skimage(golden, measured):
    for i, name in enumerate(golden['names'].tolist()):
        raw, val = measured[name]
        if not golden['has_region'][i]:
            assert not raw.any() and not val.any(), name
            continue
        r0, c0, r1, c1 = golden['bbox'][i]
        assert raw[nm.I_A] == golden['area'][i] and (raw[nm.I_X0], raw[nm.I_Y0], raw[nm.I_X1], raw[nm.I_Y1]) == (c0, r0, c1, r1), name
        # the perimeter recomputed from (n1, n2, n3) with skimage's weights: the same three products, so the same float -- EQUAL
        per = raw[nm.I_N1] * 1.0 + raw[nm.I_N2] * math.sqrt(2) + raw[nm.I_N3] * ((1 + math.sqrt(2)) / 2)
        assert per == golden['perimeter'][i], (name, per, golden['perimeter'][i])
        assert val[COL['Size.Perimeter']] == per, name
        assert val[COL['Size.Area']] == golden['area'][i] and val[COL['Identifier.Xmax']] == c1 and val[COL['Identifier.Ymin']] == r0, name


def test_floats_against_skimage(golden, measured):
    """Largest relative difference seen over all float properties of the 7 designed masks with lambda1 != lambda2 and A > 2: 1.456e-15
    (Size.MinorAxisLength of 'two blobs': 17.082104956778863 against skimage's 17.08210495677884); asserted at 16 x that (MEASURED_REL)."""
    pairs = {'Size.MajorAxisLength': 'major_axis_length', 'Size.MinorAxisLength': 'minor_axis_length', 'Shape.Eccentricity': 'eccentricity',
             'Orientation.Orientation': 'orientation', 'Shape.Extent': 'extent', 'Shape.EquivalentDiameter': 'equivalent_diameter'}
    worst, where, used = 0.0, None, 0
    for i, name in enumerate(golden['names'].tolist()):
        raw, val = measured[name]
        A = int(raw[nm.I_A])
        if A <= 2:
            continue
        n20, n02 = A * int(raw[nm.I_SXX]) - int(raw[nm.I_SX]) ** 2, A * int(raw[nm.I_SYY]) - int(raw[nm.I_SY]) ** 2
        n11 = A * int(raw[nm.I_SXY]) - int(raw[nm.I_SX]) * int(raw[nm.I_SY])
        if n11 == 0 and n20 == n02:                       # lambda1 == lambda2: orientation and eccentricity are conventions
            continue
        used += 1
        got = {c: val[COL[c]] for c in pairs}
        got['cx'], got['cy'] = val[COL['Identifier.CentroidX']], val[COL['Identifier.CentroidY']]
        want = {c: float(golden[k][i]) for c, k in pairs.items()}
        want['cy'], want['cx'] = (float(v) for v in golden['centroid'][i])
        for c in got:
            rel = abs(got[c] - want[c]) / max(abs(want[c]), 1e-300) if got[c] != want[c] else 0.0
            if rel > worst:
                worst, where = rel, (name, c, got[c], want[c])
    print(f'{used} masks, largest relative difference {worst:.3e} at {where}')
    assert used >= 7
    assert worst <= 16 * MEASURED_REL, (worst, where)


def _expanded_stats(x):
    """The intensity statistics of derive() straight from the sample list, with numpy."""
    x = np.asarray(x, np.float64)
    mean, med = x.mean(), np.median(x)
    d = x - mean
    m2, m3, m4 = (d ** 2).mean(), (d ** 3).mean(), (d ** 4).mean()
    p = np.bincount(x.astype(np.int64), minlength=256) / len(x)
    p = p[p > 0]
    return {'Min': x.min(), 'Max': x.max(), 'Mean': mean, 'Median': med, 'MeanMedianDiff': mean - med, 'Std': x.std(),
            'IQR': np.percentile(x, 75) - np.percentile(x, 25), 'MAD': np.median(np.abs(x - med)),
            'Skewness': m3 / m2 ** 1.5 if m2 > 0 else 0.0, 'Kurtosis': m4 / m2 ** 2 - 3.0 if m2 > 0 else 0.0,
            'HistEnergy': (p * p).sum(), 'HistEntropy': -(p * np.log(p)).sum()}


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 8, 37, 400, 1001])
def test_histogram_statistics_against_the_pixel_list(n):
    rng = np.random.default_rng(n)
    for x in (rng.integers(0, 256, n), np.clip(rng.gamma(2.0, 20.0, n), 0, 255).astype(np.int64), rng.integers(100, 104, n), np.full(n, 77)):
        raw = np.zeros(16, np.int64)
        raw[nm.I_A], raw[nm.I_X1], raw[nm.I_Y1], raw[nm.I_HULL2] = n, n, 1, 2 * n
        val = nm.derive(raw, np.bincount(x, minlength=256))[1][0]
        want = _expanded_stats(x)
        for k, w in want.items():
            g = val[COL['Nucleus.Intensity.' + k]]
            if k in ('Min', 'Max', 'Median', 'IQR', 'MAD'):
                assert g == w, (k, n, g, w)
            else:
                assert abs(g - w) <= 1e-12 * abs(w), (k, n, g, w)


def test_degenerate_cases_are_finite_and_defined():
    masks = cases.small_masks()
    tile = cases.tiles(cases.H_SMALL, cases.W_SMALL)['random']
    rows = {k: nm.morph_reference(tile, m) for k, m in masks.items()}
    for tname, t in cases.tiles(cases.H_SMALL, cases.W_SMALL).items():       # constant tiles: no intensity variance
        for k, m in masks.items():
            cols, val = nm.derive(*nm.morph_reference(t, m), origin=(1000, 2000))
            assert cols == nm.COLUMNS and val.shape == (1, len(nm.COLUMNS)) and np.isfinite(val).all(), (tname, k)
    v = lambda name, c: nm.derive(*rows[name])[1][0][COL[c]]
    assert not nm.derive(*rows['empty'])[1].any()                                               # A == 0: zeros
    for c, w in {'Size.Area': 1, 'Size.Perimeter': 0, 'Shape.Circularity': 0, 'Size.MajorAxisLength': 0, 'Size.MinorAxisLength': 0, 'Shape.Eccentricity': 0,
                 'Shape.MinorMajorAxisRatio': 1, 'Orientation.Orientation': 0, 'Shape.Extent': 1, 'Shape.Solidity': 1, 'Nucleus.Intensity.Std': 0,
                 'Nucleus.Intensity.Skewness': 0, 'Nucleus.Intensity.Kurtosis': 0, 'Nucleus.Intensity.HistEnergy': 1, 'Nucleus.Intensity.HistEntropy': 0}.items():
        assert v('pixel', c) == w, c                                                            # A == 1: P == 0, lambda1 == lambda2 == 0
    assert v('disc r=7', 'Orientation.Orientation') == 0 and v('disc r=7', 'Shape.Eccentricity') == 0        # lambda1 == lambda2 > 0
    assert v('disc r=7', 'Shape.MinorMajorAxisRatio') == 1 and v('disc r=7', 'Shape.Solidity') < 1
    assert v('horizontal line', 'Size.MinorAxisLength') == 0 and v('horizontal line', 'Shape.Eccentricity') == 1
    assert v('annulus', 'Shape.Solidity') < 0.8 and v('two blobs', 'Shape.Solidity') < 0.5
    # slide coordinates: the origin shifts the position columns and nothing else
    a, b = nm.derive(*rows['annulus'])[1][0], nm.derive(*rows['annulus'], origin=(1000, 2000))[1][0]
    shift = {'Identifier.CentroidX': 1000, 'Identifier.Xmin': 1000, 'Identifier.Xmax': 1000, 'Identifier.CentroidY': 2000, 'Identifier.Ymin': 2000, 'Identifier.Ymax': 2000}
    assert all(b[COL[c]] - a[COL[c]] == shift.get(c, 0) for c in nm.COLUMNS)


def test_hull_against_qhull_and_the_crack_length():
    from scipy.spatial import ConvexHull
    for name, m in cases.all_masks().items():
        raw, _ = nm.morph_reference(np.zeros(m.shape + (3,), np.uint8), m)
        ys, xs = np.nonzero(m)
        if len(ys) == 0:
            assert raw[nm.I_HULL2] == 0
            continue
        pts = np.concatenate([np.stack([xs + dx, ys + dy], 1) for dx in (0, 1) for dy in (0, 1)])
        assert raw[nm.I_HULL2] == int(round(2 * ConvexHull(pts).volume)), name
        assert raw[nm.I_HULL2] >= 2 * raw[nm.I_A], name
        # every set pixel has four sides: the ones that are no crack are shared by two set pixels
        inner = int((m[:, 1:] & m[:, :-1]).sum() + (m[1:] & m[:-1]).sum())
        assert raw[nm.I_E] == 4 * raw[nm.I_A] - 2 * inner, name
    full = nm.morph_reference(np.zeros((256, 256, 3), np.uint8), np.ones((256, 256), bool))[0]
    # (the sums of a 256-px frame still fit 32 bits, A * Sxx of the central moments does not; the GPU tests add a 1024-px frame whose Sxx does not)
    assert full[nm.I_E] == 4 * 256 and full[nm.I_A] * full[nm.I_SXX] > 2 ** 32 and full[nm.I_HULL2] == 2 * 256 * 256


def test_stain_table_and_value():
    lut, k = nm.stain_constants()
    assert lut.dtype == np.int32 and lut.shape == (256,) and (np.diff(lut) <= 0).all() and lut[255] == 0 and lut[0] == lut[1]
    assert lut.max() < 2 ** 19 and np.abs(k).max() < 2 ** 19
    assert nm.haematoxylin(np.array([255, 255, 255], np.uint8)) == 0                                 # white: no stain
    hem = np.array([0.65, 0.70, 0.29]) / np.linalg.norm([0.65, 0.70, 0.29])
    for od in (0.5, 1.0, 2.0):                                                                       # pure haematoxylin of density od
        rgb = np.rint(255 * np.exp(-od * hem)).astype(np.uint8)
        assert abs(int(nm.haematoxylin(rgb)) - od * 255 / math.log(255)) <= 2.0, od
    eos = np.array([0.07, 0.99, 0.11]) / np.linalg.norm([0.07, 0.99, 0.11])
    assert int(nm.haematoxylin(np.rint(255 * np.exp(-1.0 * eos)).astype(np.uint8))) <= 2             # pure eosin: none
    h = nm.haematoxylin(cases.tiles(16, 16)['random'])
    assert h.min() >= 0 and h.max() <= 255 and h.dtype == np.int64


def test_rows_and_npz_round_trip(tmp_path):
    masks = cases.small_masks()
    tile = cases.tiles(cases.H_SMALL, cases.W_SMALL)['random']
    pairs = [nm.morph_reference(tile, m) for m in masks.values()]
    raw, hist = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]).astype(np.int32)
    origin = np.stack([np.arange(len(raw)) * 48, np.arange(len(raw)) * 96 + 5], 1)
    r2, h2, o2 = nm.unpack_rows(nm.pack_rows(raw, hist, origin))
    assert nm.pack_rows(raw, hist, origin).shape == (len(raw), nm.ROW)
    assert np.array_equal(r2, raw) and np.array_equal(h2, hist) and np.array_equal(o2, origin) and h2.dtype == np.int32
    ids, label, score = np.arange(len(raw))[::-1], np.arange(len(raw)) % 5, np.linspace(0.1, 0.9, len(raw))
    t = nm.read_npz(nm.write_npz(str(tmp_path / 't.npz'), ids, raw, hist, label, score, origin))
    assert t['columns'].tolist() == list(nm.COLUMNS) and t['values'].dtype == np.float64 and t['values'].shape == (len(raw), len(nm.COLUMNS))
    assert np.array_equal(t['values'], nm.derive(raw, hist, origin)[1]) and np.isfinite(t['values']).all()
    assert t['raw'].dtype == np.int64 and t['hist'].dtype == np.int32 and np.array_equal(t['raw'], raw) and np.array_equal(t['hist'], hist)
    assert np.array_equal(t['nuclei_id'], ids) and np.array_equal(t['label'], label) and np.array_equal(t['score'], score) and np.array_equal(t['origin'], origin)
    with pytest.raises(ValueError):
        nm.write_npz(str(tmp_path / 'bad.npz'), ids[:-1], raw, hist, label, score)
    with pytest.raises(ValueError):
        nm.derive(raw, hist[:, ::-1] * 2)                         # a histogram that does not hold A samples


def test_cli_flag():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import infer_wsi
    p = infer_wsi.build_parser()
    base = ['slide.npy', 'cfg.py', 'w.pth']
    assert p.parse_args(base).nuclei_morph is False
    a = p.parse_args(base + ['--nuclei-morph', '--nuclei-feat', '--nuclei-graph', '--merge'])
    assert a.nuclei_morph is True and a.nuclei_feat is True and a.nuclei_graph is True
