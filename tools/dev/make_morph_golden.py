"""Writes tests/golden/nucmorph_skimage.npz: scikit-image's regionprops of the designed masks of tests/nucmorph_cases.py, which
tests/test_nucmorph_host.py pins nuhtc_amd.nucmorph (morph_reference + derive) to.  Needs scikit-image (the fixture in the tree was made
with 0.18.3), so it runs under an interpreter that has it -- the project's own environment need not:

    python tools/dev/make_morph_golden.py [out.npz]

Per mask (the empty one has no region: its row is zeros and `has_region` is 0): area, bbox (min_row, min_col, max_row, max_col), centroid
(row, col), perimeter, major_axis_length, minor_axis_length, eccentricity, orientation, extent, equivalent_diameter; the masks themselves
travel bit-packed, so the test can tell that it measures what skimage measured."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

FLOATS = ('perimeter', 'major_axis_length', 'minor_axis_length', 'eccentricity', 'orientation', 'extent', 'equivalent_diameter')


def main(out):
    import skimage
    from skimage.measure import regionprops
    import nucmorph_cases as cases
    masks = cases.all_masks()
    n = len(masks)
    z = dict(names=np.array(list(masks)), has_region=np.zeros(n, np.int64), area=np.zeros(n, np.int64), bbox=np.zeros((n, 4), np.int64),
             centroid=np.zeros((n, 2), np.float64), skimage_version=np.array(skimage.__version__))
    z.update({k: np.zeros(n, np.float64) for k in FLOATS})
    for i, (name, m) in enumerate(masks.items()):
        z[f'mask_{i}'] = np.packbits(m, axis=-1, bitorder='little')
        z[f'shape_{i}'] = np.array(m.shape, np.int64)
        if not m.any():
            continue
        (rp,) = regionprops(m.astype(np.uint8))          # the whole mask as ONE region, however many components it has
        z['has_region'][i] = 1
        z['area'][i], z['bbox'][i], z['centroid'][i] = rp.area, rp.bbox, rp.centroid
        for k in FLOATS:
            z[k][i] = getattr(rp, k)
    np.savez_compressed(out, **z)
    print(f'{out}: {n} masks, scikit-image {skimage.__version__}, numpy {np.__version__}')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'nucmorph_skimage.npz'))
