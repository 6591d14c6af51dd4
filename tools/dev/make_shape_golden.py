"""Writes tests/golden/nucshape_skimage.npz: scikit-image's regionprops(...).moments_hu of the random blobs of tests/nucshape_cases.py
(golden_blobs: 40 masks of 3 .. 60 pixels a side), which tests/test_nucshape_host.py pins nuhtc_amd.nucshape (shape_reference + derive) to.
Needs scikit-image (the fixture in the tree was made with 0.18.3, the version histomicstk's Hu moments come from), so it runs under an
interpreter that has it -- the project's own environment need not:

    python tools/dev/make_shape_golden.py [out.npz]

It needs numpy, skimage and the cases file.  The masks travel in the file (bit-packed, with their shapes), so the test can tell that it
measures what skimage measured.  Every mask is one region: regionprops(mask.astype(np.uint8)) labels the set pixels 1, connected or not,
as histomicstk hands a one-nucleus crop to it.  hu float64 (n, 7)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main(out):
    import skimage
    from skimage.measure import regionprops
    import nucshape_cases as cases
    masks = cases.golden_blobs()
    hu = np.zeros((len(masks), 7), np.float64)
    for i, m in enumerate(masks):
        props = regionprops(m.astype(np.uint8))
        assert len(props) == 1
        hu[i] = props[0].moments_hu
    np.savez_compressed(out, hu=hu, shapes=np.array([m.shape for m in masks], np.int64),
                        bits=np.concatenate([np.packbits(m.ravel(), bitorder='little') for m in masks]),
                        skimage_version=np.array(skimage.__version__))
    print(f'{out}: {len(masks)} masks, scikit-image {skimage.__version__}, numpy {np.__version__}')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'nucshape_skimage.npz'))
