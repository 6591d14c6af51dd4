#!/usr/bin/env python
"""Same command line as the reference's tools/wsi_feat_extract.py: a per-nucleus feature table for every slide of a folder, from the
GeoJSON a detection run wrote, into <segdir>/<id>/nuclei_feat.db (SQLite, one table `nuclei_features`).

    python tools/wsi_feat_extract.py DATADIR --segdir SEGDIR [--start 0] [--end N] [--mag 40] [--reverse] [--bs_size 1024]
                                     [--num_workers 8] [--slide_ext .svs] [--geojson merged|plain] [--device 0]
                                     [--gradient [--edge-thr LEVELS]] [--shape] [--fsd]

For every slide id (the sorted, extension-stripped names in DATADIR, sliced as the reference slices them) it reads
<segdir>/<id>/<id>_merged.geojson (`--geojson plain`: <id>.geojson, whose nuclei_id is the position in the file), opens the slide as
tools/infer_wsi.py does (`.npy` array slides, tiled `.tif` / `.svs`) and measures every nucleus ON THE GPU (nuhtc_amd/ringfeat.py: the
slide is walked in blocks, frames are gathered and rings filled on the device, then the project's morphometry and texture kernels run).
There is no fallback without a GPU.  A slide without its GeoJSON is reported and skipped.

The table: Label (always 1), the 29 columns of nuhtc_amd/nucmorph.py and the 26 of nuhtc_amd/nuctex.py ('.' replaced by '_', as the
reference does), score, type, class_id, nuclei_id, x_min, y_min, x_max, y_max (the vertex extremes).  What those modules state holds here:
  * the intensity scale (Nucleus.Intensity.*) and the grey levels (Haralick.*) are THE PROJECT'S OWN fixed-point haematoxylin scale, not
    histomicstk's 8-bit stain image and crop-dependent grey limits: the columns have histomicstk's names and meaning, not its numbers;
  * Identifier.* are slide pixels at level 0;
  * of histomicstk's shape families, the Hu moments and the fractal dimension come with --shape and the Fourier descriptors
    (Shape.FSD1..6) with --fsd (both below): every histomicstk family is produced.  FSD is the
    only histomicstk family that is not produced from the mask: it is a function of the ordered ring.
--gradient adds the eight Nucleus.Gradient.* columns of nuhtc_amd/nucgrad.py between the Haralick columns and score: the gradient
magnitude of the same haematoxylin scale (Mag.Mean, Mag.Std in grey levels per pixel, Mag.Skewness, Mag.Kurtosis, Mag.HistEntropy and
Mag.HistEnergy of a ten-bin histogram over the nucleus's own range) and an edge count (Canny.Sum, Canny.Mean).  The edge count is THE
PROJECT'S OWN definition -- the mask pixels whose gradient is at least --edge-thr grey levels per pixel (default 0.25) and a local maximum
along its quantised direction; scikit-image's Canny with its Gaussian smoothing and hysteresis, which histomicstk calls, is NOT
reproduced: the two columns have its names and meaning, not its numbers.  The gradient is taken on a frame with a margin of 2 pixels
round the nucleus's rectangle (pixels beyond the slide read as zeros); a nucleus whose rectangle plus that margin exceeds 256 pixels has
NULL in the eight columns and is counted on stderr.  The other columns are the same bytes with and without the flag.
--shape adds the eight columns of nuhtc_amd/nucshape.py last among the feature columns (behind the gradient columns when both flags are
given, behind the Haralick columns otherwise, before score): Shape.HuMoments1..7, scikit-image's moments_hu of the mask (its (row,
column) convention, which decides the sign of the seventh), and Shape.FractalDimension, minus the slope of ln N on ln s over the box
sizes s = 4, 8, .. up to the rectangle's smaller side -- histomicstk's names and meaning; the box counts are the project's own definition
(boxes anchored at the rectangle's corner, written from the numpy-100 recipe histomicstk uses, not compared with histomicstk itself).
Both are functions of the mask alone and every measured nucleus has them: there is no NULL.  The other columns are the same bytes with
and without the flag.
--fsd adds the six columns of nuhtc_amd/nucfsd.py, Shape.FSD1..6, last among the feature columns (behind the shape columns when both flags
are given, before score): the share of six frequency bands in the spectrum of the boundary's tangent angle, taken at 128 points spaced
evenly along the perimeter.  histomicstk's names and meaning, THE PROJECT'S OWN DEFINITION, not compared with histomicstk: the ring is
walked in CONTOUR order (histomicstk hands its routine the boundary pixels in raster order), and the resampling is exact -- the GPU decides
in integers which edge of the ring holds each point (csrc/nucfsd.hip, on the rings the fill already uploaded).  Every measured nucleus
has them: there is no NULL.  The other columns are the same bytes with and without the flag.
Only TRACED RINGS are measured -- integer vertices on pixel centres, edges along the eight chain directions: what tools/infer_wsi.py
writes, here and in the reference.  The measured pixels are the ring's border and everything it encloses (holes filled).  Arbitrary
polygons (float coordinates, other edge directions), nuclei wider or taller than 256 pixels and rings that leave the slide are left out
and counted; the closing line on stderr gives, per slide, the rows written and the rows left out by reason.

Resume, as the reference: a database that already holds every nuclei_id of the file skips the slide; otherwise only the missing nuclei
are measured and appended.  A database whose columns differ from the requested ones (written without --gradient, --shape or --fsd and run with
it, or the other way round) is neither appended to nor altered: the slide is skipped with a message that names the file and the difference.
NOT as the reference: a database under 1 MB is kept -- the reference deletes it as broken, but a complete
small table is complete.

--mag is accepted for parity.  Rings are level-0 coordinates and are measured in level-0 pixels at every magnification (the reference
upsamples its crops by 40 / mag first); with --mag other than 40 that is said once on stderr.  --bs_size and --num_workers are accepted
and not used: batches are the blocks of the slide walk, and there is no worker pool."""
import json
import os
import sys
from argparse import ArgumentParser

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    """tools/wsi_feat_extract.py:239-250 of the reference, then flags of our own: three here, and those of every family of measurements
    that has any (nuhtc_amd.ringfeat.FAMILIES: --gradient and --edge-thr, --shape, --fsd, each defined beside what it selects)."""
    p = ArgumentParser(allow_abbrev=False)
    p.add_argument('datadir', help='path to folder containing raw wsi image files')
    p.add_argument('--segdir', help='path to folder containing segmentation files')
    p.add_argument('--start', type=int, default=0, help='start index')
    p.add_argument('--end', type=int, default=None, help='end index')
    p.add_argument('--mag', type=int, default=40, help='magnification of the slide')
    p.add_argument('--reverse', action='store_true', default=False, help='reverse the order of slide ids')
    p.add_argument('--bs_size', type=int, default=1024, help='batch size for nuclei feature extraction')
    p.add_argument('--num_workers', type=int, default=8, help='number of workers for parallel processing')
    # ---- not in the reference
    p.add_argument('--slide_ext', type=str, default='.svs', help='ext name of wsi (.svs, .tif, .npy)')
    p.add_argument('--geojson', choices=('merged', 'plain'), default='merged', help='<id>_merged.geojson or <id>.geojson')
    p.add_argument('--device', type=int, default=0, help='GPU of the measurement')
    from nuhtc_amd import ringfeat
    for fam in ringfeat.FAMILIES:
        if fam.flags:
            fam.flags(p)
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def slide_ids(datadir, start=0, end=None, reverse=False):
    """tools/wsi_feat_extract.py:132-141 of the reference: sorted, extension-stripped names, reversed first and sliced after."""
    ids = sorted(os.path.splitext(name)[0] for name in os.listdir(datadir))
    if reverse:
        ids = ids[::-1]
    return ids[start:end] if end is not None else ids[start:]


def extract_slide(slide_path, geojson_path, db_path, device=0, log=print, edge_thr=1, **keywords):
    """One slide -> (rows written, {reason: left out}, {keyword: nuclei without that family's columns}), or None when the table already
    holds every nucleus of the file.  keywords: gradient=, shape=, fsd= of nuhtc_amd.ringfeat (edge_thr in quarter grey levels); the
    third part has an entry per selected family that a nucleus can lack.  An existing table with another column set: a string that says
    what differs, and the file is not touched."""
    from nuhtc_amd import ringfeat, slides
    why = ringfeat.column_mismatch(db_path, **keywords)
    if why:
        return why
    with open(geojson_path) as f:
        features = json.load(f)
    every = [int(f['properties']['nuclei_id']) if 'nuclei_id' in (f.get('properties') or {}) else k for k, f in enumerate(features)]
    todo = set(ringfeat.missing_ids(db_path, every))
    if not todo:
        return None
    if len(todo) < len(every):
        log(f'skipped {len(every) - len(todo)}/{len(every)} nuclei')
        log(f'left {len(todo)} nuclei')
    # only the missing nuclei are measured, each under the id it has in the whole file (a nucleus left out before is tried, and left
    # out, again)
    features = [dict(f, properties=dict(f.get('properties') or {}, nuclei_id=i)) for f, i in zip(features, every) if i in todo]
    m = ringfeat.measure(slides.open_array_slide(slide_path), features, device=device, edge_thr=edge_thr, **keywords)
    _, values = ringfeat.table(m, **keywords)
    n = ringfeat.write_db(db_path, values, m['score'], m['type'], m['label'], m['nuclei_id'], m['rect'], **keywords)
    return n, m['left_out'], ringfeat.lacking(m, **keywords)


def main(argv=None):
    args = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('wsi_feat_extract.py needs a GPU (there is no fallback)')
    edge_thr = 1
    if args.gradient:
        from nuhtc_amd import nucgrad
        try:
            edge_thr = nucgrad.threshold(args.edge_thr)
        except ValueError as e:
            raise SystemExit(f'--edge-thr: {e}')
    if args.mag != 40:
        print(f'--mag {args.mag}: rings are level-0 coordinates and are measured in level-0 pixels; the reference would upsample every crop by '
              f'{40 / args.mag:g} first, this tool does not', file=sys.stderr)
    from nuhtc_amd import ringfeat
    keywords = {f.keyword: getattr(args, f.keyword) for f in ringfeat.FAMILIES if f.keyword}
    said = {f.keyword: f.lacking for f in ringfeat.FAMILIES}
    ids = slide_ids(args.datadir, args.start, args.end, args.reverse)
    suffix = '_merged.geojson' if args.geojson == 'merged' else '.geojson'
    report = []
    for k, sid in enumerate(ids):
        print(f'\n[{k + 1}/{len(ids)}]process: {sid}')
        gj = os.path.join(args.segdir, sid, sid + suffix)
        if not os.path.exists(gj):
            print(f'not found {sid}, skipped\n')
            continue
        spath = os.path.join(args.datadir, sid + args.slide_ext)
        if not os.path.exists(spath):
            print(f'no slide {spath}, skipped\n')
            continue
        db = os.path.join(args.segdir, sid, 'nuclei_feat.db')
        got = extract_slide(spath, gj, db, device=args.device, edge_thr=edge_thr, **keywords)
        if got is None:
            print(f'skipped:{sid}\n')
            continue
        if isinstance(got, str):
            print(f'skipped:{sid}: {db} was written with other columns and is left as it is ({got})\n')
            report.append(f'{sid}: skipped, {db} holds other columns ({got})')
            continue
        n, left, lack = got
        print(f'{sid}: {n} rows')
        report.append(f'{sid}: {n} rows written, left out ' + (', '.join(f'{v} {r}' for r, v in left.items() if v) or 'none') +
                      ''.join(f', {v} without {said[k]}' for k, v in lack.items() if v))
    print('; '.join(report) if report else 'no slide measured', file=sys.stderr)


if __name__ == '__main__':
    main()
