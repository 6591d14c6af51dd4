"""Per-nucleus feature table from a WRITTEN GeoJSON: the reference's tools/wsi_feat_extract.py (one crop per nucleus, the polygon filled
into a mask, histomicstk on a CPU pool, an SQLite table `nuclei_features`) on the GPU.  The measurements are the project's existing
ones -- nuhtc_op_nucleus_morph and nuhtc_op_nucleus_texture, nucmorph.derive and nuctex.derive, all unchanged; this module is the path
in front of them and behind them:

    parse      GeoJSON features -> integer rings, rectangles, scores, labels, class names, nuclei_id
    measure    the slide in blocks, per block and frame size: nuhtc_op_frame_gather (slide pixels -> one frame per nucleus),
               nuhtc_op_ring_fill (ring -> bit mask, csrc/ringfeat.hip), the two measurement ops -> raw, hist, glcm (integers)
    table      nucmorph.derive beside nuctex.derive -> the named float64 columns
    write_db / read_db / missing_ids     the SQLite file and the reference's resume rule

Morphometry and texture are two of the five FAMILIES of measurements (the table below: what each is measured on, its C entry, its
integers, its columns); gradient=True, shape=True and fsd=True select the other three.  measure, table, table_columns, db_columns,
column_mismatch and write_db turn these keywords into a selection (`select`) at entry; everything below iterates that selection and
names no family.

What is measured is the nucleus the DOCUMENT describes: the traced ring with its holes filled (contours.fill_rings defines the pixel set;
the device equals it bit for bit), independent of the tile frames of the run that wrote it.  Only traced rings are measured -- integer
vertices, edges along the eight chain directions: what tools/infer_wsi.py writes, here and in the reference.  Anything else is left out
and counted by reason (REASONS).  Level 0 only: rings are level-0 coordinates.

A nucleus's frame is the square of side S = 32, 64, 128 or 256 (the smallest that holds its rectangle) whose corner is the rectangle's
minimum corner; raw is in frame pixels and `origin` is that corner, which derive needs for the Identifier.* columns (slide pixels).

Gradient frames (measure(gradient=True), `gradient_frames`).  The frames above have no margin, which is right for kernels that read only
the pixels under the mask and wrong for a gradient, which reads the neighbours of every mask pixel (histomicstk's crop has a margin of 5
pixels).  With the selection every nucleus ADDITIONALLY gets a gradient frame whose corner is max(rect_min - 2, 0) per axis and whose side
is the smallest of 32 / 64 / 128 / 256 that holds the rectangle and 2 pixels beyond it; ring fill and gather for these frames are the
same two ops in the same block walk and chunking (the block is read with 2 more pixels to the left and above), and the morphometry and
texture frames and their values are unchanged.  A nucleus whose rectangle plus margin exceeds 256 pixels has no gradient frame: its row
of `grad` is zero, `grad_ok` is False and the eight columns are NULL in the table.  Pixels of a gradient frame beyond the slide read as
zeros, as the gather defines: a nucleus within 2 pixels of the slide's right or lower edge sees a black margin there.

The measurement ops want an engine handle, but not a finalized one: nuhtc_create validates the config and allocates NOTHING on the
device (every allocation is nuhtc_finalize's), so measure() makes a handle from the default config, never finalizes it, and destroys it
on the way out.  No config file, no checkpoint."""
import ctypes
import os
import sqlite3
from collections import namedtuple

import numpy as np

from . import nucfsd, nucgrad, nucmorph, nucshape, nuctex
from .nuclei import stain_constants

SIDES = (32, 64, 128, 256)
MAX_SIDE = SIDES[-1]
HALO = MAX_SIDE                 # a block is read with this many pixels to the right and below: a frame never leaves its block's read
GRAD_MARGIN = 2                 # pixels of a gradient frame round the rectangle (the doubled central difference reads 1, the edge test 2)
CHUNK = 4096                    # the measurement ops' limit on B
REASONS = ('non_integer', 'no_ring', 'too_large', 'off_slide', 'not_traced')
TABLE = 'nuclei_features'
DB_NAME = 'nuclei_feat.db'


def bucket(side):
    """The frame side of a rectangle whose larger side is `side` pixels (1 .. 256)."""
    for s in SIDES:
        if side <= s:
            return s
    raise ValueError(f'a rectangle of side {side} has no frame (at most {MAX_SIDE})')


def parse(features):
    """GeoJSON features -> dict(rings: list of int32 (k, 2) without the closing vertex, rect int64 (n, 4) = x_min, y_min, x_max, y_max
    of the vertices (inclusive), score float64 (n,), label int64 (n,), type: list of str, nuclei_id int64 (n,), left_out: {reason:
    count}).  One entry per Polygon feature that can be measured; nuclei_id is properties.nuclei_id where present, the feature's
    position in the list otherwise.  Left out and counted: 'non_integer' (a coordinate that is not an integer), 'no_ring' (no ring,
    or a ring without a vertex), 'too_large' (a rectangle wider or taller than 256 pixels).  A feature that is no Polygon is skipped
    without a count."""
    left = {r: 0 for r in REASONS}
    rings, rect, score, label, kind, ids = [], [], [], [], [], []
    for pos, f in enumerate(features):
        geom = f.get('geometry') or {}
        if geom.get('type') != 'Polygon':
            continue
        coords = geom.get('coordinates') or []
        try:
            r = np.asarray(coords[0], np.float64) if len(coords) else np.zeros((0, 2))
        except (TypeError, ValueError):
            r = np.zeros((0, 2))
        if r.ndim != 2 or r.shape[1] != 2 or len(r) == 0:
            left['no_ring'] += 1
            continue
        if not np.isfinite(r).all() or not np.array_equal(r, np.rint(r)) or np.abs(r).max() >= 2 ** 30:
            left['non_integer'] += 1
            continue
        r = r.astype(np.int64)
        if len(r) > 1 and (r[0] == r[-1]).all():
            r = r[:-1]
        x0, y0, x1, y1 = int(r[:, 0].min()), int(r[:, 1].min()), int(r[:, 0].max()), int(r[:, 1].max())
        if x1 - x0 + 1 > MAX_SIDE or y1 - y0 + 1 > MAX_SIDE:
            left['too_large'] += 1
            continue
        props = f.get('properties') or {}
        rings.append(np.ascontiguousarray(r, np.int32))
        rect.append((x0, y0, x1, y1))
        score.append(float(props.get('score', 0.0)))
        label.append(int(props.get('label', 0)))
        kind.append(str((props.get('classification') or {}).get('name', '')))
        ids.append(int(props['nuclei_id']) if 'nuclei_id' in props else pos)
    return dict(rings=rings, rect=np.asarray(rect, np.int64).reshape(-1, 4), score=np.asarray(score, np.float64),
                label=np.asarray(label, np.int64), type=kind, nuclei_id=np.asarray(ids, np.int64), left_out=left)


def frame_sides(rect):
    """rect int (n, 4) -> int64 (n,): the frame side of every rectangle."""
    rect = np.asarray(rect, np.int64).reshape(-1, 4)
    side = np.maximum(rect[:, 2] - rect[:, 0], rect[:, 3] - rect[:, 1]) + 1
    return np.array([bucket(int(s)) for s in side], np.int64)


def gradient_frames(rect):
    """rect int (n, 4) -> (origin int64 (n, 2), side int64 (n,)): the gradient frame of every rectangle (module docstring) -- the corner
    max(rect_min - 2, 0) per axis and the smallest side that reaches 2 pixels beyond rect_max; side 0 where 256 is not enough."""
    rect = np.asarray(rect, np.int64).reshape(-1, 4)
    origin = np.maximum(rect[:, :2] - GRAD_MARGIN, 0)
    need = (rect[:, 2:] + GRAD_MARGIN + 1 - origin).max(1) if len(rect) else np.zeros(0, np.int64)
    return origin, np.array([bucket(int(s)) if s <= MAX_SIDE else 0 for s in need], np.int64)


def add_gradient_flags(parser):
    """The command-line form of the gradient selection (tools/wsi_feat_extract.py): --gradient and --edge-thr LEVELS, grey levels per
    pixel; nucgrad.threshold turns LEVELS into T."""
    parser.add_argument('--gradient', action='store_true', default=False,
                        help='add the eight Nucleus.Gradient.* columns (nuhtc_amd/nucgrad.py): the magnitude statistics, and Canny.Sum / Canny.Mean as '
                             'the project\'s own edge count (thresholded local maxima of the gradient; scikit-image\'s Canny is not reproduced)')
    parser.add_argument('--edge-thr', type=float, default=0.25, metavar='LEVELS',
                        help='with --gradient: the least gradient of an edge pixel in grey levels per pixel, 0.25 .. 360.5 in steps of 0.25')


def add_shape_flags(parser):
    """The command-line form of the shape selection (tools/wsi_feat_extract.py): --shape."""
    parser.add_argument('--shape', action='store_true', default=False,
                        help='add Shape.HuMoments1..7 (scikit-image\'s moments_hu, which histomicstk calls) and Shape.FractalDimension (histomicstk\'s '
                             'name and meaning; the box counts are the project\'s own definition, nuhtc_amd/nucshape.py) behind the other feature columns')


def add_fsd_flags(parser):
    """The command-line form of the Fourier-descriptor selection (tools/wsi_feat_extract.py): --fsd."""
    parser.add_argument('--fsd', action='store_true', default=False,
                        help='add Shape.FSD1..6 (histomicstk\'s names and meaning, the project\'s own definition, nuhtc_amd/nucfsd.py: the ring walked in '
                             'contour order and resampled exactly at 128 points; not compared with histomicstk) last among the feature columns')


# keyword   the argument of measure / table / table_columns / db_columns / column_mismatch / write_db that selects the family; None: always
# flags     parser -> None: adds the family's command-line flags (tools/wsi_feat_extract.py); None: it has none
# frame     the frames it is measured on, a Plan of PLANS: 'plain' (frame_sides, at the rectangle's corner) or 'margin' (gradient_frames)
# call      the C entry; reads: what it takes -- 'tiles' (the frames' pixels and the masks), 'masks', or 'rings' (the vertices and offsets
#           the fill uploaded: the ring, no frame; such a family rides on the plain frames' walk)
# ints      its extra integer arguments: (keyword of measure, least, most, what the values are called)
# fields    its result: (name in measure()'s dict, shape behind n, dtype)
# derive    (the fields of some nuclei, their origins (n, 2)) -> (columns, float64 (n, len(columns)))
# columns   the names of its table columns
# lacking   None: every measured nucleus has the family.  Otherwise what the tool's closing line calls a nucleus without its frame;
#           measure() then adds <first field>_ok and <first field>_origin, table() has NaN in its columns and write_db writes NULL
Family = namedtuple('Family', 'keyword flags frame call reads ints fields derive columns lacking')

MORPH = Family(None, None, 'plain', 'nuhtc_op_nucleus_morph', 'tiles', (), (('raw', (nucmorph.RAW,), 'int64'), ('hist', (nucmorph.BINS,), 'int32')),
               lambda f, origin: nucmorph.derive(f[0], f[1], origin), nucmorph.COLUMNS, None)
TEX = Family(None, None, 'plain', 'nuhtc_op_nucleus_texture', 'tiles', (), (('glcm', (len(nuctex.OFFSETS), nuctex.CELLS), 'int32'),),
             lambda f, origin: nuctex.derive(f[0]), nuctex.COLUMNS, None)
# the rows of nuhtc_amd.nucgrad on a second, wider frame per nucleus (module docstring), with the edge threshold `edge_thr` (quarter grey
# levels); a nucleus whose rectangle plus margin exceeds 256 pixels has no such frame: a zero row, grad_ok False, NULL in the eight columns
GRADIENT = Family('gradient', add_gradient_flags, 'margin', 'nuhtc_op_nucleus_gradient', 'tiles', (('edge_thr', nucgrad.T_MIN, nucgrad.T_MAX, 'quarter levels'),),
                  (('grad', (nucgrad.ROW,), 'int64'),), lambda f, origin: nucgrad.derive(f[0]), nucgrad.COLUMNS,
                  'gradient columns (rectangle plus margin over 256 px)')
# the rows of nuhtc_amd.nucshape (the seven Shape.HuMoments* and Shape.FractalDimension) on the masks of the morphometry: nothing outside
# the mask is read, so the plain frames serve, and every measured nucleus has its row
SHAPE = Family('shape', add_shape_flags, 'plain', 'nuhtc_op_nucleus_shape', 'masks', (), (('shape', (nucshape.ROW,), 'int64'),),
               lambda f, origin: nucshape.derive(f[0]), nucshape.COLUMNS, None)
# the rows of nuhtc_amd.nucfsd (the six Shape.FSD*) on the rings and offsets the fill already uploaded -- no mask, no frame, nothing more
# is uploaded; a ring the fill kept is traced, has a vertex and at most 256 pixels a side, so its row has the status 0 or 1: no NULL either
FSD = Family('fsd', add_fsd_flags, 'plain', 'nuhtc_op_ring_fsd', 'rings', (), (('fsd', (nucfsd.ROW,), 'int32'),),
             lambda f, origin: nucfsd.derive(f[0]), nucfsd.COLUMNS, None)
FAMILIES = (MORPH, TEX, GRADIENT, SHAPE, FSD)               # the order of the table's columns, and of the launches on one chunk of a plan's frames
EDGE_THR = nucgrad.T_DEFAULT                                # measure()'s default of the gradient's extra integer

# frame     the `frame` of the families measured on it
# frames    rect (n, 4) -> (origin int64 (n, 2), side int64 (n,); 0: the nucleus has no such frame)
# margin    pixels a frame may start before its rectangle: every block is read with so many more to the left and above
# strict    what the fill's status means.  True: 1 raises, 2 is counted 'not_traced' and the nucleus has no row in the result.  False: it is
#           ignored -- a ring that is not traced gives a zero mask and a zero row here, and the strict plan takes the nucleus out
Plan = namedtuple('Plan', 'frame frames margin strict')
PLANS = (Plan('plain', lambda rect: (rect[:, :2], frame_sides(rect)), 0, True), Plan('margin', gradient_frames, GRAD_MARGIN, False))


def select(**keywords):
    """gradient= / shape= / fsd= -> the selected families, in the order of FAMILIES whatever the order of the keywords; the families
    without a keyword are always among them.  TypeError for a keyword that selects no family."""
    for k in keywords:
        if k not in [f.keyword for f in FAMILIES if f.keyword]:
            raise TypeError(f'{k!r} selects no family of nuclei measurements (' + ', '.join(f.keyword for f in FAMILIES if f.keyword) + ')')
    return tuple(f for f in FAMILIES if f.keyword is None or keywords.get(f.keyword))


def _ok(fam):
    """The key of measure()'s result that says which nuclei have the family `fam` (one with `lacking`)."""
    return fam.fields[0][0] + '_ok'


def lacking(m, **keywords):
    """measure()'s result -> {keyword: the nuclei that lack that family's frame}, an entry per selected family with `lacking`."""
    return {f.keyword: int((~m[_ok(f)]).sum()) for f in select(**keywords) if f.lacking}


def block_plan(rect, slide_hw, block=2048):
    """The walk of measure(): -> (blocks, off_slide).  blocks: list of (x, y, w, h, idx) -- the part of the slide [x, x + w) x [y, y + h)
    that is read for the block (`block` pixels and a 256-pixel halo to the right and below, cut at the slide's edge) and the rows idx of
    `rect` it owns, row-major over the blocks that own any.  A nucleus belongs to the block that holds its rectangle's minimum corner;
    its rectangle is at most 256 pixels wide and tall, so it lies inside what the block reads.  off_slide: the rows whose rectangle
    leaves the slide (owned by no block)."""
    rect = np.asarray(rect, np.int64).reshape(-1, 4)
    H, W = int(slide_hw[0]), int(slide_hw[1])
    block = int(block)
    if block < 1:
        raise ValueError('block_plan: block must be positive')
    inside = (rect[:, 0] >= 0) & (rect[:, 1] >= 0) & (rect[:, 2] < W) & (rect[:, 3] < H)
    idx = np.nonzero(inside)[0]
    key = (rect[idx, 1] // block) * ((W + block - 1) // block + 1) + rect[idx, 0] // block
    order = np.argsort(key, kind='stable')
    blocks = []
    for k in np.unique(key):
        own = idx[order[np.searchsorted(key[order], k, 'left'):np.searchsorted(key[order], k, 'right')]]
        bx, by = int(rect[own[0], 0] // block) * block, int(rect[own[0], 1] // block) * block
        blocks.append((bx, by, min(block + HALO, W - bx), min(block + HALO, H - by), own))
    return blocks, np.nonzero(~inside)[0]


def _slide_hw(slide):
    if hasattr(slide, 'read_region'):
        w, h = slide.dimensions if hasattr(slide, 'dimensions') else slide.level_dimensions[0]
        return int(h), int(w)
    return int(slide.shape[0]), int(slide.shape[1])


def read_block(slide, x, y, w, h):
    """(h, w, 3) uint8 RGB, contiguous: level 0 of the slide at (x, y) -- an array slide is sliced, anything with read_region is asked."""
    if hasattr(slide, 'read_region'):
        a = slide.read_region((int(x), int(y)), 0, (int(w), int(h)))
        if hasattr(a, 'convert'):
            a = a.convert('RGB')
        a = np.asarray(a)
    else:
        a = slide[y:y + h, x:x + w]
    a = np.ascontiguousarray(np.asarray(a)[..., :3], np.uint8)
    if not a.flags.writeable:              # a whole row band of a read-only memory map is contiguous as it is: the upload wants its own copy
        a = a.copy()
    if a.shape != (h, w, 3):
        raise ValueError(f'the slide gave {a.shape} for a {h} x {w} block')
    return a


class _Ops:
    """The device steps on torch tensors of one device: the two kernels of csrc/ringfeat.hip (engine-free) and `run`, any entry of FAMILIES
    -- the mask-list ops behind a never-finalized engine handle (module docstring)."""

    def __init__(self, device=0):
        import torch
        from . import hip
        if not torch.cuda.is_available():
            raise RuntimeError('no HIP device visible: the per-nucleus measurements have no CPU path')
        self.torch, self.hip, self.lib = torch, hip, hip.load()
        self.index = device if isinstance(device, int) else (torch.device(device).index or 0)
        self.device = torch.device('cuda', self.index)
        cfg = hip.default_config()
        self.h = ctypes.c_void_p()
        rc = self.lib.nuhtc_create(ctypes.byref(cfg), self.index, ctypes.byref(self.h))
        if rc:
            raise RuntimeError(f'nuhtc_create failed ({rc}): {self.lib.nuhtc_last_error(None).decode()}')
        lut, k = stain_constants()                  # the haematoxylin value of the entries that read 'tiles'
        self.lut = torch.from_numpy(lut).to(self.device)
        self.k = (ctypes.c_int32 * 3)(*[int(v) for v in k])

    def close(self):
        if self.h:
            self.lib.nuhtc_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _need(self, t, dtype, what):
        if t.device != self.device or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f'{what}: a contiguous {dtype} tensor on {self.device}')
        return ctypes.c_void_p(t.data_ptr())

    def gather(self, block, bx, by, origin, S):
        """block uint8 (bh, bw, 3) whose pixel (0, 0) is the slide pixel (bx, by), origin int32 (n, 2) -> frames uint8 (n, S, S, 3)."""
        t = self.torch
        n = int(origin.shape[0])
        frames = t.empty(n, S, S, 3, dtype=t.uint8, device=self.device)
        rc = self.lib.nuhtc_op_frame_gather(self.index, self._need(block, t.uint8, 'block'), int(block.shape[0]), int(block.shape[1]), int(bx), int(by),
                                            self._need(origin, t.int32, 'origin'), n, int(S), ctypes.c_void_p(frames.data_ptr()), self._stream())
        if rc:
            raise RuntimeError(f'nuhtc_op_frame_gather failed ({rc})')
        return frames

    def fill(self, verts, ring_off, origin, S):
        """verts int32 (nv, 2), ring_off int64 (n + 1,), origin int32 (n, 2) -> (masks int32 (n, S, S // 32), status int32 (n,))."""
        t = self.torch
        n = int(origin.shape[0])
        masks = t.empty(n, S, S // 32, dtype=t.int32, device=self.device)
        status = t.empty(n, dtype=t.int32, device=self.device)
        if int(ring_off.shape[0]) != n + 1:
            raise ValueError('fill: ring_off has one entry more than origin has rows')
        rc = self.lib.nuhtc_op_ring_fill(self.index, self._need(verts, t.int32, 'verts'), int(verts.shape[0]), self._need(ring_off, t.int64, 'ring_off'),
                                         self._need(origin, t.int32, 'origin'), n, int(S), ctypes.c_void_p(masks.data_ptr()),
                                         ctypes.c_void_p(status.data_ptr()), self._stream())
        if rc:
            raise RuntimeError(f'nuhtc_op_ring_fill failed ({rc})')
        return masks, status

    def pairs(self, n):
        """int32 (n, 2) on the device: the pairs (i, 0) of the mask-list ops with B = n and K = 1."""
        t = self.torch
        pairs = t.zeros(n, 2, dtype=t.int32, device=self.device)
        pairs[:, 0] = t.arange(n, dtype=t.int32, device=self.device)
        return pairs

    def run(self, fam, pairs, frames=None, masks=None, verts=None, ring_off=None, ints=()):
        """One entry of FAMILIES on one chunk of n nuclei -> its fields, device tensors (n, ...) in the entry's order.  pairs: pairs(n); of
        frames uint8 (n, S, S, 3), masks int32 (n, S, S // 32) and the verts and ring_off of fill(), what the entry reads; ints: its extra
        integers.  A mask-list op runs with B = n and K = 1 behind the never-finalized handle, a ring op on the arrays of fill()."""
        t = self.torch
        n = int(pairs.shape[0])
        outs = [t.empty(n, *tail, dtype=getattr(t, dt), device=self.device) for _, tail, dt in fam.fields]
        if fam.reads == 'rings':
            status = t.empty(n, dtype=t.int32, device=self.device)
            rc = getattr(self.lib, fam.call)(self.index, self._need(verts, t.int32, 'verts'), int(verts.shape[0]), self._need(ring_off, t.int64, 'ring_off'), n,
                                             *[ctypes.c_void_p(o.data_ptr()) for o in outs], ctypes.c_void_p(status.data_ptr()), self._stream())
            if rc:
                raise RuntimeError(f'{fam.call} failed ({rc})')
            return outs
        S = int(masks.shape[1])
        rc = self.hip.op_nucleus(self.lib, self.h, fam, (n, 1, S, S), masks, pairs, outs, self._stream(), tiles=frames, stain=(self.lut, self.k), ints=ints)
        if rc:
            raise RuntimeError(f'{fam.call} failed ({rc}): {self.lib.nuhtc_last_error(self.h).decode()}')
        return outs


def pack_rings(rings):
    """list of (k, 2) integer rings -> (verts int32 (sum k, 2), ring_off int64 (n + 1,))."""
    lens = np.array([len(r) for r in rings], np.int64)
    verts = np.ascontiguousarray(np.concatenate([np.asarray(r, np.int32).reshape(-1, 2) for r in rings], 0)) if len(rings) else np.zeros((0, 2), np.int32)
    return verts, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def measure(slide, features, device=0, block=2048, timings=None, edge_thr=EDGE_THR, **keywords):
    """slide: an (H, W, 3) uint8 RGB array (a memory-mapped .npy slide) or anything with read_region (level 0 is read); features: GeoJSON
    features, or the result of parse().  The slide is walked in blocks of `block` pixels (block_plan): every block that owns a nucleus is
    read once and uploaded once, and per block, plan of frames (PLANS) and frame side, in chunks of at most 4096 nuclei, the gather, the
    ring fill and the selected families of that plan run on the device.  -> dict(raw int64 (n, 16), hist int32 (n, 256), glcm int32 (n, 2,
    136), origin int64 (n, 2), rect, score, label, type, nuclei_id, left_out) for the n measured nuclei, in the order of the features.
    left_out counts parse()'s reasons, 'off_slide' (the rectangle leaves the slide) and 'not_traced' (the ring fill's status 2: an edge
    off the chain directions).  `timings`: a dict that receives the seconds spent in read, upload, gather, fill and measure (each stage
    synchronised: for tools/bench_ringfeat.py).  gradient=True, shape=True, fsd=True (`select`): the result gains the fields of that
    family -- grad int64 (n, 18) with the edge threshold `edge_thr` (quarter grey levels, 1 .. 1442), shape int64 (n, 24), fsd int32
    (n, 644) -- and for a family a nucleus can lack (gradient: the rectangle plus margin exceeds 256 pixels) grad_ok bool (n,), False at
    such a nucleus's zero row, and grad_origin int64 (n, 2); every other field is the same bytes as without."""
    sel = select(**keywords)
    import time
    import torch
    p = features if isinstance(features, dict) and 'rings' in features else parse(features)
    left = dict(p['left_out'])
    n = len(p['rings'])
    rect = p['rect']
    ints = dict(edge_thr=edge_thr)
    for f in sel:
        for name, lo, hi, unit in f.ints:
            if not lo <= int(ints[name]) <= hi:
                raise ValueError(f'measure: {name} {ints[name]} outside {lo} .. {hi} {unit}')
    res = {name: np.zeros((n,) + tail, dt) for f in sel for name, tail, dt in f.fields}
    keep = np.zeros(n, bool)
    plans = [(plan, [f for f in sel if f.frame == plan.frame]) for plan in PLANS]
    plans = [(plan, fams, *plan.frames(rect)) for plan, fams in plans if fams]          # (plan, its selected families, origin (n, 2), side (n,))
    margin = max(plan.margin for plan, *_ in plans)
    blocks, off = block_plan(rect, _slide_hw(slide), block)
    left['off_slide'] += len(off)

    def lap(name, t0):
        if timings is not None:
            torch.cuda.synchronize(ops.device)
            timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    with _Ops(device) as ops, torch.cuda.device(ops.device):
        for bx, by, bw, bh, own in blocks:
            t0 = time.perf_counter()
            if margin:                               # frames with a margin start up to `margin` pixels before the block
                bw, bh = bw + bx - max(bx - margin, 0), bh + by - max(by - margin, 0)
                bx, by = max(bx - margin, 0), max(by - margin, 0)
            host = read_block(slide, bx, by, bw, bh)
            t0 = lap('read', t0)
            dev = torch.from_numpy(host).to(ops.device)
            t0 = lap('upload', t0)
            for plan, fams, origins, sides in plans:
                for S in SIDES:
                    mine = own[sides[own] == S]
                    for c0 in range(0, len(mine), CHUNK):
                        idx = mine[c0:c0 + CHUNK]
                        verts, ring_off = pack_rings([p['rings'][i] for i in idx])
                        origin = torch.from_numpy(np.ascontiguousarray(origins[idx], np.int32)).to(ops.device)
                        verts_d, off_d = torch.from_numpy(verts).to(ops.device), torch.from_numpy(ring_off).to(ops.device)
                        t0 = time.perf_counter()
                        frames = ops.gather(dev, bx, by, origin, S) if any(f.reads == 'tiles' for f in fams) else None
                        t0 = lap('gather', t0)
                        masks, status = ops.fill(verts_d, off_d, origin, S)
                        t0 = lap('fill', t0)
                        pairs = ops.pairs(len(idx))
                        got = [ops.run(f, pairs, frames, masks, verts_d, off_d, [ints[name] for name, *_ in f.ints]) for f in fams]
                        t0 = lap('measure', t0)
                        if plan.strict:
                            st = status.cpu().numpy()
                            if (st == 1).any():
                                raise RuntimeError('ring fill: a vertex outside its own frame (the frame is the rectangle of the vertices: this cannot happen)')
                            keep[idx] = st == 0
                            left['not_traced'] += int((st != 0).sum())
                        for f, outs in zip(fams, got):
                            for (name, _, _), o in zip(f.fields, outs):
                                res[name][idx] = o.cpu().numpy()
    rows = np.nonzero(keep)[0]
    out = {name: a[rows] for name, a in res.items()}
    out.update(origin=rect[rows, :2].copy(), rect=rect[rows], score=p['score'][rows], label=p['label'][rows], type=[p['type'][i] for i in rows],
               nuclei_id=p['nuclei_id'][rows], left_out=left)
    for plan, fams, origins, sides in plans:
        for f in fams:
            if f.lacking:
                out.update({_ok(f): sides[rows] > 0, f.fields[0][0] + '_origin': origins[rows]})
    return out


def table_columns(**keywords):
    """The names of table()'s columns: the COLUMNS of the selected families in the order of FAMILIES -- the 29 of nucmorph, the 26 of
    nuctex and, with the selections, the 8 of nucgrad, then the 8 of nucshape and then the 6 of nucfsd."""
    return sum((f.columns for f in select(**keywords)), ())


def table(m, **keywords):
    """measure()'s result -> (columns, float64 (n, 55)): nucmorph.derive(raw, hist, origin) beside nuctex.derive(glcm).  gradient=True (of
    a measure(gradient=True)): (n, 63), nucgrad.derive(grad) behind them, NaN in the eight columns of a nucleus without a gradient frame.
    shape=True (of a measure(shape=True)): eight more columns, nucshape.derive(shape), last -- behind the gradient's when both are
    selected (n, 71), behind the texture's otherwise (n, 63); they are never NaN.  fsd=True (of a measure(fsd=True)): six more columns,
    nucfsd.derive(fsd), behind all of these; they are never NaN."""
    cols, vals = (), []
    for f in select(**keywords):
        c, v = f.derive([m[name] for name, _, _ in f.fields], m['origin'])
        cols, vals = cols + tuple(c), vals + [np.where(np.asarray(m[_ok(f)], bool)[:, None], v, np.nan) if f.lacking else v]
    return cols, np.concatenate(vals, 1)


def db_columns(**keywords):
    """[(name, SQLite type)] of the table `nuclei_features`, in order: Label (always 1, as histomicstk labels a one-nucleus crop), the 29
    nucmorph.COLUMNS and the 26 nuctex.COLUMNS (REAL; every '.' of a name replaced by '_', as the reference does before to_sql), with
    the selections the 8 nucgrad.COLUMNS, then the 8 nucshape.COLUMNS and then the 6 nucfsd.COLUMNS in the same form, score, type, class_id,
    nuclei_id, and the vertex extremes x_min, y_min, x_max, y_max."""
    cols = [('Label', 'INTEGER')] + [(c.replace('.', '_'), 'REAL') for c in table_columns(**keywords)]
    return cols + [('score', 'REAL'), ('type', 'TEXT'), ('class_id', 'INTEGER'), ('nuclei_id', 'INTEGER'),
                   ('x_min', 'INTEGER'), ('y_min', 'INTEGER'), ('x_max', 'INTEGER'), ('y_max', 'INTEGER')]


def column_mismatch(path, **keywords):
    """None when `path` holds no table nuclei_features or one with exactly the columns of db_columns(**keywords); otherwise what
    differs, in words: such a table is neither appended to nor altered."""
    want = [c for c, _ in db_columns(**keywords)]
    got = read_db(path)
    if got is None:
        return None
    have = [c for c, _ in got['columns']]
    if have == want:
        return None
    extra, lack = [c for c in have if c not in want], [c for c in want if c not in have]
    return ('it has columns that were not requested: ' + ', '.join(extra) if extra else '') + ('; ' if extra and lack else '') + \
           ('it lacks the requested columns: ' + ', '.join(lack) if lack else '') or 'its columns are in another order'


def write_db(path, values, score, kind, class_id, nuclei_id, rect, **keywords):
    """Appends one row per nucleus to the table nuclei_features of the SQLite file `path` (created with db_columns(**keywords) when
    missing): values float (n, 55) = table()[1], or with gradient=True (n, 63), with shape=True eight columns more, with fsd=True six
    more, table(m, **keywords)[1].  A NaN in a column of a family that a nucleus can lack (table()) is written as NULL; a NaN anywhere
    else is a ValueError.  A file of any size is kept -- the reference deletes a database under 1 MB as broken; a complete small table is
    complete.  ValueError, with the file untouched, when it holds a table with another column set (column_mismatch).  -> the number of
    rows written."""
    sel = select(**keywords)
    values = np.asarray(values, np.float64).reshape(-1, sum(len(f.columns) for f in sel))
    rect = np.asarray(rect, np.int64).reshape(-1, 4)
    n = len(values)
    if not (len(score) == len(kind) == len(class_id) == len(nuclei_id) == len(rect) == n):
        raise ValueError('write_db: one row per nucleus in every field')
    if np.isnan(values[:, [not f.lacking for f in sel for _ in f.columns]]).any():
        raise ValueError('write_db: a NaN in a column that every nucleus has')
    cols = db_columns(**keywords)
    why = column_mismatch(path, **keywords)
    if why:
        raise ValueError(f'write_db: {path} holds another column set ({why})')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    conn = sqlite3.connect(path)
    try:
        conn.execute(f'CREATE TABLE IF NOT EXISTS {TABLE} ({", ".join(f"{c} {t}" for c, t in cols)})')
        real = values.astype(object)                 # Python floats, and None where a nucleus lacks a family
        real[np.isnan(values)] = None
        rows = [(1, *real[i], float(score[i]), str(kind[i]), int(class_id[i]), int(nuclei_id[i]), *map(int, rect[i])) for i in range(n)]
        conn.executemany(f'INSERT INTO {TABLE} ({", ".join(c for c, _ in cols)}) VALUES ({", ".join("?" * len(cols))})', rows)
        conn.commit()
    finally:
        conn.close()
    return n


def read_db(path):
    """-> dict(columns: [(name, type)], rows: list of tuples in rowid order) of the table nuclei_features; None when the file or the table
    does not exist."""
    if not os.path.exists(path):
        return None
    conn = sqlite3.connect(path)
    try:
        info = conn.execute(f'PRAGMA table_info({TABLE})').fetchall()
        if not info:
            return None
        return dict(columns=[(r[1], r[2]) for r in info], rows=conn.execute(f'SELECT * FROM {TABLE} ORDER BY rowid').fetchall())
    finally:
        conn.close()


def missing_ids(path, nuclei_id):
    """The reference's resume rule: the ids of `nuclei_id` that the table of `path` does not hold yet, in their order (all of them when
    there is no table; none when it holds every one: the slide is done)."""
    ids = [int(i) for i in nuclei_id]
    got = read_db(path)
    if got is None:
        return ids
    at = [c for c, _ in got['columns']].index('nuclei_id')
    have = {r[at] for r in got['rows']}
    return [i for i in ids if i not in have]
