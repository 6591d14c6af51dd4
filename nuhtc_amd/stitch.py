"""Scoring images that are larger than a tile: the protocol of the reference's `CoNSePCocoDataset.evaluate`
(nuhtc/datasets/WSI_coco_CoNSeP.py:117-426), on the host (numpy).

The reference cuts each image into overlapping tiles, drops the detections close to an inner tile edge, pastes every remaining mask into
a frame of the whole image, runs one mask-NMS per image and scores the survivors against the image's instance map.  A frame per
candidate is 1 MB for a CoNSeP image and there are thousands of candidates, so everything here works on the CROP of a mask -- the
bounding box of its set pixels in image coordinates plus the pixels inside it -- and never builds a frame: intersections are taken over
the overlap of two boxes, the pair tables by looking the crop's pixels up in the instance map.  The results are integers (kept indices,
intersection and area tables, label maps); the statistics come from them through nuhtc_amd.evaluation's *_tables functions.

tools/eval_consep.py is the front end; the device route (csrc/stitch.hip, Engine.stitch_*) produces the same tables.
"""
import os

import numpy as np

from . import evaluation as E


# ----------------------------------------------------------------------------- tiles
def tile_grid(height, width, tile=256, stride=93):
    """The tiles an image is cut into, row-major: list of dict(loc, ox, oy, first_col, last_col, first_row, last_row).  CoNSeP: a 9 x 9 grid
    of 256-pixel tiles at stride 93 over 1000 x 1000.  (size - tile) / stride must be a whole number on both axes."""
    if tile < 32 or tile % 32:
        raise ValueError(f'tiles are square with a side that is a multiple of 32, not {tile}')
    if stride < 1 or height < tile or width < tile or (height - tile) % stride or (width - tile) % stride:
        raise ValueError(f'a {height} x {width} image is not covered by whole tiles of {tile} at stride {stride}: '
                         '(size - tile) / stride must be an integer on both axes')
    ny, nx = (height - tile) // stride + 1, (width - tile) // stride + 1
    return [dict(loc=j * nx + i, ox=i * stride, oy=j * stride, first_col=i == 0, last_col=i == nx - 1, first_row=j == 0, last_row=j == ny - 1)
            for j in range(ny) for i in range(nx)]


def tile_meta(image, t):
    """The int32 [8] record csrc/stitch.hip takes for a tile of tile_grid."""
    return [int(image), t['ox'], t['oy'], int(t['first_col']), int(t['last_col']), int(t['first_row']), int(t['last_row']), t['loc']]


# ----------------------------------------------------------------------------- ground truth
def remap_types(inst_type):
    """CoNSeP's seven types -> the four classes of the paper, 0-based (WSI_coco_CoNSeP.py:78-81): 3|4 -> 3, 5|6|7 -> 4, then - 1."""
    t = np.asarray(inst_type).astype(int).flatten()
    t[(t == 3) | (t == 4)] = 3
    t[(t == 5) | (t == 6) | (t == 7)] = 4
    return t - 1


def gt_from_mat(inst_map, inst_type):
    """-> (inst_map (H, W) int32 whose value is row + 1, labels (n_t,), n_t).  Row t is id t + 1 for EVERY t < inst_map.max() (:77: the
    one-hot planes of np.eye): an id that occurs nowhere is still a row, of area 0, and counts as a false negative."""
    inst_map = np.asarray(inst_map).astype(np.int32)
    n_t = int(inst_map.max()) if inst_map.size else 0
    labels = remap_types(inst_type)
    if len(labels) != n_t:
        raise ValueError(f'inst_type has {len(labels)} rows, inst_map ids run to {n_t}')
    if inst_map.min() < 0:
        raise ValueError('inst_map holds a negative id')
    return inst_map, labels, n_t


def load_fold(data):
    """<data>/Images/<name>.png + <data>/Labels/<name>.mat (inst_map, inst_type), the layout `get_img` / `get_img_inst_map` read
    -> sorted names, {name: (H, W, 3) uint8 RGB}, {name: gt_from_mat(...)}."""
    import scipy.io as sio
    from PIL import Image
    names = sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(data, 'Labels')) if f.endswith('.mat'))
    images, gts = {}, {}
    for n in names:
        images[n] = np.array(Image.open(os.path.join(data, 'Images', n + '.png')).convert('RGB'))
        m = sio.loadmat(os.path.join(data, 'Labels', n + '.mat'))
        gts[n] = gt_from_mat(m['inst_map'], m['inst_type'])
    return names, images, gts


# ----------------------------------------------------------------------------- candidates
class Candidates:
    """The candidates of one image in the reference's order (tile location row-major, then class, then slot): box (n, 4) int x0, y0, x1, y1
    (exclusive) of the set pixels in image pixels (zeros for an empty mask), area, score (float32), label, crops: list of (h, w) bool."""

    def __init__(self):
        self.box, self.area, self.score, self.label, self.crops = [], [], [], [], []

    def add(self, mask, ox, oy, score, label):
        mask = np.asarray(mask).astype(bool)
        ys, xs = np.nonzero(mask)
        if len(ys) == 0:                                       # an empty mask stays a candidate (it is kept: nothing overlaps it)
            self.box.append((0, 0, 0, 0))
            self.crops.append(np.zeros((0, 0), bool))
        else:
            y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
            self.box.append((x0 + ox, y0 + oy, x1 + ox, y1 + oy))
            self.crops.append(mask[y0:y1, x0:x1].copy())
        self.area.append(len(ys))
        self.score.append(score)
        self.label.append(label)

    def freeze(self):
        self.box = np.asarray(self.box, dtype=np.int64).reshape(-1, 4)
        self.area = np.asarray(self.area, dtype=np.int64)
        self.score = np.asarray(self.score, dtype=np.float32)
        self.label = np.asarray(self.label, dtype=int)
        return self

    def __len__(self):
        return len(self.area)

    def frame(self, i, height, width):
        """Candidate i pasted into a frame of the image (tests and small images only)."""
        m = np.zeros((height, width), bool)
        x0, y0, x1, y1 = self.box[i]
        m[y0:y1, x0:x1] = self.crops[i]
        return m


def select_tile(boxes, t, tile=256, fg_thr=0.1, discard_offset=4):
    """The candidate rules of :198-211 on the (n, 5) float boxes of one tile -> bool (n,): score >= fg_thr (false for NaN), and not within
    discard_offset of an INNER tile edge, judged on the float box and not on the mask."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 5)
    lo, hi = np.float32(discard_offset), np.float32(tile) - np.float32(discard_offset)
    sel = boxes[:, 4] >= np.float32(fg_thr)
    if not t['first_col']:
        sel &= ~(boxes[:, 0] < lo)
    if not t['last_col']:
        sel &= ~(boxes[:, 2] > hi)
    if not t['first_row']:
        sel &= ~(boxes[:, 1] < lo)
    if not t['last_row']:
        sel &= ~(boxes[:, 3] > hi)          # the reference compares y2 with the tile WIDTH (:211); tiles are square here
    return sel


def add_tile(cands, result, t, tile=256, fg_thr=0.1, discard_offset=4):
    """Adds the detections of one tile -- `result` = (bbox_results, segm_results) per class, what Engine.results returns -- that pass
    select_tile, in class-major order (the np.concatenate of bbox2result)."""
    bbox_res, segm_res = result
    for c, (bx, sg) in enumerate(zip(bbox_res, segm_res)):
        sel = select_tile(bx, t, tile, fg_thr, discard_offset)
        for j in np.nonzero(sel)[0]:
            cands.add(sg[j], t['ox'], t['oy'], bx[j][4], c)


# ----------------------------------------------------------------------------- image-level mask-NMS
def visiting_order(score):
    """Descending score, equal scores in descending candidate index: the convention evaluation.mask_nms pins."""
    return np.argsort(np.asarray(score), kind='stable')[::-1]


def crop_inter(c, i, j):
    """Common pixels of candidates i and j."""
    bi, bj = c.box[i], c.box[j]
    x0, y0, x1, y1 = max(bi[0], bj[0]), max(bi[1], bj[1]), min(bi[2], bj[2]), min(bi[3], bj[3])
    if x1 <= x0 or y1 <= y0:
        return 0
    a = c.crops[i][y0 - bi[1]:y1 - bi[1], x0 - bi[0]:x1 - bi[0]]
    b = c.crops[j][y0 - bj[1]:y1 - bj[1], x0 - bj[0]:x1 - bj[0]]
    return int(np.count_nonzero(a & b))


def mask_nms_crops(c, thr=0.02):
    """`mask_nms` over the candidates of an image (:303): visiting_order, a kept mask removes every later one with
    inter / max(union, 1) > thr, decided in float64 on the integer counts.  -> kept candidate indices in visiting order."""
    order = visiting_order(c.score)
    n = len(order)
    box, area = c.box[order], c.area[order]
    alive = np.ones(n, bool)
    kept = []
    for a in range(n):
        if not alive[a]:
            continue
        kept.append(order[a])
        later = np.nonzero(alive[a + 1:])[0] + a + 1
        if thr >= 0:          # disjoint boxes share no pixel: 0 / union > thr only under a negative threshold
            b = box[later]
            later = later[(b[:, 0] < box[a, 2]) & (b[:, 2] > box[a, 0]) & (b[:, 1] < box[a, 3]) & (b[:, 3] > box[a, 1])]
        for k in later:
            inter = crop_inter(c, order[a], order[k])
            if np.float64(inter) / np.float64(max(area[a] + area[k] - inter, 1)) > thr:
                alive[k] = False
    return np.asarray(kept, dtype=int)


# ----------------------------------------------------------------------------- tables and maps of the kept predictions
def pair_tables_crops(gt_map, n_t, c, kept):
    """-> (inter (n_t, n_p) float64, area_t (n_t,), area_p (n_p,)) with integer values: evaluation.pair_tables in the image frame."""
    inter = np.zeros((n_t, len(kept)))
    for q, i in enumerate(kept):
        x0, y0, x1, y1 = c.box[i]
        rows = gt_map[y0:y1, x0:x1][c.crops[i]]
        inter[:, q] = np.bincount(rows, minlength=n_t + 1)[1:n_t + 1]
    area_t = np.bincount(gt_map.ravel(), minlength=n_t + 1)[1:n_t + 1].astype(np.float64)
    return inter, area_t, c.area[kept].astype(np.float64)


def render_crops(c, kept, height, width):
    """`convert_format(..., 'conic')` in the image frame -> (inst_map, type_map) (H, W) int32: the 1-based position in kept order and the
    class + 1, two independent maxima over the masks covering a pixel."""
    inst = np.zeros((height, width), np.int32)
    typ = np.zeros((height, width), np.int32)
    for q, i in enumerate(kept):
        x0, y0, x1, y1 = c.box[i]
        m = c.crops[i]
        v = inst[y0:y1, x0:x1]
        v[m] = q + 1                                           # ascending q: the highest id wins
        v = typ[y0:y1, x0:x1]
        v[m] = np.maximum(v[m], c.label[i] + 1)
    return inst, typ


def centroids(box):
    """`inst_centroid` of :338-341 from the (n, 4) image boxes: x + w / 2, y + h / 2 of maskUtils.toBbox of the full-frame run-length
    mask.  toBbox looks at the ends of the runs only and, for a run that spans two columns (a mask touching the bottom of column x and the
    top of column x + 1), sets the rows to the whole height (cocomask.to_bbox restates it): such a mask touches row 0 and row H - 1, so
    that IS its tight box and the crop's box gives the same numbers.  An empty mask gives (0, 0)."""
    box = np.asarray(box, dtype=np.float64).reshape(-1, 4)
    return np.stack([box[:, 0] + (box[:, 2] - box[:, 0]) / 2, box[:, 1] + (box[:, 3] - box[:, 1]) / 2], 1)


def pred_mat(inst_map, labels, box):
    """The HoVer-Net style dictionary `save=True` writes per image (:342-349)."""
    n = len(labels)
    return {'inst_map': np.asarray(inst_map), 'inst_type': np.reshape(np.asarray(labels, dtype=int) + 1, (-1, 1)),
            'inst_centroid': centroids(box), 'inst_uid': np.arange(1, n + 1).reshape(-1, 1)}


# ----------------------------------------------------------------------------- a fold
class FoldScores:
    """What an evaluation accumulates per image, from integer tables whichever route built them."""

    def __init__(self, num_classes):
        self.nc = num_classes
        self.stats, self.mpq_info, self.lines = {}, [], []
        self.cm = np.zeros((num_classes + 1, num_classes + 1))

    def add(self, name, inter, area_t, area_p, gt_labels, pred_labels):
        s = E.stat_calc_tables(inter, area_t, area_p)
        line = f'\n{name.rjust(8)}'
        for k, v in (s or {}).items():
            self.stats.setdefault(k, []).append(v)
            if k not in ('tp', 'fp', 'fn', 'iou'):
                line += f', {k}:{v:.4f}'
        self.lines.append(line)
        self.mpq_info.append(E.multi_stat_calc_tables(inter, area_t, area_p, gt_labels, pred_labels, self.nc))
        E.update_confusion_matrix_tables(self.cm, inter, area_t, area_p, gt_labels, pred_labels)
        return line

    def summary(self):
        out = {k: float(np.mean(v)) for k, v in self.stats.items() if k not in ('tp', 'fp', 'fn', 'iou')}
        if self.mpq_info:
            out.update({k: float(v) for k, v in E.aggregate_mpq(self.mpq_info).items()})
        return out


def score_image_host(c, gt, height, width, thr=0.02, want_maps=False):
    """The host route for one image: Candidates + gt_from_mat(...) -> dict(kept, labels, inter, area_t, area_p[, inst_map, type_map])."""
    gt_map, _, n_t = gt
    kept = mask_nms_crops(c, thr)
    inter, area_t, area_p = pair_tables_crops(gt_map, n_t, c, kept)
    out = dict(kept=kept, labels=c.label[kept], box=c.box[kept], inter=inter, area_t=area_t, area_p=area_p)
    if want_maps:
        out['inst_map'], out['type_map'] = render_crops(c, kept, height, width)
    return out
