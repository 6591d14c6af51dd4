"""Designed inputs shared by tests/test_stitch_host.py and tests/test_hip_stitch.py: small images cut into overlapping tiles, as raw
per-tile detection arrays (what nuhtc_infer leaves on the device), and their full-frame reference built with the pinned functions of
nuhtc_amd.evaluation.  151 x 122 pixels, 64-pixel tiles at stride 29: a 4 x 3 grid whose tile offsets are no multiples of 32."""
import numpy as np

from nuhtc_amd import evaluation as E
from nuhtc_amd import stitch as S

W, H, TILE, STRIDE, K, C = 151, 122, 64, 29, 8, 4
FG, OFFSET, THR = 0.1, 4, 0.02
GRID = S.tile_grid(H, W, TILE, STRIDE)


class Tiles:
    """boxes (n_tiles, K, 5) float32, labels (n_tiles, K), counts (n_tiles,), masks (n_tiles, K, TILE, TILE) bool."""

    def __init__(self, grid=GRID, k=K, tile=TILE):
        n = len(grid)
        self.grid, self.tile = grid, tile
        self.boxes = np.zeros((n, k, 5), np.float32)
        self.labels = np.zeros((n, k), np.int32)
        self.counts = np.zeros(n, np.int32)
        self.masks = np.zeros((n, k, tile, tile), bool)

    def add(self, loc, mask, score, label, box=None):
        """A detection in tile `loc`; box defaults to the float tight box of the mask, well inside the tile unless the mask is not."""
        r = int(self.counts[loc])
        assert r < self.boxes.shape[1]
        self.counts[loc] += 1
        if box is None:
            ys, xs = np.nonzero(mask)
            box = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1) if len(ys) else (20, 20, 30, 30)
        self.boxes[loc, r] = (*box, score)
        self.labels[loc, r] = label
        self.masks[loc, r] = mask
        return r

    def add_global(self, frame, score, label, margin=OFFSET):
        """An object given in the image frame, detected in every tile that holds it `margin` pixels inside: the duplicates the image-level NMS
        exists for.  The copy in tile `loc` scores score - loc * 1e-4, so every score is distinct."""
        ys, xs = np.nonzero(frame)
        for t in self.grid:
            if xs.min() - t['ox'] >= margin and ys.min() - t['oy'] >= margin and xs.max() + 1 - t['ox'] <= self.tile - margin and \
                    ys.max() + 1 - t['oy'] <= self.tile - margin and self.counts[t['loc']] < self.boxes.shape[1]:
                self.add(t['loc'], frame[t['oy']:t['oy'] + self.tile, t['ox']:t['ox'] + self.tile], np.float32(score) - np.float32(t['loc'] * 1e-4), label)

    def results(self, loc):
        """(bbox_results, segm_results) of a tile as Engine.results returns them."""
        n = int(self.counts[loc])
        d, l = self.boxes[loc, :n], self.labels[loc, :n]
        return [d[l == c] for c in range(C)], [[self.masks[loc, j] for j in range(n) if l[j] == c] for c in range(C)]

    def candidates(self):
        """The host route's candidates of the image."""
        c = S.Candidates()
        for t in self.grid:
            S.add_tile(c, self.results(t['loc']), t, self.tile, FG, OFFSET)
        return c.freeze()


def frame_rect(y0, y1, x0, x1, h=H, w=W):
    m = np.zeros((h, w), bool)
    m[y0:y1, x0:x1] = True
    return m


def tile_mask(pixels=(), rects=(), tile=TILE):
    m = np.zeros((tile, tile), bool)
    for y0, y1, x0, x1 in rects:
        m[y0:y1, x0:x1] = True
    for y, x in pixels:
        m[y, x] = True
    return m


def designed():
    """-> (Tiles, gt) with every decision the protocol makes present at least once; see the tests for what each detection is for."""
    t = Tiles()
    rng = np.random.RandomState(5)
    # threshold: inter / union = 2 / 100 is kept, 3 / 100 is removed (tiles 0 and 1: offsets 0 and 29)
    a = tile_mask(rects=[(50, 51, 5, 56)])                                       # 51 px, image row 50, columns 5..55
    b = tile_mask(rects=[(50, 51, 54 - 29, 56 - 29), (51, 52, 5, 54)])           # tile 1: 2 px on a, 49 px below
    t.add(0, a, 0.99, 3)           # (the higher class under the earlier position: the shared pixels take id and type from different masks)
    t.add(1, b, 0.98, 1)
    c = tile_mask(rects=[(56, 57, 5, 56)])                                       # 51 px
    d = tile_mask(rects=[(56, 57, 53 - 29, 56 - 29), (57, 58, 5, 54)])           # 3 px on c, 49 below: 52 px, union 100
    t.add(0, c, 0.97, 0)
    t.add(1, d, 0.96, 1)
    # chain in tile 11 (last column, last row): X kills Y, Z overlaps Y only and survives
    t.add(11, tile_mask(rects=[(40, 50, 20, 30)]), 0.95, 2)
    t.add(11, tile_mask(rects=[(40, 50, 25, 35)]), 0.94, 2)
    t.add(11, tile_mask(rects=[(40, 50, 32, 42)]), 0.93, 3)
    # bit 31 of the last word of a tile row, and of the tile: the last column's tile may hold boxes up to its right edge
    t.add(11, tile_mask(pixels=[(63, 63), (62, 63), (63, 31), (63, 32)]), 0.92, 1)
    # an empty mask: stays a candidate, is kept, has no partner
    t.add(5, tile_mask(), 0.91, 0)
    # score filter
    t.add(5, tile_mask(rects=[(10, 14, 40, 44)]), np.float32(FG), 1)           # equal to fg_thr: a candidate
    t.add(5, tile_mask(rects=[(10, 14, 46, 50)]), np.nextafter(np.float32(FG), np.float32(0)), 1)
    t.add(5, tile_mask(rects=[(10, 14, 52, 56)]), np.float32('nan'), 1)
    # objects all over the image, seen by several tiles each; some overlap their neighbours a little, some a lot
    for k in range(26):
        h, w = rng.randint(5, 15, 2)
        y, x = rng.randint(0, H - h), rng.randint(0, W - w)
        f = frame_rect(y, y + h, x, x + w)
        f[y, x] = False                                         # not quite a rectangle
        t.add_global(f, 0.3 + 0.6 * rng.rand(), int(rng.randint(C)))
    # ground truth: ids 1..9, id 4 absent; types 1..7 and the remap
    inst = np.zeros((H, W), np.int32)
    inst[50:51, 5:56] = 1
    inst[56:58, 5:56] = 2
    inst[98:108, 107:117] = 3                      # under X of the chain (tile 11: offsets 87, 58)
    inst[98:108, 119:129] = 5
    inst[0:20, 0:20] = 6
    inst[30:60, 60:100] = 7
    inst[100:122, 0:40] = 8
    inst[121, 150] = 9
    types = np.array([1, 2, 3, 4, 5, 6, 7, 1, 2])
    return t, S.gt_from_mat(inst, types)


def full_frame_reference(c, gt, thr=THR):
    """The pinned functions on full frames: evaluation.mask_nms, stat_calc, multi_stat_calc, update_confusion_matrix, convert_format."""
    gt_map, gt_labels, n_t = gt
    frames = np.stack([c.frame(i, H, W) for i in range(len(c))]) if len(c) else np.zeros((0, H, W), bool)
    pm, kept = E.mask_nms(frames, c.score, thr=thr)
    labels = c.label[kept]
    tm = np.stack([gt_map == i + 1 for i in range(n_t)])
    cm = E.update_confusion_matrix(np.zeros((C + 1, C + 1)), tm, pm, gt_labels, labels)
    return dict(kept=kept, labels=labels, stat=E.stat_calc(tm, pm), multi=E.multi_stat_calc(tm, pm, gt_labels, labels, C), cm=cm,
                maps=E.convert_format(pm, labels, H, W, C, 'conic'), frames=frames)
