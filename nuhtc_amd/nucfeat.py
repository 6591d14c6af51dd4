"""Per-nucleus embeddings: the FPN maps of a tile averaged under the final mask of a nucleus (the learned descriptor the engine has
already computed, per nucleus; `Engine.features` is the same mean per tile).  The reference's per-nucleus table
(tools/wsi_feat_extract.py, tools/nuclei_feat_extract.py: hand-crafted features keyed by `nuclei_id`) is what this stands in for;
the file tools/infer_wsi.py --nuclei-feat writes is keyed the same way.

Definition.  For a binary mask M (H x W, A = M.sum() > 0) and level l with stride s_l (mask pixels per map cell) and map x_l (H_l, W_l, 64):

    w_l(i, j) = number of mask pixels (y, x) with y // s_l == i and x // s_l == j
    e_l[c]    = sum over (i, j) of w_l(i, j) * x_l[i, j, c] / A
    embedding = concat(e_0, e_1, e_2, e_3)              256 values, level 0 first (the layout of Engine.features)

the mean over the nucleus's pixels of each map upsampled piecewise-constant.  A == 0 gives zeros.  The device computes it in float32
(csrc/nucfeat.hip: one fused multiply-add chain per level and channel over the non-zero cells, one division); this module is the float64
restatement and the bound between the two."""
import numpy as np

DIM = 256
U = 2.0 ** -24                  # unit roundoff of float32


def cell_weights(mask, stride, shape):
    """int64 (h, w) = `shape`: how many set pixels of `mask` fall into each cell of side `stride`."""
    m = np.asarray(mask, bool)
    ys, xs = np.nonzero(m)
    w = np.zeros(tuple(int(v) for v in shape), np.int64)
    np.add.at(w, (ys // int(stride), xs // int(stride)), 1)
    return w


def pool_reference(maps, strides, mask_bool):
    """maps: four arrays (h_l, w_l, 64) of ONE tile; strides: four ints; mask_bool: (H, W) -> float64 (256,)."""
    out = np.zeros(DIM, np.float64)
    area = int(np.asarray(mask_bool, bool).sum())
    if area == 0:
        return out
    for l, (x, s) in enumerate(zip(maps, strides)):
        x = np.asarray(x, np.float64)
        w = cell_weights(mask_bool, s, x.shape[:2])
        out[64 * l:64 * l + 64] = np.tensordot(w.astype(np.float64), x, axes=([0, 1], [0, 1])) / area
    return out


def pool_bound(maps, strides, mask_bool):
    """float64 (256,): the largest |device - pool_reference| float32 arithmetic allows, per output: (n + 3) * 2**-24 * sum(w * |x|) / A with
    n the non-zero cells of the level.  A sum of n float32 terms in ANY order is within ((1 + u)**(n - 1) - 1) * sum |term| of the exact
    sum; the products w * x (w an integer below 2**24: exact) add at most one rounding each and the division one more: (1 + u)**(n + 1) - 1,
    which stays below (n + 3) u while n**2 * u < 4, i.e. for every mask of fewer than 8192 cells a level."""
    out = np.zeros(DIM, np.float64)
    area = int(np.asarray(mask_bool, bool).sum())
    if area == 0:
        return out
    for l, (x, s) in enumerate(zip(maps, strides)):
        x = np.abs(np.asarray(x, np.float64))
        w = cell_weights(mask_bool, s, x.shape[:2])
        n = int(np.count_nonzero(w))
        out[64 * l:64 * l + 64] = (n + 3) * U * np.tensordot(w.astype(np.float64), x, axes=([0, 1], [0, 1])) / area
    return out


def pack_mask_words(mask_bool):
    """(..., H, W) bool -> int32 (..., H, (W + 31) // 32): bit x & 31 of word x >> 5, the padding bits zero (the layout of the engine's masks)."""
    m = np.asarray(mask_bool, bool)
    W = m.shape[-1]
    wpr = (W + 31) // 32
    row = np.zeros(m.shape[:-1] + (wpr * 32,), np.uint8)
    row[..., :W] = m
    return np.packbits(row, axis=-1, bitorder='little').view(np.uint32).view(np.int32).reshape(m.shape[:-1] + (wpr,))


def unpack_mask_words(words, W=None):
    """int32 / uint32 (..., H, wpr) -> bool (..., H, W) (W: the image width, default wpr * 32)."""
    w = np.ascontiguousarray(words).view(np.uint32)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (w.shape[-1] * 4,)), axis=-1, bitorder='little').astype(bool)
    return bits if W is None else bits[..., :W]


def write_npz(path, nuclei_id, features, label, score):
    """The per-nucleus table of a slide: nuclei_id int64 (n,), features float32 (n, 256), label int64 (n,), score float64 (n,), row k for
    the k-th feature of the GeoJSON written beside it.  nuclei_id is that nucleus's position in <id>.geojson (with a cross-tile merge the
    table holds the merged file's nuclei, still numbered by their position in <id>.geojson)."""
    features = np.ascontiguousarray(features, np.float32).reshape(-1, DIM)
    nuclei_id = np.ascontiguousarray(nuclei_id, np.int64)
    if not (len(nuclei_id) == len(features) == len(label) == len(score)):
        raise ValueError('write_npz: one row per nucleus in every field')
    with open(path, 'wb') as f:
        np.savez(f, nuclei_id=nuclei_id, features=features, label=np.ascontiguousarray(label, np.int64), score=np.ascontiguousarray(score, np.float64))
    return path


def read_npz(path):
    """-> dict(nuclei_id, features, label, score) of a file write_npz wrote."""
    with np.load(path) as z:
        return {k: z[k] for k in ('nuclei_id', 'features', 'label', 'score')}
