"""Neighbourhood enrichment of a slide: do nuclei of class b sit next to nuclei of class a more often than the tissue's layout alone would
give?  The label-permutation test of histoCAT and squidpy's `nhood_enrichment`: the positions are kept, the labels are shuffled P times,
the class-pair contacts are recounted each time, and the observed count is read as a z-score and an empirical p-value against the
shuffled ones.  It needs no area and no edge correction, because the null model lives on the same point set -- what spatial.py's counts
lack.  Counted on the GPU (csrc/cellenrich.hip, `nuhtc_cell_enrichment`); tools/infer_wsi.py --nuclei-enrichment writes it as
<id>_nuclei_enrichment.npz.  Not in the reference.

Definition, integers only.

Inputs.  n points in HALF pixels, int32 (n, 2), from `cellpoints.quantize_centres`, with |p| < 2**27 and n <= 2**24
(`cellpoints.MAX_POINTS`); labels, int32, one per point; C classes, 1 <= C <= 14; a radius r, 1 <= r <= 16384 half pixels; P permutations,
1 <= P <= 1024; a seed, 0 <= seed <= 2**32 - 1.

Neighbours.  An ordered pair (i, j), i != j, is a CONTACT when dx * dx + dy * dy <= r * r.  The radius is inclusive and coincident points
are contacts: the rule of bin 0 of spatial.py with the single edge r.

Permutation pi_p of 0 .. n - 1, p = 1 .. P.  All arithmetic is mod 2**32.
  * fmix(v), the murmur3 finaliser: v ^= v >> 16; v *= 0x85EBCA6B; v ^= v >> 13; v *= 0xC2B2AE35; v ^= v >> 16.
  * n <= 1: the identity.  Otherwise h = max(1, ceil(bitlength(n - 1) / 2)) and mask = 2**h - 1.
  * base = fmix(seed + 0x9E3779B9 * p), key_k = fmix(base + 0x7F4A7C15 * (k + 1)) for k = 0 .. 5.
  * F(x), a six-round balanced Feistel network on 2 h bits: L = x >> h, R = x & mask; round k sets (L, R) = (R, L ^ (fmix(R + key_k) &
    mask)); the result is (L << h) | R.  F is a bijection of 0 .. 4**h - 1.
  * pi_p(i) by cycle-walking: x = F(i), then x = F(x) while x >= n.  i < n lies on a cycle of F that returns to a value below n, so the
    walk ends; 4**h < 4 n, so the expected walk is under four steps.
The shuffled labels are lab_p[i] = lab[pi_p(i)].  EVERY row takes part, a label outside 0 .. C - 1 included; such a label is counted in
no row and no column, as everywhere else.

Outputs.
  observed    int64 (C, C):    the contacts (i, j) with label_i = a and label_j = b.  Symmetric.
  perm_counts int64 (P, C, C): row p - 1 is the same count under lab_p.
  class_n     int64 (C,):      the points of each class.

The result is a pure function of (points, labels, C, r, P, seed), bitwise the same on every call.  The ORDER of the rows is part of the
input: pi acts on row numbers, so the same points in another order give other perm_counts (with the same distribution).  `observed` and
`class_n` do not depend on the row order.

`enrichment_reference` is the brute-force restatement (every pair in int64, no grid, `permutation` in numpy): the oracle the device result
must EQUAL.  `derive` turns the integers into the statistics on the host, in float64 and without NaNs: `mean` and `std` of perm_counts
over p (ddof 0), `z` = (observed - mean) / std (0 where std is 0), `p_enriched` = (1 + #{p: perm >= observed}) / (P + 1) and `p_depleted`
= (1 + #{p: perm <= observed}) / (P + 1), all (C, C).  The generator is not numpy's: csrc/cellenrich_host.h holds the same definition
in C++ for the kernels, and `nuhtc_enrichment_permutation` exports it for the host alone, so a disagreement names the generator and not
the kernel."""
import numpy as np

from . import cellpoints
from .cellpoints import MAX_CLASSES, MAX_POINTS, MAX_R, half_pixel_radius

MAX_PERMS = 1024
MAX_SEED = (1 << 32) - 1
ROUNDS = 6
_M32 = np.uint64(0xFFFFFFFF)

DERIVED_KEYS = ('mean', 'std', 'z', 'p_enriched', 'p_depleted')
NPZ_KEYS = ('nuclei_id', 'xy', 'label', 'radius_px', 'perms', 'seed', 'observed', 'perm_counts', 'class_n') + DERIVED_KEYS


def check_args(num_classes, r, perms, seed):
    """num_classes 1..14, r 1..16384 half pixels, perms 1..1024, seed 0..2**32-1, all whole numbers: ValueError otherwise."""
    whole = all(float(v) == int(v) for v in (num_classes, r, perms, seed))
    if not (whole and 1 <= int(num_classes) <= MAX_CLASSES and 1 <= int(r) <= MAX_R and 1 <= int(perms) <= MAX_PERMS and 0 <= int(seed) <= MAX_SEED):
        raise ValueError(f'enrichment: num_classes 1..{MAX_CLASSES}, r 1..{MAX_R} half pixels, perms 1..{MAX_PERMS}, seed 0..2**32-1 '
                         f'(got num_classes={num_classes}, r={r}, perms={perms}, seed={seed})')


def _fmix(v):
    """The murmur3 finaliser on uint64 arrays (or scalars) holding values below 2**32."""
    v = np.asarray(v, np.uint64)
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x85EBCA6B)) & _M32
    v = v ^ (v >> np.uint64(13))
    v = (v * np.uint64(0xC2B2AE35)) & _M32
    return v ^ (v >> np.uint64(16))


def round_keys(seed, p):
    """-> the six round keys of permutation p (1-based) under `seed`, Python integers."""
    base = int(_fmix((int(seed) + 0x9E3779B9 * int(p)) & 0xFFFFFFFF))
    return [int(_fmix((base + 0x7F4A7C15 * (k + 1)) & 0xFFFFFFFF)) for k in range(ROUNDS)]


def half_bits(n):
    """h of the definition for n >= 2."""
    return max(1, (int(n - 1).bit_length() + 1) // 2)


def permutation(n, seed, p, with_steps=False):
    """pi_p of the definition -> int64 (n,): entry i is pi_p(i).  With `with_steps`, also the applications of F each element took."""
    n = int(n)
    if not (0 <= n <= MAX_POINTS and 1 <= int(p) <= MAX_PERMS and 0 <= int(seed) <= MAX_SEED):
        raise ValueError(f'permutation: n 0..2**24, p 1..{MAX_PERMS}, seed 0..2**32-1 (got n={n}, p={p}, seed={seed})')
    out = np.arange(n, dtype=np.int64)
    steps = np.zeros(n, np.int64)
    if n > 1:
        h = np.uint64(half_bits(n))
        mask = (np.uint64(1) << h) - np.uint64(1)
        keys = [np.uint64(k) for k in round_keys(seed, p)]
        x = out.astype(np.uint64)
        todo = np.arange(n)                                      # the elements still walking
        while len(todo):
            v = x[todo]
            L, R = v >> h, v & mask
            for key in keys:
                L, R = R, L ^ (_fmix((R + key) & _M32) & mask)
            v = (L << h) | R
            x[todo] = v
            steps[todo] += 1
            todo = todo[v >= np.uint64(n)]
        out = x.astype(np.int64)
    return (out, steps) if with_steps else out


def contacts(points, r):
    """The ordered contacts of points int64 (n, 2) within r half pixels, pair by pair -> (i int64 (M,), j int64 (M,)), i != j."""
    r2 = int(r) * int(r)
    ii, jj = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for rows, d2 in cellpoints.pair_blocks(points, 512):
        within = d2 <= r2
        within[rows - rows[0], rows] = False                     # j != i (a coincident OTHER point stays)
        a, b = np.nonzero(within)
        ii.append(rows[a])
        jj.append(b.astype(np.int64))
    return np.concatenate(ii), np.concatenate(jj)


def enrichment_reference(points, labels, num_classes, r, perms, seed):
    """The definition: the contacts once, pair by pair in int64, then one bincount per labelling.  points int (n, 2) half pixels, labels
    int (n,), r in HALF pixels -> (observed int64 (C, C), perm_counts int64 (P, C, C), class_n int64 (C,)).  O(n^2) time, rows in blocks of
    512, and memory for the list of all contacts (16 bytes each): for n of a few thousand."""
    check_args(num_classes, r, perms, seed)
    p, lab = cellpoints.reference_points(points, labels, 'enrichment_reference')
    n, C, P = len(p), int(num_classes), int(perms)
    if n > MAX_POINTS:
        raise ValueError(f'enrichment_reference: at most 2**24 points (got {n})')
    ci, cj = contacts(p, r)
    known = (lab >= 0) & (lab < C)
    cls = np.where(known, lab, C)                                # C: counted in no row and no column

    def table(c):
        return np.bincount(c[ci] * (C + 1) + c[cj], minlength=(C + 1) * (C + 1)).reshape(C + 1, C + 1)[:C, :C].astype(np.int64)

    perm_counts = np.zeros((P, C, C), np.int64)
    for k in range(P):
        perm_counts[k] = table(cls[permutation(n, seed, k + 1)])
    return table(cls), perm_counts, np.bincount(lab[known], minlength=C).astype(np.int64)


def call(points, labels, num_classes, r, perms, seed, observed, perm_counts, class_n, bounds=None, device=0):
    """nuhtc_cell_enrichment on torch tensors of cuda:`device` (points, labels int32; observed (C, C), perm_counts (P, C, C), class_n (C,)
    int64; contiguous; r in HALF pixels) -> the library's return code, nothing raised: 0 or hip.E_INVALID / hip.E_HIP.  bounds = (x_min,
    y_min, x_max, y_max) of the points, computed on the host when not given."""
    return cellpoints.launch('nuhtc_cell_enrichment', device, points, labels, (int(num_classes), int(r), int(perms), int(seed) & MAX_SEED),
                             (observed, perm_counts, class_n), bounds)


def build(points, labels, num_classes, radius_px, perms, seed=0, device=0):
    """The contact counts of `points` (int (n, 2) half pixels, see cellpoints.quantize_centres) with `labels` (n,) on cuda:`device`: numpy
    in, (observed int64 (C, C), perm_counts int64 (P, C, C), class_n int64 (C,)) out.  The order of the rows is part of the input (see the
    module's docstring).  There is no host route: without the library or a GPU this raises."""
    import torch
    C, r, P = int(num_classes), half_pixel_radius(radius_px), int(perms)
    check_args(C, r, perms, seed)
    p, lab, dev, p_d, lab_d, bounds = cellpoints.resident(points, labels, 'enrichment', device)
    out = [torch.zeros(shape, dtype=torch.int64, device=dev) for shape in ((C, C), (P, C, C), (C,))]
    cellpoints.raise_for(call(p_d, lab_d, C, r, P, seed, *out, bounds=bounds, device=device), 'nuhtc_cell_enrichment')
    return tuple(t.cpu().numpy() for t in out)


def host_permutation(n, seed, p):
    """pi_p from the library's host-only export nuhtc_enrichment_permutation (the C++ of csrc/cellenrich_host.h; no GPU is touched) ->
    int32 (n,); ValueError when the library refuses the arguments."""
    import ctypes
    from . import hip
    out = np.zeros(max(int(n), 1), np.int32)
    rc = hip.load().nuhtc_enrichment_permutation(int(n), int(seed) & MAX_SEED, int(p), out.ctypes.data_as(ctypes.c_void_p))
    if rc:
        raise ValueError(f'nuhtc_enrichment_permutation: invalid arguments (n={n}, p={p})')
    return out[:int(n)]


def derive(observed, perm_counts):
    """The statistics of the integers, in float64 -> dict of (C, C) arrays:
      mean, std   of perm_counts over the permutations (ddof 0)
      z           (observed - mean) / std, 0 where std is 0
      p_enriched  (1 + #{p: perm_counts[p] >= observed}) / (P + 1)
      p_depleted  (1 + #{p: perm_counts[p] <= observed}) / (P + 1)
    Never NaN.  The p-values are empirical: their smallest value is 1 / (P + 1)."""
    obs = np.asarray(observed, np.int64)
    pc = np.asarray(perm_counts, np.int64)
    if obs.ndim != 2 or obs.shape[0] != obs.shape[1] or pc.ndim != 3 or pc.shape[1:] != obs.shape or pc.shape[0] < 1:
        raise ValueError('derive: observed (C, C), perm_counts (P, C, C) with P >= 1')
    P = pc.shape[0]
    mean, std = pc.mean(axis=0, dtype=np.float64), pc.std(axis=0, dtype=np.float64)
    z = np.divide(obs - mean, std, out=np.zeros(obs.shape, np.float64), where=std > 0)
    return dict(mean=mean, std=std, z=z, p_enriched=(1 + (pc >= obs[None]).sum(axis=0)) / (P + 1.0),
                p_depleted=(1 + (pc <= obs[None]).sum(axis=0)) / (P + 1.0))


def write_npz(path, nuclei_id, xy, label, observed, perm_counts, class_n, radius_px, seed):
    """<id>_nuclei_enrichment.npz, the header row i for the i-th row of <id>_nuclei_graph.npz / <id>_nuclei_feat.npz:
      nuclei_id int64 (n,), xy float64 (n, 2) (the unquantised centre in slide px), label int64 (n,): the rows, in the order pi acted on
      radius_px float64, perms int64, seed int64 as 0-d arrays
      observed int64 (C, C), perm_counts int64 (P, C, C), class_n int64 (C,): the integers of the definition
      mean, std, z, p_enriched, p_depleted float64 (C, C): `derive`."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    observed = np.ascontiguousarray(observed, np.int64)
    perm_counts = np.ascontiguousarray(perm_counts, np.int64)
    class_n = np.ascontiguousarray(class_n, np.int64).reshape(-1)
    C = len(class_n)
    if observed.shape != (C, C) or perm_counts.ndim != 3 or perm_counts.shape[1:] != (C, C):
        raise ValueError('write_npz: observed (C, C), perm_counts (P, C, C), class_n (C,)')
    check_args(C, half_pixel_radius(radius_px), len(perm_counts), seed)
    with open(path, 'wb') as f:
        np.savez(f, **head, radius_px=np.asarray(float(radius_px), np.float64), perms=np.asarray(len(perm_counts), np.int64),
                 seed=np.asarray(int(seed), np.int64), observed=observed, perm_counts=perm_counts, class_n=class_n, **derive(observed, perm_counts))
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)
