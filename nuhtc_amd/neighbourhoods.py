"""Cellular neighbourhoods of a slide: what kind of tissue each nucleus sits in.  The class composition of every nucleus's window (itself
and its k nearest neighbours) is a small integer vector; the vectors are clustered by k-means into K neighbourhood types; each nucleus gets
its type, each type its composition -- the cellular-neighbourhood analysis of CODEX / histoCAT / squidpy (Goltsev 2018, Schuerch 2020).
Stated in integers (fixed-point centres, exact k-means++ picks from prefix sums, ties to the smaller index), so the result is a pure
function of (rows, k, radius, K, seed), bitwise the same on every run.  Computed on the GPU (csrc/cellhood.hip,
`nuhtc_cell_neighbourhoods`, on the tensors `nuhtc_cell_graph` left on the device); tools/infer_wsi.py --nuclei-neighbourhoods writes it
as <id>_nuclei_neighbourhoods.npz.  Not in the reference.

Definition.

Inputs.  n <= 2**24 points in half pixels, as `cellpoints.quantize_centres` gives them, with one label each; C classes, 1..14; the
graph's r (1..16384 half pixels) and k (1..32); K types, 1..32; seed, 0..2**32-1; max_iter, 1..1000; optionally given centres q0, int32
(K, C), every entry 0..34000.

Window.  w[i] is int (C,).  w[i][c] is the number of rows of label c among row i itself and the rows `nuhtc_cell_graph` lists for i at
(r, k): the first k by (d2, j) within the inclusive radius.  A label outside 0..C-1 is counted in no class.  So sum(w[i]) <= k + 1 <= 33,
and a row whose window holds only unknown labels has the zero vector.

Generator.  fmix is the murmur3 finaliser of enrichment.py / csrc/cellenrich_host.h, mod 2**32.  For j = 0..K-1:
b = fmix(seed + 0x9E3779B9 * (j + 1)) and u_j = (fmix(b + 0x7F4A7C15) << 32) | fmix(b + 2 * 0x7F4A7C15).

Seeding (k-means++ in exact integers; used only when no centres are given).  row_0 = u_0 mod n.  For j = 1..K-1:
g_i = min over the rows chosen so far of sum_c (w[i][c] - w[row][c])**2, in plain count units (g_i <= 2 * 33**2, so the total
T = sum g_i <= 2**24 * 2178 < 2**36).  If T == 0 then row_j = row_0.  Otherwise t = u_j mod T, and row_j is the smallest i whose
inclusive prefix sum of g exceeds t.  q[j] = 1024 * w[row_j].

Lloyd in fixed point (F = 10 bits).  D(i, j) = sum_c (1024 * w[i][c] - q[j][c])**2, in int64.  Bounds: a term is at most 34000**2 <
2**31; with centres the update made (means of windows) D stays below 2 * 33792**2 < 2**32, with given centres below 14 * 34000**2 <
2**34; summed over 2**24 rows below 2**58.  Iteration t = 1, 2, ..: a_t[i] = argmin_j D(i, j), a tie going to the smaller j (so a
duplicate centre stays empty).  If a_t == a_{t-1} (a_0 all -1), stop: converged, n_iter = t.  If t == max_iter, stop: not converged,
n_iter = max_iter.  Otherwise update: for every type with m_j > 0 members and member sum s_j,
q[j][c] = floor((2 * 1024 * s_j[c] + m_j) / (2 * m_j)), which rounds half up; an empty type keeps its q.  With given centres: q = q0,
one assignment, no update, n_iter = 0, converged.

Outputs, all integers.
  window      int32 (n, C)   the windows w
  hood        int32 (n,)     the final a
  centre_q    int32 (K, C)   the centres the final assignment was made against
  centre_sum  int64 (K, C)   the window sums of that assignment
  centre_n    int64 (K,)     the member counts of that assignment
  seed_rows   int32 (K,)     the seeding rows, -1 with given centres
  inertia     int64          sum_i D(i, hood[i])
  n_iter, converged          as defined above

Edge cases.  n = 0 gives empty outputs; the centres are q0 or zeros, seed_rows is -1, n_iter 0, converged.  The ORDER of the rows is
part of the input, as in enrichment.py: the seeding picks row numbers.

`neighbourhoods_reference` restates all of the above in numpy int64 on top of `cellgraph.graph_reference` (`windows_of` and
`cluster_reference` are its two halves, usable on a neighbour list alone): the oracle the device result must EQUAL.  `derive` makes the
float64 side on the host.  The generator, the pick rule, the rounding and D are also plain C++ in csrc/cellhood_host.h, which the
kernels use and the library exports for the host alone (`host_draws`, `host_rule`), so a disagreement names the rule and not the kernel.

Not provided: radius windows (their counts have no bound), choosing K by a criterion, restarts, type-to-type adjacency, and a cohort fit
over several slides -- a cohort is served by giving the centres of one fitted slide (`read_centres`, --neighbourhood-centres)."""
import numpy as np

from . import cellgraph, cellpoints
from .cellgraph import MAX_K
from .cellpoints import MAX_CLASSES, MAX_POINTS, MAX_R, half_pixel_radius  # noqa: F401 (re-exported)
from .enrichment import MAX_SEED, _fmix

MAX_TYPES = 32
MAX_ITER = 1000
FRAC_BITS = 10
ONE = 1 << FRAC_BITS                  # a count of 1 in the centres' fixed point
MAX_CENTRE = 34000                    # a given centre: 0 .. 34000 (1024 * 33 = 33792 is the largest a fit can make)
_M32 = 0xFFFFFFFF

INT_NAMES = ('window', 'hood', 'centre_q', 'centre_sum', 'centre_n', 'seed_rows')
INT_TYPES = (np.int32, np.int32, np.int32, np.int64, np.int64, np.int32)
SCALAR_KEYS = ('inertia', 'n_iter', 'converged')
DERIVED_KEYS = ('composition', 'fraction', 'enrichment_log2', 'hood_class_count', 'hood_size', 'order_by_size', 'inertia_per_nucleus')
PARAM_KEYS = ('radius_px', 'k', 'types', 'seed', 'max_iter', 'centres_given')
NPZ_KEYS = ('nuclei_id', 'xy', 'label') + INT_NAMES + SCALAR_KEYS + DERIVED_KEYS + PARAM_KEYS


def check_args(num_classes, r, k, types, seed=0, max_iter=100):
    """num_classes 1..14, r 1..16384 half pixels, k 1..32, types 1..32, seed 0..2**32-1, max_iter 1..1000, all whole numbers: ValueError
    otherwise."""
    v = (num_classes, r, k, types, seed, max_iter)
    whole = all(float(x) == int(x) for x in v)
    if not (whole and 1 <= int(num_classes) <= MAX_CLASSES and 1 <= int(r) <= MAX_R and 1 <= int(k) <= MAX_K and 1 <= int(types) <= MAX_TYPES
            and 0 <= int(seed) <= MAX_SEED and 1 <= int(max_iter) <= MAX_ITER):
        raise ValueError(f'neighbourhoods: num_classes 1..{MAX_CLASSES}, r 1..{MAX_R} half pixels, k 1..{MAX_K}, types 1..{MAX_TYPES}, seed 0..2**32-1, '
                         f'max_iter 1..{MAX_ITER} (got num_classes={num_classes}, r={r}, k={k}, types={types}, seed={seed}, max_iter={max_iter})')


def as_centres(centres, types, num_classes):
    """Given centres -> int64 (K, C); ValueError unless whole numbers 0..34000 of that shape."""
    raw = np.asarray(centres)
    q = raw.astype(np.int64)
    if q.shape != (int(types), int(num_classes)) or not np.array_equal(q, raw) or (q.size and (q.min() < 0 or q.max() > MAX_CENTRE)):
        raise ValueError(f'neighbourhoods: given centres are whole numbers 0..{MAX_CENTRE} of shape (types, num_classes) = ({types}, {num_classes}) '
                         f'(got shape {raw.shape})')
    return q


# ---- the definition
def draws(seed, types):
    """u_0 .. u_{K-1} of the generator -> a list of Python integers below 2**64."""
    fmix = lambda v: int(_fmix(v & _M32))
    out = []
    for j in range(int(types)):
        b = fmix(int(seed) + 0x9E3779B9 * (j + 1))
        out.append((fmix(b + 0x7F4A7C15) << 32) | fmix(b + 2 * 0x7F4A7C15))
    return out


def windows_of(neighbors, labels, num_classes):
    """The windows of a neighbour list: neighbors int (n, k) rows or -1, labels int (n,) -> int64 (n, C).  ValueError for an index outside
    -1..n-1."""
    lab = np.asarray(labels, np.int64).reshape(-1)
    n, C = len(lab), int(num_classes)
    nb = np.asarray(neighbors, np.int64)
    nb = nb.reshape(n, nb.size // n if n else 0)
    if nb.size and (nb.min() < -1 or nb.max() >= n):
        raise ValueError('neighbourhoods: a neighbour index outside -1..n-1')
    cls = np.where((lab >= 0) & (lab < C), lab, C)               # C: counted in no class
    w = np.zeros((n, C + 1), np.int64)
    rows = np.arange(n)
    w[rows, cls] += 1                                            # the row itself
    for col in range(nb.shape[1]):
        there = nb[:, col] >= 0
        np.add.at(w, (rows[there], cls[nb[there, col]]), 1)
    return np.ascontiguousarray(w[:, :C])


def pick(prefix, t):
    """The smallest i whose inclusive prefix sum exceeds t (prefix int64 (n,) non-decreasing, 0 <= t < prefix[-1])."""
    return int(np.searchsorted(prefix, int(t), side='right'))


def seeding(w, types, seed):
    """The seeding rows of windows w int64 (n, C), n >= 1 -> a list of K Python integers."""
    n, u = len(w), draws(seed, types)
    rows = [u[0] % n]
    g = ((w - w[rows[0]]) ** 2).sum(1)
    for j in range(1, int(types)):
        T = int(g.sum())
        rows.append(rows[0] if T == 0 else pick(np.cumsum(g), u[j] % T))
        g = np.minimum(g, ((w - w[rows[-1]]) ** 2).sum(1))
    return rows


def distances(w, q, block=1 << 16):
    """D of the definition: w int64 (n, C), q int64 (K, C) -> yields (row slice, int64 (b, K)) in blocks of rows."""
    for i0 in range(0, len(w), block):
        rows = slice(i0, min(i0 + block, len(w)))
        d = ONE * w[rows, None, :] - q[None, :, :]
        yield rows, (d * d).sum(2)


def assign(w, q):
    """-> (a int64 (n,): argmin_j D with ties to the smaller j, inertia: the sum of the minima, a Python integer)."""
    a, total = np.zeros(len(w), np.int64), 0
    for rows, D in distances(w, q):
        a[rows] = D.argmin(1)                                    # the first of equals
        total += int(D.min(1).sum())
    return a, total


def member_sums(w, a, types):
    """-> (s int64 (K, C), m int64 (K,)): the window sums and the members of each type under the assignment a."""
    s = np.zeros((int(types), w.shape[1]), np.int64)
    np.add.at(s, a, w)
    return s, np.bincount(a, minlength=int(types)).astype(np.int64)


def rounded_means(s, m, q):
    """The update: floor((2 * 1024 * s + m) / (2 * m)) where m > 0, q where m == 0."""
    mm = np.maximum(m, 1)[:, None]
    return np.where(m[:, None] > 0, (2 * ONE * s + mm) // (2 * mm), q)


def cluster_reference(window, types, seed, max_iter, centres=None):
    """Seeding and Lloyd of the definition on windows int (n, C) -> (hood int32 (n,), centre_q int32 (K, C), centre_sum int64 (K, C),
    centre_n int64 (K,), seed_rows int32 (K,), inertia, n_iter, converged).  Time and memory O(n K C) per iteration."""
    w = np.ascontiguousarray(window, np.int64)
    n, C = w.shape
    K = int(types)
    check_args(C, 1, 1, K, seed, max_iter)
    rows = np.full(K, -1, np.int32)
    q = np.zeros((K, C), np.int64) if centres is None else as_centres(centres, K, C)
    if n == 0:
        return np.zeros(0, np.int32), q.astype(np.int32), np.zeros((K, C), np.int64), np.zeros(K, np.int64), rows, 0, 0, True
    if centres is not None:
        a, inertia = assign(w, q)
        n_iter, converged = 0, True
    else:
        rows = np.asarray(seeding(w, K, seed), np.int32)
        q = ONE * w[rows]
        before = np.full(n, -1, np.int64)
        for t in range(1, int(max_iter) + 1):
            a, inertia = assign(w, q)
            n_iter, converged = t, bool(np.array_equal(a, before))
            if converged or t == int(max_iter):
                break
            q = rounded_means(*member_sums(w, a, K), q)
            before = a
    s, m = member_sums(w, a, K)
    return a.astype(np.int32), q.astype(np.int32), s, m, rows, int(inertia), int(n_iter), bool(converged)


def neighbourhoods_reference(points, labels, num_classes, r, k, types, seed=0, max_iter=100, centres=None):
    """The definition on top of cellgraph.graph_reference: points int (n, 2) half pixels, labels int (n,), r in HALF pixels -> (window
    int32 (n, C), hood, centre_q, centre_sum, centre_n, seed_rows, inertia, n_iter, converged).  The graph is O(n^2): for n of a few
    thousand; `windows_of` and `cluster_reference` take a neighbour list of any size."""
    check_args(num_classes, r, k, types, seed, max_iter)
    neighbors = cellgraph.graph_reference(points, labels, num_classes, r, k)[0]
    w = windows_of(neighbors, labels, num_classes)
    return (w.astype(np.int32),) + cluster_reference(w, types, seed, max_iter, centres)


# ---- the device
def outputs(n, num_classes, types, device, fill=0):
    """The six output tensors of `call` for n rows on `device` (one row at least each), every entry `fill`."""
    import torch
    n, C, K = max(int(n), 1), int(num_classes), int(types)
    shapes = (((n, C), torch.int32), ((n,), torch.int32), ((K, C), torch.int32), ((K, C), torch.int64), ((K,), torch.int64), ((K,), torch.int32))
    return [torch.full(s, fill, dtype=t, device=device) for s, t in shapes]


def call(neighbors, labels, n, k, num_classes, types, seed, max_iter, centres_given, window, hood, centre_q, centre_sum, centre_n, seed_rows, device=0):
    """nuhtc_cell_neighbourhoods on torch tensors of cuda:`device` (contiguous; neighbors (n, k) and labels (n,) int32 as nuhtc_cell_graph
    took and left them; the outputs as `outputs` makes them, centre_q holding the given centres when `centres_given`) -> (the library's
    return code, n_iter, converged, inertia), nothing raised: the code is 0 or hip.E_INVALID / hip.E_HIP; the three are None unless it is 0."""
    import ctypes
    import torch
    from . import hip
    fn = hip.load().nuhtc_cell_neighbourhoods
    counts = (ctypes.c_int64 * 3)(-1, -1, -1)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    dev = torch.device('cuda', device)
    with torch.cuda.device(dev):
        rc = fn(int(device), vp(neighbors), vp(labels), int(n), int(k), int(num_classes), int(types), int(seed) & MAX_SEED, int(max_iter),
                int(bool(centres_given)), vp(centre_q), vp(window), vp(hood), vp(centre_sum), vp(centre_n), vp(seed_rows), counts,
                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return (rc,) + ((int(counts[0]), bool(counts[1]), int(counts[2])) if rc == 0 else (None, None, None))


def from_neighbors(neighbors, labels, num_classes, types, seed=0, max_iter=100, centres=None, device=0):
    """The device call on a neighbour list alone: neighbors int (n, k) numpy, labels int (n,) -> the nine results of
    `neighbourhoods_reference`.  ValueError when the library refuses (an index outside -1..n-1)."""
    import torch
    lab = np.ascontiguousarray(np.asarray(labels).reshape(-1), np.int32)
    n, C, K = len(lab), int(num_classes), int(types)
    nb = np.asarray(neighbors)
    k = nb.size // n if n else (nb.shape[1] if nb.ndim == 2 else 1)
    nb = np.ascontiguousarray(nb.reshape(n, k), np.int32)
    check_args(C, 1, k, K, seed, max_iter)
    dev = torch.device('cuda', device)
    nb_d = torch.from_numpy(nb if n else np.full((1, k), -1, np.int32)).to(dev)
    lab_d = torch.from_numpy(lab if n else np.zeros(1, np.int32)).to(dev)
    return _run(nb_d, lab_d, n, k, C, K, seed, max_iter, centres, dev, device)


def _run(nb_d, lab_d, n, k, C, K, seed, max_iter, centres, dev, device):
    import torch
    out = outputs(n, C, K, dev)
    if centres is not None:
        out[2].copy_(torch.from_numpy(as_centres(centres, K, C).astype(np.int32)))
    rc, n_iter, converged, inertia = call(nb_d, lab_d, n, k, C, K, seed, max_iter, centres is not None, *out, device=device)
    cellpoints.raise_for(rc, 'nuhtc_cell_neighbourhoods')
    sizes = (n, n, K, K, K, K)
    return tuple(t[:s].cpu().numpy() for t, s in zip(out, sizes)) + (inertia, n_iter, converged)


def build(points, labels, num_classes, radius_px, k, types, seed=0, max_iter=100, centres=None, device=0):
    """The neighbourhoods of `points` (int (n, 2) half pixels, see cellpoints.quantize_centres) with `labels` (n,) on cuda:`device`: numpy
    in, the nine results of `neighbourhoods_reference` out.  The graph is built by `cellgraph.call`; its tensors stay on the device and go
    to nuhtc_cell_neighbourhoods as they are.  `centres`: int (types, num_classes) to assign against without fitting.  There is no host
    route: without the library or a GPU this raises."""
    import torch
    C, k, K, r = int(num_classes), int(k), int(types), half_pixel_radius(radius_px)
    check_args(C, r, k, K, seed, max_iter)
    if centres is not None:
        centres = as_centres(centres, K, C)
    p, lab, dev, p_d, lab_d, bounds = cellpoints.resident(points, labels, 'neighbourhoods', device)
    n = len(p)
    graph = [torch.full((max(n, 1), w), fill, dtype=torch.int32, device=dev) for w, fill in ((k, -1), (k, -1), (C, 0))]
    if n:
        cellpoints.raise_for(cellgraph.call(p_d, lab_d, C, r, k, *graph, bounds=bounds, device=device), 'nuhtc_cell_graph')
    else:
        lab_d = torch.zeros(1, dtype=torch.int32, device=dev)
    return _run(graph[0], lab_d, n, k, C, K, seed, max_iter, centres, dev, device)


# ---- host-only exports of the library (the C++ of csrc/cellhood_host.h; no GPU is touched)
def host_draws(seed, types):
    import ctypes
    from . import hip
    out = np.zeros(MAX_TYPES, np.uint64)
    if hip.load().nuhtc_neighbourhood_draws(int(seed) & MAX_SEED, int(types), out.ctypes.data_as(ctypes.c_void_p)):
        raise ValueError(f'nuhtc_neighbourhood_draws: invalid arguments (types={types})')
    return [int(v) for v in out[:int(types)]]


def host_rule(what, a, b, c=0):
    """The library's host export of one rule of csrc/cellhood_host.h -> a Python integer: 'pick' (a: inclusive prefix int64 array, b: t),
    'round' (a: s, b: m, c: the q an empty type keeps), 'distance' (a: window int (C,), b: centre int (C,))."""
    import ctypes
    from . import hip
    fn = hip.load().nuhtc_neighbourhood_rule
    out = ctypes.c_int64(-1)
    if what == 'pick':
        arr = np.ascontiguousarray(a, np.int64)
        rc = fn(0, arr.ctypes.data_as(ctypes.c_void_p), None, len(arr), int(b), 0, ctypes.byref(out))
    elif what == 'round':
        rc = fn(1, None, None, int(a), int(b), int(c), ctypes.byref(out))
    elif what == 'distance':
        x, y = np.ascontiguousarray(a, np.int64), np.ascontiguousarray(b, np.int64)
        rc = fn(2, x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), len(x), len(y), 0, ctypes.byref(out))
    else:
        raise ValueError(what)
    if rc:
        raise ValueError(f'nuhtc_neighbourhood_rule: invalid arguments ({what})')
    return int(out.value)


# ---- the host side
def _as_outputs(window, hood, centre_q, centre_sum, centre_n, seed_rows):
    w, a, q, s, m, rows = [np.ascontiguousarray(x, t) for x, t in zip((window, hood, centre_q, centre_sum, centre_n, seed_rows), INT_TYPES)]
    if w.ndim != 2 or q.ndim != 2 or q.shape != s.shape or q.shape[1] != w.shape[1] or m.shape != (len(q),) or rows.shape != (len(q),) or a.shape != (len(w),):
        raise ValueError('neighbourhoods: window (n, C), hood (n,), centre_q and centre_sum (K, C), centre_n and seed_rows (K,)')
    if len(a) and (a.min() < 0 or a.max() >= len(q)):
        raise ValueError('neighbourhoods: a type is 0..K-1')
    return w, a, q, s, m, rows


def derive(hood, centre_sum, centre_n, inertia, labels):
    """The float64 side of the integers -> dict, never NaN:
      composition         float64 (K, C)  centre_sum / centre_n: the mean window of each type, 0 for an empty type
      fraction            float64 (K, C)  composition, each row normalised to sum 1 (0 for a row of zeros)
      enrichment_log2     float64 (K, C)  log2 of fraction over the slide-wide window fraction of the class, 0 where either is 0
      hood_class_count    int64 (K, C)    the nuclei of class c whose OWN type is j (a label outside 0..C-1 is counted nowhere)
      hood_size           int64 (K,)      centre_n
      order_by_size       int64 (K,)      the types by descending size, ties to the smaller j
      inertia_per_nucleus float64 0-d     inertia / 1024**2 / n, in squared counts (0 without nuclei)"""
    s, m = np.asarray(centre_sum, np.int64), np.asarray(centre_n, np.int64).reshape(-1)
    a, lab = np.asarray(hood, np.int64).reshape(-1), np.asarray(labels, np.int64).reshape(-1)
    K, C = s.shape
    if len(m) != K or len(lab) != len(a):
        raise ValueError('derive: centre_sum (K, C), centre_n (K,), one label per entry of hood')
    comp = np.divide(s, m[:, None], out=np.zeros((K, C), np.float64), where=m[:, None] > 0)
    tot = comp.sum(1, keepdims=True)
    frac = np.divide(comp, tot, out=np.zeros((K, C), np.float64), where=tot > 0)
    slide = s.sum(0)
    slide = np.divide(slide, slide.sum(), out=np.zeros(C, np.float64), where=slide.sum() > 0)
    both = (frac > 0) & (slide[None, :] > 0)
    ratio = np.divide(frac, slide[None, :], out=np.ones((K, C), np.float64), where=both)
    known = (lab >= 0) & (lab < C)
    counts = np.zeros((K, C), np.int64)
    np.add.at(counts, (a[known], lab[known]), 1)
    return dict(composition=comp, fraction=frac, enrichment_log2=np.where(both, np.log2(ratio), 0.0), hood_class_count=counts, hood_size=m.copy(),
                order_by_size=np.argsort(-m, kind='stable').astype(np.int64),
                inertia_per_nucleus=np.asarray(int(inertia) / float(ONE * ONE) / len(a) if len(a) else 0.0, np.float64))


def write_npz(path, nuclei_id, xy, label, window, hood, centre_q, centre_sum, centre_n, seed_rows, inertia, n_iter, converged, radius_px, k, seed=0,
              max_iter=100):
    """<id>_nuclei_neighbourhoods.npz, row i for the i-th row of <id>_nuclei_graph.npz / <id>_nuclei_feat.npz:
      nuclei_id int64 (n,), xy float64 (n, 2) (the unquantised centre in slide px), label int64 (n,)
      the six integer arrays of the definition (INT_NAMES); inertia, n_iter, converged as int64 0-d arrays
      the arrays of `derive` (DERIVED_KEYS)
      radius_px float64, k, types, seed, max_iter, centres_given int64 as 0-d arrays (centres_given: seed_rows holds -1)."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    arrays = _as_outputs(window, hood, centre_q, centre_sum, centre_n, seed_rows)
    if len(arrays[1]) != len(head['label']):
        raise ValueError('write_npz: one type per nucleus')
    K, C = arrays[2].shape
    check_args(C, half_pixel_radius(radius_px), k, K, seed, max_iter)
    i64 = lambda v: np.asarray(int(v), np.int64)
    with open(path, 'wb') as f:
        np.savez(f, **head, **dict(zip(INT_NAMES, arrays)), inertia=i64(inertia), n_iter=i64(n_iter), converged=i64(bool(converged)),
                 **derive(arrays[1], arrays[3], arrays[4], inertia, head['label']), radius_px=np.asarray(float(radius_px), np.float64), k=i64(k),
                 types=i64(K), seed=i64(seed), max_iter=i64(max_iter), centres_given=i64(bool(len(arrays[5]) and arrays[5][0] < 0 and int(n_iter) == 0)))
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote (NPZ_KEYS)."""
    return cellpoints.read_npz(path, NPZ_KEYS)


def read_centres(path, k=None, radius_px=None, num_classes=None):
    """The centres of a file write_npz wrote, to assign another slide against -> int32 (K, C).  ValueError when the file is not one, or
    when its k, radius_px or class count is not the run's (each compared when given): a window of another graph counts other things."""
    try:
        z = cellpoints.read_npz(path, ('centre_q', 'k', 'radius_px'))
    except (OSError, KeyError, ValueError) as e:
        raise ValueError(f'neighbourhoods: {path} is no file of --nuclei-neighbourhoods ({e})')
    q = z['centre_q']
    if q.ndim != 2 or not (1 <= q.shape[0] <= MAX_TYPES and 1 <= q.shape[1] <= MAX_CLASSES):
        raise ValueError(f'neighbourhoods: {path} holds centres of shape {q.shape}')
    for name, mine, theirs in (('k', k, int(z['k'])), ('radius_px', radius_px, float(z['radius_px'])), ('num_classes', num_classes, q.shape[1])):
        if mine is not None and float(mine) != float(theirs):
            raise ValueError(f'neighbourhoods: the centres of {path} were fitted at {name} = {theirs:g}, this run has {float(mine):g}')
    return as_centres(q, q.shape[0], q.shape[1]).astype(np.int32)
