"""Nucleus territories of a slide: the nearest-nucleus raster of the nucleus centres -- which nucleus, and so which cell class, each piece
of the plane belongs to, the question none of the other per-slide analyses answers (who relates to whom: cellgraph.py, spatial.py,
clusters.py, mst.py, proximity.py, enrichment.py; how much mass lies where: density.py; which annotated region holds what: regions.py,
margin.py).  It is the Voronoi family of the nucleus-architecture literature in raster form: the area of a nucleus' territory as a local
crowding measure, the territory area by class (the tumour / stroma / immune compartment shares of a slide without an annotation), the
length of the border between the territories of two classes, and a distance-to-nearest-nucleus map.  On the lattice of density.py the
owner of a site is the argmin of an integer pair: unique, exact, local, bitwise repeatable and checkable by brute force -- no circumcentre
(a rational that needs more than 64 bits) and no tie rule for cocircular points.  Computed on the GPU (csrc/cellterritory.hip,
`nuhtc_cell_territory`); tools/infer_wsi.py --nuclei-territory writes it as <id>_nuclei_territory.npz.  Not in the reference.

Definition.

Inputs.  n points in HALF pixels, int32 (n, 2), from `cellpoints.quantize_centres`, with |p| < 2**27 and 0 <= n <= 2**24; labels, int32, one
per point; C classes, 1 <= C <= 14; the reach R in half pixels, an integer with 1 <= R <= 16384; the pitch s in half pixels, an integer
with 1 <= s <= 2**20; the window in lattice units, integers gx0, gy0, W, H with W, H >= 1, W * H <= 2**28 (this module's own cap: one
int32 per site and map here, where density has 12 C bytes per site -- a whole slide at a few pixels of pitch does not fit in 2**24 sites)
and every site coordinate |g * s| < 2**28 (checked on the host in 64 bits); and the points' bounding box, computed by the caller.

Sites.  Site (u, v) of the window lies at q = ((gx0 + u) * s, (gy0 + v) * s): the lattice of density.py, anchored at the slide's origin.

Competitors.  The rows with a label in 0..C-1 compete.  A row with any other label owns nothing and blocks nothing, as if it were absent
(density's "counted nowhere").

Owner.  owner[v][u] is the competitor i that minimises the pair (d2(q, p_i), i) among those with d2(q, p_i) <= R * R.  The reach is
inclusive; a tie in d2 goes to the smaller row; the value is -1 when no competitor is in reach.  nearest_d2[v][u] is that d2, or -1.  Both
are int32 (H, W).  The owner of a site does not depend on the window: a sub-window is a slice of the full map.

Tallies.  They are OVER THE WINDOW and so do depend on it: a site's 4-neighbours are those inside the window, and a territory cut by the
window's edge is counted as far as the window goes.
  area         int32 (n,)    the sites a row owns
  border       int32 (n,)    its sites with at least one 4-neighbour whose owner differs (an owner of -1 counts as different)
  open         0 / 1 (n,)    the row owns a site on the window's outer row or column, or a site that has a 4-neighbour with owner -1: the
                             reach or the window bounds such a territory, not its neighbours, and its area is NOT a Voronoi area
                             (int32 flags on the device, uint8 in the file)
  contact      int64 (C, C)  over every ordered pair (site, 4-neighbour) with owners i != j, both >= 0, one count at [label_i][label_j]:
                             symmetric by construction; the diagonal counts borders between two nuclei of one class
  class_sites  int64 (C,)    the sites owned by each class
  free_sites   int64 0-d     the sites nobody owns; class_sites.sum() + free_sites == W * H

Bit budget.  |q - p| < 2**28 + 2**27, so the differences are exact int32; the box test against R comes before the products; d2 <= 2**28;
(d2, row) packs into one 64-bit key, so the argmin is one compare; area <= 2**28; a site adds at most 4 to an entry of contact
(csrc/cellgrid_host.h has the argument).

Default window.  `window(bounds, R, s)` is density's with h = R: every site that can be owned.  The entry point accepts any window.

`territory_reference` is the brute-force int64 restatement (every site against every row, no grid): the oracle the device result must
EQUAL in every output.  `derive` makes the float64 side on the host.

The adjacency as an edge list (the discrete Delaunay graph) and the number of distinct neighbours per nucleus are adjacency.py's, read off
this module's owner map on the device.  Out of scope: the empty-space function F (derivable from nearest_d2 when the maps are kept); tissue clipping other than the reach -- a nucleus at the tissue border owns
the plane up to R beyond it, and is `open`.  The exact Voronoi diagram stays out of scope; this is its lattice form, at the
stated resolution s."""
import numpy as np

from . import cellpoints, density
from .cellpoints import COORD_LIMIT, MAX_CLASSES, MAX_POINTS, MAX_R, centres, half_pixel_radius, quantize_centres  # noqa: F401 (re-exported)
from .density import MAX_PITCH, SITE_LIMIT, window  # noqa: F401 (the lattice and the default window are density's, with h = R)

MAX_SITES = 1 << 28
INT_NAMES = ('area', 'border', 'open', 'contact', 'class_sites', 'free_sites')
MAP_NAMES = ('owner', 'nearest_d2')
DERIVED_KEYS = ('area_px2', 'closed', 'n_closed', 'closed_area_mean_px2', 'closed_area_std_px2', 'area_disorder', 'class_area_share',
                'free_share', 'contact_share')
NPZ_KEYS = ('nuclei_id', 'xy', 'label') + INT_NAMES + DERIVED_KEYS + ('reach_px', 'pitch_px', 'origin_px', 'window')


def check_args(num_classes, r, s, win=None):
    """density.check_lattice with this module's cap of 2**28 sites."""
    density.check_lattice('territory', 'reach', 'r', MAX_SITES, num_classes, r, s, win)


def tally(owner, labels, num_classes, n=None):
    """The tallies of an owner map int (H, W) over its own window, from the definition: -> (area int32 (n,), border int32 (n,), open uint8
    (n,), contact int64 (C, C), class_sites int64 (C,), free_sites int64 0-d).  numpy on the host; `territory_reference` ends with it."""
    own = np.asarray(owner, np.int64)
    lab = np.asarray(labels, np.int64).reshape(-1)
    n, C = len(lab) if n is None else int(n), int(num_classes)
    H, W = own.shape
    differs, beside_free = np.zeros((H, W), bool), np.zeros((H, W), bool)
    contact = np.zeros((C, C), np.int64)
    for here, there in (((slice(None), slice(1, None)), (slice(None), slice(0, -1))), ((slice(None), slice(0, -1)), (slice(None), slice(1, None))),
                        ((slice(1, None), slice(None)), (slice(0, -1), slice(None))), ((slice(0, -1), slice(None)), (slice(1, None), slice(None)))):
        a, b = own[here], own[there]                           # a site and its neighbour on one of the four sides
        differs[here] |= a != b
        beside_free[here] |= b < 0
        pair = (a != b) & (a >= 0) & (b >= 0)
        np.add.at(contact, (lab[a[pair]], lab[b[pair]]), 1)
    rim = np.zeros((H, W), bool)
    rim[0, :] = rim[-1, :] = rim[:, 0] = rim[:, -1] = True
    owned = own >= 0
    area = np.bincount(own[owned], minlength=n)
    border = np.bincount(own[owned & differs], minlength=n)
    is_open = np.bincount(own[owned & (rim | beside_free)], minlength=n) > 0
    class_sites = np.bincount(lab[own[owned]], minlength=C).astype(np.int64)
    return (area.astype(np.int32), border.astype(np.int32), is_open.astype(np.uint8), contact, class_sites,
            np.asarray(int(H * W - owned.sum()), np.int64))


def territory_reference(points, labels, num_classes, r, s, win, block=4096):
    """The definition in int64: points int (n, 2) half pixels, labels int (n,), r and s in HALF pixels, win = (gx0, gy0, W, H) ->
    (owner int32 (H, W), nearest_d2 int32 (H, W)) + the six of `tally`.  Every site against EVERY competing row, no grid, `block` sites at a
    time (a few (block, n) int64 temporaries).  Meant for about 1e4 sites by a few thousand points."""
    check_args(num_classes, r, s, win)
    p, lab = cellpoints.reference_points(points, labels, 'territory_reference')
    C, r, s = int(num_classes), int(r), int(s)
    gx0, gy0, W, H = (int(v) for v in win)
    rows = np.flatnonzero((lab >= 0) & (lab < C))              # the competitors, ascending: the first minimum is the smaller row
    q = p[rows]
    owner, d2min = np.full(H * W, -1, np.int64), np.full(H * W, -1, np.int64)
    v, u = np.divmod(np.arange(H * W, dtype=np.int64), W)
    qx, qy = (gx0 + u) * s, (gy0 + v) * s
    block = max(1, min(int(block), (1 << 22) // max(len(q), 1)))              # a temporary of at most 32 MiB
    far = np.iinfo(np.int64).max
    for k0 in range(0, H * W if len(q) else 0, block):
        sl = slice(k0, k0 + block)
        d2 = (qx[sl, None] - q[None, :, 0]) ** 2 + (qy[sl, None] - q[None, :, 1]) ** 2
        d2[d2 > r * r] = far
        j = d2.argmin(1)                                       # the first of the minima
        best = d2[np.arange(len(j)), j]
        owner[sl] = np.where(best < far, rows[j], -1)
        d2min[sl] = np.where(best < far, best, -1)
    owner = owner.astype(np.int32).reshape(H, W)
    return (owner, d2min.astype(np.int32).reshape(H, W)) + tally(owner, lab, C)


def call(points, labels, num_classes, r, s, win, owner, nearest_d2, area, border, is_open, contact, class_sites, free_sites, bounds=None, device=0):
    """nuhtc_cell_territory on torch tensors of cuda:`device` (contiguous; owner and nearest_d2 int32 (H, W), area, border and is_open int32
    (n,), contact int64 (C, C), class_sites int64 (C,), free_sites int64 (1,); r and s in HALF pixels, win = (gx0, gy0, W, H)) -> the library's
    return code, nothing raised: 0 or hip.E_INVALID / hip.E_HIP.  bounds = (x_min, y_min, x_max, y_max) of the points, computed on the host
    when not given."""
    return cellpoints.launch('nuhtc_cell_territory', device, points, labels, (int(num_classes), int(r), int(s)) + tuple(int(v) for v in win),
                             (owner, nearest_d2, area, border, is_open, contact, class_sites, free_sites), bounds)


def outputs(n, num_classes, win, device, fill=0):
    """The eight output tensors of `call` for n points and a window on `device`, every entry `fill`."""
    import torch
    C, hw = int(num_classes), (int(win[3]), int(win[2]))
    shapes = ((hw, torch.int32), (hw, torch.int32), ((int(n),), torch.int32), ((int(n),), torch.int32), ((int(n),), torch.int32),
              ((C, C), torch.int64), ((C,), torch.int64), ((1,), torch.int64))
    return [torch.full(shape, fill, dtype=t, device=device) for shape, t in shapes]


def build(points, labels, num_classes, reach_px, pitch_px, win=None, maps=False, device=0):
    """The territories of `points` (int (n, 2) half pixels, see cellpoints.quantize_centres) with `labels` (n,) on cuda:`device`: numpy in,
    (tallies, window, maps) out -- tallies the six arrays of INT_NAMES (open as uint8, free_sites 0-d), maps (owner, nearest_d2) with
    maps=True and None otherwise: the two rasters are copied off the device only when asked for.  Without `win` the window is the default
    one of the points' bounding box (one site at the origin for no points, or where the pitch steps over every site in reach); ValueError
    when it exceeds 2**28 sites.  There is no host route: without the library or a GPU this raises."""
    n, C, r, s, win, dev, p_d, lab_d, bounds = density.lattice_points('territory', check_args, points, labels, num_classes, reach_px, pitch_px, win, device)
    out = outputs(n, C, win, dev)
    cellpoints.raise_for(call(p_d, lab_d, C, r, s, win, *out, bounds=bounds, device=device), 'nuhtc_cell_territory')
    area, border, is_open, contact, class_sites, free_sites = (t.cpu().numpy() for t in out[2:])
    tallies = (area, border, is_open.astype(np.uint8), contact, class_sites, free_sites.reshape(()))
    return tallies, win, ((out[0].cpu().numpy(), out[1].cpu().numpy()) if maps else None)


def derive(area, is_open, contact, class_sites, free_sites, labels, s):
    """The float64 side of the tallies (s, the pitch, in HALF pixels; labels (n,) the rows' labels) -> dict, never a NaN:
      area_px2              float64 (n,)   area * (s / 2)**2: a site stands for a square of the pitch
      closed                uint8 (n,)     1 where open == 0 and the row owns a site: its neighbours bound the territory on every side,
                                           and area_px2 is its Voronoi area at the resolution s.  (A row that owns nothing -- it does not
                                           compete, a coincident row in front of it took every site, or the pitch steps over it -- has no
                                           territory and is not closed.)
      n_closed              int64 (C,)     the closed territories of each class
      closed_area_mean_px2, closed_area_std_px2  float64 (C,)  over them (the population standard deviation), 0 where there are none
      area_disorder         float64 (C,)   1 - 1 / (1 + std / mean), the form mst.derive uses for lengths; 0 where the mean is 0
      class_area_share      float64 (C,)   class_sites over the OWNED sites, zeros when nothing is owned
      free_share            float64 0-d    free_sites over all sites of the window
      contact_share         float64 (C, C) contact / contact.sum(), zeros when empty"""
    area, is_open = np.asarray(area, np.int64).reshape(-1), np.asarray(is_open, np.int64).reshape(-1)
    contact, class_sites, free = np.asarray(contact, np.int64), np.asarray(class_sites, np.int64).reshape(-1), int(np.asarray(free_sites).reshape(-1)[0])
    lab = np.asarray(labels, np.int64).reshape(-1)
    C = len(class_sites)
    if not (len(area) == len(is_open) == len(lab)) or contact.shape != (C, C) or (area < 0).any() or (contact < 0).any() or free < 0 or not 1 <= int(s) <= MAX_PITCH:
        raise ValueError('derive: area, open and labels are (n,), contact (C, C), class_sites (C,), nothing negative, and s is 1..2**20 half pixels')
    area_px2 = area.astype(np.float64) * (int(s) / 2.0) ** 2
    closed = (is_open == 0) & (area > 0)
    n_closed, mean, std, disorder = np.zeros(C, np.int64), np.zeros(C), np.zeros(C), np.zeros(C)
    for c in range(C):
        a = area_px2[closed & (lab == c)]
        n_closed[c] = len(a)
        if len(a):
            mean[c], std[c] = a.mean(), a.std()
            disorder[c] = 1.0 - 1.0 / (1.0 + std[c] / mean[c]) if mean[c] > 0 else 0.0
    owned, pairs = int(class_sites.sum()), int(contact.sum())
    share = class_sites / float(owned) if owned else np.zeros(C)
    return dict(area_px2=area_px2, closed=closed.astype(np.uint8), n_closed=n_closed, closed_area_mean_px2=mean, closed_area_std_px2=std,
                area_disorder=disorder, class_area_share=share.astype(np.float64), free_share=np.asarray(free / float(owned + free) if owned + free else 0.0, np.float64),
                contact_share=contact / float(pairs) if pairs else np.zeros((C, C)))


def write_npz(path, nuclei_id, xy, label, tallies, win, reach_px, pitch_px, maps=None):
    """<id>_nuclei_territory.npz, the header row i for the i-th row of <id>_nuclei_graph.npz / <id>_nuclei_feat.npz:
      nuclei_id int64 (n,), xy float64 (n, 2) (the unquantised centre in slide px), label int64 (n,)
      area, border int32 (n,), open uint8 (n,), contact int64 (C, C), class_sites int64 (C,), free_sites int64 0-d: the tallies of the
      definition, over the file's window
      the arrays of `derive` (DERIVED_KEYS)
      reach_px float64 0-d, and pitch_px, origin_px and window of density.lattice_npz
      with maps = (owner, nearest_d2): owner, nearest_d2 int32 (H, W) behind them."""
    head = cellpoints.npz_header(nuclei_id, xy, label)
    area, border, is_open, contact, class_sites, free_sites = tallies
    n = len(head['label'])
    area, border = np.ascontiguousarray(area, np.int32).reshape(-1), np.ascontiguousarray(border, np.int32).reshape(-1)
    is_open = np.ascontiguousarray(is_open, np.uint8).reshape(-1)
    contact, class_sites = np.ascontiguousarray(contact, np.int64), np.ascontiguousarray(class_sites, np.int64).reshape(-1)
    free_sites = np.asarray(free_sites, np.int64).reshape(())
    r, s = half_pixel_radius(reach_px), half_pixel_radius(pitch_px)
    win = tuple(int(v) for v in win)
    C = len(class_sites)
    check_args(C, r, s, win)
    if not (len(area) == len(border) == len(is_open) == n) or contact.shape != (C, C):
        raise ValueError('write_npz: area, border and open have one entry per nucleus, contact is (C, C)')
    if int(class_sites.sum()) + int(free_sites) != win[2] * win[3]:
        raise ValueError('write_npz: class_sites and free_sites do not sum to the window\'s W * H')
    more = {}
    if maps is not None:
        owner, nearest = (np.ascontiguousarray(m, np.int32) for m in maps)
        if owner.shape != (win[3], win[2]) or nearest.shape != owner.shape:
            raise ValueError('write_npz: the maps are not the window\'s H x W')
        more = dict(owner=owner, nearest_d2=nearest)
    d = derive(area, is_open, contact, class_sites, free_sites, head['label'], s)
    with open(path, 'wb') as f:
        np.savez(f, **head, area=area, border=border, open=is_open, contact=contact, class_sites=class_sites, free_sites=free_sites, **d,
                 reach_px=np.asarray(float(reach_px), np.float64), **density.lattice_npz(win, s, pitch_px), **more)
    return path


def read_npz(path):
    """-> dict of the arrays of a file write_npz wrote: NPZ_KEYS, and MAP_NAMES behind them when the file holds the maps."""
    with np.load(path) as z:
        return {key: z[key] for key in NPZ_KEYS + tuple(k for k in MAP_NAMES if k in z.files)}
