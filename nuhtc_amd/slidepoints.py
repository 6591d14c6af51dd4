"""The per-slide point analyses of the slide path as ONE table: which flag of tools/infer_wsi.py selects each, how its arguments become
the parameters of its module (cellgraph, spatial, clusters, mst, proximity, density, territory, adjacency, alphacomplex, outline, neighbourhoods, enrichment, regions, margin: they hold the definitions), which file it writes
beside the documents and what the closing message says of it.  cellpoints.py is what the modules share and is imported by them; this
module imports them, one at a time and only when its flag is given.

The order of ANALYSES is fixed: it is the order of the files and of the clauses of the closing message.  `select` turns the parsed
arguments into a selection, `run` works a selection off on one point set; both name no analysis.  A new analysis is a module with
check_args / build / write_npz and one row here (plus its argparse lines in the tool).

ANALYSES is the table of the analyses of the points ALONE.  An analysis with a second input -- regions.py: the points against the regions
of a GeoJSON, and margin.py: the same points by distance to the regions' boundaries -- is a row of WITH_INPUT behind it, handled by
`select` and `run` after the six: the same columns, one more that fetches the second input for a slide, or says that the slide has none
(then nothing is written for it), and two that say how the input is read and what `build` takes behind it.

AGAINST_CHANCE, between the two, holds the analyses that hold the points against a null model on the same points -- enrichment.py: the
label-permutation test.  Its rows have the columns of ANALYSES and take no second input.

OF_THE_PLANE, directly behind ANALYSES, holds the analyses that ask about the plane BETWEEN the points -- territory.py: which nucleus owns
each site of a lattice.  Its rows have the columns of ANALYSES and take no second input; their window depends on the slide, so `run`
reports a refusal of `build` (a default window above the cap) in the flag's name.

OF_THE_BORDERS, directly behind OF_THE_PLANE, holds the analyses that ask where the pieces of that plane MEET -- adjacency.py: which
territories touch, the discrete Delaunay graph.  Its rows have the columns of ANALYSES, take no second input, and share the late refusal
of OF_THE_PLANE: they build the same window.

OF_THE_CIRCLES, directly behind OF_THE_BORDERS, holds the analyses that state those borders in the continuum, by empty circles through two
points -- alphacomplex.py: the exact Delaunay edges and triangles within a radius, what adjacency.py reads off a lattice.  Its rows have
the columns of ANALYSES and take no second input and no window.

OF_THE_OUTLINES, directly behind OF_THE_CIRCLES, holds the analyses that close those circles' triangles into shapes -- outline.py: the
rings and the components of the alpha complex, written as an .npz and, beside it, as a GeoJSON of regions that a later run reads with
--nuclei-regions or --nuclei-margin.  Its rows have the columns of ANALYSES and take no second input and no window.

OF_THE_COMPANY, directly behind OF_THE_OUTLINES, holds the analyses that ask what company each of the same rows keeps --
neighbourhoods.py: the class composition of every nucleus's window of nearest neighbours, clustered into neighbourhood types.  Its rows
have the columns of ANALYSES and take no second input and no window; the centres of an earlier run, when given, are read while the
arguments are checked, and their class count is held against the model's only in `build`, so `run` reports that refusal in the flag's
name too.  `select` visits ANALYSES, OF_THE_PLANE, OF_THE_BORDERS, OF_THE_CIRCLES, OF_THE_OUTLINES, OF_THE_COMPANY, AGAINST_CHANCE and
WITH_INPUT in that order."""
import importlib
import os
from collections import namedtuple

import numpy as np

from . import cellpoints

# cli, flag, suffix   the argparse attribute, the flag as the user types it and the file beside the documents
# module   the module of nuhtc_amd that holds the definition, imported on first use (`module_of`)
# params   (module, args) -> the parameters `build` takes behind num_classes, in the units of the command line; ValueError when unusable
# check    (module, params) -> the module's check_args on them with one class (the model is not loaded yet); ValueError
# write    (module, path, (nuclei_id, xy, label), what build returned, num_classes, params, context) -> write_npz
# said     (module, what build returned, params) -> the clause of the closing message, without ' in <file>'
# second   rows of WITH_INPUT only: (module, params, slide name) -> the second input `build` takes behind num_classes, or None when the
#          slide has none; `missing` (params, slide name) -> the clause that says so; `order` (params) -> the order the module's
#          read_geojson puts the regions in; `more` (params) -> what `build` takes behind (edges, edge_region, G)
Analysis = namedtuple('Analysis', 'cli flag suffix module params check write said second missing order more', defaults=(None, None, None, None))

BY_NAMES = ('any', 'class')                   # the modules' BY, backwards
_half = cellpoints.half_pixel_radius


def module_of(an):
    return importlib.import_module('.' + an.module, __package__)


def _analysis(word, module, params, check, write, said):
    return Analysis('nuclei_' + word, '--nuclei-' + word, f'_nuclei_{word}.npz', module, params, check, write, said)


def _density_said(m, found, p):
    cnt, wgt, win = found
    peaks = m.derive(cnt, wgt, _half(p[0]))['peak_site']
    peak_px = ', '.join('none' if u < 0 else f'({(win[0] + u) * p[1]:g}, {(win[1] + v) * p[1]:g})' for u, v in peaks.tolist())
    return f'density maps of {win[2]} x {win[3]} sites ({p[0]:g} px bandwidth, {p[1]:g} px pitch; peak px per class: {peak_px})'


ANALYSES = (
    _analysis('graph', 'cellgraph',                                   # the edges to the rows
              lambda m, a: (a.graph_radius, a.graph_k),
              lambda m, p: m.check_args(1, _half(p[0]), p[1]),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, head[0], head[1], *found, head[2], *p),
              lambda m, found, p: f'{int((found[0] >= 0).sum())} edges (k {p[1]}, {p[0]:g} px)'),
    _analysis('spatial', 'spatial',                                   # pair counts over the same rows
              lambda m, a: (m.edges_from_step(a.spatial_step, a.spatial_bins),),
              lambda m, p: None,
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, p[0], *found, tiles_area_px=ctx['tiles_area_px']),
              lambda m, found, p: f'{int(found[0].sum())} ordered pairs within {p[0][-1] / 2:g} px ({len(p[0])} bins)'),
    _analysis('clusters', 'clusters',                                 # which of the same rows belong together
              lambda m, a: (a.cluster_radius, a.cluster_min, m.BY[a.cluster_by]),
              lambda m, p: m.check_args(1, _half(p[0]), p[1], p[2]),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, *found, radius_px=p[0], min_pts=p[1], by_class=p[2]),
              lambda m, found, p: (f'{len(found[3])} clusters and {int((found[0] < 0).sum())} isolated nuclei ({p[0]:g} px, {p[1]} nuclei, '
                                   f'by {BY_NAMES[p[2]]})')),
    _analysis('mst', 'mst',                                           # the shortest edges that hold the same rows together
              lambda m, a: (a.mst_radius, m.BY[a.mst_by]),
              lambda m, p: m.check_args(1, _half(p[0]), p[1]),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, *found[:3], C, radius_px=p[0], by_class=p[1]),
              lambda m, found, p: f'{found[3]} forest edges in {found[4]} trees ({p[0]:g} px, by {BY_NAMES[p[1]]})'),
    _analysis('proximity', 'proximity',                               # which of the same rows touch: the Gabriel graph and the RNG
              lambda m, a: (a.proximity_radius, m.BY[a.proximity_by]),
              lambda m, p: m.check_args(1, _half(p[0]), p[1]),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, *found[:4], C, radius_px=p[0], by_class=p[1]),
              lambda m, found, p: f'{found[4]} Gabriel edges, {found[5]} of them RNG edges ({p[0]:g} px, by {BY_NAMES[p[1]]})'),
    _analysis('density', 'density',                                   # where on the slide the same rows lie: class-wise kernel rasters
              lambda m, a: (a.density_bandwidth, a.density_pitch),
              lambda m, p: m.check_args(1, _half(p[0]), _half(p[1])),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, *found, *p),
              _density_said),
)


def _territory_said(m, found, p):
    (area, border, is_open, contact, class_sites, free_sites), win, maps = found
    closed = (is_open == 0) & (area > 0)
    px2 = area[closed] * float(p[1]) ** 2
    median = f'{float(np.median(px2)):g} px^2' if closed.any() else 'none'
    top = f'class {int(class_sites.argmax())} with {class_sites.max() / class_sites.sum():.1%} of the owned sites' if class_sites.sum() else 'nothing owned'
    return (f'territories of {int((area > 0).sum())} nuclei on {win[2]} x {win[3]} sites ({p[0]:g} px reach, {p[1]:g} px pitch; {int(closed.sum())} '
            f'closed, median area {median}; largest area share: {top})')


OF_THE_PLANE = (
    _analysis('territory', 'territory',                               # which of the same rows owns each piece of the plane: the nearest-nucleus raster
              lambda m, a: (a.territory_reach, a.territory_pitch, None, bool(a.territory_maps)),     # build's reach_px, pitch_px, win, maps
              lambda m, p: m.check_args(1, _half(p[0]), _half(p[1])),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, found[0], found[1], p[0], p[1], maps=found[2]),
              _territory_said),
)


def _adjacency_said(m, found, p):
    (edges, shared, degree), (area, border, is_open, contact, class_sites, free_sites), win = found[:3]
    closed = (is_open == 0) & (area > 0)
    mean = f'{float(degree[closed].mean()):.2f}' if closed.any() else 'none'
    return (f'{len(edges)} territory borders between {int((degree > 0).sum())} nuclei on {win[2]} x {win[3]} sites ({p[0]:g} px reach, {p[1]:g} px '
            f'pitch; {int(closed.sum())} closed territories, mean neighbours {mean})')


OF_THE_BORDERS = (
    _analysis('adjacency', 'adjacency',                               # which of the same rows' territories touch: the discrete Delaunay graph
              lambda m, a: (a.adjacency_reach, a.adjacency_pitch),    # build's reach_px, pitch_px
              lambda m, p: m.check_args(1, _half(p[0]), _half(p[1])),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, found[0], found[1], found[2], p[0], p[1]),
              _adjacency_said),
)


OF_THE_CIRCLES = (
    _analysis('alpha', 'alphacomplex',                                # which of the same rows are Delaunay neighbours within a radius: the alpha complex
              lambda m, a: (a.alpha_radius, m.BY[a.alpha_by]),
              lambda m, p: m.check_args(1, _half(p[0]), p[1]),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, *found[:5], C, radius_px=p[0], by_class=p[1]),
              lambda m, found, p: (f'{found[5]} alpha-complex edges, {found[6]} of them Gabriel edges, {int(((found[2] >= 0).sum(1) == 1).sum())} on the '
                                   f'outline ({p[0]:g} px radius, by {BY_NAMES[p[1]]})')),
)


def _outline_said(m, found, p):
    ring_area2, component, K = found[2], found[4], found[8]
    area, nuclei = np.zeros(K, np.int64), np.bincount(component[component >= 0], minlength=K)
    np.add.at(area, found[3], ring_area2)
    top = f'the largest of {area.max() / 8:g} px^2 with {int(nuclei[area.argmax()])} nuclei' if K else 'none'
    return (f'{K} alpha-shape components in {found[7]} rings, {int((ring_area2 < 0).sum())} of them holes ({p[0]:g} px radius, by {BY_NAMES[p[1]]}; '
            f'{top}; components of fewer than {p[2]} nuclei left out of the GeoJSON)')


OF_THE_OUTLINES = (
    _analysis('outline', 'outline',                                   # which shapes the same rows' triangles make: the rings and components of the alpha complex
              lambda m, a: (a.outline_radius, m.BY[a.outline_by], a.outline_min_nuclei),
              lambda m, p: m.check_args(1, _half(p[0]), p[1], p[2]),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, *found[:6], C, radius_px=p[0], by_class=p[1], min_nuclei=p[2]),
              _outline_said),
)


def _neighbourhoods_params(m, a):
    given = a.neighbourhood_centres
    centres = m.read_centres(given, k=a.neighbourhood_k, radius_px=a.neighbourhood_radius) if given else None
    types = len(centres) if given else a.neighbourhood_types               # given centres bring their own number of types
    return (a.neighbourhood_radius, a.neighbourhood_k, types, a.neighbourhood_seed, a.neighbourhood_iters, centres)


def _neighbourhoods_said(m, found, p):
    hood, centre_sum, centre_n, n_iter, converged = found[1], found[3], found[4], found[7], found[8]
    used, top = int((centre_n > 0).sum()), int(centre_n.argmax())
    how = 'assigned to given centres' if p[5] is not None else f"{n_iter} iterations, {'converged' if converged else 'not converged'}; seed {p[3]}"
    largest = (f'the largest, type {top}, holds {int(centre_n[top])} nuclei around class {int(centre_sum[top].argmax())}' if used else 'no nuclei')
    return f'{used} of {len(centre_n)} neighbourhood types in use ({how}; k {p[1]}, {p[0]:g} px); {largest}'


OF_THE_COMPANY = (
    _analysis('neighbourhoods', 'neighbourhoods',                     # what company each of the same rows keeps: k-means of the kNN windows' class counts
              _neighbourhoods_params,
              lambda m, p: m.check_args(1, _half(p[0]), *p[1:5]),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, *found, radius_px=p[0], k=p[1], seed=p[3], max_iter=p[4]),
              _neighbourhoods_said),
)


def _enrichment_said(m, found, p):
    obs, perm, cn = found
    z = m.derive(obs, perm)['z']
    a, b = divmod(int(abs(z).argmax()), len(cn))
    return (f'{int(obs.sum())} contacts within {p[0]:g} px against {p[1]} label permutations (seed {p[2]}; largest |z|: class {a} next to '
            f'class {b}, z {z[a, b]:+.2f})')


AGAINST_CHANCE = (
    _analysis('enrichment', 'enrichment',                             # whether the same rows' classes touch more often than chance
              lambda m, a: (a.enrichment_radius, a.enrichment_perms, a.enrichment_seed),
              lambda m, p: m.check_args(1, _half(p[0]), p[1], p[2]),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, *found, radius_px=p[0], seed=p[2]),
              _enrichment_said),
)


WITH_INPUT = (
    _analysis('regions', 'regions',                                   # which annotated regions hold the same rows: the census per region
              lambda m, a: (a.nuclei_regions, a.regions_order),
              lambda m, p: m.source_check(p[0]),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, *found[1], found[0], p[1]),
              lambda m, found, p: (f'{int((found[1][1] > 0).sum())} nuclei inside {len(found[0].names)} regions of {os.path.basename(found[2])} '
                                   f'({int(found[1][2].sum())} on a boundary, order {p[1]})'))
    ._replace(second=lambda m, p, name: m.source_for(p[0], name),
              missing=lambda p, name: f'no {name}.geojson in {p[0]}: no {name}_nuclei_regions.npz',
              order=lambda p: p[1], more=lambda p: ()),
    _analysis('margin', 'margin',                                     # how far from the regions' boundaries the same rows lie: the bands per region
              lambda m, a: (a.nuclei_margin, m.thresholds_from_step(a.margin_step, a.margin_bands)),
              lambda m, p: m.source_check(p[0]),
              lambda m, path, head, found, C, p, ctx: m.write_npz(path, *head, *found[1], p[1], found[0]),
              lambda m, found, p: (f'{int((found[1][2] < len(p[1])).sum())} nuclei within {p[1][-1] / 2:g} px of the boundaries of {len(found[0].names)} '
                                   f'regions of {os.path.basename(found[2])} ({len(p[1])} bands)'))
    ._replace(second=lambda m, p, name: m.source_for(p[0], name),
              missing=lambda p, name: f'no {name}.geojson in {p[0]}: no {name}_nuclei_margin.npz',
              order=lambda p: 'file', more=lambda p: (p[1],)),
)


def _build(an, m, pts, labels, num_classes, params, name, device):
    """What `run` writes from: build's results, or for a row of WITH_INPUT (the table read, build's results, the file), None without a file."""
    if an.second is None:
        return m.build(pts, labels, num_classes, *params, device=device)
    source = an.second(m, params, name)
    if source is None:
        return None
    table = m.read_geojson(source, an.order(params))
    return table, m.build(pts, labels, num_classes, table.edges, table.edge_region, len(table.names), *an.more(params), device=device), source


def select(args, need_gpu=True):
    """The parsed arguments of tools/infer_wsi.py -> the selection: ((analysis, params), ..) of the flags given, in the order of ANALYSES, OF_THE_PLANE,
    OF_THE_BORDERS, OF_THE_CIRCLES, OF_THE_OUTLINES, OF_THE_COMPANY, AGAINST_CHANCE and WITH_INPUT.
    SystemExit in the name of the flag when its arguments are unusable and then, with need_gpu, when no GPU is visible.  A flag the
    namespace does not hold is not given."""
    chosen = []
    for an in ANALYSES + OF_THE_PLANE + OF_THE_BORDERS + OF_THE_CIRCLES + OF_THE_OUTLINES + OF_THE_COMPANY + AGAINST_CHANCE + WITH_INPUT:
        if not getattr(args, an.cli, False):
            continue
        m = module_of(an)
        try:
            params = an.params(m, args)
            an.check(m, params)
        except ValueError as e:
            raise SystemExit(f'{an.flag}: {e}')
        if need_gpu:
            import torch
            if not torch.cuda.is_available():
                raise SystemExit(f'{an.flag}: no GPU is visible (there is no fallback)')
        chosen.append((an, params))
    return tuple(chosen)


def run(selection, rows, boxes, labels, num_classes, out_dir, name, device, context):
    """A selection on ONE point set: the boxes (n, 4) of the rows `rows` of the per-nucleus files, quantised once, with `labels` (n,), on
    cuda:`device`.  Every selected analysis is built and written as <out_dir>/<name><suffix>; context = dict(tiles_area_px=..) is what a
    file states beyond its own flags.  -> the clauses of the closing message, in the order of ANALYSES."""
    pts, xy = cellpoints.quantize_centres(boxes), cellpoints.centres(boxes)
    clauses = []
    for an, params in selection:
        m = module_of(an)
        try:
            found = _build(an, m, pts, labels, num_classes, params, name, device)
        except ValueError as e:
            if an not in OF_THE_PLANE + OF_THE_BORDERS + OF_THE_COMPANY:
                raise
            raise SystemExit(f'{an.flag}: {e}')
        if found is None:
            clauses.append(an.missing(params, name))
            continue
        an.write(m, os.path.join(out_dir, name + an.suffix), (rows, xy, labels), found, num_classes, params, context)
        clauses.append(f'{an.said(m, found, params)} in {name}{an.suffix}')
    return clauses
