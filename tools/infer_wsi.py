#!/usr/bin/env python
"""WSI inference with the reference's command line (tools/infer_wsi.py:309-356: same flags, same defaults) over array slides,
sharded across GPUs.

    python tools/infer_wsi.py <source> <config> <checkpoint> --patch --seg --stitch --patch_size 256 --step_size 192 \
                               --batch_size 16 --save_dir out --mode qupath [--slide_ext .npy]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 tools/infer_wsi.py ...   (one rank per GPU)

<source> is the reference's folder of slides: every file in it goes through `seg_and_patch` (nuhtc_amd/slides.py: process list
-> <save_dir>/process_list_autogen.csv, `--seg` tissue segmentation, masks/<id>.png, `--patch` tile coordinates ->
patches/<id>.npz, `--stitch` stitches/<id>.jpg; a slide whose coordinate file -- that .npz or the reference's patches/<id>.h5 -- exists is skipped unless --no_auto_skip), then every
slide of the process list that has a coordinate file and no <id>_merged.geojson yet (:445-458) is tiled, inferred and written.
A slide is a level-0 RGB array (`.npy`, memory-mapped; pass `--slide_ext .npy`) or a store directory: OpenSlide / HDF5 do not
exist offline.  Beyond the reference, <source> may be ONE slide: a `.npy` file (`--patch` is then implied: the
grid np.arange(0, size, step), or the tissue tiles with --seg, or the origins of --coords), a store directory
(nuhtc_amd.tilestore.write_store) or an `.npz` with `tiles` (N,P,P,3) + `coords` (N,2).  Every rank cuts only the tiles of its
own shard; tissue segmentation runs on rank 0.
Output (like the reference, :659-693), for every detection that survives the per-tile filter + mask-NMS:
  --mode qupath : <save_dir>/nuclei/<id>/<id>.geojson and <id>_point.geojson (flat lists of QuPath features); run
                  tools/nuclei_merge.py on the .geojson for the cross-tile merge (or pass --merge to do it here on rank 0)
  --mode dsa    : <id>_dsa.json (HistomicsUI polyline elements)
  --mode coco   : coco_nuclei.json (per-tile images + RLE annotations) and <save_dir>/imgs/<id>/<annidx>.png
  --mode sql    : <id>_dql.db (contour table + R-tree)
  --mode all    : everything.
  --det         : <save_dir>/<id>/infer/img_<x>_<y>.jpg overlays of every tile with detections (score >= --score-thr; :504-512).
  --nuclei-feat : (not in the reference) <id>_nuclei_feat.npz beside the documents: `features` float32 (n, 256), the FPN maps of a nucleus's tile
                  averaged under its mask on the GPU (nuhtc_amd/nucfeat.py), with `nuclei_id` int64, `label` and `score`; row k belongs to the
                  k-th feature of <id>.geojson and nuclei_id[k] = k -- with --merge to the k-th feature of <id>_merged.geojson, and
                  nuclei_id[k] is that nucleus's position in <id>.geojson.  The documents are the same bytes with and without the flag.
  --nuclei-graph: (not in the reference) <id>_nuclei_graph.npz beside the documents: for every row --nuclei-feat writes (every record, or the
                  merge's survivors) its --graph-k nearest nuclei within --graph-radius px, their distances and the class census of that
                  disc, built on rank 0's GPU after the gather (nuhtc_amd/cellgraph.py): `nuclei_id`, `xy` (the centres of
                  <id>_point.geojson), `neighbors` (rows of this file, -1 = none), `dist` (px, inf = none), `class_count`, `label`.  Row-aligned
                  with <id>_nuclei_feat.npz when both flags are given; every other file is the same bytes with and without the flag.
  --nuclei-spatial: (not in the reference) <id>_nuclei_spatial.npz beside the documents, for the same rows as --nuclei-graph: the counts of
                  ordered pairs of nuclei by class pair and distance bin (edges at --spatial-step px, 2 x --spatial-step, .. up to
                  --spatial-bins of them: 256 px by default) and every nucleus's distance to the nearest nucleus of each class, counted
                  on rank 0's GPU after the gather (nuhtc_amd/spatial.py): `pair_hist`, `class_n`, `nn_d2` / `nn_dist`, `edges_px`, the
                  derived `mean_within` and `G`, and `K_tiles_area` / `L_tiles_area`, Ripley's K and L under the area of the inferred
                  tiles (`tiles_area_px` = tiles x step_size^2; no edge correction, no estimate of the tissue area).  Every other file
                  is the same bytes with and without the flag.  There is no route without a GPU.
  --nuclei-clusters: (not in the reference) <id>_nuclei_clusters.npz beside the documents, for the same rows as --nuclei-graph: which
                  nuclei belong together -- DBSCAN within --cluster-radius px (32 by default) and --cluster-min nuclei (5, the nucleus itself
                  counted), over all nuclei or, with --cluster-by class, among nuclei of one label -- found on rank 0's GPU after the gather
                  (nuhtc_amd/clusters.py): per nucleus `cluster` (-1 = isolated), `core`, `degree`; per cluster `size`, `n_core`,
                  `class_count`, `sum_xy`, `bbox` (half pixels) and the derived `centroid_px`, `bbox_px`, `class_fraction`; per slide
                  `n_clusters`, `n_noise`, `class_clustered_share`.  A border nucleus joins the nearest core nucleus's cluster (ties: the
                  smaller row), so the file is a pure function of the rows.  Every other file is the same bytes with and without the flag.
                  There is no route without a GPU.
  --nuclei-mst:   (not in the reference) <id>_nuclei_mst.npz beside the documents, for the same rows as --nuclei-graph: the minimum
                  spanning forest of the nuclei over the edges of at most --mst-radius px (64 by default), over all nuclei or, with
                  --mst-by class, among nuclei of one label -- built on rank 0's GPU after the gather (nuhtc_amd/mst.py): `edges` (rows of
                  this file, i < j, ascending), `edge_d2` (half pixels squared), `tree` per nucleus, and the derived `edge_len_px`,
                  `mst_degree`, `tree_size`, `tree_length_px`, `edge_class_count`, `n_trees`, `n_edges`, `length_mean_px`,
                  `length_std_px`, `length_min_max_ratio`, `length_disorder`.  Ties are broken by (d2, i, j), so the file is a pure
                  function of the rows; cutting the forest at any length t <= radius gives the components of the t-radius graph.  Every
                  other file is the same bytes with and without the flag.  There is no route without a GPU.
  --nuclei-proximity: (not in the reference) <id>_nuclei_proximity.npz beside the documents, for the same rows as --nuclei-graph: the Gabriel
                  graph and the relative neighbourhood graph (RNG) of the nuclei, the parameter-free "who touches whom" relations, over
                  the pairs at most --proximity-radius px apart (64 by default), over all nuclei or, with --proximity-by class, among
                  nuclei of one label -- built on rank 0's GPU after the gather (nuhtc_amd/proximity.py): `edges` (the Gabriel edges, rows
                  of this file, i < j, ascending), `edge_d2` (half pixels squared), `edge_rng` (1: an RNG edge too), `degree` (n, 2), and
                  the derived `edge_len_px`, `gabriel_class_count`, `rng_class_count`, `mean_len_px`, `other_class_share`,
                  `gabriel_class_enrichment`, `n_edges`, `n_rng`.  Both graphs are unique without a tie rule, so the file is a pure
                  function of the rows.  Every other file is the same bytes with and without the flag.  There is no route without a GPU.
  --nuclei-density: (not in the reference) <id>_nuclei_density.npz beside the documents, from the same rows as --nuclei-graph: class-wise
                  density maps of the nuclei ("where on the slide": a TIL map, a cellularity map, a heat map for a viewer) on a lattice of
                  --density-pitch px (64 by default) anchored at the slide's origin, with the Epanechnikov kernel of --density-bandwidth
                  px (128 by default) -- built on rank 0's GPU after the gather (nuhtc_amd/density.py): `count` int32 and `weight` int64
                  (C, H, W), exact integers (the nuclei within the bandwidth of every site, and the sum of h^2 - d^2 over them in half
                  pixels), the derived `density_per_px2`, `share`, `class_total`, `colocalisation`, `peak_site`, and `bandwidth_px`,
                  `pitch_px`, `origin_px` (the px position of site (0, 0)), `window` (gx0, gy0, W, H in lattice units).  No tissue-area
                  normalisation and no edge correction.  Every other file is the same bytes with and without the flag.  There is no route
                  without a GPU.
  --nuclei-territory: (not in the reference) <id>_nuclei_territory.npz beside the documents, from the same rows as --nuclei-graph: which
                  nucleus, and so which class, each piece of the plane belongs to -- the nearest-nucleus raster (the Voronoi family in
                  raster form) on the lattice of --nuclei-density with a pitch of --territory-pitch px (4 by default): a site belongs to
                  the nearest nucleus within --territory-reach px (64 by default, inclusive; a tie goes to the smaller row), or to
                  nobody -- built on rank 0's GPU after the gather (nuhtc_amd/territory.py): per nucleus `area`, `border` (sites) and
                  `open` (1: the reach or the window bounds the territory, not its neighbours -- its area is no Voronoi area), `contact`
                  int64 (C, C) (the border between the territories of two classes, in site pairs), `class_sites`, `free_sites`, the
                  derived `area_px2`, `closed`, `n_closed`, `closed_area_mean_px2`, `closed_area_std_px2`, `area_disorder`,
                  `class_area_share`, `free_share`, `contact_share`, and `reach_px`, `pitch_px`, `origin_px`, `window`; with
                  --territory-maps also the two rasters `owner` and `nearest_d2` int32 (H, W).  Exact integers, a pure function of the
                  rows.  A default window above 2**28 sites is refused: coarsen the pitch.  Every other file is the same bytes with and
                  without the flag.  There is no route without a GPU.
  --nuclei-adjacency: (not in the reference) <id>_nuclei_adjacency.npz beside the documents, from the same rows as --nuclei-graph: which
                  nuclei are neighbours -- the discrete Delaunay graph: two nuclei are adjacent when their territories (the raster of
                  --nuclei-territory, here with --adjacency-reach px, 64 by default, and --adjacency-pitch px, 4 by default) touch along
                  a side of a site (4-adjacency: a diagonal meeting is none) -- built on rank 0's GPU after the gather
                  (nuhtc_amd/adjacency.py): `edges` int32 (m, 2) in ascending (i, j) order, `shared` int32 (m,) (the common border in
                  lattice steps), `degree` int32 (n,), the territory tallies the graph was read off (`area`, `border`, `open`, `contact`,
                  `class_sites`, `free_sites`; `contact` is the graph's `shared` summed by class pair), the derived `edge_d2`, `edge_px`,
                  `border_px`, `class_edge_count`, `class_border`, `neighbour_class`, `n_closed`, `closed_degree_mean`, `n_edges`, and
                  `reach_px`, `pitch_px`, `window`.  Exact integers, a pure function of the rows.  A default window above 2**28 sites is
                  refused: coarsen the pitch.  Every other file is the same bytes with and without the flag.  There is no route
                  without a GPU.
  --nuclei-alpha: (not in the reference) <id>_nuclei_alpha.npz beside the documents, for the same rows as --nuclei-graph: the alpha complex
                  of the nucleus centres -- the exact Delaunay edges within a radius, the continuous statement of what
                  --nuclei-adjacency reads off a lattice: two nuclei are joined when some circle of radius at most --alpha-radius px (32
                  by default, so the longest edge is 64 px) passes through both and has no other nucleus strictly inside, over all nuclei
                  or, with --alpha-by class, among nuclei of one label -- built on rank 0's GPU after the gather
                  (nuhtc_amd/alphacomplex.py): `edges` int32 (m, 2) in ascending (i, j) order, `edge_d2`, `apex` int32 (m, 2) (the third
                  corner of the empty circumcircle on either side, or -1), `edge_gabriel`, `degree` int32 (n, 2), the derived
                  `edge_len_px`, `voronoi_px`, `edge_kind`, `triangles`, `triangle_area_px2`, `triangle_circumradius_px`,
                  `class_edge_count`, `outline_class_count`, `on_outline`, `n_edges`, `n_gabriel`, `n_triangles`, `n_degenerate`,
                  `alpha_area_px2`, and `radius_px`, `by_class`.  Exact integers (every decision compares two rationals in int64), unique
                  without a tie rule: cocircular points keep both diagonals, and `n_degenerate` counts them.  Every other file is the
                  same bytes with and without the flag.  There is no route without a GPU.
  --nuclei-outline: (not in the reference) <id>_nuclei_outline.npz and <id>_nuclei_outline.geojson beside the documents, for the same rows
                  as --nuclei-graph: the alpha shape of the nucleus centres as polygons -- the outline edges of the alpha complex at
                  --outline-radius px (32 by default; the limits of --alpha-radius), over all nuclei or with --outline-by class among
                  nuclei of one label, linked into rings and grouped into components on rank 0's GPU after the gather
                  (nuhtc_amd/outline.py): `ring_vertex`, `ring_start`, `ring_area2` (positive: an outer ring, negative: a hole),
                  `component_of_ring`, `component` (per nucleus, -1 in no triangle), `component_label`, the derived `area_px2`,
                  `hole_area_px2`, `perimeter_px`, `n_holes`, `n_nuclei`, `class_count`, `n_components`, `n_rings`, `largest_component`,
                  `area_share_by_label`, and `radius_px`, `by_class`.  The GeoJSON holds one Polygon per component with at least
                  --outline-min-nuclei nuclei (3 by default), outer ring first, in the form --nuclei-regions and --nuclei-margin read in a
                  LATER run.  Rings that touch themselves at a pinch vertex are written as they are.  Every other file is the same bytes
                  with and without the flag.  There is no route without a GPU.
  --nuclei-neighbourhoods: (not in the reference) <id>_nuclei_neighbourhoods.npz beside the documents, from the same rows as --nuclei-graph:
                  what kind of tissue each nucleus sits in -- the cellular-neighbourhood analysis of CODEX / histoCAT / squidpy.  The class
                  counts of every nucleus's window (itself and its --neighbourhood-k nearest neighbours within --neighbourhood-radius px;
                  10 and 64 by default) are clustered by k-means into --neighbourhood-types types (8 by default; k-means++ from
                  --neighbourhood-seed, at most --neighbourhood-iters Lloyd iterations, 100 by default), all in integers on rank 0's GPU
                  after the gather (nuhtc_amd/neighbourhoods.py), so the file is a pure function of the rows IN THEIR ORDER: `window`
                  int32 (n, C), `hood` (the type of each nucleus), `centre_q` (fixed point, 1024 = one nucleus), `centre_sum`, `centre_n`,
                  `seed_rows`, `inertia`, `n_iter`, `converged`, the derived `composition`, `fraction`, `enrichment_log2`,
                  `hood_class_count`, `hood_size`, `order_by_size`, `inertia_per_nucleus`, and `radius_px`, `k`, `types`, `seed`,
                  `max_iter`, `centres_given`.  --neighbourhood-centres FILE.npz assigns against the centres of an earlier run's file
                  without fitting (its k, radius and class count must be this run's; its number of types is taken): types defined on
                  one slide, applied to a cohort.  No radius windows, no choice of K, no restarts.  Every other file is the same bytes
                  with and without the flag.  There is no route without a GPU.
  --nuclei-enrichment: (not in the reference) <id>_nuclei_enrichment.npz beside the documents, from the same rows as --nuclei-graph: whether
                  nuclei of one class lie next to nuclei of another more often than chance -- the neighbourhood-enrichment permutation
                  test (histoCAT, squidpy's nhood_enrichment).  The contacts (ordered pairs at most --enrichment-radius px apart, 64 by
                  default) are counted by class pair under the observed labels and under --enrichment-perms shuffles of the labels over
                  the same positions (1000 by default; the generator is a function of the row count, --enrichment-seed and the shuffle's
                  number, so the file is a pure function of the rows IN THEIR ORDER), on rank 0's GPU after the gather
                  (nuhtc_amd/enrichment.py): `observed` int64 (C, C), `perm_counts` int64 (P, C, C), `class_n`, the derived `mean`, `std`,
                  `z`, `p_enriched`, `p_depleted`, and `radius_px`, `perms`, `seed`.  No area and no edge correction are needed: the null
                  model lives on the same points.  Every other file is the same bytes with and without the flag.  There is no route
                  without a GPU.
  --nuclei-regions PATH: (not in the reference) <id>_nuclei_regions.npz beside the documents, from the same rows as --nuclei-graph: which
                  annotated regions hold each nucleus, and the nuclei of each class inside every region.  PATH is a GeoJSON of Polygon and
                  MultiPolygon features (QuPath annotations, a tissue outline) used for every slide, or a directory holding
                  <slide_id>.geojson; a slide without a file gets no output and a clause saying so.  Even-odd and half-open in exact
                  integers on half pixels, built on rank 0's GPU after the gather (nuhtc_amd/regions.py): `region` (the largest index
                  holding the nucleus, -1: none; with --regions-order area the features are sorted by descending area, so that is the
                  innermost), `depth`, `on_boundary`, `census` int64 (G, C), the derived `area_px2`, `density_per_px2`, `class_fraction`,
                  `n_inside`, `n_outside`, `class_share_inside`, and the regions themselves: `names`, `ring_start`, `edges`, `edge_region`,
                  `area2`, `order`.  The area is the one the file states (shoelace; not verified).  Every other file is the same bytes
                  with and without the flag.  There is no route without a GPU.
  --nuclei-margin PATH: (not in the reference) <id>_nuclei_margin.npz beside the documents, from the same rows as --nuclei-graph: the nuclei
                  of each class by distance to the boundary of every region, inside it and outside it -- the invasive-margin profile
                  ("distance to annotation" in bands).  PATH as for --nuclei-regions (a GeoJSON for every slide, or a directory of
                  <slide_id>.geojson; a slide without a file gets no output and a clause saying so), the regions in file order.  The bands
                  are --margin-bands steps of --margin-step px (10 of 50 by default: 0-50, 50-100, ..; step x bands <= 8192 px).  "Is the
                  distance at most e" is decided in exact integers on half pixels, inclusive, on rank 0's GPU after the gather
                  (nuhtc_amd/margin.py): `band_census` int64 (G, 2, B, C) [region][0 outside / 1 inside][band][class], `census` int64
                  (G, C) (the nuclei inside, as --nuclei-regions counts them), per nucleus `band` (the nearest band over all regions, B:
                  none), `band_region`, `band_inside`, `thresholds`, the derived `band_edges_px`, `inside_beyond`, `profile`,
                  `class_fraction`, `n_near`, and the regions themselves: `names`, `ring_start`, `edges`, `edge_region`, `area2`.  No
                  per-nucleus distance value and no density per band (a band's area is no integer statement).  Every other file is the
                  same bytes with and without the flag.  There is no route without a GPU.
  --nuclei-morph: (the reference's tools/wsi_feat_extract.py table, computed on the GPU) <id>_nuclei_morph.npz beside the documents, for the
                  same rows: `columns` and `values` float64 (n, F) -- size, shape, orientation, position and haematoxylin-intensity features
                  under histomicstk's names, derived on the host (nuhtc_amd/nucmorph.py derive) from the integers every rank's GPU measured
                  under the final mask (`raw` int64 (n, 16), `hist` int32 (n, 256), `origin`) -- with `nuclei_id`, `label`, `score`.
                  Row-aligned with <id>_nuclei_feat.npz and <id>_nuclei_graph.npz; every other file is the same bytes with and without the
                  flag.  There is no route without a GPU.
  --nuclei-texture: (the 26 Haralick columns of the same table) <id>_nuclei_texture.npz beside the documents, for the same rows: `columns`
                  and `values` float64 (n, 26) -- Haralick.<feature>.Mean / .Range over the offsets (0, 1) and (1, 0), derived on the host
                  (nuhtc_amd/nuctex.py derive) from the grey-level co-occurrence counts every rank's GPU took under the final mask (`glcm`
                  int32 (n, 2, 136): 16 levels of the haematoxylin value, the upper triangle) -- with `nuclei_id`, `label`, `score`.
                  Row-aligned with the other per-nucleus files; every other file is the same bytes with and without the flag.  There is no
                  route without a GPU."""
import argparse
import os
import sys

# 16 hardware queues instead of the HIP runtime's 4 (read when the runtime initialises; an exported value wins): see tools/bench_wsi.py
os.environ.setdefault('GPU_MAX_HW_QUEUES', '16')

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    """The reference's parser (tools/infer_wsi.py:309-356), flag for flag and default for default (pinned by
    tests/test_cli_parity.py against a table read off the reference), plus this build's own flags at the end.
    allow_abbrev=False: with abbreviations `--patch` would be taken for a prefix of `--patch_size`."""
    p = argparse.ArgumentParser(allow_abbrev=False)
    p.add_argument('source', help='path to folder containing raw wsi image files (or one array slide / tile store)')
    p.add_argument('config', help='Config file')
    p.add_argument('checkpoint', help='Checkpoint file')
    p.add_argument('--device', default='cuda:0', help='Device used for inference')
    p.add_argument('--score-thr', type=float, default=0.35, help='score threshold')
    p.add_argument('--async-test', action='store_true', help='whether to set async options for async inference.')
    p.add_argument('--step_size', type=int, default=256, help='step_size')
    p.add_argument('--patch_size', type=int, default=256, help='patch_size')
    p.add_argument('--patch', default=False, action='store_true')
    p.add_argument('--seg', default=False, action='store_true')
    p.add_argument('--stitch', default=False, action='store_true')
    p.add_argument('--no_auto_skip', default=False, action='store_true')
    p.add_argument('--save_dir', type=str, help='directory to save processed data')
    p.add_argument('--preset', default=None, type=str, help='predefined profile of default segmentation and filter parameters (.csv)')
    p.add_argument('--patch_level', type=int, default=0, help='downsample level at which to patch')
    p.add_argument('--mag', '--magnification', type=int, default=40, help='magnification for the slide', dest='mag')
    p.add_argument('--batch_size', type=int, default=32, help='batch size of image dataset during inference')
    p.add_argument('--num_workers', type=int, default=8, help='number workers of image dataset during inference')
    p.add_argument('--margin', type=int, default=0, help='discard the contour which distance is less than margin number pixels to edges')
    p.add_argument('--min_area', type=int, default=10, help='discard the area less than min_area')
    p.add_argument('--process_list', type=str, default=None, help='name of list of images to process with parameters (.csv)')
    p.add_argument('--slide_ext', type=str, default='.svs', help='ext name of wsi')
    p.add_argument('--mode', type=str, default='qupath', help='mode of save format')
    p.add_argument('--det', default=False, action='store_true')
    # ---- not in the reference
    p.add_argument('--seg_downsample', type=int, default=64, help='downsample of the (virtual) pyramid level seg_level / vis_level -1 resolve to (reference: the level nearest 64x)')
    p.add_argument('--coords', default=None, help="coordinate file of a single .npy slide: .npy (N,2), .npz with `coords` [+ `patch_size`], or the reference's own patches/<id>.h5")
    p.add_argument('--gpus', type=int, default=1, help='one rank per GPU: the tool starts itself N times under torch.distributed.run (a child process) unless a launcher already did')
    p.add_argument('--merge', action='store_true', help='also run the cross-tile merge (tools/nuclei_merge.py) on rank 0 -> <id>_merged.geojson')
    p.add_argument('--overlap_threshold', type=float, default=0.05)
    p.add_argument('--seg-on', choices=('host', 'gpu'), default='host', dest='seg_on',
                   help="where --seg / --patch compute the tissue mask and select the tiles: 'host' (numpy / scipy) or 'gpu' (rank 0's own device; same files)")
    p.add_argument('--rle-on', choices=('host', 'gpu'), default='host', dest='rle_on',
                   help="where --mode coco / all encode the run-length masks: 'host' (numpy + a Python loop per nucleus) or 'gpu' (every rank's own device; same files)")
    p.add_argument('--nuclei-feat', action='store_true', dest='nuclei_feat',
                   help='also write <id>_nuclei_feat.npz: the 256-d embedding of every written nucleus (FPN maps averaged under its mask on the GPU), keyed by nuclei_id')
    p.add_argument('--nuclei-morph', action='store_true', dest='nuclei_morph',
                   help='also write <id>_nuclei_morph.npz: size, shape and haematoxylin-intensity features of every written nucleus, from integers '
                        'measured under its mask on the GPU (rows as in <id>_nuclei_feat.npz)')
    p.add_argument('--nuclei-texture', action='store_true', dest='nuclei_texture',
                   help='also write <id>_nuclei_texture.npz: the 26 Haralick texture features of every written nucleus, from grey-level co-occurrence '
                        'counts taken under its mask on the GPU (rows as in <id>_nuclei_feat.npz)')
    p.add_argument('--nuclei-graph', action='store_true', dest='nuclei_graph',
                   help='also write <id>_nuclei_graph.npz: the --graph-k nearest nuclei of every written nucleus within --graph-radius, their distances and '
                        'the class counts around it, built on the GPU (rows as in <id>_nuclei_feat.npz)')
    p.add_argument('--graph-radius', type=float, default=64.0, dest='graph_radius',
                   help='radius of --nuclei-graph in slide px, a multiple of 0.5 up to 8192 (default 64 px: 16 um at 40x)')
    p.add_argument('--graph-k', type=int, default=8, dest='graph_k', help='neighbours kept per nucleus by --nuclei-graph, 1..32 (default 8)')
    p.add_argument('--nuclei-spatial', action='store_true', dest='nuclei_spatial',
                   help='also write <id>_nuclei_spatial.npz: pair counts by class pair and distance bin and the nearest nucleus of every class for every '
                        'written nucleus, counted on the GPU (rows as in <id>_nuclei_feat.npz)')
    p.add_argument('--spatial-step', type=float, default=8.0, dest='spatial_step',
                   help='width of a distance bin of --nuclei-spatial in slide px, a multiple of 0.5 (default 8 px)')
    p.add_argument('--spatial-bins', type=int, default=32, dest='spatial_bins',
                   help='distance bins of --nuclei-spatial, 1..32; the reach is step x bins <= 8192 px (default 32: 256 px, 64 um at 40x)')
    p.add_argument('--nuclei-clusters', action='store_true', dest='nuclei_clusters',
                   help='also write <id>_nuclei_clusters.npz: the DBSCAN cluster of every written nucleus (-1: isolated) and the size, class counts, '
                        'centroid and box of every cluster, found on the GPU (rows as in <id>_nuclei_feat.npz)')
    p.add_argument('--cluster-radius', type=float, default=32.0, dest='cluster_radius',
                   help='radius of --nuclei-clusters in slide px, a multiple of 0.5 up to 8192 (default 32 px: 8 um at 40x)')
    p.add_argument('--cluster-min', type=int, default=5, dest='cluster_min',
                   help='nuclei within the radius, the nucleus itself counted, that make a core nucleus of --nuclei-clusters (default 5)')
    p.add_argument('--cluster-by', choices=('any', 'class'), default='any', dest='cluster_by',
                   help="--nuclei-clusters over all nuclei ('any') or only among nuclei of the same label ('class')")
    p.add_argument('--nuclei-mst', action='store_true', dest='nuclei_mst',
                   help='also write <id>_nuclei_mst.npz: the minimum spanning forest of the written nuclei (edges, their lengths, the tree of every '
                        'nucleus and the edge-length statistics), built on the GPU (rows as in <id>_nuclei_feat.npz)')
    p.add_argument('--mst-radius', type=float, default=64.0, dest='mst_radius',
                   help='longest edge of --nuclei-mst in slide px, a multiple of 0.5 up to 8192 (default 64 px: 16 um at 40x)')
    p.add_argument('--mst-by', choices=('any', 'class'), default='any', dest='mst_by',
                   help="--nuclei-mst over all nuclei ('any') or only among nuclei of the same label ('class')")
    p.add_argument('--nuclei-proximity', action='store_true', dest='nuclei_proximity',
                   help='also write <id>_nuclei_proximity.npz: the Gabriel graph and the relative neighbourhood graph of the written nuclei (edges, '
                        'their lengths, the degrees, which classes touch), built on the GPU; rows as in --nuclei-graph')
    p.add_argument('--proximity-radius', type=float, default=64.0, dest='proximity_radius',
                   help='longest edge of --nuclei-proximity in slide px, a multiple of 0.5 up to 8192 (default 64 px: 16 um at 40x)')
    p.add_argument('--proximity-by', choices=('any', 'class'), default='any', dest='proximity_by',
                   help="--nuclei-proximity over all nuclei ('any') or only among nuclei of the same label ('class')")
    p.add_argument('--nuclei-density', action='store_true', dest='nuclei_density',
                   help='also write <id>_nuclei_density.npz: class-wise density maps of the written nuclei on a lattice anchored at the slide origin '
                        '(counts and Epanechnikov weights per site, exact integers), built on the GPU; from the rows of --nuclei-graph')
    p.add_argument('--density-bandwidth', type=float, default=128.0, dest='density_bandwidth',
                   help='kernel radius of --nuclei-density in slide px, a multiple of 0.5 up to 8192 (default 128 px: 32 um at 40x)')
    p.add_argument('--density-pitch', type=float, default=64.0, dest='density_pitch',
                   help='distance between the sites of --nuclei-density in slide px, a multiple of 0.5 (default 64 px)')
    p.add_argument('--nuclei-territory', action='store_true', dest='nuclei_territory',
                   help='also write <id>_nuclei_territory.npz: which written nucleus owns each site of a lattice anchored at the slide origin (the '
                        'nearest-nucleus raster: territory areas, borders and class contacts, exact integers), built on the GPU; from the rows of --nuclei-graph')
    p.add_argument('--territory-reach', type=float, default=64.0, dest='territory_reach',
                   help='farthest a site of --nuclei-territory may lie from its nucleus in slide px, a multiple of 0.5 up to 8192 (default 64 px: 16 um at 40x)')
    p.add_argument('--territory-pitch', type=float, default=4.0, dest='territory_pitch',
                   help='distance between the sites of --nuclei-territory in slide px, a multiple of 0.5 (default 4 px)')
    p.add_argument('--territory-maps', action='store_true', dest='territory_maps',
                   help='--nuclei-territory also stores the rasters `owner` and `nearest_d2` (one int32 per site each)')
    p.add_argument('--nuclei-adjacency', action='store_true', dest='nuclei_adjacency',
                   help='also write <id>_nuclei_adjacency.npz: which written nuclei are neighbours (the discrete Delaunay graph: their territories touch '
                        'on the lattice; edges, shared border lengths and degrees, exact integers), built on the GPU; from the rows of --nuclei-graph')
    p.add_argument('--adjacency-reach', type=float, default=64.0, dest='adjacency_reach',
                   help='the reach of the territories of --nuclei-adjacency in slide px, a multiple of 0.5 up to 8192 (default 64 px)')
    p.add_argument('--adjacency-pitch', type=float, default=4.0, dest='adjacency_pitch',
                   help='distance between the sites of --nuclei-adjacency in slide px, a multiple of 0.5 (default 4 px)')
    p.add_argument('--nuclei-alpha', action='store_true', dest='nuclei_alpha',
                   help='also write <id>_nuclei_alpha.npz: the alpha complex of the written nuclei (the exact Delaunay edges and triangles within a '
                        'radius: edges, apexes, Gabriel flags and degrees, exact integers), built on the GPU; from the rows of --nuclei-graph')
    p.add_argument('--alpha-radius', type=float, default=32.0, dest='alpha_radius',
                   help='largest empty circle of --nuclei-alpha in slide px, a multiple of 0.5 up to 256 (default 32 px: the longest edge is 64 px)')
    p.add_argument('--alpha-by', choices=('any', 'class'), default='any', dest='alpha_by',
                   help="--nuclei-alpha over all nuclei ('any') or only among nuclei of the same label ('class')")
    p.add_argument('--nuclei-outline', action='store_true', dest='nuclei_outline',
                   help='also write <id>_nuclei_outline.npz and <id>_nuclei_outline.geojson: the alpha shape of the written nuclei as polygons (the rings and '
                        'components of the alpha complex, exact integers; the GeoJSON is what --nuclei-regions / --nuclei-margin read), traced on the GPU; '
                        'from the rows of --nuclei-graph')
    p.add_argument('--outline-radius', type=float, default=32.0, dest='outline_radius',
                   help='largest empty circle of --nuclei-outline in slide px, a multiple of 0.5 up to 256 (default 32 px)')
    p.add_argument('--outline-by', choices=('any', 'class'), default='any', dest='outline_by',
                   help="--nuclei-outline over all nuclei ('any') or only among nuclei of the same label ('class')")
    p.add_argument('--outline-min-nuclei', type=int, default=3, dest='outline_min_nuclei',
                   help='components of --nuclei-outline with fewer nuclei are left out of the GeoJSON (default 3; the .npz holds them all)')
    p.add_argument('--nuclei-neighbourhoods', action='store_true', dest='nuclei_neighbourhoods',
                   help='also write <id>_nuclei_neighbourhoods.npz: the class counts of every written nucleus\'s window of nearest neighbours, clustered '
                        'by integer k-means into neighbourhood types (the cellular-neighbourhood analysis), on the GPU; from the rows of --nuclei-graph')
    p.add_argument('--neighbourhood-k', type=int, default=10, dest='neighbourhood_k',
                   help='neighbours in the window of --nuclei-neighbourhoods beside the nucleus itself, 1..32 (default 10)')
    p.add_argument('--neighbourhood-radius', type=float, default=64.0, dest='neighbourhood_radius',
                   help='radius of that window in slide px, a multiple of 0.5 up to 8192 (default 64 px: 16 um at 40x)')
    p.add_argument('--neighbourhood-types', type=int, default=8, dest='neighbourhood_types',
                   help='neighbourhood types K of --nuclei-neighbourhoods, 1..32 (default 8)')
    p.add_argument('--neighbourhood-seed', type=int, default=0, dest='neighbourhood_seed',
                   help='seed of the k-means++ seeding of --nuclei-neighbourhoods, 0..2**32-1 (default 0)')
    p.add_argument('--neighbourhood-iters', type=int, default=100, dest='neighbourhood_iters',
                   help='most Lloyd iterations of --nuclei-neighbourhoods, 1..1000 (default 100)')
    p.add_argument('--neighbourhood-centres', default=None, dest='neighbourhood_centres', metavar='FILE.npz',
                   help='assign against the centres of an earlier <id>_nuclei_neighbourhoods.npz instead of fitting (same k, radius and classes)')
    p.add_argument('--nuclei-enrichment', action='store_true', dest='nuclei_enrichment',
                   help='also write <id>_nuclei_enrichment.npz: the contacts of the written nuclei by class pair, observed and under label permutations, '
                        'with z-scores and empirical p-values (the neighbourhood-enrichment test), counted on the GPU; from the rows of --nuclei-graph')
    p.add_argument('--enrichment-radius', type=float, default=64.0, dest='enrichment_radius',
                   help='contact radius of --nuclei-enrichment in slide px, a multiple of 0.5 up to 8192 (default 64 px: 16 um at 40x)')
    p.add_argument('--enrichment-perms', type=int, default=1000, dest='enrichment_perms',
                   help='label permutations of --nuclei-enrichment, 1..1024 (default 1000)')
    p.add_argument('--enrichment-seed', type=int, default=0, dest='enrichment_seed',
                   help='seed of the permutations of --nuclei-enrichment, 0..2**32-1 (default 0)')
    p.add_argument('--nuclei-regions', default=None, dest='nuclei_regions', metavar='PATH',
                   help='also write <id>_nuclei_regions.npz: which regions of a GeoJSON (one file for every slide, or a directory of <slide_id>.geojson) '
                        'hold each written nucleus and the nuclei per class inside every region, exact, built on the GPU; from the rows of --nuclei-graph')
    p.add_argument('--regions-order', choices=('file', 'area'), default='file', dest='regions_order',
                   help="the regions of --nuclei-regions in file order ('file') or by descending area, so that a nucleus's region is the innermost ('area')")
    p.add_argument('--nuclei-margin', default=None, dest='nuclei_margin', metavar='PATH',
                   help='also write <id>_nuclei_margin.npz: the written nuclei per class by distance band to the boundary of every region of a GeoJSON '
                        '(PATH as for --nuclei-regions), inside and outside it, exact, built on the GPU; from the rows of --nuclei-graph')
    p.add_argument('--margin-step', type=float, default=50.0, dest='margin_step',
                   help='width of a band of --nuclei-margin in slide px, a multiple of 0.5 (default 50 px)')
    p.add_argument('--margin-bands', type=int, default=10, dest='margin_bands',
                   help='bands of --nuclei-margin on either side of a boundary, 1..32, step x bands at most 8192 px (default 10)')
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def run_slide(args, model, bag, slide_id, rank, local_rank, world):
    """The reference's per-slide loop (:460-693): tiles -> detections -> per-tile filter + mask-NMS -> records -> the one gather ->
    rank 0 writes the documents.  The tile list is sharded in contiguous blocks over the ranks."""
    import torch
    from nuhtc_amd import contours, nuclei, parallel, slidepoints, wsi
    coords = bag.coords
    lo, hi = parallel.shard_range(len(bag), rank, world)
    tiles = bag.view(lo, hi)                                  # this rank's tiles only, cut / decoded a batch at a time while earlier batches run
    want = lambda m: args.mode in (m, 'all')
    rle_gpu = want('coco') and args.rle_on == 'gpu'                  # strings and boxes come off the device with the records (nuhtc_rle_encode)
    sel = nuclei.select(**{k.keyword: getattr(args, k.cli, False) for k in nuclei.KINDS})     # the per-nucleus tables asked for
    rec = wsi.infer_tiles(model, tiles, coords[lo:hi], args.batch_size, rle=rle_gpu, **nuclei.keywords(sel))
    # contours are traced on the rank that owns the tile; two variable-length gathers: records, then ring vertices
    rings = rec['ring']                                              # traced on the GPU (nuhtc_mask_contours)
    keep = [i for i, r in enumerate(rings) if len(r) >= 3]          # reference :536 tests the CLOSED contour (mask2inst appends the first point): only one-pixel contours go
    P = bag.patch_size
    rles = []
    if rle_gpu:
        rles = rec['rle']
    elif want('coco'):                                               # RLE of the instance inside its tile (:611-613)
        from nuhtc_amd import cocomask
        for i in keep:
            crop, x0, y0 = rec['mask'][i]
            ox, oy = (int(v) for v in coords[lo + rec['tile'][i]])
            full = np.zeros((P, P), np.uint8)
            full[y0 - oy:y0 - oy + crop.shape[0], x0 - ox:x0 - ox + crop.shape[1]] = crop
            rles.append(cocomask.encode(full)['counts'].encode('ascii'))
    if args.det:                                                      # :504-512, per tile with detections; a second pass through the API (debug output)
        from nuhtc_amd.apis import inference_detector, save_result
        det_dir = os.path.join(args.save_dir, slide_id, 'infer')
        os.makedirs(det_dir, exist_ok=True)
        for i0 in range(0, len(tiles), args.batch_size):
            batch = [t for t in tiles[i0:i0 + args.batch_size]]
            for k, res in enumerate(inference_detector(model, batch)):
                if sum(len(b) for b in res[0]):
                    x, y = (int(v) for v in coords[lo + i0 + k])
                    save_result(model, batch[k], res, score_thr=args.score_thr, out_file=os.path.join(det_dir, f'img_{x}_{y}.jpg'))
    # the one exchange of the path: every rank's records (head, ring vertices, mask crops, RLE strings) in a single all-gather
    dev = torch.device('cuda', local_rank) if world > 1 and torch.cuda.is_available() else torch.device('cpu')
    parts = wsi.pack_records(rec, keep, tile_base=lo, rles=rles)
    parts, row_parts = parts[:5], parts[5:]                          # one part per selected kind: they travel behind the documents' parts
    if want('qupath'):
        # every rank writes the GeoJSON text of ITS records (the reference's one Python loop over all nuclei, :533-585 + json.dump :659-664,
        # is seconds per slide on the writing rank); the bytes travel in the same gather and rank 0 only concatenates
        h0, v0 = parts[0].numpy(), parts[1].numpy()
        lab = h0[:, 5].astype(np.int32)
        ptxt, pstart = contours.ring_features_text(v0, h0[:, 6].astype(np.int64), lab, h0[:, 4], model.CLASSES)
        parts += [torch.from_numpy(ptxt), torch.from_numpy(pstart), torch.from_numpy(contours.point_features_text(h0[:, :4], lab, h0[:, 4], model.CLASSES))]
    rows_at = len(parts)                                              # the rows of this rank's records, kind by kind: more parts of the same gather
    parts += row_parts
    if rle_gpu:                                                       # bbox / area of the annotations: rank 0 parses no string
        kp = np.asarray(keep, np.int64)
        parts.append(torch.from_numpy(np.ascontiguousarray(rec['rle_bbox'][kp], np.int32)))
        parts.append(torch.tensor([rec['rle_host']], dtype=torch.int32))
    parts.append(torch.tensor([rank], dtype=torch.int32))           # who sent it (printed by rank 0)
    gathered = parallel.gather_blobs([t.to(dev) for t in parts])
    heads = [g[0] for g in gathered]
    vparts = [g[1] for g in gathered]
    bparts = [g[4] if want('coco') else None for g in gathered]
    xparts = [g[-3].cpu().numpy() if rle_gpu else None for g in gathered]
    if rank != 0:
        return
    if rle_gpu:
        print(f'--rle-on gpu: {int(sum(int(g[-2][0]) for g in gathered))} of {int(sum(len(g[0]) for g in gathered))} run-length masks fell back to the host encoder',
              file=sys.stderr)
    if want('coco'):
        from nuhtc_amd import cocomask
    from nuhtc_amd import outputs
    name = slide_id
    out_dir = os.path.join(args.save_dir, 'nuclei', name)
    os.makedirs(out_dir, exist_ok=True)
    dsa, annts, per_tile = [], [], {}
    sql = outputs.SqlContourWriter(os.path.join(out_dir, name + '_dql.db')) if want('sql') else None
    n_records = int(sum(len(h) for h in heads))
    feat_rows = None                                                  # rows of <id>_nuclei_feat.npz: every record, or the merge's survivors
    for h, v, bl, xb in zip(heads, vparts, bparts, xparts):
        if not (want('dsa') or want('coco') or sql):       # the per-record loop serves the other document kinds only
            break
        h, v = h.cpu().numpy(), v.cpu().numpy()
        bl = bl.cpu().numpy().tobytes() if bl is not None else b''
        off = boff = 0
        for r, row in enumerate(h):
            nv, annidx, nb = int(row[6]), int(row[7]), int(row[8])
            ring = v[off:off + nv].astype(np.int64)
            off += nv
            label, score = int(row[5]), float(row[4])
            elementidx = len(per_tile.setdefault(annidx, []))
            per_tile[annidx].append(label)
            if want('dsa'):
                dsa.append(outputs.dsa_element(ring, label, model.CLASSES))
            if want('coco'):
                rle = {'size': [P, P], 'counts': bl[boff:boff + nb].decode('ascii')}
                boff += nb
                bbox = [float(c) for c in xb[r]] if xb is not None else cocomask.to_bbox(rle)
                annts.append({'bbox': bbox, 'area': bbox[2] * bbox[3], 'image_id': annidx, 'category_id': label, 'id': len(annts),
                              'iscrowd': 0, 'segmentation': rle})
            if sql:
                sql.add(annidx, elementidx, ring, label, score, model.CLASSES)
    msg = f'{len(bag)} tiles on {world} rank(s): {n_records} nuclei after per-tile mask-NMS'
    if world > 1:
        msg += f' (records of ranks {sorted(int(g[-1][0]) for g in gathered)}, tiles per rank {[parallel.shard_range(len(bag), r, world)[1] - parallel.shard_range(len(bag), r, world)[0] for r in range(world)]})'
    if want('qupath'):
        body, start = contours.concat_feature_texts([g[5].cpu().numpy() for g in gathered], [g[6].cpu().numpy() for g in gathered])
        outputs.write_text_list(os.path.join(out_dir, name + '.geojson'), body)
        outputs.write_text_list(os.path.join(out_dir, name + '_point.geojson'), contours.concat_feature_texts([g[7].cpu().numpy() for g in gathered])[0])
        if args.merge:
            kept = wsi.merge_gathered(gathered, args.overlap_threshold, device=local_rank if world > 1 else (torch.device(args.device).index or 0))
            outputs.write_text_list(os.path.join(out_dir, name + '_merged.geojson'), contours.join_features_text(body, start, kept))
            msg += f', {len(kept)} after the cross-tile merge'
            feat_rows = np.asarray(kept, np.int64)
    points = slidepoints.select(args)                                 # the per-slide point analyses asked for
    if sel or points:                                                 # the rows of the per-nucleus files, and their labels and scores
        hall = np.concatenate([h.cpu().numpy() for h in heads], 0).reshape(-1, 9)
        rows = np.arange(n_records, dtype=np.int64) if feat_rows is None else feat_rows
    for i, kind in enumerate(sel):
        kind.write(os.path.join(out_dir, name + kind.suffix), rows, wsi.gathered_rows(kind, gathered, rows, part=rows_at + i),
                   hall[rows, 5].astype(np.int64), hall[rows, 4])
        msg += f', {len(rows)} {kind.said} in {name}{kind.suffix}'
    if points:                                                        # one point set for all of them: only what the gather already delivered
        said = slidepoints.run(points, rows, hall[rows, :4], hall[rows, 5].astype(np.int64), len(model.CLASSES), out_dir, name,
                               local_rank if world > 1 else (torch.device(args.device).index or 0),
                               dict(tiles_area_px=float(len(bag)) * float(args.step_size) ** 2))
        msg += ''.join(', ' + clause for clause in said)
    if want('dsa'):
        outputs.write_json(os.path.join(out_dir, name + '_dsa.json'), outputs.dsa_document(dsa))
    if want('coco'):
        from PIL import Image
        img_dir = os.path.join(args.save_dir, 'imgs', name)
        os.makedirs(img_dir, exist_ok=True)
        imgs = []
        for annidx in sorted(per_tile):
            imgs.append(outputs.coco_tile_image(annidx, P, P, per_tile[annidx], model.CLASSES))
            Image.fromarray(bag[annidx][0]).save(os.path.join(img_dir, f'{annidx}.png'))
        outputs.write_json(os.path.join(out_dir, 'coco_nuclei.json'),
                           {'images': imgs, 'annotations': annts, 'categories': outputs.coco_categories(model.CLASSES)})
    if sql:
        sql.close()
    print(msg)


def main(argv=None):
    args = parse_args(argv)
    if args.save_dir is None:
        raise SystemExit('--save_dir is required (the reference joins it with "patches" / "masks" / "stitches" at once, :360-362)')
    if args.mode not in ('qupath', 'dsa', 'coco', 'sql', 'all'):
        raise SystemExit(f'--mode {args.mode}: one of qupath, dsa, coco, sql, all')
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:      # no launcher: become one (before anything here touches the GPU)
        from nuhtc_amd import parallel
        raise SystemExit(parallel.self_launch(args.gpus, __file__, sys.argv[1:] if argv is None else argv))
    import torch
    from nuhtc_amd import parallel, slidepoints, slides, tilestore
    from nuhtc_amd.apis import init_detector
    if args.seg_on == 'gpu' and not torch.cuda.is_available():
        raise SystemExit('--seg-on gpu: no GPU is visible (there is no fallback; --seg-on host is the host route)')
    if args.rle_on == 'gpu' and args.mode in ('coco', 'all'):
        if not torch.cuda.is_available():
            raise SystemExit('--rle-on gpu: no GPU is visible (there is no fallback; --rle-on host is the host route)')
        if args.patch_size % 32:
            raise SystemExit(f'--rle-on gpu: --patch_size {args.patch_size} is not a multiple of 32 (the device encodes bit-packed rows of 32 pixels; use --rle-on host)')
    if args.nuclei_morph and not torch.cuda.is_available():
        raise SystemExit('--nuclei-morph: no GPU is visible (there is no fallback)')
    if args.nuclei_texture and not torch.cuda.is_available():
        raise SystemExit('--nuclei-texture: no GPU is visible (there is no fallback)')
    slidepoints.select(args)                                  # the per-slide point analyses: their arguments, then a GPU
    # the process group is formed AFTER seg_and_patch: rank 0's host phase (segmentation, masks, patching, stitching of every slide of the
    # folder) has no time bound, and a rank waiting in an RCCL barrier is aborted by the watchdog after 10 minutes
    rank, local_rank, world = parallel.env_ranks()
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f'--gpus {args.gpus} but WORLD_SIZE={world}')
    say = print if rank == 0 else (lambda *a, **k: None)
    if args.async_test:
        say('--async-test: accepted; the reference never reads it in this tool either')
    say(f'--num_workers {args.num_workers}: accepted; tiles are cut from memory-mapped arrays by the rank that owns them (no DataLoader workers)')
    patch_save_dir = os.path.join(args.save_dir, 'patches')
    mask_save_dir = os.path.join(args.save_dir, 'masks')
    stitch_save_dir = os.path.join(args.save_dir, 'stitches')
    process_list = os.path.join(args.save_dir, args.process_list) if args.process_list else None
    directories = {'source': args.source, 'save_dir': args.save_dir, 'patch_save_dir': patch_save_dir, 'mask_save_dir': mask_save_dir,
                   'stitch_save_dir': stitch_save_dir}
    src = os.path.normpath(args.source)
    is_store = os.path.isdir(src) and os.path.isfile(os.path.join(src, 'slide.npy')) and os.path.isfile(os.path.join(src, 'coords.npy'))
    single = is_store or os.path.isfile(src)                  # beyond the reference: ONE slide instead of a folder
    if rank == 0:
        for key, val in directories.items():
            print('{} : {}'.format(key, val))
            if key not in ['source']:
                os.makedirs(val, exist_ok=True)
    seg_params, filter_params, vis_params, patch_params = slides.default_parameters(args.preset)
    say({'seg_params': seg_params, 'filter_params': filter_params, 'patch_params': patch_params, 'vis_params': vis_params})
    from nuhtc_amd.config import Config, set_test_scale_factor
    cfg = Config.fromfile(args.config)
    sf = set_test_scale_factor(cfg, args.mag)          # reference :416-419: scale_factor = 80 / mag
    say('scale_factor: ', sf)
    # this tool owns its process: the submitting thread goes onto the GPU's NUMA node (NUHTC_HOST_AFFINITY=0 leaves it alone)
    model = init_detector(cfg, args.checkpoint, device=f'cuda:{local_rank}' if world > 1 else args.device, max_batch=args.batch_size,
                          bind_host=os.environ.get('NUHTC_HOST_AFFINITY', '1') != '0')
    model.CLASSES = ('T', 'I', 'C', 'D', 'E')[:model.opts['num_classes']]
    model.opts.update(margin=args.margin, min_area=args.min_area, mask_nms_thr=0.05)

    # ---- seg_and_patch on rank 0 (:430-435), everybody else waits for the process list and the coordinate files
    jobs = []                                                 # (slide_id, bag factory)
    if single and (is_store or src.endswith('.npz')):         # the tiles / coordinates come with the source: nothing to segment or patch
        slide_id = os.path.splitext(os.path.basename(src))[0]
        jobs.append((slide_id, lambda: tilestore.open_source(src, args.patch_size, args.step_size)))
    else:
        folder, names, ext = (os.path.dirname(src) or '.', [os.path.basename(src)], os.path.splitext(src)[1]) if single else (src, None, args.slide_ext)
        if rank == 0:
            if single and args.coords is not None:            # explicit origins: they ARE the coordinate file
                c, ps = tilestore._load_coords(args.coords)
                sid = os.path.splitext(names[0])[0]
                slides.save_coords(slides.coords_path(patch_save_dir, sid), c, ps or args.patch_size, 0, sid)
            slides.seg_and_patch(folder, args.save_dir, patch_save_dir, mask_save_dir, stitch_save_dir, seg_params=seg_params,
                                 filter_params=filter_params, vis_params=vis_params, patch_params=patch_params,
                                 patch_size=args.patch_size, step_size=args.step_size, seg=args.seg, use_default_params=False,
                                 save_mask=True, stitch=args.stitch, patch_level=args.patch_level, patch=args.patch or single,
                                 process_list=process_list, no_auto_skip=args.no_auto_skip or (single and args.coords is None),
                                 slides=names, seg_downsample=args.seg_downsample, seg_on=args.seg_on,
                                 device=local_rank if world > 1 else (torch.device(args.device).index or 0))
        parallel.host_phase_done(args.save_dir, rank, world)      # the other ranks poll a marker file (no collective, no timeout)
        for entry in slides.slide_list(args.save_dir):        # Dataset_All_Bags over process_list_autogen.csv (:437-439)
            slide_id = entry.split(ext)[0] if ext else entry
            if not slides.has_coords(patch_save_dir, slide_id):     # patches/<id>.npz, or the reference's own patches/<id>.h5
                say(f'\nskip {slide_id} due to no coord file')
                continue
            spath = os.path.join(folder, entry)                # the list holds file names; the reference rebuilds them as slide_id + slide_ext (:452)
            if not os.path.exists(spath):
                spath = os.path.join(folder, slide_id + ext)

            def make(spath=spath, slide_id=slide_id):
                c, ps, lvl = slides.load_coords(patch_save_dir, slide_id)
                if lvl != 0:                                   # (a reference-made .h5 can carry another level; tiles are cut from level 0 here)
                    raise SystemExit(f'{slide_id}: coordinate file was made for patch_level {lvl}; only patch_level 0 is supported')
                return tilestore.TileBag(slides.open_array_slide(spath), c, ps)
            jobs.append((slide_id, make))
    parallel.init_from_env()
    total = len(jobs)
    for k, (slide_id, make) in enumerate(jobs):
        say('\nprogress: {}/{}'.format(k, total))
        say(slide_id)
        # a slide that already has its merged file is done (:456-458); in single-slide mode the run is the request: always redone
        if not single and os.path.exists(os.path.join(args.save_dir, 'nuclei', slide_id, f'{slide_id}_merged.geojson')):
            say(f'skip {slide_id} due to existing results')
            continue
        run_slide(args, model, make(), slide_id, rank, local_rank, world)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()                                        # every rank is past the marker
        parallel.host_phase_cleanup(args.save_dir, rank, world)


if __name__ == '__main__':
    main()
