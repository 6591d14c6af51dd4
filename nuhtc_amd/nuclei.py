"""The per-nucleus measurements of the slide path as ONE table: what the engine exports per kept detection (csrc/nucfeat.hip,
nucmorph.hip, nuctex.hip; nuhtc_amd.nucfeat, .nucmorph, .nuctex define the values), how a batch's fields become the rows that travel
with the records (nuhtc_amd.wsi) and which file tools/infer_wsi.py writes from them.

The order of KINDS is fixed: it is the order of the export blob's fields, of the launches behind nuhtc_export_kept and of the parts
pack_records appends behind the five document parts.  Engine.export_async, EnginePipeline.submit and wsi.infer_tiles turn their
keywords into a selection (`select`) at entry; everything below iterates that selection and names no kind."""
from collections import namedtuple

import numpy as np

from . import nucfeat, nucmorph, nuctex
from .nucmorph import stain_constants            # the table and coefficients of the kinds that read tile pixels (Engine._morph_constants)

# keyword   the argument of export_async / submit / infer_tiles
# fields    the export-blob fields: (name, shape behind the capacity, dtype); Engine.export_read returns them under these names
# call      the C entry that fills them from the list nuhtc_export_kept wrote; reads_tiles: it takes the tiles of the last inference
# key       the record key of the rows; dtype, width: one travelling row
# rows      (the fields of some detections, their tile origins (n, 2) or (2,)) -> the travelling rows
# cli, suffix, write, said   tools/infer_wsi.py: the argparse attribute, the file beside the documents, write(path, nuclei_id, rows, label,
#           score) and what the closing message says it holds
Kind = namedtuple('Kind', 'keyword fields call reads_tiles key dtype width rows cli suffix write said')


def _write_morph(path, nuclei_id, rows, label, score):
    raw, hist, origin = nucmorph.unpack_rows(rows)
    return nucmorph.write_npz(path, nuclei_id, raw, hist, label, score, origin)


FEAT = Kind('nucfeat', (('feat', (256,), 'float32'),), 'nuhtc_nucleus_features', False, 'feat', np.float32, nucfeat.DIM,
            lambda f, origin: f[0], 'nuclei_feat', '_nuclei_feat.npz', nucfeat.write_npz, 'embeddings')
MORPH = Kind('nucmorph', (('morph_raw', (16,), 'int64'), ('morph_hist', (256,), 'int32')), 'nuhtc_nucleus_morph', True, 'morph', np.int64, nucmorph.ROW,
             lambda f, origin: nucmorph.pack_rows(f[0], f[1], origin), 'nuclei_morph', '_nuclei_morph.npz', _write_morph,
             f'rows of {len(nucmorph.COLUMNS)} features')
TEX = Kind('nuctex', (('tex', (2, 136), 'int32'),), 'nuhtc_nucleus_texture', True, 'tex', np.int64, nuctex.ROW,
           lambda f, origin: nuctex.pack_rows(f[0]), 'nuclei_texture', '_nuclei_texture.npz',
           lambda path, nuclei_id, rows, label, score: nuctex.write_npz(path, nuclei_id, nuctex.unpack_rows(rows), label, score),
           f'rows of {len(nuctex.COLUMNS)} features')
KINDS = (FEAT, MORPH, TEX)


def select(**keywords):
    """nucfeat= / nucmorph= / nuctex= -> the selected kinds, in the order of KINDS."""
    return tuple(k for k in KINDS if keywords.get(k.keyword))


def keywords(sel):
    """A selection -> the keyword arguments that select it."""
    return {k.keyword: True for k in sel}


def carried(rec):
    """The kinds whose rows a record dict (or one batch's part of it) carries, in the order of KINDS."""
    return tuple(k for k in KINDS if k.key in rec)
