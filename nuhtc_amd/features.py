"""Tile embeddings of a slide for slide-level models (the reference's tools/extract_features_nuhtc.py, CLAM-style bags).

Per slide: the level-0 tiles of its coordinate file (`Whole_Slide_Bag_FP`, tools/wsi_core/WholeSlideImage.py:832-898: read, RGB,
PIL `img.resize(target)` when a target size applies) -> `model_feat` (Swin-T + FPN, per-level channel means, (n, 256) float32) ->
<feat_dir>/h5_files/<id>.h5 (`features` + `coords`, save_hdf5's layout) and <feat_dir>/pt_files/<id>.pt (torch.save of the features).

On the device the batches run through a pipeline of features_only engines (nuhtc_features: backbone + FPN + the pooling kernel, no
heads); the tiles of a rank are its contiguous shard (parallel.shard_range), one gather brings every rank's rows to rank 0, which
writes them in coordinate-file order.  The features of a tile do not depend on the batch it ran in (csrc/pool.hip), so the engine
capacity (ENGINE_BATCH) and the number of ranks change no bit of the output."""
import os

import numpy as np

ENGINE_BATCH = 64          # tiles per nuhtc_features call: a --batch_size of 256 tiles is read as one host batch and run as 4 device batches


def target_size(patch_size, custom_downsample=1, target_patch_size=-1):
    """Whole_Slide_Bag_FP (:853-858): target_patch_size > 0 wins, else custom_downsample > 1 gives patch_size // custom_downsample, else
    no resize (None).  -> (w, h) or None."""
    if target_patch_size > 0:
        return (int(target_patch_size),) * 2
    if custom_downsample > 1:
        return (int(patch_size) // int(custom_downsample),) * 2
    return None


def resize_tiles(tiles, target):
    """`Image.fromarray(tile).resize(target)` per tile, Pillow's default filter for RGB as the reference calls it (:891-892)."""
    if target is None:
        return tiles
    from PIL import Image
    out = np.empty((len(tiles), target[1], target[0], 3), np.uint8)
    for k, t in enumerate(tiles):
        out[k] = np.asarray(Image.fromarray(np.ascontiguousarray(t)).resize(target))
    return out


def shard_features(model, bag, lo, hi, batch_size=256, target=None, depth=4, engine_batch=ENGINE_BATCH):
    """(hi - lo, 256) float32 embeddings of bag tiles [lo, hi): host batches of `batch_size` tiles (read, resized), run in device batches
    of at most `engine_batch` through a pipeline of `depth` features_only engines.  Channels as the reference's ndarray path (CH_SWAP)."""
    from . import hip
    n = max(0, hi - lo)
    out = np.zeros((n, 256), np.float32)
    if n == 0:
        return out
    P = bag.patch_size
    hw = (target[1], target[0]) if target is not None else (P, P)
    mb = max(1, min(int(engine_batch), int(batch_size)))
    pipe = model.feature_pipeline(hw, depth=depth, max_batch=mb)

    def collect():
        _, B, _, i0 = pipe.collect()
        out[i0:i0 + B] = pipe.last_features[:B].cpu().numpy()

    view = bag.view(lo, hi)
    for h0 in range(0, n, batch_size):
        tiles = resize_tiles(view[h0:min(n, h0 + batch_size)], target)
        for d0 in range(0, len(tiles), mb):
            if pipe.full():
                collect()
            pipe.submit(tiles[d0:d0 + mb], hip.CH_SWAP, tag=h0 + d0)
    while pipe.pending:
        collect()
    return out


def slide_features(model, bag, batch_size=256, target=None, rank=0, world=1, depth=4, device=None, feat_fn=None):
    """Embeddings of every tile of `bag` in coordinate order, on rank 0 (None on the other ranks): each rank computes its contiguous
    shard, one gather (parallel.gather_blobs) brings the rows to every rank.  `feat_fn(bag, lo, hi)` replaces the device step (tests)."""
    import torch
    from . import parallel
    lo, hi = parallel.shard_range(len(bag), rank, world)
    if feat_fn is None:
        feats = shard_features(model, bag, lo, hi, batch_size=batch_size, target=target, depth=depth)
    else:
        feats = np.asarray(feat_fn(bag, lo, hi), np.float32).reshape(-1, 256)
    dev = device if device is not None else torch.device('cpu')
    gathered = parallel.gather_blobs([torch.from_numpy(feats).to(dev), torch.tensor([lo, hi], dtype=torch.int64, device=dev)])
    if rank != 0:
        return None
    parts = sorted(((int(g[1][0]), int(g[1][1]), g[0].cpu().numpy()) for g in gathered), key=lambda t: t[0])
    pos = 0
    for a, b, f in parts:
        if a != pos or len(f) != b - a:
            raise RuntimeError(f'feature gather: rank rows [{a}, {b}) do not continue at {pos}')
        pos = b
    if pos != len(bag):
        raise RuntimeError(f'feature gather: {pos} rows for {len(bag)} tiles')
    return np.concatenate([f for _, _, f in parts], 0) if parts else np.zeros((0, 256), np.float32)


def write_slide(feat_dir, slide_id, features, coords):
    """<feat_dir>/h5_files/<id>.h5 (features + coords, save_hdf5 layout) and <feat_dir>/pt_files/<id>.pt (torch.save of the features as a
    float32 tensor), as tools/extract_features_nuhtc.py:253-272.  -> (h5 path, pt path)."""
    import torch
    from . import h5coords
    h5 = os.path.join(feat_dir, 'h5_files', slide_id + '.h5')
    pt = os.path.join(feat_dir, 'pt_files', slide_id + '.pt')
    h5coords.write_features(h5, features, coords)
    torch.save(torch.from_numpy(np.ascontiguousarray(features, np.float32)), pt)
    return h5, pt


def read_slide_list(csv_path):
    """`Dataset_All_Bags` (WholeSlideImage.py:900-909): the `slide_id` column of the CSV, as strings."""
    import csv
    with open(csv_path, newline='') as f:
        rows = list(csv.DictReader(f))
    if rows and 'slide_id' not in rows[0]:
        raise KeyError(f'{csv_path}: no slide_id column')
    return [r['slide_id'] for r in rows]
