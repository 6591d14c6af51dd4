#!/usr/bin/env python
"""Tile feature extraction with the reference's command line (tools/extract_features_nuhtc.py:180-209: same flags, same defaults), on
the MI355X, sharded across GPUs.

    python tools/extract_features_nuhtc.py --config <config> --checkpoint <ckpt> --data_h5_dir <dir> --data_slide_dir <dir> \
        --slide_ext .npy --csv_path <list.csv> --feat_dir <out> [--batch_size 256] [--target_patch_size 224 | --custom_downsample 2] [--gpus N]

For every `slide_id` of the CSV (Dataset_All_Bags): the tiles at the origins of <data_h5_dir>/patches/<id>.h5 (the reference's coordinate
file; its .npz twin is read as well) are cut from <data_slide_dir>/<id><slide_ext> -- a level-0 array slide (`.npy`) or a tiled TIFF / SVS
(nuhtc_amd.slides.open_array_slide; OpenSlide does not exist here) --, resized with Pillow when a target size applies, and embedded by
`model_feat` (Swin-T + FPN, channel means of the four levels: (n, 256) float32).  Output as the reference's:
  <feat_dir>/h5_files/<id>.h5   datasets `features` (n, 256) float32 and `coords` (n, 2) int64, chunks (1, ...), maxshape (None, ...)
  <feat_dir>/pt_files/<id>.pt   torch.save of the features
A slide whose .pt exists when the run starts is skipped unless --no_auto_skip.  The config's test scale factor is used as it stands
(the reference has no --mag here).  Coordinate files made for a patch level other than 0 are rejected, as tools/infer_wsi.py does.

Stated deviations:
  --stain_norm  is refused.  The reference passes `stain_norm=` to a Whole_Slide_Bag_FP that has no such parameter, so as committed every
                slide fails there with a TypeError that its `try` reduces to "ERROR: <id>.h5"; nothing in it defines what the
                normalisation would be.  This tool does what the reference evidently intends without the flag: no stain normalisation.
  --gpus N      one rank per GPU (contiguous shards of the tiles, one gather to rank 0, which writes the files in coordinate order) instead
                of nn.DataParallel; the rows do not depend on the number of ranks or on --batch_size (csrc/pool.hip).
  --batch_size  is the host batch (tiles read and resized together); the device runs it in batches of at most 64 tiles
                (nuhtc_amd.features.ENGINE_BATCH) on a pipeline of four features-only engines."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    """The reference's parser (tools/extract_features_nuhtc.py:180-209) flag for flag and default for default (pinned by
    tests/test_features_host.py against a table read off the reference), plus --gpus.  allow_abbrev=False as the other tools."""
    p = argparse.ArgumentParser(description='Feature Extraction', allow_abbrev=False)
    p.add_argument('--config', type=str, default=None, help='Config file')
    p.add_argument('--checkpoint', type=str, default=None, help='Checkpoint file')
    p.add_argument('--data_h5_dir', type=str, default=None)
    p.add_argument('--data_slide_dir', type=str, default=None)
    p.add_argument('--slide_ext', type=str, default='.svs')
    p.add_argument('--csv_path', type=str, default=None)
    p.add_argument('--feat_dir', type=str, default=None)
    p.add_argument('--batch_size', type=int, default=256)
    p.add_argument('--no_auto_skip', default=False, action='store_true')
    p.add_argument('--stain_norm', default=False, action='store_true')
    p.add_argument('--custom_downsample', type=int, default=1)
    p.add_argument('--target_patch_size', type=int, default=-1)
    # ---- not in the reference
    p.add_argument('--gpus', type=int, default=1, help='one rank per GPU: the tool starts itself N times under torch.distributed.run (a child process) unless a launcher already did')
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


STAIN_NORM_REFUSED = ('--stain_norm is not supported: the reference passes it to a Whole_Slide_Bag_FP that has no such parameter (every slide '
                      'then fails with a TypeError) and defines no stain normalisation; run without it (no stain normalisation)')


def check_args(args):
    """Argument errors the run cannot start with (SystemExit with a message)."""
    if args.stain_norm:
        raise SystemExit(STAIN_NORM_REFUSED)
    if args.csv_path is None:
        raise SystemExit('CSV path must be provided (--csv_path)')
    for k in ('config', 'data_h5_dir', 'data_slide_dir', 'feat_dir'):
        if getattr(args, k) is None:
            raise SystemExit(f'--{k} is required')
    if args.batch_size < 1:
        raise SystemExit('--batch_size must be positive')


def run(args, model=None, rank=0, local_rank=0, world=1, feat_fn=None, log=print):
    """The slide loop (:224-276).  `model`: a Detector (built from --config / --checkpoint when None); `feat_fn(bag, lo, hi)` replaces the
    device step (host tests).  -> list of (slide_id, status) with status 'done', 'skipped' or 'error'."""
    from nuhtc_amd import features, slides
    say = log if rank == 0 else (lambda *a, **k: None)
    slide_ids = features.read_slide_list(args.csv_path)
    pt_dir = os.path.join(args.feat_dir, 'pt_files')
    if rank == 0:
        os.makedirs(args.feat_dir, exist_ok=True)
        os.makedirs(pt_dir, exist_ok=True)
        os.makedirs(os.path.join(args.feat_dir, 'h5_files'), exist_ok=True)
    dest_files = os.listdir(pt_dir) if os.path.isdir(pt_dir) else []          # listed once, before the loop (:231)
    dev = None
    if world > 1:
        import torch
        if torch.cuda.is_available() and os.environ.get('NUHTC_DIST_BACKEND', 'nccl') != 'gloo':
            dev = torch.device('cuda', local_rank)
    done = []
    for k, entry in enumerate(slide_ids):
        slide_id = entry.split(args.slide_ext)[0]
        say('\nprogress: {}/{}'.format(k, len(slide_ids)))
        say(slide_id)
        if not args.no_auto_skip and slide_id + '.pt' in dest_files:
            say('skipped {}'.format(slide_id))
            done.append((slide_id, 'skipped'))
            continue
        t0 = time.time()
        # host side first, the same on every rank (a slide that cannot be opened is skipped by all of them before any collective)
        try:
            coords, patch_size, level = slides.load_coords(os.path.join(args.data_h5_dir, 'patches'), slide_id)
            if level != 0:
                raise SystemExit(f'{slide_id}: coordinate file was made for patch_level {level}; only patch_level 0 is supported')
            from nuhtc_amd import tilestore
            bag = tilestore.TileBag(slides.open_array_slide(os.path.join(args.data_slide_dir, slide_id + args.slide_ext)), coords, patch_size)
        except (OSError, KeyError, ValueError) as e:
            say('ERROR:', slide_id + '.h5')
            say(f'Exception: {e}')
            done.append((slide_id, 'error'))
            continue
        target = features.target_size(patch_size, args.custom_downsample, args.target_patch_size)
        say(f'patch_size {patch_size}, patch_level {level}, {len(bag)} tiles; target patch size: {target}')
        feats = features.slide_features(model, bag, batch_size=args.batch_size, target=target, rank=rank, world=world, device=dev, feat_fn=feat_fn)
        if rank == 0:
            h5, pt = features.write_slide(args.feat_dir, slide_id, feats, bag.coords)
            say('\ncomputing features for {} took {} s'.format(h5, time.time() - t0))
            say('features size: ', feats.shape)
            say('coordinates size: ', bag.coords.shape)
        done.append((slide_id, 'done'))
    return done


def main(argv=None):
    args = parse_args(argv)
    check_args(args)
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:      # no launcher: become one (before anything here touches the GPU)
        from nuhtc_amd import parallel
        raise SystemExit(parallel.self_launch(args.gpus, __file__, sys.argv[1:] if argv is None else argv))
    from nuhtc_amd import parallel
    from nuhtc_amd.apis import init_detector
    from nuhtc_amd.config import Config
    rank, local_rank, world = parallel.env_ranks()
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f'--gpus {args.gpus} but WORLD_SIZE={world}')
    cfg = Config.fromfile(args.config)
    model = init_detector(cfg, args.checkpoint, device=f'cuda:{local_rank}', max_batch=min(args.batch_size, 64),
                          bind_host=os.environ.get('NUHTC_HOST_AFFINITY', '1') != '0')
    parallel.init_from_env()
    run(args, model, rank, local_rank, world)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()


if __name__ == '__main__':
    main()
