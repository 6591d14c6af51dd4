"""Host-side driver of one libnuhtc_hip engine (one per GPU / process).

Plays the role of the reference's `HybridTaskCascade_Cus` module object (nuhtc/models/htc_cus.py): holds the
weights on the device and turns a batch of uint8 tiles into `(bbox_results, segm_results)` per tile, in the
exact format `inference_detector` returns (mmdet/apis/inference.py:90-153).  torch is used for
device buffers and the current stream only; every computation happens inside the HIP library.
"""
import ctypes
import os
import sys

import numpy as np
import torch

from . import hip, nuclei, ringfeat


class HipError(RuntimeError):
    pass


class _DevView:
    """Zero-copy view of a raw device pointer for torch.as_tensor (CUDA array interface v2)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(int(s) for s in shape), typestr=typestr, data=(int(ptr), False),
                                             version=2, strides=None)


_TYPESTR = {0: '<f4', 1: '<i4', 2: '|u1', 3: '<u4'}
_TORCH = {0: torch.float32, 1: torch.int32, 2: torch.uint8, 3: torch.int32}


class Engine:
    EXPORT_BUFFERS = 3          # pinned host buffers of export_async: batches per pipeline slot (2) + 1, see export_async

    _bound = {}                 # thread id -> number of live engines that placed that thread (the last one to close restores its mask)
    _logged = False

    def __init__(self, state_dict, device=0, max_batch=16, tile=(256, 256), num_classes=5, bind_host=None, **cfg_overrides):
        if not torch.cuda.is_available():
            raise HipError('no HIP device visible: nuhtc_amd has no CPU path (the CPU oracle lives under oracle/ and is test-only)')
        self.lib = hip.load()
        self.device = torch.device('cuda', device if isinstance(device, int) else torch.device(device).index or 0)
        cfg = hip.default_config()
        cfg.num_classes = num_classes
        # `tile` is the image size (h, w), any size: the buffers the library sees are (h, w rounded up to a multiple of 32: bit-packed
        # mask rows) with the image in the top-left corner; like the reference's test pipeline the library resizes the image, pads the
        # network input to a multiple of 32 and clips boxes / pastes masks with the un-padded sizes (nuhtc_config.valid_h / valid_w)
        self.image_hw = (int(tile[0]), int(tile[1]))
        cfg.tile_h, cfg.tile_w = self.image_hw[0], -(-self.image_hw[1] // 32) * 32
        cfg.valid_h, cfg.valid_w = self.image_hw
        cfg.max_batch = int(max_batch)
        for k, v in cfg_overrides.items():
            if not hasattr(cfg, k):
                raise KeyError(f'unknown engine option {k}')
            if k == 'stage_stds':
                for i in range(3):
                    for j in range(4):
                        cfg.stage_stds[i][j] = float(v[i][j])
            elif k in ('mean', 'std'):
                for i in range(3):
                    getattr(cfg, k)[i] = float(v[i])
            else:
                setattr(cfg, k, v)
        self.cfg = cfg
        # The submitting thread belongs on the GPU's NUMA node (hip.bind_host_thread) -- before the first queue
        # exists.  Opt-in (bind_host=True, or NUHTC_HOST_AFFINITY=1 when the argument is None): narrowing the caller's CPU mask is
        # the caller's decision; close() gives the mask back when the last engine that placed this thread goes.
        self._placed_thread = None
        if bind_host is None:
            bind_host = os.environ.get('NUHTC_HOST_AFFINITY', '0') == '1'
        if bind_host:
            import threading
            try:
                before = os.sched_getaffinity(0)
                if hip.bind_host_thread(self.device.index):
                    tid = threading.get_ident()
                    Engine._bound[tid] = Engine._bound.get(tid, 0) + 1
                    self._placed_thread = tid
                    now = os.sched_getaffinity(0)
                    if not Engine._logged and now != before:
                        Engine._logged = True
                        print(f'nuhtc_amd: the submitting thread now runs on {len(now)} of its {len(before)} CPUs, the NUMA node of GPU {self.device.index} '
                              '(bind_host=True / NUHTC_HOST_AFFINITY=1; the mask is restored when the engine is closed)', file=sys.stderr)
                else:
                    import warnings
                    warnings.warn(f'nuhtc_amd: bind_host requested but the submitting thread was not placed: {hip.bind_reason}')
            except RuntimeError:          # placement is an optimisation: a device the runtime cannot name is reported by nuhtc_create below
                pass
        self.h = ctypes.c_void_p()
        rc = self.lib.nuhtc_create(ctypes.byref(cfg), self.device.index, ctypes.byref(self.h))
        if rc:
            raise HipError(f'nuhtc_create failed ({rc}): {self.lib.nuhtc_last_error(None).decode()}')
        from .weights import schema
        names = schema(num_classes)
        for name, t in state_dict.items():
            if name not in names:      # buffers / EMA / optimizer entries: not part of the path (the library rejects them)
                continue
            a = np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)
            if a.ndim == 0:
                a = a.reshape(1)
            shape = (ctypes.c_int64 * a.ndim)(*a.shape)
            self._check(self.lib.nuhtc_load_weight(self.h, name.encode(), a.ctypes.data_as(ctypes.c_void_p), shape, a.ndim))
        self._check(self.lib.nuhtc_finalize(self.h))
        # a stream of the engine's own (nuhtc_stream): EnginePipeline runs the engine on it; any other stream works as well
        self.stream = torch.cuda.ExternalStream(self.lib.nuhtc_stream(self.h), device=self.device)
        B, K = cfg.max_batch, cfg.max_per_img
        self.features_only = bool(cfg.features_only)
        if self.features_only:         # (nuhtc_features only: no detection buffers; nuhtc_infer refuses the engine before it reads `dets`)
            with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
                self.feat = torch.zeros(B, 256, dtype=torch.float32, device=self.device)
            self.stream.synchronize()
            self.dets = hip.Dets()
            return
        # allocated and zero-filled ON the engine's stream (hipStreamNonBlocking: nothing would order memsets of the caller's stream
        # before the first batch there), so the blocks also live in the allocator pool of the stream they are used on
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            self.feat = torch.zeros(B, 256, dtype=torch.float32, device=self.device)
            self.boxes = torch.zeros(B, K, 5, dtype=torch.float32, device=self.device)
            self.labels = torch.zeros(B, K, dtype=torch.int32, device=self.device)
            self.counts = torch.zeros(B, dtype=torch.int32, device=self.device)
            self.masks = torch.zeros(B, K, cfg.tile_h, cfg.tile_w // 32, dtype=torch.int32, device=self.device)
            self.areas = torch.zeros(B, K, dtype=torch.int32, device=self.device)
            self.keep = torch.zeros(B, K, dtype=torch.uint8, device=self.device)
        self.stream.synchronize()       # creation is synchronous anyway (nuhtc_finalize): the zero fills are complete whatever stream the caller uses
        self.dets = hip.Dets(self.boxes.data_ptr(), self.labels.data_ptr(), self.counts.data_ptr(), self.masks.data_ptr(),
                             self.areas.data_ptr(), self.keep.data_ptr())

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc:
            if not self.h:
                raise HipError('this engine was closed (Engine.close(), or evicted from the Detector cache of max_engines sizes): '
                               'ask the Detector for the engine again instead of keeping it')
            raise HipError(f'libnuhtc_hip error {rc}: {self.lib.nuhtc_last_error(self.h).decode()}')

    def close(self):
        if getattr(self, 'h', None) and self.h.value:
            self.lib.nuhtc_destroy(self.h)
            self.h = ctypes.c_void_p()
        tid = getattr(self, '_placed_thread', None)
        if tid is not None:
            self._placed_thread = None
            import threading
            Engine._bound[tid] = Engine._bound.get(tid, 1) - 1
            if Engine._bound[tid] <= 0:
                Engine._bound.pop(tid, None)
                if threading.get_ident() == tid:          # only the placed thread itself can take its mask back
                    hip.restore_host_thread()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def to_device(self, tiles):
        """(B,H,W,3) uint8 ndarray / tensor -> contiguous device tensor."""
        if isinstance(tiles, np.ndarray):
            tiles = torch.from_numpy(np.ascontiguousarray(tiles))
        if tiles.dtype != torch.uint8 or tiles.dim() != 4 or tiles.shape[-1] != 3:
            raise ValueError('tiles must be uint8 (B,H,W,3)')
        if tuple(tiles.shape[1:3]) != self.image_hw:
            raise ValueError(f'tile size {tuple(tiles.shape[1:3])} != engine tile size {self.image_hw}')
        tiles = tiles.to(self.device, non_blocking=True)
        if self.cfg.tile_w != self.image_hw[1]:          # row pitch of the library's buffers: width rounded up to 32 (content ignored)
            tiles = torch.nn.functional.pad(tiles, (0, 0, 0, self.cfg.tile_w - self.image_hw[1]))
        return tiles.contiguous()

    # ------------------------------------------------------------------ hot path
    def infer_async(self, tiles_dev, channel_mode=hip.CH_AS_IS):
        """Enqueue the whole path for a device-resident batch; outputs land in self.boxes/labels/counts/masks/keep."""
        B = tiles_dev.shape[0]
        self._last_tiles = tiles_dev          # (kept alive until the next call: buffer('img') is computed from them on request)
        self._morph_src = (tiles_dev, channel_mode)     # what nuhtc_nucleus_morph / nuhtc_nucleus_texture read: set by the inferences only, tiles and mode together
        self._check(self.lib.nuhtc_infer(self.h, ctypes.c_void_p(tiles_dev.data_ptr()), B, channel_mode, self._stream(),
                                         ctypes.byref(self.dets)))
        return B

    def features_async(self, tiles_dev, channel_mode=hip.CH_AS_IS, out=None):
        """Enqueue backbone + FPN + the per-level channel means (nuhtc_features) for a device-resident batch; the (B, 256) float32
        embeddings land in self.feat[:B], or in `out` (a contiguous (B, 256) float32 device tensor).  Returns B."""
        B = tiles_dev.shape[0]
        dst = self.feat if out is None else out
        if dst.dtype != torch.float32 or not dst.is_contiguous() or dst.shape[0] < B or tuple(dst.shape[1:]) != (256,) or dst.device != self.device:
            raise ValueError('features_async: out must be a contiguous float32 (B, 256) tensor on the engine\'s device')
        self._last_tiles = tiles_dev
        self._check(self.lib.nuhtc_features(self.h, ctypes.c_void_p(tiles_dev.data_ptr()), B, channel_mode, self._stream(),
                                            ctypes.c_void_p(dst.data_ptr())))
        return B

    def features(self, tiles, channel_mode=hip.CH_AS_IS):
        """(N, H, W, 3) uint8 tiles (host or device) -> (N, 256) float32 ndarray: per tile the channel means of the FPN levels 0..3
        over the padded grid (the reference's `model_feat`), max_batch tiles per call."""
        t = self.to_device(tiles)
        out = torch.empty(t.shape[0], 256, dtype=torch.float32, device=self.device)
        for i in range(0, t.shape[0], self.cfg.max_batch):
            self.features_async(t[i:i + self.cfg.max_batch], channel_mode, out=out[i:i + self.cfg.max_batch])
        return out.cpu().numpy()

    def infer_fixed_load_async(self, tiles_dev, rois_dev, n_dets, channel_mode=hip.CH_AS_IS):
        B, n_rois = tiles_dev.shape[0], rois_dev.shape[1]
        self._last_tiles = tiles_dev
        self._morph_src = (tiles_dev, channel_mode)     # what nuhtc_nucleus_morph / nuhtc_nucleus_texture read: set by the inferences only, tiles and mode together
        self._check(self.lib.nuhtc_infer_fixed_load(self.h, ctypes.c_void_p(tiles_dev.data_ptr()), B, channel_mode,
                                                    ctypes.c_void_p(rois_dev.data_ptr()), n_rois, n_dets, self._stream(),
                                                    ctypes.byref(self.dets)))
        return B

    def check(self):
        self._check(self.lib.nuhtc_check(self.h, self._stream()))

    def contours_async(self, B, cap=256, kept_only=True):
        """Enqueue the outer-contour trace (cv2.findContours(...)[0][0] of tools/infer_wsi.py:51-54) of the last infer's
        masks on the device; results in self.contour_xy (B,K,cap,2) int16 / self.contour_n (B,K) int32."""
        K = self.cfg.max_per_img
        if getattr(self, 'contour_xy', None) is None or self.contour_xy.shape[2] != cap:
            self.contour_xy = torch.zeros(self.cfg.max_batch, K, cap, 2, dtype=torch.int16, device=self.device)
            self.contour_n = torch.zeros(self.cfg.max_batch, K, dtype=torch.int32, device=self.device)
        dets = self.dets if kept_only else hip.Dets(self.boxes.data_ptr(), self.labels.data_ptr(), self.counts.data_ptr(),
                                                    self.masks.data_ptr(), self.areas.data_ptr(), None)
        self._check(self.lib.nuhtc_mask_contours(self.h, ctypes.byref(dets), B, cap, ctypes.c_void_p(self.contour_xy.data_ptr()),
                                                 ctypes.c_void_p(self.contour_n.data_ptr()), self._stream()))

    def contours(self, B, cap=256, kept_only=True):
        """-> per tile, dict slot -> (n,2) int64 open contour in tile pixels.  Contours that overflow the device
        capacities are traced by the host mirror (nuhtc_amd.contours) from the mask."""
        from . import contours as host
        self.contours_async(B, cap, kept_only)
        n = self.contour_n[:B].cpu().numpy()
        out = []
        for b in range(B):
            d = {}
            slots = np.nonzero(n[b])[0]
            if len(slots):
                xy = self.contour_xy[b, torch.from_numpy(slots).to(self.device)].cpu().numpy()
                for k, sl in enumerate(slots):
                    if n[b, sl] > 0:
                        d[int(sl)] = xy[k, :n[b, sl]].astype(np.int64)
                    else:
                        words = self.masks[b, sl].cpu().numpy().view(np.uint32)
                        bits = np.unpackbits(words.view(np.uint8).reshape(self.cfg.tile_h, self.cfg.tile_w // 8), axis=-1, bitorder='little')
                        d[int(sl)] = host.trace_outer_contour(bits.astype(bool))
            out.append(d)
        return out

    def rle_encode(self, words, H, W, run_cap=1024, n=None, pool_cap=None, out=None):
        """COCO run-length strings and boxes of bit-packed masks on the device (nuhtc_rle_encode: cocomask.encode(m)['counts'] and
        cocomask.to_bbox, byte for byte).  words: contiguous int32 device tensor (n_max, H * W // 32), rows of W // 32 words, pixel x in
        bit x & 31 of word x >> 5.  n: None (all n_max masks) or an int32 device tensor whose first element is the number of masks (read on
        the device).  pool_cap: bytes of the string pool (default: what run_cap allows per mask, at most 5 characters per count).
        out: (len, off, bytes, bbox) device tensors to write into (int32 (n_max,), int32 (n_max + 1,), uint8 (>= pool_cap,), int32
        (n_max, 4)); fresh zero-filled ones otherwise.
        -> (len, off, bytes, bbox): len[i] bytes of string i or -1 (more than run_cap runs: encode that one on the host), off the
        exclusive scan of max(len, 0) with the total in off[n], string i = bytes[off[i]:off[i] + len[i]] where it ends inside the pool,
        bbox[i] = x, y, w, h.  Synchronous."""
        if words.device != self.device or words.dtype != torch.int32 or not words.is_contiguous() or words.dim() != 2 or words.shape[1] * 32 != H * W:
            raise ValueError('rle_encode: words must be a contiguous int32 (n, H * W // 32) tensor on the engine\'s device')
        n_max = int(words.shape[0])
        if pool_cap is None:
            pool_cap = max(1, n_max) * 5 * min(int(run_cap), H * W + 1) if out is None else int(out[2].numel())
        if out is None:
            out = (torch.zeros(n_max, dtype=torch.int32, device=self.device), torch.zeros(n_max + 1, dtype=torch.int32, device=self.device),
                   torch.zeros(max(1, int(pool_cap)), dtype=torch.uint8, device=self.device), torch.zeros(n_max, 4, dtype=torch.int32, device=self.device))
        ln, off, data, bbox = out
        if ln.numel() < n_max or off.numel() < n_max + 1 or data.numel() < pool_cap or bbox.numel() < 4 * n_max:
            raise ValueError('rle_encode: an output tensor is smaller than the call needs')
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = self.lib.nuhtc_rle_encode(self.device.index, vp(words), vp(n) if n is not None else None, n_max, int(H), int(W), int(run_cap),
                                       vp(ln), vp(off), vp(data), int(pool_cap), vp(bbox), self._stream())
        if rc:
            raise HipError(f'nuhtc_rle_encode failed ({rc})')
        torch.cuda.current_stream(self.device).synchronize()
        return ln, off, data, bbox

    def export_async(self, B, cap=None, contour_cap=256, crop_words_per_det=128, rle=False, rle_bytes_per_det=256, rle_run_cap=hip.RLE_MAX_RUNS,
                     nucfeat=False, nucmorph=False, nuctex=False):
        """After infer_async: enqueue, on the current stream, everything the slide loop needs from the batch -- the outer
        contours (nuhtc_mask_contours), a gather of the kept detections, in (tile, slot) order (nuhtc_export_kept), and their
        masks cropped to their bounding rectangles into one word pool (nuhtc_export_crops) -- into fixed-capacity pinned host
        buffers.  No host synchronisation: every device -> host copy of a result would otherwise block the submitting thread
        behind the other batches in flight.  Read with export_read() once the stream (or an event recorded after this call) has
        completed.  The full 8 KB masks stay on the device (export_full_mask fetches one when a crop did not fit the pool).
        rle=True: the COCO run-length string and box of every kept detection's full-tile mask as well (nuhtc_rle_encode on the compacted
        masks): the blob gains rle_len [cap], rle_off [cap + 1], rle_bbox [cap, 4] and rle_bytes [cap * rle_bytes_per_det], and the strings
        leave in the same single copy.  rle_run_cap defaults to the most the kernel takes (60 KB of LDS positions): its workgroups have 1024
        threads, two of them fill a CU's 2048 thread slots and 2 x 60 KB fit its 160 KB of LDS, so a smaller capacity would buy no occupancy
        and only send ragged masks to the host encoder.  The image width must be a multiple of 32 (the mask rows are the frame the strings describe).
        nucfeat=True: the embedding of every kept detection as well (nuhtc_nucleus_features: the FPN maps x0..x3 of its tile averaged under
        its mask, nuhtc_amd.nucfeat.pool_reference): the blob gains feat [cap, 256] float32, 1 KB per detection in the same single copy.
        nucmorph=True: the morphometry integers of every kept detection as well (nuhtc_nucleus_morph on the tiles of the last infer_async,
        which the caller keeps alive until the stream has passed this call; nuhtc_amd.nucmorph.morph_reference): the blob gains morph_raw
        [cap, 16] int64 and morph_hist [cap, 256] int32, 1152 bytes per detection in the same single copy.
        nuctex=True: the grey-level co-occurrence counts of every kept detection as well (nuhtc_nucleus_texture, on the same tiles;
        nuhtc_amd.nuctex.glcm_reference): the blob gains tex [cap, 2, 136] int32, 1088 bytes per detection in the same single copy."""
        sel = nuclei.select(nucfeat=nucfeat, nucmorph=nucmorph, nuctex=nuctex)    # below this line no kind is named (nuhtc_amd.nuclei)
        K, W = self.cfg.max_per_img, self.cfg.tile_h * (self.cfg.tile_w // 32)
        if rle and self.cfg.tile_w != self.image_hw[1]:
            raise ValueError(f'export_async(rle=True): image width {self.image_hw[1]} is not a multiple of 32')
        # default capacity: 96 kept detections per tile on average at the x2 resize of a 40x slide, scaled with the nuclei per tile at
        # larger factors (20x slides: x4 -> four times the nuclei per 256-px tile); a batch over it falls back for that batch only
        per_tile = 96 * max(1, int(round((float(self.cfg.scale_factor) / 2.0) ** 2)))
        cap = int(cap or min(self.cfg.max_batch * K, per_tile * self.cfg.max_batch))
        pool = cap * int(crop_words_per_det)
        rle_pool = cap * int(rle_bytes_per_det) if rle else 0
        ex = getattr(self, '_ex', None)
        if ex is None or ex['cap'] != cap or ex['ccap'] != contour_cap or ex['pool'] != pool or ex['rle_pool'] != rle_pool or ex['kinds'] != sel:
            dev = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=self.device)
            names = dict(nk=((2,), torch.int32), idx=((cap,), torch.int64), boxes=((cap, 5), torch.float32), labels=((cap,), torch.int32),
                         cn=((cap,), torch.int32), crop_box=((cap, 4), torch.int32), crop_area=((cap,), torch.int32),
                         crop_off=((cap + 1,), torch.int32), crop_words=((pool,), torch.int32), xy=((cap, contour_cap, 2), torch.int16))
            if rle:
                names.update(rle_len=((cap,), torch.int32), rle_off=((cap + 1,), torch.int32), rle_bbox=((cap, 4), torch.int32),
                             rle_bytes=((rle_pool,), torch.uint8))
            for kind in sel:
                names.update({f: ((cap,) + tail, getattr(torch, dt)) for f, tail, dt in kind.fields})
            # every field is a view into ONE device buffer and ONE pinned host buffer: a batch's results leave the device in a single
            # copy (each asynchronous copy on a compute stream costs a hand-over between the copy engine and the kernels)
            offs, total = {}, 0
            for k, (sh, dt) in names.items():
                offs[k] = total
                total += (int(np.prod(sh)) * torch.empty(0, dtype=dt).element_size() + 255) // 256 * 256
            blob_dev = torch.zeros(total, dtype=torch.uint8, device=self.device)
            # EXPORT_BUFFERS = 3 pinned host buffers, used in turn.  A pipeline slot holds up to two exported batches (A running or
            # done, B queued behind it); when A has been collected and the slot is resubmitted (C) BEFORE A's views are unpacked, C's
            # copy must not land in A's buffer nor in B's: three buffers.  The views of a collected batch stay intact until the second
            # export_async after the one that filled them (i.e. until the slot's next-but-one batch is enqueued)
            blob_hosts = [torch.zeros(total, dtype=torch.uint8).pin_memory() for _ in range(self.EXPORT_BUFFERS)]
            view = lambda blob, k: blob[offs[k]:offs[k] + int(np.prod(names[k][0])) * torch.empty(0, dtype=names[k][1]).element_size()].view(names[k][1]).view(*names[k][0])
            ex = self._ex = dict(cap=cap, ccap=contour_cap, pool=pool, rle_pool=rle_pool, kinds=sel, blob_dev=blob_dev, blob_hosts=blob_hosts, turn=0,
                                 hosts=[{k: view(b, k) for k in names} for b in blob_hosts], dev={k: view(blob_dev, k) for k in names})
            ex['dev']['words'] = dev(cap, W, dtype=torch.int32)          # full masks of the kept detections: device only
        self.contours_async(B, contour_cap)
        d = ex['dev']
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        # compaction of the kept detections on the device (nuhtc_export_kept), then one asynchronous copy per field
        self._check(self.lib.nuhtc_export_kept(self.h, ctypes.byref(self.dets), B, vp(self.contour_n), vp(self.contour_xy), contour_cap, cap,
                                               vp(d['nk']), vp(d['idx']), vp(d['boxes']), vp(d['labels']), vp(d['cn']), vp(d['xy']), vp(d['words']),
                                               self._stream()))
        self._check(self.lib.nuhtc_export_crops(self.h, vp(d['words']), vp(d['nk']), cap, vp(d['crop_box']), vp(d['crop_area']), vp(d['crop_off']),
                                                vp(d['crop_words']), pool, self._stream()))
        if rle:     # behind nuhtc_export_kept on the same stream: n is read from nk[0] on the device
            rc = self.lib.nuhtc_rle_encode(self.device.index, vp(d['words']), vp(d['nk']), cap, self.cfg.tile_h, self.cfg.tile_w, int(rle_run_cap),
                                           vp(d['rle_len']), vp(d['rle_off']), vp(d['rle_bytes']), rle_pool, vp(d['rle_bbox']), self._stream())
            if rc:
                raise HipError(f'nuhtc_rle_encode failed ({rc})')
        for kind in sel:    # behind nuhtc_export_kept on the same stream: the list and its length are read from idx / nk[0] on the device
            self._nucleus_async(kind, B, d['idx'], d['nk'], cap, [d[f] for f, _, _ in kind.fields])
        ex['turn'] = (ex['turn'] + 1) % self.EXPORT_BUFFERS
        ex['host'] = ex['hosts'][ex['turn']]
        ex['blob_hosts'][ex['turn']].copy_(ex['blob_dev'], non_blocking=True)
        ex['B'] = B
        self._read_turn = None          # (EnginePipeline.collect points export_read() at the buffer of the batch it returns)
        return ex['turn']

    def export_read(self, turn=None):
        """-> dict of numpy views (n kept detections: tile index in the batch, slot, box+score, label, contour length
        (<= 0: traced by the host mirror), contour vertices, bit-packed mask words) of the pinned buffers export_async
        filled, or None when the batch held more kept detections than the buffers (use the synchronous path then).
        The views stay valid through the next TWO export_async calls of this engine (EXPORT_BUFFERS = 3 host buffers used in turn:
        a slot of an EnginePipeline may be resubmitted before the batch it just delivered is unpacked), not the one after those;
        `turn` selects the buffer of an earlier export_async (its return value) when the next batch has been enqueued already.
        Raises on the capacity flag of that inference (what check() reports)."""
        if turn is None:
            turn = getattr(self, '_read_turn', None)
        ex = self._ex['hosts'][self._ex['turn'] if turn is None else turn]
        if int(ex['nk'][1]):
            raise HipError('connected-component proposals exceeded max_cc_proposals on at least one tile (NUHTC_E_CAPACITY)')
        n = int(ex['nk'][0])
        if n > self._ex['cap']:
            return None
        K = self.cfg.max_per_img
        idx = ex['idx'][:n].numpy()
        off = ex['crop_off'].numpy()
        g = dict(n=n, tile=idx // K, slot=idx % K, boxes=ex['boxes'][:n].numpy(), labels=ex['labels'][:n].numpy(), cn=ex['cn'][:n].numpy(),
                 xy=ex['xy'][:n].numpy(), crop_box=ex['crop_box'][:n].numpy(), crop_area=ex['crop_area'][:n].numpy(), crop_off=off[:n],
                 crop_words=ex['crop_words'].numpy().view(np.uint32), crop_total=int(off[self._ex['cap']]), pool=self._ex['pool'])
        if 'rle_len' in ex:         # exported with rle=True: string k = rle_bytes[rle_off[k]:rle_off[k] + rle_len[k]] where it ends inside rle_pool
            roff = ex['rle_off'].numpy()
            g.update(rle_len=ex['rle_len'][:n].numpy(), rle_off=roff[:n], rle_bbox=ex['rle_bbox'][:n].numpy(), rle_bytes=ex['rle_bytes'].numpy(),
                     rle_total=int(roff[n]), rle_pool=self._ex['rle_pool'])
        for kind in self._ex['kinds']:      # row k of every field belongs to detection k
            g.update({f: ex[f][:n].numpy() for f, _, _ in kind.fields})
        return g

    def _nucleus_async(self, kind, B, idx, n_dev, cap, outs):
        """Enqueue the kernel of one kind of per-nucleus measurement (nuhtc_amd.nuclei) on the current stream: the entries idx[:min(n_dev[0],
        cap)] (device tensors: tile * max_per_img + slot, as nuhtc_export_kept writes them) of the last infer_async into the device tensors
        `outs`, one per field of the kind.  The kinds that read pixels read the tiles of that inference."""
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        src = ()
        if kind.reads_tiles:
            (lut, k), (tiles, mode) = self._morph_constants(), self._morph_src
            src = (vp(tiles), mode, vp(lut), k)
        self._check(getattr(self.lib, kind.call)(self.h, ctypes.byref(self.dets), B, *src, vp(idx), vp(n_dev), cap, *[vp(o) for o in outs], self._stream()))

    def _nucleus_sync(self, kind, B, tile, slot):
        """The fields of one kind for the detections (tile[i], slot[i]) of the last infer_async, on a list made here -> tuple of ndarrays."""
        n = len(tile)
        if n == 0:
            return tuple(np.zeros((0,) + tail, dt) for _, tail, dt in kind.fields)
        idx = torch.from_numpy(np.asarray(tile, np.int64) * self.cfg.max_per_img + np.asarray(slot, np.int64)).to(self.device)
        cnt = torch.tensor([n], dtype=torch.int32, device=self.device)
        outs = [torch.zeros(n, *tail, dtype=getattr(torch, dt), device=self.device) for _, tail, dt in kind.fields]
        self._nucleus_async(kind, B, idx, cnt, n, outs)
        return tuple(o.cpu().numpy() for o in outs)

    def nucleus_features(self, B, tile, slot):
        """Embeddings of the detections (tile[i], slot[i]) of the last infer_async, synchronously (nuhtc_nucleus_features on a list made
        here; export_async(nucfeat=True) is the asynchronous route) -> float32 (n, 256) ndarray."""
        return self._nucleus_sync(nuclei.FEAT, B, tile, slot)[0]

    def _morph_constants(self):
        """(device int32 [256] table, host int32 [3] coefficients) of the haematoxylin value, built once (nuclei.stain_constants)."""
        if getattr(self, '_morph_k', None) is None:
            lut, k = nuclei.stain_constants()
            self._morph_lut = torch.from_numpy(lut).to(self.device)
            self._morph_k = (ctypes.c_int32 * 3)(*[int(v) for v in k])
        return self._morph_lut, self._morph_k

    def nucleus_morph(self, B, tile, slot):
        """Morphometry integers of the detections (tile[i], slot[i]) of the last infer_async, synchronously (nuhtc_nucleus_morph on a list
        made here; the asynchronous route is export_async) -> (raw int64 (n, 16), hist int32 (n, 256)) ndarrays."""
        return self._nucleus_sync(nuclei.MORPH, B, tile, slot)

    def nucleus_texture(self, B, tile, slot):
        """Co-occurrence counts of the detections (tile[i], slot[i]) of the last infer_async, synchronously (nuhtc_nucleus_texture on a list
        made here; the asynchronous route is export_async) -> int32 (n, 2, 136) ndarray."""
        return self._nucleus_sync(nuclei.TEX, B, tile, slot)[0]

    def export_full_mask(self, k):
        """(tile_h, tile_w) bool mask of exported detection k of the last export_async (synchronous device read: the rare crop that
        did not fit the pool, or a contour the device could not trace)."""
        words = self._ex['dev']['words'][k].cpu().numpy().view(np.uint32)
        return np.unpackbits(words.view(np.uint8).reshape(self.cfg.tile_h, self.cfg.tile_w // 8), axis=-1, bitorder='little').astype(bool)

    def results(self, B, with_masks=True):
        """Device outputs of the last infer -> list of (bbox_results, segm_results) exactly like the reference
        (`bbox2result` mmdet/core/bbox/transforms.py:100-117; `get_seg_masks` list-of-bool-arrays per class)."""
        self.check()
        counts = self.counts[:B].cpu().numpy()
        boxes = self.boxes[:B].cpu().numpy()
        labels = self.labels[:B].cpu().numpy()
        nc = self.cfg.num_classes
        H, W = self.cfg.tile_h, self.cfg.tile_w
        out = []
        for b in range(B):
            n = int(counts[b])
            d, l = boxes[b, :n], labels[b, :n]
            bbox_res = [d[l == c] for c in range(nc)]
            if with_masks and n:
                words = self.masks[b, :n].cpu().numpy().view(np.uint32)
                bits = np.unpackbits(words.view(np.uint8).reshape(n, H, W // 8), axis=-1, bitorder='little').astype(bool)[..., :self.image_hw[1]]
                segm_res = [[bits[j] for j in range(n) if l[j] == c] for c in range(nc)]
            else:
                segm_res = [[] for _ in range(nc)]
            out.append((bbox_res, segm_res))
        return out

    def __call__(self, tiles, channel_mode=hip.CH_AS_IS):
        t = self.to_device(tiles)
        out = []
        for i in range(0, t.shape[0], self.cfg.max_batch):
            chunk = t[i:i + self.cfg.max_batch]
            B = self.infer_async(chunk, channel_mode)
            out.extend(self.results(B))
        return out

    # ------------------------------------------------------------------ parity-test access
    def enable_token_dump(self):
        p = ctypes.c_void_p()
        self._check(self.lib.nuhtc_get_buffer(self.h, b'__enable_token_dump', ctypes.byref(p), None, None, None))

    def buffer(self, name):
        """Copy of an intermediate tensor of the last infer call (see nuhtc_get_buffer)."""
        p = ctypes.c_void_p()
        shape = (ctypes.c_int64 * 6)()
        nd, dt = ctypes.c_int(), ctypes.c_int()
        self._check(self.lib.nuhtc_get_buffer(self.h, name.encode(), ctypes.byref(p), shape, ctypes.byref(nd), ctypes.byref(dt)))
        torch.cuda.current_stream(self.device).synchronize()
        shp = [shape[i] for i in range(nd.value)]
        view = torch.as_tensor(_DevView(p.value, shp, _TYPESTR[dt.value]), device=self.device)
        return view.clone()

    def op_gemm(self, A, W, bias=None, act=0, pipe='fp32'):
        """C = act(A @ W.T + bias) by the engine's GEMM kernel; pipe 'fp32' (v_mfma_f32_32x32x2_f32) or 'split' (exact 3-way bf16
        split of both operands on v_mfma_f32_32x32x16_bf16)."""
        M, K = A.shape
        N = W.shape[0]
        C = torch.empty(M, N, dtype=torch.float32, device=self.device)
        bp = bias.data_ptr() if bias is not None else None
        if pipe == 'fp32':
            self._check(self.lib.nuhtc_op_gemm(self.h, A.data_ptr(), W.data_ptr(), bp, C.data_ptr(), M, N, K, act, self._stream()))
        else:
            wh = np.ascontiguousarray(W.detach().cpu().numpy(), dtype=np.float32)
            self._check(self.lib.nuhtc_op_gemm_split(self.h, A.data_ptr(), W.data_ptr(), wh.ctypes.data_as(ctypes.c_void_p), bp, C.data_ptr(),
                                                     M, N, K, act, self._stream()))
        return C

    def op_ln_gemm(self, x, w, bias, ln_g, ln_b, rows=None, act=0):
        """act(LayerNorm(x[rows]) @ w.T + bias) with the norm in the product's A path (csrc/gemm.hip A_LN, statistics by ln_stats_kernel);
        x (T, K) on the device, rows: optional device int32 (M,) row indices, the rest anywhere."""
        T, K = x.shape
        M = int(rows.shape[0]) if rows is not None else T
        N = w.shape[0]
        out = torch.empty(M, N, dtype=torch.float32, device=self.device)
        h = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        wh, gh, bh = h(w), h(ln_g), h(ln_b)
        bias_h = h(bias) if bias is not None else None
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
        self._check(self.lib.nuhtc_op_ln_gemm(self.h, x.data_ptr(), T, rows.data_ptr() if rows is not None else None, vp(wh), vp(bias_h), vp(gh), vp(bh),
                                              out.data_ptr(), M, N, K, act, self._stream()))
        return out

    def op_gemm_ln_gemm(self, a, wp, bp, w, bias, ln_g, ln_b, res=None, row_map=None, act=0):
        """y[row_map] = a @ wp.T + bp (+ res[row_map]); c = act(LayerNorm(y) @ w.T + bias) the way the engine chains them: the producer's
        epilogue leaves the row statistics per 96 columns, the consumer merges them (csrc/gemm.hip stats_out / A_LN).  -> (y, c)."""
        M, Kp = a.shape
        K, N = wp.shape[0], w.shape[0]
        y = torch.zeros(M, K, dtype=torch.float32, device=self.device)
        c = torch.empty(M, N, dtype=torch.float32, device=self.device)
        h = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32) if t is not None else None
        wph, bph, wh, bh, gh, lbh = h(wp), h(bp), h(w), h(bias), h(ln_g), h(ln_b)
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None
        self._check(self.lib.nuhtc_op_gemm_ln_gemm(self.h, a.data_ptr(), vp(wph), vp(bph), res.data_ptr() if res is not None else None,
                                                   row_map.data_ptr() if row_map is not None else None, vp(wh), vp(bh), vp(gh), vp(lbh),
                                                   y.data_ptr(), c.data_ptr(), M, Kp, K, N, act, self._stream()))
        return y, c

    def op_merge_ln_gemm(self, x, B, H, W, w, ln_g, ln_b):
        """PatchMerging in one launch (csrc/gemm.hip A_LN over two segments per row): x (B*H*W, C) tokens on the device; w (2C, 4C), ln_g / ln_b (4C)
        in the reference's nn.Unfold column order (transformer.py:363-385).  -> (B*H/2*W/2, 2C)."""
        C = x.shape[1]
        y = torch.empty(B * (H // 2) * (W // 2), 2 * C, dtype=torch.float32, device=self.device)
        h = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        wh, gh, bh = h(w), h(ln_g), h(ln_b)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self.lib.nuhtc_op_merge_ln_gemm(self.h, x.data_ptr(), B, H, W, C, vp(wh), vp(gh), vp(bh), y.data_ptr(), self._stream()))
        return y

    def op_swin_mlp(self, x, ln_g, ln_b, w1, b1, w2, b2):
        """x + W2 gelu(W1 LN(x) + b1) + b2 by the fused FFN kernel (csrc/mlp.hip); x (T, C) and the vectors on the device, w1 / w2 anywhere."""
        T, C = x.shape
        out = torch.empty_like(x)
        w1h = np.ascontiguousarray(w1.detach().cpu().numpy(), dtype=np.float32)
        w2h = np.ascontiguousarray(w2.detach().cpu().numpy(), dtype=np.float32)
        self._check(self.lib.nuhtc_op_swin_mlp(self.h, x.data_ptr(), ln_g.data_ptr(), ln_b.data_ptr(), w1h.ctypes.data_as(ctypes.c_void_p), b1.data_ptr(),
                                               w2h.ctypes.data_as(ctypes.c_void_p), b2.data_ptr(), out.data_ptr(), T, C, self._stream()))
        return out

    def op_swin_proj_mlp(self, x, att, wp, bp, ln_g, ln_b, w1, b1, w2, b2):
        """x' = x + Wp att + bp; x' + W2 gelu(W1 LN(x') + b1) + b2: the fused second half of a Swin block (csrc/mlp.hip with the attention
        projection in front); x, att (T, C) and the vectors on the device, the weight matrices anywhere."""
        T, C = x.shape
        out = torch.empty_like(x)
        h = lambda w: np.ascontiguousarray(w.detach().cpu().numpy(), dtype=np.float32)
        wph, w1h, w2h = h(wp), h(w1), h(w2)
        cp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self.lib.nuhtc_op_swin_proj_mlp(self.h, x.data_ptr(), att.data_ptr(), cp(wph), bp.data_ptr(), ln_g.data_ptr(), ln_b.data_ptr(), cp(w1h),
                                                    b1.data_ptr(), cp(w2h), b2.data_ptr(), out.data_ptr(), T, C, self._stream()))
        return out

    def op_roi_align(self, feat_nhwc, rois, P, scale, sr):
        N, H, W, C = feat_nhwc.shape
        R = rois.shape[0]
        out = torch.empty(R, P, P, C, dtype=torch.float32, device=self.device)
        self._check(self.lib.nuhtc_op_roi_align(self.h, feat_nhwc.data_ptr(), N, H, W, rois.data_ptr(), R, P, float(scale), int(sr),
                                                out.data_ptr(), self._stream()))
        return out

    def op_nms(self, boxes, scores, thr):
        n = boxes.shape[0]
        keep = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._check(self.lib.nuhtc_op_nms(self.h, boxes.data_ptr(), scores.data_ptr(), n, float(thr), keep.data_ptr(), cnt.data_ptr(),
                                          self._stream()))
        return keep[:int(cnt.item())].long()

    def op_cc_mask(self, sem_pred, H, W):
        """Thresholded mask of the connected-component proposals: semantic logits (B, h, w) on the device -> bilinear
        (align_corners) to (H, W), 5x5 Gaussian, > 0 -> (B, H, W) uint8."""
        B, h, w = sem_pred.shape
        sem_pred = sem_pred.contiguous().float()
        out = torch.empty(B, H, W, dtype=torch.uint8, device=self.device)
        self._check(self.lib.nuhtc_op_cc_mask(self.h, sem_pred.data_ptr(), B, h, w, int(H), int(W), out.data_ptr(), self._stream()))
        return out

    def op_cc_proposals(self, mask, open=True, min_area=10, cap=512):
        """The rest of the chain on a (B, H, W) 0/1 mask on the device: optional opening, hole filling, 4-connected labels, boxes.
        Returns dict(opened, filled, labels (root = raster index of the component's first pixel, -1 background), stats (B, H*W, 5:
        area, xmin, ymin, xmax, ymax at the root), area (B, H*W), boxes (B, cap, 4), counts (B,), overflow (images over cap))."""
        B, H, W = mask.shape
        mask = mask.contiguous().to(torch.uint8)
        dev = dict(dtype=torch.int32, device=self.device)
        r = dict(opened=torch.empty_like(mask), filled=torch.empty_like(mask), labels=torch.empty(B, H, W, **dev),
                 stats=torch.empty(B, H * W, 5, **dev), boxes=torch.zeros(B, cap, 4, dtype=torch.float32, device=self.device),
                 counts=torch.empty(B, **dev), overflow=torch.empty(1, **dev))
        self._check(self.lib.nuhtc_op_cc_proposals(self.h, mask.data_ptr(), B, H, W, 1 if open else 0, int(min_area), int(cap),
                                                   *(r[k].data_ptr() for k in ('opened', 'filled', 'labels', 'stats', 'boxes', 'counts', 'overflow')),
                                                   self._stream()))
        r['area'] = r['stats'][..., 0]
        r['overflow'] = int(r['overflow'].item())
        return r

    def op_conv3(self, x, w, bias=None, act=0, pipe='split', nimg_dev=None, N2=0, w2=None, b2=None, act2=0, store_out=1, res2=None,
                 wn1=None, bn1=None, more=(), out=None, out2=None, out3=None, outn1=None, more_out2=None):
        """3x3 convolution 64 -> 64 (zero padding 1) through the engine's dispatch (nuhtc_op_conv3): x (nimg, H, W, 64) NHWC on the device,
        w (64, 64, 3, 3), bias (64,) anywhere; pipe 'split' (halo kernel, csrc/conv.hip) or 'fp32' (implicit GEMM, csrc/gemm.hip).
        nimg_dev: device int32 (1,) image count.  N2 = 32 / 64 fuses out2 = act2(x' @ w2.T + b2) on the activated output x'; res2 (device,
        like x) gives out3 = res2 + out2; wn1 (64,) / bn1 (1,) give outn1 = x' @ wn1 + bn1; `more` holds further maps (device, nimg
        images each) through the same layers, whose second outputs come back in more_out2.  Outputs not given are allocated (empty).
        Returns dict(out, out2, out3, outn1, more_out2)."""
        nimg, H, W, C = x.shape
        h = lambda t: np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32) if t is not None else None
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
        dp = lambda t: t.data_ptr() if t is not None else None
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        wh, bh, w2h, b2h, wn1h, bn1h = h(w), h(bias), h(w2), h(b2), h(wn1), h(bn1)
        if out is None:
            out = new(nimg, H, W, 64)
        if N2 and out2 is None:
            out2 = new(nimg, H, W, N2)
        if res2 is not None and out3 is None:
            out3 = new(nimg, H, W, 64)
        if wn1 is not None and outn1 is None:
            outn1 = new(nimg, H, W)
        more = list(more)
        if more_out2 is None:
            more_out2 = [new(nimg, m.shape[1], m.shape[2], N2 or 32) for m in more]
        a = hip.Conv3Args(inp=x.data_ptr(), out=dp(out), w=vp(wh), bias=vp(bh), nimg=nimg, H=H, W=W, act=int(act),
                          nimg_dev=dp(nimg_dev), pipe=hip.PIPE_FP32 if pipe == 'fp32' else hip.PIPE_BF16_SPLIT, N2=int(N2), w2=vp(w2h),
                          b2=vp(b2h), act2=int(act2), store_out=int(store_out), out2=dp(out2), res2=dp(res2), out3=dp(out3), wn1=vp(wn1h),
                          bn1=vp(bn1h), outn1=dp(outn1), n_more=len(more))
        for k, m in enumerate(more[:3]):
            a.more_in[k], a.more_out2[k], a.more_H[k], a.more_W[k] = m.data_ptr(), more_out2[k].data_ptr(), m.shape[1], m.shape[2]
        self._check(self.lib.nuhtc_op_conv3(self.h, ctypes.byref(a), self._stream()))
        return dict(out=out, out2=out2, out3=out3, outn1=outn1, more_out2=more_out2)

    def op_window_msa(self, x, ln_g, ln_b, qkv_w, qkv_b, rel_table, shifted, pipe='split', order='token', out=None):
        """The attention half of a Swin block up to the attention output, before proj (nuhtc_op_window_msa): x (B, H, W, C) tokens before
        LN1 on the device; ln_g / ln_b (C,), qkv_w (3C, C), qkv_b (3C,), rel_table (169, C / 32) anywhere.  pipe 'split' or 'fp32' (the
        engine's route for that pipe and C); order 'token' (row b*H*W + y*W + x) or 'compact' (the non-padding rows of the shift state's window
        image in window order).  Returns out (B*H*W, C), allocated when not given."""
        B, H, W, C = x.shape
        h = lambda t: np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        arrs = [h(t) for t in (ln_g, ln_b, qkv_w, qkv_b, rel_table)]
        want = [(C,), (C,), (3 * C, C), (3 * C,), (169, C // 32)]
        if [a.shape for a in arrs] != want:
            raise ValueError(f'op_window_msa: weight shapes {[a.shape for a in arrs]}, expected {want}')
        if out is None:
            out = torch.empty(B * H * W, C, dtype=torch.float32, device=self.device)
        a = hip.WmsaArgs(x=x.data_ptr(), out=out.data_ptr(), ln_g=vp(arrs[0]), ln_b=vp(arrs[1]), qkv_w=vp(arrs[2]), qkv_b=vp(arrs[3]),
                         rel_table=vp(arrs[4]), B=B, H=H, W=W, C=C, shifted=int(bool(shifted)),
                         pipe=hip.PIPE_FP32 if pipe == 'fp32' else hip.PIPE_BF16_SPLIT,
                         out_order=hip.ORDER_COMPACT if order == 'compact' else hip.ORDER_TOKEN)
        self._check(self.lib.nuhtc_op_window_msa(self.h, ctypes.byref(a), self._stream()))
        return out

    # ------------------------------------------------------------------ the front and the small dense kernels, op by op
    def op_patch_embed(self, tiles, valid_hw, scale, channel_mode, mean, std, w, b, ln_g, ln_b, want_img=True):
        """Resize + Normalize + Pad + patch embedding + LayerNorm(96) of device uint8 tiles (B, th, tw, 3) whose image is the top-left
        valid_hw (nuhtc_op_patch_embed); w (96, 3, 4, 4), b, ln_g, ln_b (96,) anywhere.  -> (tok (B * Hn/4 * Wn/4, 96), img (B, Hn, Wn, 3) or
        None): the tokens by patch_embed_tiles_kernel, the normalised padded image by preproc_kernel from the same tables."""
        B, th, tw, _ = tiles.shape
        h = lambda t: np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        wh, bh, gh, lbh = h(w), h(b), h(ln_g), h(ln_b)
        if wh.shape != (96, 3, 4, 4) or bh.shape != (96,) or gh.shape != (96,) or lbh.shape != (96,) or tiles.dtype != torch.uint8:
            raise ValueError('op_patch_embed: uint8 tiles, w (96, 3, 4, 4), b / ln_g / ln_b (96,)')
        Hv, Wv = int(valid_hw[0] * float(scale) + 0.5), int(valid_hw[1] * float(scale) + 0.5)
        Hn, Wn = -(-Hv // 32) * 32, -(-Wv // 32) * 32
        tok = torch.empty(B * (Hn // 4) * (Wn // 4), 96, dtype=torch.float32, device=self.device)
        img = torch.empty(B, Hn, Wn, 3, dtype=torch.float32, device=self.device) if want_img else None
        f3 = lambda v: (ctypes.c_float * 3)(*[float(x) for x in v])
        self._check(self.lib.nuhtc_op_patch_embed(self.h, tiles.data_ptr(), B, th, tw, int(valid_hw[0]), int(valid_hw[1]), float(scale), int(channel_mode),
                                                  f3(mean), f3(std), vp(wh), vp(bh), vp(gh), vp(lbh), tok.data_ptr(),
                                                  img.data_ptr() if img is not None else None, self._stream()))
        return tok, img

    def op_layernorm(self, x, g, b, out=None):
        """LayerNorm (eps 1e-5) of the rows of x (rows, C) by the plain kernels of csrc/swin.hip (nuhtc_op_layernorm); all on the device."""
        rows, C = x.shape
        if out is None:
            out = torch.empty_like(x)
        self._check(self.lib.nuhtc_op_layernorm(self.h, x.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr(), rows, C, self._stream()))
        return out

    def op_merge_ln(self, x, g, b, out=None):
        """PatchMerging's gather + LayerNorm(4C) (merge_ln_kernel): x (B, H, W, C), g / b (4C,) in the kernel's order k = (kh*2+kw)*C + c, all
        on the device.  -> (B * H/2 * W/2, 4C)."""
        B, H, W, C = x.shape
        if out is None:
            out = torch.empty(B * (H // 2) * (W // 2), 4 * C, dtype=torch.float32, device=self.device)
        self._check(self.lib.nuhtc_op_merge_ln(self.h, x.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr(), B, H, W, C, self._stream()))
        return out

    def op_fpn_lateral(self, x, w, bias, ln_g=None, ln_b=None, parent=None):
        """An FPN lateral as run_fpn launches it (nuhtc_op_fpn_lateral): x (B, H, W, C) on the device, w (64, C), bias (64,), ln_g / ln_b (C,)
        anywhere (None: no norm, the fp32 pipe's form), parent (B, H/2, W/2, 64) on the device or None.  -> (B, H, W, 64)."""
        B, H, W, C = x.shape
        h = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32) if t is not None else None
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
        wh, bh, gh, lbh = h(w), h(bias), h(ln_g), h(ln_b)
        out = torch.empty(B, H, W, 64, dtype=torch.float32, device=self.device)
        self._check(self.lib.nuhtc_op_fpn_lateral(self.h, x.data_ptr(), B, H, W, C, vp(wh), vp(bh), vp(gh), vp(lbh),
                                                  parent.data_ptr() if parent is not None else None, out.data_ptr(), self._stream()))
        return out

    def op_sem_fuse(self, g0, g1, g2, g3):
        """relu(g0) + sum of relu(align-corners bilinear upsampling of g1..g3) (sem_fuse_kernel); g_i (B, H >> i, W >> i, 64) on the device."""
        B, H, W, _ = g0.shape
        out = torch.empty_like(g0)
        self._check(self.lib.nuhtc_op_sem_fuse(self.h, g0.data_ptr(), g1.data_ptr(), g2.data_ptr(), g3.data_ptr(), out.data_ptr(), B, H, W, self._stream()))
        return out

    def op_pointwise64(self, x, w, b, out, rows_dev=None, rows_mul=1, sigmoid=False):
        """out[row] = w . x[row] + b over the rows of x (rows, 64) (conv1x1_n1_kernel), all on the device; rows_dev (device int32 (1,)) selects the
        grid-strided form limited to min(rows, rows_dev * rows_mul) rows, with a sigmoid on request.  Writes into `out` (rows,)."""
        self._check(self.lib.nuhtc_op_pointwise64(self.h, x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), x.shape[0],
                                                  rows_dev.data_ptr() if rows_dev is not None else None, int(rows_mul), int(bool(sigmoid)), self._stream()))
        return out

    def op_fpn_mean_pool(self, maps):
        """Per-channel means of four maps (B, hw_l, 64) on the device -> (B, 256), level-major (the pooling of nuhtc_features, csrc/pool.hip)."""
        B = maps[0].shape[0]
        ptrs = (ctypes.c_void_p * 4)(*[m.data_ptr() for m in maps])
        hw = (ctypes.c_int32 * 4)(*[int(m.shape[1]) for m in maps])
        feat = torch.empty(B, 256, dtype=torch.float32, device=self.device)
        self._check(self.lib.nuhtc_op_fpn_mean_pool(self.h, ptrs, hw, B, feat.data_ptr(), self._stream()))
        return feat

    # ------------------------------------------------------------------ the detection tail, op by op (csrc/roi.hip)
    def _i32(self, v):
        return v if isinstance(v, torch.Tensor) else torch.tensor(np.atleast_1d(np.asarray(v)), dtype=torch.int32, device=self.device)

    def op_bbox_tail(self, h, cls_w, cls_b, reg_w, reg_b, rois, r, stds, img_hw, refine, cls=None, reg=None):
        """The tail of one bbox head (nuhtc_op_bbox_tail): h (cap, 256) and rois (cap, 5) on the device, fc_cls / fc_reg weights and biases
        anywhere (the checkpoint's layout), r: the device-side RoI count (int or device int32 (1,)).  Rows below r of cls (cap, 16: nc + 2
        used) and reg (cap, 4) are written, and with `refine` rois is regressed IN PLACE.  Returns (cls, reg), allocated when not given."""
        f = lambda t: np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        cw, cb, rw, rb = f(cls_w), f(cls_b), f(reg_w), f(reg_b)
        nc, cap = cw.shape[0] - 2, h.shape[0]
        if cw.shape != (nc + 2, 256) or cb.shape != (nc + 2,) or rw.shape != (4, 256) or rb.shape != (4,):
            raise ValueError('op_bbox_tail: fc_cls (nc + 2, 256) / (nc + 2,), fc_reg (4, 256) / (4,) expected')
        if cls is None:
            cls = torch.empty(cap, 16, dtype=torch.float32, device=self.device)
        if reg is None:
            reg = torch.empty(cap, 4, dtype=torch.float32, device=self.device)
        r_dev = self._i32(r)
        a = hip.BboxTailArgs(h=h.data_ptr(), cls_w=vp(cw), cls_b=vp(cb), reg_w=vp(rw), reg_b=vp(rb), nc=nc, cap=cap, refine=int(bool(refine)),
                             stds=(ctypes.c_float * 4)(*[float(v) for v in stds]), img_w=float(img_hw[1]), img_h=float(img_hw[0]),
                             r_dev=r_dev.data_ptr(), rois=rois.data_ptr(), cls=cls.data_ptr(), reg=reg.data_ptr())
        self._check(self.lib.nuhtc_op_bbox_tail(self.h, ctypes.byref(a), self._stream()))
        return cls, reg

    def op_det_post(self, rois, cls, reg2, roi_off, roi_cnt, nc, stds, img_hw, scale, score_thr, nms_iou, max_per_img, limit=None, cap=None):
        """Ensemble + Seesaw candidates + multiclass NMS + labels / mask RoIs (nuhtc_op_det_post): rois (T, 5), cls = the three stages'
        (T, 16) logits and reg2 (T, 4) on the device; roi_off / roi_cnt per tile (sequences or device int32).  cap: candidates per tile
        (a multiple of 64; default: room for every (roi, class) pair).  Returns dict(dets (B, max_per_img, 5), labels, counts, mask_rois,
        det_off, det_total, cand_count (B,), cand_scores / cand_ids (B, cap), cand_boxes (B, cap, 4))."""
        off, cnt = self._i32(roi_off), self._i32(roi_cnt)
        B = int(cnt.shape[0])
        if cap is None:
            cap = max(64, -(-int(cnt.max().item()) * nc // 64) * 64)
        K = int(max_per_img)
        dev = dict(dtype=torch.int32, device=self.device)
        fl = dict(dtype=torch.float32, device=self.device)
        r = dict(dets=torch.zeros(B, K, 5, **fl), labels=torch.zeros(B, K, **dev), counts=torch.zeros(B, **dev), mask_rois=torch.zeros(B * K, 5, **fl),
                 det_off=torch.zeros(B, **dev), det_total=torch.zeros(1, **dev), cand_count=torch.zeros(B, **dev),
                 cand_scores=torch.zeros(B, cap, **fl), cand_ids=torch.zeros(B, cap, **dev), cand_boxes=torch.zeros(B, cap, 4, **fl))
        a = hip.DetPostArgs(rois=rois.data_ptr(), cls0=cls[0].data_ptr(), cls1=cls[1].data_ptr(), cls2=cls[2].data_ptr(), reg2=reg2.data_ptr(),
                            roi_off=off.data_ptr(), roi_cnt=cnt.data_ptr(), B=B, nc=int(nc), total=int(rois.shape[0]), cap=int(cap),
                            stds=(ctypes.c_float * 4)(*[float(v) for v in stds]), img_w=float(img_hw[1]), img_h=float(img_hw[0]),
                            scale=float(scale), score_thr=float(score_thr), nms_iou=float(nms_iou), max_per_img=K,
                            limit=K if limit is None else int(limit), **{k: v.data_ptr() for k, v in r.items()})
        self._check(self.lib.nuhtc_op_det_post(self.h, ctypes.byref(a), self._stream()))
        return r

    def op_paste(self, prob, mask_rois, det_off, det_counts, max_keep, H, W, vH, vW, scale, thr=0.5, masks=None, areas=None):
        """Mask paste (nuhtc_op_paste): prob (D, 28, 28), mask_rois (D, 5) on the device -> (masks (B, max_keep, H, W // 32) int32 words,
        areas (B, max_keep)); slots from det_counts[b] on are left as they are (zero when allocated here)."""
        off, cnt = self._i32(det_off), self._i32(det_counts)
        B = int(cnt.shape[0])
        if masks is None:
            masks = torch.zeros(B, max_keep, H, W // 32, dtype=torch.int32, device=self.device)
        if areas is None:
            areas = torch.zeros(B, max_keep, dtype=torch.int32, device=self.device)
        a = hip.PasteArgs(prob=prob.data_ptr(), mask_rois=mask_rois.data_ptr(), det_off=off.data_ptr(), det_counts=cnt.data_ptr(), B=B,
                          D=int(prob.shape[0]), max_keep=int(max_keep), H=int(H), W=int(W), vH=int(vH), vW=int(vW), scale=float(scale),
                          thr=float(thr), masks=masks.data_ptr(), areas=areas.data_ptr())
        self._check(self.lib.nuhtc_op_paste(self.h, ctypes.byref(a), self._stream()))
        return masks, areas

    def op_tile_post(self, dets, labels, areas, det_counts, masks, H, W, vH, vW, margin=2, min_area=10, thr=0.05, keep=None):
        """Per-tile filter + mask-NMS (nuhtc_op_tile_post): dets (B, max_keep, 5), labels, areas (B, max_keep), masks (B, max_keep, H, W // 32)
        on the device -> keep (B, max_keep) uint8; slots from det_counts[b] on are left as they are (zero when allocated here)."""
        cnt = self._i32(det_counts)
        B, K = int(dets.shape[0]), int(dets.shape[1])
        if keep is None:
            keep = torch.zeros(B, K, dtype=torch.uint8, device=self.device)
        a = hip.TilePostArgs(dets=dets.data_ptr(), labels=labels.data_ptr(), areas=areas.data_ptr(), det_counts=cnt.data_ptr(),
                             masks=masks.data_ptr(), keep=keep.data_ptr(), B=B, max_keep=K, H=int(H), W=int(W), vH=int(vH), vW=int(vW),
                             margin=int(margin), min_area=int(min_area), thr=float(thr))
        self._check(self.lib.nuhtc_op_tile_post(self.h, ctypes.byref(a), self._stream()))
        return keep

    # ------------------------------------------------------------------ the RPN half of the proposals, op by op (csrc/proposals.hip)
    def op_rpn_select(self, maps, nms_pre, img_hw, min_size, cand_boxes=None, cand_scores=None, cand_count=None):
        """Per-level selection and decode (nuhtc_op_rpn_select): maps = the four level maps (B, h_l, w_l, 32) on the device (columns 0-2
        objectness logits, 3.. deltas; stride 4 << l) -> (cand_boxes (B, 4, nms_pre, 4), cand_scores (B, 4, nms_pre), cand_count (B, 4));
        slots from the count on are left as they are (zero when allocated here)."""
        if len(maps) != 4 or any(m.dim() != 4 or m.shape[3] != 32 or m.shape[0] != maps[0].shape[0] or m.dtype != torch.float32 for m in maps):
            raise ValueError('op_rpn_select: four float32 maps (B, h, w, 32) expected')
        maps = [m.contiguous() for m in maps]
        B, K = int(maps[0].shape[0]), int(nms_pre)
        fl = dict(dtype=torch.float32, device=self.device)
        Ka = max(K, 1)
        if cand_boxes is None:
            cand_boxes = torch.zeros(B, 4, Ka, 4, **fl)
        if cand_scores is None:
            cand_scores = torch.zeros(B, 4, Ka, **fl)
        if cand_count is None:
            cand_count = torch.zeros(B, 4, dtype=torch.int32, device=self.device)
        ptrs = (ctypes.c_void_p * 4)(*[m.data_ptr() for m in maps])
        hs = (ctypes.c_int32 * 4)(*[int(m.shape[1]) for m in maps])
        ws = (ctypes.c_int32 * 4)(*[int(m.shape[2]) for m in maps])
        self._check(self.lib.nuhtc_op_rpn_select(self.h, ptrs, hs, ws, B, K, int(img_hw[0]), int(img_hw[1]), float(min_size), cand_boxes.data_ptr(),
                                                 cand_scores.data_ptr(), cand_count.data_ptr(), self._stream()))
        return cand_boxes, cand_scores, cand_count

    def op_nms_levels(self, boxes, scores, counts, iou_thr, max_keep, route=0, dets=None, src=None):
        """Level-wise batched NMS (nuhtc_op_nms_levels): boxes (B, G, slot, 4), scores (B, G, slot) on the device, counts (B, G) (array or
        device int32) -> (dets (B, max_keep, 5), src (B, max_keep) flat index into scores, counts (B,)).  route 0: launch_nms_levels (the
        engine's RPN route), 1: launch_nms with the group as id.  Rows from the count on are left as they are (zero when allocated here)."""
        B, G, slot = (int(v) for v in scores.shape)
        if tuple(boxes.shape) != (B, G, slot, 4):
            raise ValueError('op_nms_levels: boxes (B, G, slot, 4) and scores (B, G, slot) expected')
        cnt = self._i32(np.asarray(counts).reshape(-1) if not isinstance(counts, torch.Tensor) else counts)
        if cnt.numel() != B * G:
            raise ValueError('op_nms_levels: counts (B, G) expected')
        K = int(max_keep)
        if dets is None:
            dets = torch.zeros(B, max(K, 1), 5, dtype=torch.float32, device=self.device)
        if src is None:
            src = torch.zeros(B, max(K, 1), dtype=torch.int32, device=self.device)
        out_counts = torch.zeros(B, dtype=torch.int32, device=self.device)
        self._check(self.lib.nuhtc_op_nms_levels(self.h, boxes.contiguous().data_ptr(), scores.contiguous().data_ptr(), cnt.contiguous().data_ptr(), B, G, slot,
                                                 float(iou_thr), K, int(route), dets.data_ptr(), src.data_ptr(), out_counts.data_ptr(), self._stream()))
        return dets, src, out_counts

    def op_build_rois(self, rpn_dets=None, rpn_counts=None, cc_boxes=None, cc_counts=None, fixed=None, B=None, rois=None, cap=None):
        """RoI list assembly (nuhtc_op_build_rois): per image cat(cc_boxes (B, cc_cap, 4) below cc_counts, rpn_dets (B, rpn_cap, 5) below
        rpn_counts), cc_boxes None: the RPN rows alone; or `fixed` (B, n_fixed, 4).  Returns dict(rois (cap, 5), roi_off, roi_cnt (B,), total
        (1,)); rows of rois from total on are left as they are (zero when allocated here)."""
        dev = dict(dtype=torch.int32, device=self.device)
        if fixed is not None:
            B, nf = int(fixed.shape[0]), int(fixed.shape[1])
            need = B * nf
        else:
            B, nf = int(rpn_dets.shape[0]), 0
            rpn_counts = self._i32(rpn_counts)
            need = B * int(rpn_dets.shape[1])
            if cc_boxes is not None:
                cc_counts = self._i32(cc_counts)
                need += B * int(cc_boxes.shape[1])
        if rois is None:
            rois = torch.zeros(max(need if cap is None else int(cap), 1), 5, dtype=torch.float32, device=self.device)
        cap = int(rois.shape[0]) if cap is None else int(cap)
        r = dict(rois=rois, roi_off=torch.zeros(B, **dev), roi_cnt=torch.zeros(B, **dev), total=torch.zeros(1, **dev))
        ptr = lambda t: t.data_ptr() if t is not None else None
        self._check(self.lib.nuhtc_op_build_rois(self.h, ptr(cc_boxes), ptr(cc_counts), int(cc_boxes.shape[1]) if cc_boxes is not None else 1,
                                                 ptr(rpn_dets), ptr(rpn_counts), int(rpn_dets.shape[1]) if rpn_dets is not None else 1,
                                                 ptr(fixed), nf, B, cap, rois.data_ptr(), r['roi_off'].data_ptr(), r['roi_cnt'].data_ptr(),
                                                 r['total'].data_ptr(), self._stream()))
        return r

    # ------------------------------------------------------------------ the RoI feature block, op by op (csrc/roi.hip)
    def op_attn_pool(self, feat, tau, route='auto', out=None):
        """One attention-pool table (nuhtc_op_attn_pool): feat (B, HW, 64) or (B, H, W, 64) float32 on the device -> G of the same shape.
        route 'auto' (what the engine picks), 'gemm' (HW % 32 == 0), 'kernel' or 'fp16'."""
        if feat.dtype != torch.float32 or feat.shape[-1] != 64 or feat.dim() not in (3, 4):
            raise ValueError('op_attn_pool: a float32 map (B, HW, 64) or (B, H, W, 64) expected')
        feat = feat.contiguous()
        B, HW = int(feat.shape[0]), int(feat.numel() // (feat.shape[0] * 64))
        if out is None:
            out = torch.empty_like(feat)
        self._check(self.lib.nuhtc_op_attn_pool(self.h, feat.data_ptr(), B, HW, float(tau), hip.AP_ROUTES[route], out.data_ptr(), self._stream()))
        return out

    def op_roi_feats(self, x0, x1, sem, x0sem, G2, G3, rois, r, P, out=None, fb_flag=None):
        """The fused RoI features (nuhtc_op_roi_feats): x0, sem, x0sem (B, H0, W0, 64), x1 (B, H1, W1, 64), the tables G2 (B, H2, W2, 64), G3
        (B, H3, W3, 64) and rois (cap, 5) on the device, r: the live rows (int or device int32 (1,)), P 7 or 14.  Returns dict(out (cap, P * P,
        64), and for P = 7 fb_flag (cap,) uint8 -- the kernel form of each RoI -- and counts (3,): big, mid-size, giant list lengths); rows
        from r on are left as they are (zero when allocated here)."""
        maps = (x0, x1, G2, G3)
        if any(m.dim() != 4 or m.shape[3] != 64 or m.shape[0] != x0.shape[0] or m.dtype != torch.float32 for m in maps + (sem, x0sem)) \
                or sem.shape != x0.shape or x0sem.shape != x0.shape or rois.dim() != 2 or rois.shape[1] != 5 or rois.dtype != torch.float32:
            raise ValueError('op_roi_feats: float32 maps (B, H, W, 64), sem / x0sem shaped like x0 and rois (cap, 5) expected')
        x0, x1, sem, x0sem, G2, G3, rois = (t.contiguous() for t in (x0, x1, sem, x0sem, G2, G3, rois))
        cap, P = int(rois.shape[0]), int(P)
        if out is None:
            out = torch.zeros(max(cap, 1), max(P, 1) ** 2, 64, dtype=torch.float32, device=self.device)
        if fb_flag is None:
            fb_flag = torch.zeros(max(cap, 1), dtype=torch.uint8, device=self.device)
        counts = torch.zeros(3, dtype=torch.int32, device=self.device)
        r_dev = self._i32(r)
        a = hip.RoiFeatsArgs(x0=x0.data_ptr(), x1=x1.data_ptr(), sem=sem.data_ptr(), x0sem=x0sem.data_ptr(), G2=G2.data_ptr(), G3=G3.data_ptr(),
                             rois=rois.data_ptr(), r_dev=r_dev.data_ptr(), B=int(x0.shape[0]), cap=cap, P=P,
                             H=(ctypes.c_int32 * 4)(*[int(m.shape[1]) for m in (x0, x1, G2, G3)]),
                             W=(ctypes.c_int32 * 4)(*[int(m.shape[2]) for m in (x0, x1, G2, G3)]),
                             out=out.data_ptr(), fb_flag=fb_flag.data_ptr(), counts=counts.data_ptr())
        self._check(self.lib.nuhtc_op_roi_feats(self.h, ctypes.byref(a), self._stream()))
        return dict(out=out, fb_flag=fb_flag, counts=counts)

    # ------------------------------------------------------------------ scoring on the device (csrc/eval.hip)
    def op_nucleus_pool(self, maps, strides, masks, pairs, W=None, n=None, out=None):
        """Per-nucleus embeddings on raw arrays (nuhtc_op_nucleus_pool; nuhtc_amd.nucfeat.pool_reference is the float64 restatement).
        maps: four contiguous float32 device tensors (B, h_l, w_l, 64); strides: four ints, mask pixels per map cell; masks: contiguous int32
        device tensor (B, K, H, (W + 31) // 32), bit x & 31 of word x >> 5 (W: the image width, default 32 x the words of a row); pairs: int32
        device tensor (n_max, 2) of (tile, slot); n: None (all n_max entries) or an int32 device tensor whose first element is the number of
        entries (read on the device); out: a contiguous float32 (n_max, 256) device tensor to write into (rows from n on stay as they
        are), a zero-filled one otherwise.  -> out.  Synchronous."""
        if len(maps) != 4 or len(strides) != 4:
            raise ValueError('op_nucleus_pool: four maps and four strides')
        B, K, H, wpr = (int(v) for v in masks.shape)
        W = wpr * 32 if W is None else int(W)
        n_max = int(pairs.shape[0])
        for t, dt in [(m, torch.float32) for m in maps] + [(masks, torch.int32), (pairs, torch.int32)]:
            if t.device != self.device or t.dtype != dt or not t.is_contiguous():
                raise ValueError('op_nucleus_pool: contiguous tensors on the engine\'s device (float32 maps, int32 masks and pairs)')
        if any(m.dim() != 4 or m.shape[0] != B or m.shape[3] != 64 for m in maps) or tuple(pairs.shape[1:]) != (2,) or (W + 31) // 32 != wpr:
            raise ValueError('op_nucleus_pool: maps (B, h, w, 64), pairs (n, 2), masks (B, K, H, (W + 31) // 32)')
        if out is None:
            out = torch.zeros(n_max, 256, dtype=torch.float32, device=self.device)
        if out.device != self.device or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (n_max, 256):
            raise ValueError('op_nucleus_pool: out must be a contiguous float32 (n_max, 256) tensor on the engine\'s device')
        ptrs = (ctypes.c_void_p * 4)(*[m.data_ptr() for m in maps])
        i4 = lambda v: (ctypes.c_int32 * 4)(*[int(a) for a in v])
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        self._check(self.lib.nuhtc_op_nucleus_pool(self.h, ptrs, i4([m.shape[1] for m in maps]), i4([m.shape[2] for m in maps]), i4(strides), B,
                                                   vp(masks), K, H, W, vp(pairs), vp(n) if n is not None else None, n_max, vp(out), self._stream()))
        return out

    def _op_nucleus_check(self, op, tiles, masks, pairs, W=None):
        """The tiles / masks / pairs of a mask-list op (`op`: the name in the messages) -> B, K, H, W, n_max.  tiles=None: the ops that read
        no tile; W is then the frame's width (None: 32 times the words of a row)."""
        lone = tiles is None
        kinds, forms = ('contiguous int32 masks and pairs on the engine\'s device', 'masks (B, K, H, (W + 31) // 32), pairs (n, 2)') if lone else \
                       ('contiguous tensors on the engine\'s device (uint8 tiles, int32 masks and pairs)', 'tiles (B, H, W, 3), masks (B, K, H, (W + 31) // 32), pairs (n, 2)')
        for t, dt in ((masks, torch.int32), (pairs, torch.int32)) + (() if lone else ((tiles, torch.uint8),)):
            if t.device != self.device or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f'{op}: {kinds}')
        if masks.dim() != 4 or tuple(pairs.shape[1:]) != (2,) or not (lone or (tiles.dim() == 4 and tiles.shape[3] == 3)):
            raise ValueError(f'{op}: {forms}')
        B, H, W = (int(masks.shape[0]), int(masks.shape[2]), int(masks.shape[3]) * 32 if W is None else int(W)) if lone else (int(v) for v in tiles.shape[:3])
        K, n_max = int(masks.shape[1]), int(pairs.shape[0])
        if tuple(masks.shape) != (B, K, H, (W + 31) // 32):
            raise ValueError(f'{op}: {forms}')
        return B, K, H, W, n_max

    def _op_nucleus_out(self, op, out, n_max, fields):
        """The output tensors of a per-nucleus op, one per (name, shape behind n_max, dtype) of `fields`: zero-filled ones for None, else
        checked."""
        if out is None:
            return tuple(torch.zeros(n_max, *tail, dtype=getattr(torch, dt), device=self.device) for _, tail, dt in fields)
        for t, (_, tail, dt) in zip(out, fields):
            if t.device != self.device or t.dtype != getattr(torch, dt) or not t.is_contiguous() or tuple(t.shape) != (n_max,) + tail:
                said = ', '.join(f'{dt} (n_max, {", ".join(str(v) for v in tail)})' for _, tail, dt in fields)
                raise ValueError(f'{op}: out must be ' + (f'a contiguous {said} tensor' if len(fields) == 1 else f'contiguous ({said}) tensors') + ' on the engine\'s device')
        return tuple(out)

    def _op_nucleus(self, fam, tiles, masks, pairs, W, channel_mode, n, out, ints=()):
        """One mask-list op on raw arrays: `fam`, the entry of ringfeat.FAMILIES, names the C entry and its output fields; the checks,
        the outputs and hip.op_nucleus.  -> the output tensor, or the tuple of them where the entry has several."""
        op, one = fam.call[len('nuhtc_'):], len(fam.fields) == 1
        B, K, H, W, n_max = self._op_nucleus_check(op, tiles, masks, pairs, W)
        outs = self._op_nucleus_out(op, (out,) if one and out is not None else out, n_max, fam.fields)
        self._check(hip.op_nucleus(self.lib, self.h, fam, (B, K, H, W), masks, pairs, outs, self._stream(), tiles,
                                   None if tiles is None else self._morph_constants(), channel_mode, n, ints))
        return outs[0] if one else outs

    def op_nucleus_morph(self, tiles, masks, pairs, channel_mode=hip.CH_AS_IS, n=None, out=None):
        """Per-nucleus morphometry integers on raw arrays (nuhtc_op_nucleus_morph; the numpy restatement is morph_reference of
        the module nuclei.MORPH draws on).  tiles: contiguous uint8 device tensor (B, H, W, 3); masks: contiguous int32 device tensor (B, K, H, (W + 31) // 32), bit
        x & 31 of word x >> 5; pairs: int32 device tensor (n_max, 2) of (tile, slot); channel_mode: which byte is red (CH_AS_IS: byte 0,
        CH_SWAP: byte 2); n: None (all n_max entries) or an int32 device tensor whose first element is the number of entries (read on the
        device); out: (raw int64 (n_max, 16), hist int32 (n_max, 256)) contiguous device tensors to write into (rows from n on stay as they
        are), zero-filled ones otherwise.  -> (raw, hist).  Synchronous."""
        return self._op_nucleus(ringfeat.MORPH, tiles, masks, pairs, None, channel_mode, n, out)

    def op_nucleus_texture(self, tiles, masks, pairs, channel_mode=hip.CH_AS_IS, n=None, out=None):
        """Per-nucleus grey-level co-occurrence counts on raw arrays (nuhtc_op_nucleus_texture; the numpy restatement is glcm_reference of
        the module nuclei.TEX draws on).  tiles, masks, pairs, channel_mode and n as in op_nucleus_morph; out: a contiguous int32 (n_max, 2, 136) device tensor to
        write into (rows from n on stay as they are), a zero-filled one otherwise.  -> out.  Synchronous."""
        return self._op_nucleus(ringfeat.TEX, tiles, masks, pairs, None, channel_mode, n, out)

    def op_nucleus_gradient(self, tiles, masks, pairs, channel_mode=hip.CH_AS_IS, edge_thr=1, n=None, out=None):
        """Per-nucleus gradient integers on raw arrays (nuhtc_op_nucleus_gradient; the numpy restatement is nuhtc_amd.nucgrad.grad_reference).
        tiles, masks, pairs, channel_mode and n as in op_nucleus_morph; edge_thr: the edge threshold T in quarter grey levels, 1 .. 1442;
        out: a contiguous int64 (n_max, 18) device tensor to write into (rows from n on stay as they are), a zero-filled one otherwise.
        -> out.  Synchronous."""
        return self._op_nucleus(ringfeat.GRADIENT, tiles, masks, pairs, None, channel_mode, n, out, (edge_thr,))

    def op_nucleus_shape(self, masks, pairs, W=None, n=None, out=None):
        """Per-nucleus shape integers on raw arrays (nuhtc_op_nucleus_shape; the numpy restatement is nuhtc_amd.nucshape.shape_reference).
        No tile is read.  masks: contiguous int32 device tensor (B, K, H, (W + 31) // 32), bit x & 31 of word x >> 5; W: the frame's width
        (None: 32 times the words of a row); pairs and n as in op_nucleus_morph; out: a contiguous int64 (n_max, 24) device tensor to write
        into (rows from n on stay as they are), a zero-filled one otherwise.  -> out.  Synchronous."""
        return self._op_nucleus(ringfeat.SHAPE, None, masks, pairs, W, hip.CH_AS_IS, n, out)

    def op_eval_select(self, scores, counts, masks, fg_thr, thr, labels=None):
        """Score filter + greedy mask-NMS of `WSIDataset.evaluate` (nuhtc_op_eval_select): scores (B, K) float32, counts (B,), masks
        (B, K, H, W // 32) int32 words on the device -> (sel (B, K) kept slots in visiting order, -1 behind them; nsel (B,); sel_labels)."""
        B, K, H, wpr = masks.shape
        scores, cnt = scores.contiguous().float(), self._i32(counts)
        dev = dict(dtype=torch.int32, device=self.device)
        sel, nsel = torch.zeros(B, K, **dev), torch.zeros(B, **dev)
        sl = torch.zeros(B, K, **dev) if labels is not None else None
        self._check(self.lib.nuhtc_op_eval_select(self.h, scores.data_ptr(), 1, cnt.data_ptr(), masks.data_ptr(),
                                                  labels.data_ptr() if labels is not None else None, B, K, H, wpr * 32, float(fg_thr), float(thr),
                                                  sel.data_ptr(), nsel.data_ptr(), sl.data_ptr() if sl is not None else None, self._stream()))
        return sel, nsel, sl

    def op_eval_pairs(self, masks, sel, nsel, gt_maps, t_cap, cap):
        """Pair tables (nuhtc_op_eval_pairs): gt_maps (B, H, W, C) int32 row + 1 maps -> dict(area_t (B, t_cap), area_p (B, K), trips (cap, 4):
        (tile, row, position in sel, pixels), n: entries the list needs, overflow, bad)."""
        B, K, H, wpr = masks.shape
        C = int(gt_maps.shape[3])
        dev = dict(dtype=torch.int32, device=self.device)
        r = dict(area_t=torch.zeros(B, t_cap, **dev), area_p=torch.zeros(B, K, **dev), trips=torch.full((cap + 8, 4), -7, **dev))
        counters = torch.zeros(4, **dev)
        self._check(self.lib.nuhtc_op_eval_pairs(self.h, masks.data_ptr(), sel.data_ptr(), nsel.data_ptr(), gt_maps.data_ptr(), B, K, H, wpr * 32, C,
                                                 int(t_cap), int(cap), r['area_t'].data_ptr(), r['area_p'].data_ptr(), r['trips'].data_ptr(),
                                                 counters.data_ptr(), self._stream()))
        c = counters.cpu().numpy()
        r.update(n=int(c[0]), overflow=bool(c[1]), bad=bool(c[2]), guard=r['trips'][cap:], trips=r['trips'][:cap])
        return r

    def op_eval_render(self, masks, sel, nsel, labels, C, data_format='pannuke'):
        """`convert_format` of the selected predictions (nuhtc_op_eval_render) -> (B, H, W, C + 1) ('pannuke') or (B, H, W, 2) ('conic') int32."""
        B, K, H, wpr = masks.shape
        fmt = hip.EVAL_PANNUKE if data_format == 'pannuke' else hip.EVAL_CONIC
        out = torch.empty(B, H, wpr * 32, C + 1 if fmt == hip.EVAL_PANNUKE else 2, dtype=torch.int32, device=self.device)
        self._check(self.lib.nuhtc_op_eval_render(self.h, masks.data_ptr(), sel.data_ptr(), nsel.data_ptr(), labels.data_ptr(), B, K, H, wpr * 32,
                                                  int(C), fmt, out.data_ptr(), self._stream()))
        return out

    def op_eval_joint(self, true_maps, pred_maps, C, cap):
        """Joint histograms of the PanNuke protocol (nuhtc_op_eval_joint): true_maps, pred_maps (B, H, W, >= C) int32 -> dict(joint (cap, 5):
        (tile, table, true id, pred id, pixels), n, overflow, bad)."""
        B, H, W, Ct = true_maps.shape
        dev = dict(dtype=torch.int32, device=self.device)
        joint, counters = torch.full((cap + 8, 5), -7, **dev), torch.zeros(4, **dev)
        self._check(self.lib.nuhtc_op_eval_joint(self.h, true_maps.data_ptr(), Ct, pred_maps.data_ptr(), int(pred_maps.shape[3]), B, H, W, int(C),
                                                 int(cap), joint.data_ptr(), counters.data_ptr(), self._stream()))
        c = counters.cpu().numpy()
        return dict(joint=joint[:cap], guard=joint[cap:], n=int(c[0]), overflow=bool(c[1]), bad=bool(c[2]))

    def eval_async(self, B, gt_maps_dev=None, t_cap=512, fg_thr=0.1, mask_nms_thr=0.05, data_format='pannuke', fetch_maps=True,
                   trip_cap=None, joint_cap=None):
        """After infer_async: enqueue, on the current stream, the scoring of the batch (nuhtc_eval_batch) -- score filter and mask-NMS,
        and from the kept predictions the pair tables against gt_maps_dev ((B, tile_h, tile_w, C) int32 row + 1 maps of
        evaluation.gt_rows, or None), the `convert_format` label maps and, for 'pannuke' with ground truth, the joint histograms of
        the PanNuke protocol -- and one copy of the tables (with fetch_maps also the label maps) into pinned host memory.  No host
        synchronisation; read with eval_read() once the stream has completed.
        Capacities: t_cap = ground-truth instances per tile (the caller's bound: tools size it to the fold); trip_cap / joint_cap = table
        entries per batch, by default 4 and 8 per instance the batch may hold (4 * n * max_batch, 8 * n * max_batch with n = max(t_cap, 128): a
        prediction meets one or two instances, and a joint entry exists per instance, per prediction and per meeting pair, in its class
        table and in the binarised one); a batch over them is flagged and scored through its masks.  The copy has a fixed size -- the
        capacities, whatever the batch holds, since its size must be known here, before the counts exist on the host: that is why the
        capacities follow t_cap and not max_per_img (up to t_cap = 128: 0.46 MB of pairs and joint entries per batch of 16, beside the
        1.5 MB label map per tile that fetch_maps copies)."""
        K, H, W, C = self.cfg.max_per_img, self.cfg.tile_h, self.cfg.tile_w, self.cfg.num_classes
        mb = self.cfg.max_batch
        fmt = hip.EVAL_PANNUKE if data_format == 'pannuke' else hip.EVAL_CONIC
        CO = C + 1 if fmt == hip.EVAL_PANNUKE else 2
        per_tile = max(int(t_cap), 128)
        trip_cap = int(trip_cap or 4 * per_tile * mb)
        joint_cap = int(joint_cap or 8 * per_tile * mb)
        key = (int(t_cap), trip_cap, joint_cap, CO, bool(fetch_maps))
        ev = getattr(self, '_ev', None)
        if ev is None or ev['key'] != key:
            names = dict(counters=(8,), nsel=(mb,), sel=(mb, K), sel_labels=(mb, K), area_p=(mb, K), area_t=(mb, t_cap), trips=(trip_cap, 4),
                         joint=(joint_cap, 5))
            if fetch_maps:
                names['maps'] = (mb, H, W, CO)
            offs, total = {}, 0
            for k, sh in names.items():          # every table is a view into ONE int32 device buffer and ONE pinned host buffer: one copy per batch
                offs[k] = total
                total += (int(np.prod(sh)) + 63) // 64 * 64
            with torch.cuda.device(self.device):
                blob_dev = torch.zeros(total, dtype=torch.int32, device=self.device)
                maps_dev = None if fetch_maps else torch.zeros(mb, H, W, CO, dtype=torch.int32, device=self.device)
            blob_hosts = [torch.zeros(total, dtype=torch.int32).pin_memory() for _ in range(self.EXPORT_BUFFERS)]
            view = lambda blob, k: blob[offs[k]:offs[k] + int(np.prod(names[k]))].view(*names[k])
            ev = self._ev = dict(key=key, blob_dev=blob_dev, blob_hosts=blob_hosts, turn=0, dev={k: view(blob_dev, k) for k in names},
                                 hosts=[{k: view(b, k) for k in names} for b in blob_hosts], small=offs.get('maps', total),
                                 meta=[None] * self.EXPORT_BUFFERS)
            if not fetch_maps:
                ev['dev']['maps'] = maps_dev
        d = ev['dev']
        if gt_maps_dev is not None and (tuple(gt_maps_dev.shape) != (B, H, W, C) or gt_maps_dev.dtype != torch.int32 or not gt_maps_dev.is_contiguous()):
            raise ValueError(f'eval_async: gt_maps_dev must be a contiguous int32 {(B, H, W, C)} device tensor')
        self._ev_gt = gt_maps_dev          # (kept alive until the next call)
        a = hip.EvalArgs(gt_maps=gt_maps_dev.data_ptr() if gt_maps_dev is not None else None, t_cap=int(t_cap), trip_cap=trip_cap, joint_cap=joint_cap,
                         format=fmt, fg_thr=float(fg_thr), mask_nms_thr=float(mask_nms_thr), **{k: d[k].data_ptr() for k in
                         ('sel', 'nsel', 'sel_labels', 'area_t', 'area_p', 'trips', 'joint', 'counters')}, pred_maps=d['maps'].data_ptr())
        self._check(self.lib.nuhtc_eval_batch(self.h, ctypes.byref(self.dets), B, ctypes.byref(a), self._stream()))
        ev['turn'] = (ev['turn'] + 1) % self.EXPORT_BUFFERS
        n = ev['small'] + (B * H * W * CO if fetch_maps else 0)          # the tables, and the label maps of the B tiles behind them
        ev['blob_hosts'][ev['turn']][:n].copy_(ev['blob_dev'][:n], non_blocking=True)
        ev['meta'][ev['turn']] = dict(B=B, has_gt=gt_maps_dev is not None, fmt=fmt)          # what eval_read(turn) needs to slice that buffer
        return ev['turn']

    def eval_read(self, turn=None):
        """Tables of the batch eval_async scored, as numpy (call after the stream has completed): dict(nsel (B,), labels: per tile the labels
        of the kept predictions in visiting order, slots: their detection slots, maps (B, tile_h, image width, C + 1 | 2) int32 or None,
        and with ground truth area_t (B, t_cap), area_p: per tile (n_p,), pairs: per tile (rows, positions, pixels), joint: per tile the
        C + 1 tables (true ids, pred ids, pixels) of evaluation.pannuke_stats_tables ('pannuke' only), overflow: a table did not fit its
        capacity -- score the batch on the host then).  Raises when a ground-truth map held a value outside [0, t_cap].
        `turn` selects the buffer of an earlier eval_async (its return value).  Everything returned is a copy except `maps`, a VIEW of the
        pinned buffer (1.5 MB per tile: the caller converts or copies what it keeps): like the views of export_read it stays valid through
        the next TWO eval_async calls of this engine (EXPORT_BUFFERS = 3 buffers used in turn), not the one after those, and all buffers
        are replaced when a call changes a capacity or the format."""
        ev = self._ev
        turn = ev['turn'] if turn is None else turn
        h, meta = ev['hosts'][turn], ev['meta'][turn]
        B, C = meta['B'], self.cfg.num_classes
        cnt = h['counters'].numpy()
        if cnt[2] or cnt[6]:
            raise HipError('eval: a ground-truth map holds a value outside [0, t_cap] (evaluation.gt_rows numbers the rows; raise t_cap)')
        nsel = h['nsel'][:B].numpy().copy()
        out = dict(nsel=nsel, slots=[h['sel'][b, :nsel[b]].numpy().copy() for b in range(B)],
                   labels=[h['sel_labels'][b, :nsel[b]].numpy().astype(int) for b in range(B)],
                   maps=h['maps'][:B, :, :self.image_hw[1]].numpy() if 'maps' in h else None, overflow=False)
        if not meta['has_gt']:
            return out
        out['overflow'] = bool(cnt[1] or cnt[5] or cnt[0] > h['trips'].shape[0] or cnt[4] > h['joint'].shape[0])
        if out['overflow']:
            return out
        tr = h['trips'][:int(cnt[0])].numpy()
        order = np.argsort(tr[:, 0], kind='stable')
        tr = tr[order]
        cut = np.searchsorted(tr[:, 0], np.arange(B + 1))
        out['pairs'] = [(tr[cut[b]:cut[b + 1], 1], tr[cut[b]:cut[b + 1], 2], tr[cut[b]:cut[b + 1], 3]) for b in range(B)]
        out['area_t'] = h['area_t'][:B].numpy().copy()
        out['area_p'] = [h['area_p'][b, :nsel[b]].numpy().copy() for b in range(B)]
        if meta['fmt'] == hip.EVAL_PANNUKE:
            jt = h['joint'][:int(cnt[4])].numpy()
            key = jt[:, 0].astype(np.int64) * (C + 1) + jt[:, 1]
            jt = jt[np.argsort(key, kind='stable')]
            cut = np.searchsorted(np.sort(key, kind='stable'), np.arange(B * (C + 1) + 1))
            out['joint'] = [[(jt[cut[b * (C + 1) + k]:cut[b * (C + 1) + k + 1], 2], jt[cut[b * (C + 1) + k]:cut[b * (C + 1) + k + 1], 3],
                              jt[cut[b * (C + 1) + k]:cut[b * (C + 1) + k + 1], 4]) for k in range(C + 1)] for b in range(B)]
        return out

    # ------------------------------------------------------------------ scoring images larger than a tile (csrc/stitch.hip)
    def stitch_store(self, n_img, cand_cap=8192, pool_cap=1 << 20, slots=None, guard=0):
        """Device buffers for the candidates of n_img images (nuhtc_stitch_store): cand_cap records and pool_cap crop words per image, scratch
        for `slots` detection slots per gather (default: max_batch * max_per_img).  `guard`: extra elements behind every buffer, and every
        buffer filled with -7, for the tests that check nothing is written at or past a capacity."""
        slots = int(slots or self.cfg.max_batch * self.cfg.max_per_img)
        n_img, cand_cap, pool_cap = int(n_img), int(cand_cap), int(pool_cap)
        fill = -7 if guard else 0
        mk = lambda n, dt: torch.full((n + guard,), fill, dtype=dt, device=self.device)
        t = dict(box=mk(n_img * cand_cap * 4, torch.int32), area=mk(n_img * cand_cap, torch.int32), score=mk(n_img * cand_cap, torch.float32),
                 label=mk(n_img * cand_cap, torch.int32), key=mk(n_img * cand_cap, torch.int64), off=mk(n_img * cand_cap, torch.int64),
                 pool=mk(n_img * pool_cap, torch.int32), work=mk(slots * 8, torch.int32),
                 counters=torch.zeros(n_img * 4, dtype=torch.int32, device=self.device))
        st = hip.StitchStore(n_img=n_img, cand_cap=cand_cap, pool_cap=pool_cap, work_cap=slots * 8, **{k: v.data_ptr() for k, v in t.items()})
        return dict(t, struct=st, n_img=n_img, cand_cap=cand_cap, pool_cap=pool_cap)

    def stitch_reset(self, store, image=None):
        """Starts image slot `image` (all slots: None) of a store afresh, on the current stream."""
        c = store['counters'].view(-1, 4)
        (c if image is None else c[image]).zero_()

    def op_stitch_gather(self, boxes, labels, counts, masks, meta, C, store, fg_thr=0.1, discard_offset=4):
        """nuhtc_op_stitch_gather on raw device arrays: boxes (B, K, 5) float32, labels (B, K), counts (B,), masks (B, K, T, T // 32) int32
        words, meta (B, 8) int32 (stitch.tile_meta)."""
        B, K, T, _ = masks.shape
        boxes, meta = boxes.contiguous().float(), self._i32(meta)
        self._check(self.lib.nuhtc_op_stitch_gather(self.h, boxes.data_ptr(), self._i32(labels).data_ptr(), self._i32(counts).data_ptr(), masks.data_ptr(),
                                                    meta.data_ptr(), B, K, T, int(C), float(fg_thr), float(discard_offset),
                                                    ctypes.byref(store['struct']), self._stream()))

    def stitch_gather_async(self, B, meta_dev, store, fg_thr=0.1, discard_offset=4):
        """After infer_async, on the current stream and without synchronising: the detections of the batch's tiles that pass the candidate
        rules of the stitched protocol are appended to their images in `store` (nuhtc_stitch_gather).  meta_dev: (B, 8) int32 device tensor
        of stitch.tile_meta records."""
        if tuple(meta_dev.shape) != (B, 8) or meta_dev.dtype != torch.int32 or not meta_dev.is_contiguous():
            raise ValueError('stitch_gather_async: meta_dev must be a contiguous int32 (B, 8) device tensor')
        self._stitch_meta = meta_dev          # (kept alive until the next call)
        self._check(self.lib.nuhtc_stitch_gather(self.h, ctypes.byref(self.dets), B, meta_dev.data_ptr(), float(fg_thr), float(discard_offset),
                                                 ctypes.byref(store['struct']), self._stream()))

    def stitch_read(self, store, image):
        """The candidate records of a gathered image as numpy, in the REFERENCE's candidate order (tile location, class, slot): dict(n,
        need = (candidates, pool words) the image needs, overflow, dev: the device number of each candidate, box, area, score, label, off).
        Synchronises.  Raises when a label or tile record was out of range."""
        cnt = store['counters'].view(-1, 4)[image].cpu().numpy()
        if cnt[3]:
            raise HipError('stitch: a label outside [0, num_classes) or a tile record out of range')
        cap = store['cand_cap']
        n = int(min(max(cnt[0], 0), cap))
        sl = slice(image * cap, image * cap + n)
        order = np.argsort(store['key'][sl].cpu().numpy(), kind='stable')
        f = lambda k: store[k][sl].cpu().numpy()[order]
        return dict(n=n, need=(int(cnt[0]), int(cnt[1])), overflow=bool(cnt[2]) or cnt[0] > cap or cnt[1] > store['pool_cap'], dev=order.astype(np.int32),
                    box=store['box'][image * cap * 4:(image * cap + n) * 4].view(-1, 4).cpu().numpy()[order].astype(np.int64), area=f('area').astype(np.int64),
                    score=f('score'), label=f('label').astype(int), off=f('off'))

    def stitch_nms(self, store, image, rec, thr, height, width):
        """The image-level mask-NMS on the device: nuhtc_merge_overlap(NUHTC_OVERLAP_MASK) over the image's crops.  Its tie rule is lower
        index first and the evaluation's is higher candidate index first, so the records are fed in reversed candidate order.  An empty mask
        overlaps nothing and is kept (merge_overlap never keeps one, so they stay out of its input).  thr >= 0.
        -> kept candidates, as indices into `rec`, in visiting order (descending score, ties descending index)."""
        if not thr >= 0:
            raise ValueError('stitch_nms: the threshold must not be negative')
        n = rec['n']
        alive = rec['area'] == 0
        idx = np.nonzero(~alive)[0][::-1]          # reversed candidate order
        if len(idx):
            dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(self.device)
            keep = torch.zeros(len(idx), dtype=torch.uint8, device=self.device)
            pool = store['pool'][image * store['pool_cap']:(image + 1) * store['pool_cap']]
            boxes, scores, areas, offs = dev(rec['box'][idx], torch.int32), dev(rec['score'][idx], torch.float32), dev(rec['area'][idx], torch.int32), dev(rec['off'][idx], torch.int64)
            rc = self.lib.nuhtc_merge_overlap(self.device.index, boxes.data_ptr(), scores.data_ptr(), areas.data_ptr(), pool.data_ptr(), offs.data_ptr(),
                                              len(idx), store['pool_cap'], hip.OVERLAP_MASK, float(thr), 0, 0, int(width), int(height), keep.data_ptr(),
                                              self._stream())
            if rc:
                raise HipError(f'nuhtc_merge_overlap failed ({rc})')
            alive[idx[keep.cpu().numpy().astype(bool)]] = True
        order = np.argsort(rec['score'], kind='stable')[::-1]
        return order[alive[order]] if n else np.zeros(0, int)

    def _stitch_kept(self, rec, kept):
        return torch.as_tensor(np.ascontiguousarray(rec['dev'][kept]).astype(np.int32)).to(self.device) if len(kept) else torch.zeros(1, dtype=torch.int32, device=self.device)

    def stitch_pairs(self, store, image, rec, kept, gt_map_dev, t_cap, trip_cap, guard=0):
        """Pair tables of the kept predictions of an image against its ground-truth map (nuhtc_op_stitch_pairs): gt_map_dev (H, W) int32 row + 1
        -> dict(area_t (t_cap,), pairs (rows, positions, pixels), n: entries needed, overflow: entries dropped or a prediction with more than
        64 partners, partners: the latter alone).  Raises on a value out of range.  Synchronises."""
        H, W = gt_map_dev.shape
        dev = dict(dtype=torch.int32, device=self.device)
        area_t, trips, counters = torch.zeros(int(t_cap), **dev), torch.full((int(trip_cap) + guard, 3), -7, **dev), torch.zeros(4, **dev)
        k = self._stitch_kept(rec, kept)
        self._check(self.lib.nuhtc_op_stitch_pairs(self.h, ctypes.byref(store['struct']), int(image), k.data_ptr(), len(kept), gt_map_dev.data_ptr(), H, W,
                                                   int(t_cap), int(trip_cap), area_t.data_ptr(), trips.data_ptr(), counters.data_ptr(), self._stream()))
        c = counters.cpu().numpy()
        if c[2]:
            raise HipError('stitch_pairs: a ground-truth value outside [0, t_cap], or a candidate record out of range')
        tr = trips[:min(int(c[0]), int(trip_cap))].cpu().numpy()
        return dict(area_t=area_t.cpu().numpy(), pairs=(tr[:, 0], tr[:, 1], tr[:, 2]), n=int(c[0]), overflow=bool(c[1] or c[3] or c[0] > trip_cap),
                    partners=bool(c[3]), guard=trips[int(trip_cap):])

    def stitch_render(self, store, image, rec, kept, height, width):
        """inst_map, type_map (H, W) int32 device tensors of the kept predictions (nuhtc_op_stitch_render).  Synchronises."""
        dev = dict(dtype=torch.int32, device=self.device)
        inst, typ, counters = torch.empty(height, width, **dev), torch.empty(height, width, **dev), torch.zeros(4, **dev)
        k = self._stitch_kept(rec, kept)
        self._check(self.lib.nuhtc_op_stitch_render(self.h, ctypes.byref(store['struct']), int(image), k.data_ptr(), len(kept), int(height), int(width),
                                                    inst.data_ptr(), typ.data_ptr(), counters.data_ptr(), self._stream()))
        if int(counters[2]):
            raise HipError('stitch_render: a candidate record out of range')
        return inst, typ
