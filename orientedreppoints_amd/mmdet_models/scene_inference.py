"""Whole-scene detection: a DOTA scene (thousands of pixels a side) in, merged scene-coordinate detections per class out,
with the scene uploaded once as uint8 and every later step on the device.

Replaces the reference's chain `DOTA_devkit/SplitOnlyImage.py` (patches to files) -> `tools/test.py` (per-patch pipeline on the
host, results to a pickle) -> `tools/parse_pkl/parse_pkl_mege_results_for_dota_evaluation.py` (Task1 text files per class) ->
`DOTA_devkit/ResultMerge_multi_process.py:mergebypoly` (parse, translate, NMS per class):

    tile plan (`dota_devkit.img_split`)  ->  `orp_scene_tiles` / `orp_scene_tiles_resized` straight into a captured graph's
    input buffer  ->  graph replay (`PipelinedInference`)  ->  packed results stay on the device  ->  `orp_scene_collect`
    ->  one `orp_poly_nms_f64_batched`  ->  one gather, one D2H.

With `views` (test-time flip / multi-scale augmentation) every tile batch fills all of its views -- `orp_scene_tiles_flip` /
`orp_scene_tiles_resized_flip` for the mirrored ones -- and replays one augmented graph (`PipelinedAugInference`).
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from ..dota_devkit.img_split import scaled_size, split_origins
from ..mmdet_ops.nms_wrapper import poly_nms_f64_batched_device
from ..mmdet_datasets.imops import rescale_size
from ..mmdet_ops.scene_ops import (resize_tables, scene_collect, scene_tiles, scene_tiles_flip, scene_tiles_resized,
                                   scene_tiles_resized_flip)
from .graph_inference import PipelinedAugInference, PipelinedInference

DOTA_CLASSES = ('plane', 'baseball-diamond', 'bridge', 'ground-track-field', 'small-vehicle', 'large-vehicle', 'ship',
                'tennis-court', 'basketball-court', 'storage-tank', 'soccer-ball-field', 'roundabout', 'harbor',
                'swimming-pool', 'helicopter')


class _Plan(object):
    """One scene's work: per rate the (resampled) uint8 scene, the tile origins (host list and padded device tensor), the
    patch shape's entry (`_Shape`; None = the native-size route) and, once the tiles ran, the packed results
    [Tpad, m + 1, 28]."""

    def __init__(self):
        self.rates, self.scenes, self.origins, self.origins_dev, self.packed, self.shapes = [], [], [], [], [], []


class _Shape(object):
    """What the patches of one shape go through under `img_scale`: src = (w, h) of a patch, new = (w, h) after the resize,
    pad = (w, h) of the detector's input, the scale factor, the metas the host pipeline would set, and (once captured) the
    graphs of that input shape.  `img_scale=None` (a native-size view of `_AugShape`): no resize, scale factor 1."""

    def __init__(self, src, img_scale, divisor, batch):
        self.src = (int(src[0]), int(src[1]))
        new_w, new_h, self.scale_factor = (self.src + (1.0,)) if img_scale is None else rescale_size(self.src, img_scale)
        self.new = (new_w, new_h)
        self.pad = (-(-new_w // divisor) * divisor, -(-new_h // divisor) * divisor)
        # an identity resize of a square patch the divisor leaves alone: `orp_scene_tiles`' case
        self.native = self.new == self.src == self.pad and self.src[0] == self.src[1]
        self.metas = [dict(img_shape=(new_h, new_w, 3), pad_shape=(self.pad[1], self.pad[0], 3),
                           scale_factor=self.scale_factor, flip=False) for _ in range(batch)]
        self.pipe = self.tables = None


class _AugShape(object):
    """The views of the patches of one shape (`views=`): per view its `_Shape` and flip flag, the metas `aug_test` takes (per
    view, one per tile of a batch) and, once captured, the augmented graphs of these input shapes."""

    def __init__(self, shapes, flips):
        self.views = list(zip(shapes, flips))
        self.metas = [[dict(m, flip=bool(f)) for m in sh.metas] for sh, f in self.views]
        self.pipe = None


class SceneInference(object):
    """`si = SceneInference(model, subsize=1024, gap=200, rates=(1.0,), batch=1, depth=4, img_scale=None); per_class = si(scene)`;
    `SceneInference.from_config(model, cfg)` takes `img_scale`, the normalisation and the pad divisor from a config's test
    pipeline.

    scene: uint8 [H, W, 3] numpy array or tensor (host or device), BGR as `cv2.imread` gives it.  Returns one float64 [k, 9]
    array per class (8 scene coordinates + score) in the merge's visiting order -- the lines `mergesingle` would write;
    `write_task1` writes them.

    * Tiles are those of `SplitSingle` (`img_split.split_origins`: same origins, same order) for every rate; `batch` tiles run
      per captured graph, `depth` graphs in flight (`PipelinedInference`, whose half-model guard applies).  The last, partly
      filled batch repeats its last tile; the repeats are not collected.
    * `img_scale=None`: patches are fed at scale factor 1, normalised (`imnormalize` with `mean`, `std`, `to_rgb`, bit for
      bit) and nothing else.  That is the reference's test pipeline for 1024^2 patches under `orientedrepoints_r50_demo.py`
      (`img_scale=(1333, 1024)`).
    * `img_scale=(long edge, short edge)`, e.g. `(1333, 960)` of the R-101 and Swin-T configs: the test pipeline's
      `RotateResize(keep_ratio=True)` -> `Normalize` -> `Pad(size_divisor)` per patch, on the device.  A patch is
      `(min(W, subsize), min(H, subsize))` (what `SplitOnlyImage` writes for a small scene: it does not pad); it is resized
      to `imops.rescale_size(patch, img_scale)` by `orp_scene_tiles_resized` (bilinear, `align_corners=False`, rounded to
      uint8, in the fp32 arithmetic DESIGN.md fixes: within one grey level of `imops.imresize` on at most 1e-3 of the pixels,
      the band in which torch's own CPU resize differs between thread counts), padded with zeros to the divisor, and the
      graphs divide boxes and rep-points by the scale factor before the NMS (`rescale=True`), so their rows are in patch
      coordinates as the file route's are.  Graphs are kept per patch shape (four shapes, oldest dropped).  A patch
      whose resize is the identity goes through `orp_scene_tiles`.
    * `views=[(img_scale or None, flip), ...]` (at most 8): flip and multi-scale test augmentation, `MultiScaleFlipAug`'s views of
      every patch in its own order -- `from_config(model, cfg, aug=True)` reads them from the config.  Every tile batch fills all of
      its views on the device (a view's scale as `img_scale` above, None = native size; a flipped view is mirrored after its resize,
      inside the resized patch's own width, as `RandomFlip` between `RotateResize` and `Normalize` does) and replays ONE augmented
      graph: all views' forwards, the candidates mapped back to the patch, one rotated NMS over their union -- `aug_test`, bit
      for bit.  Its rows are in patch coordinates and go through the same collect and merge.  Rates and views compose: every rate
      runs all views.  Not to be combined with `img_scale`.  An overflowed tile is re-run through `model.aug_test`.
    * rates != 1: the scene is resampled once on the device with torch's bicubic `interpolate` (`align_corners=False`),
      rounded and clamped to uint8, to `img_split.scaled_size`.  This follows OpenCV's conventions but is NOT checked against
      cv2's `INTER_CUBIC` pixels.  The rate used in coordinates is `float(str(rate))`, as the patch-name grammar implies.
    * A tile whose packed result overflowed (`static_capacity`) is re-run, with the tiles of its batch, through
      `model.simple_test_batch`, and its rows take that tile's place in the order.
    * One difference from the file route: the reference writes patch results with `str(float32)` (shortest decimal) and
      parses them back as doubles, which is not the widened fp32 value (up to half an fp32 ulp away).  Here every fp32
      coordinate and score is widened exactly.  Keep decisions can differ from a files-based run only for pairs whose IoU is
      within that distance of the threshold.

    Raises ValueError for `subsize % 32 != 0` (the pipeline's `Pad(size_divisor=32)` would change the patch), for a model
    `GraphedInference` refuses (training mode, no static rnms post-processing), and -- per scene, with `img_scale=None` -- for
    a scaled scene with a side below `subsize` (the reference pipeline would upscale such a patch through
    `RotateResize(keep_ratio)`: set `img_scale`).  Segments above `ORP_NMS_MAX_BOXES` raise `OrpHipError` in the merge."""

    def __init__(self, model, subsize=1024, gap=200, rates=(1.0,), batch=1, depth=4, nms_thresh=0.1,
                 mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), to_rgb=True, img_scale=None, size_divisor=32,
                 views=None):
        subsize, gap, batch, depth = int(subsize), int(gap), int(batch), int(depth)
        if subsize <= 0 or subsize % 32 != 0:
            raise ValueError("SceneInference: subsize (%d) must be a positive multiple of 32, the test pipeline's Pad divisor" % subsize)
        if img_scale is not None:
            img_scale = tuple(int(v) for v in img_scale)
            if len(img_scale) != 2 or min(img_scale) <= 0:
                raise ValueError("SceneInference: img_scale must be None or two positive edge bounds, e.g. (1333, 960)")
        self.img_scale, self.size_divisor = img_scale, int(size_divisor)
        self.views = None if views is None else self._check_views(views)
        if self.views is not None and img_scale is not None:
            raise ValueError("SceneInference: give the scales in views, not in img_scale as well")
        if self.size_divisor <= 0 or self.size_divisor % 8 != 0:
            raise ValueError("SceneInference: size_divisor must be a positive multiple of 8 (16 bytes of an output row per lane)")
        if not 0 <= gap < subsize:
            raise ValueError("SceneInference: gap (%d) must be in [0, subsize)" % gap)
        if batch < 1 or depth < 1 or len(rates) == 0:
            raise ValueError("SceneInference: batch, depth and the number of rates must be at least 1")
        if getattr(model, 'training', False):
            raise ValueError("SceneInference: the model must be in eval mode (GraphedInference refuses a training-mode model)")
        cfg = model.test_cfg
        if cfg.nms.get('type', 'rnms') != 'rnms' or not cfg.get('static_postprocess', True):
            raise ValueError("SceneInference: the model's test_cfg must use the static rnms post-processing (GraphedInference needs it)")
        self.model, self.subsize, self.gap, self.batch, self.depth = model, subsize, gap, batch, depth
        self.rates = [(r, float(str(r))) for r in rates]
        if any(not v > 0 for _, v in self.rates):
            raise ValueError("SceneInference: rates must be positive")
        self.nms_thresh = float(nms_thresh)
        self.mean, self.std, self.to_rgb = np.asarray(mean, np.float32), np.asarray(std, np.float32), bool(to_rgb)
        self.num_classes = model.bbox_head.num_classes - 1
        self.metas = [dict(img_shape=(subsize, subsize, 3), pad_shape=(subsize, subsize, 3), scale_factor=1.0, flip=False)
                      for _ in range(batch)]
        self.pipe = None                           # the native-size graphs (img_scale=None)
        self._shapes = {}                          # (width, height) of a patch -> _Shape (img_scale set; at most 4)
        self._aug_shapes = {}                      # (width, height) of a patch -> _AugShape (views set; at most 4)
        self._origins = {}                         # (width, height) of a scaled scene -> (host list, padded device tensor)
        self.fallback_tiles = 0                    # tiles re-run because their packed result overflowed (all calls)

    @staticmethod
    def _check_views(views):
        """views -> [(img_scale tuple or None, flip bool)]; ValueError for anything else."""
        out = []
        if not isinstance(views, (list, tuple)) or not 1 <= len(views) <= 8:
            raise ValueError("SceneInference: views must be a list of 1 to 8 (img_scale or None, flip) pairs")
        for v in views:
            if not isinstance(v, (list, tuple)) or len(v) != 2 or not isinstance(v[1], (bool, np.bool_)):
                raise ValueError("SceneInference: a view is (img_scale or None, flip), got %r" % (v,))
            scale = v[0]
            if scale is not None:
                if not isinstance(scale, (list, tuple)) or len(scale) != 2 or \
                        not all(isinstance(e, (int, np.integer)) and e > 0 for e in scale):
                    raise ValueError("SceneInference: a view's img_scale must be None or two positive edge bounds, got %r" % (scale,))
                scale = (int(scale[0]), int(scale[1]))
            out.append((scale, bool(v[1])))
        return out

    @classmethod
    def from_config(cls, model, cfg, aug=False, **kw):
        """`SceneInference(model, ...)` with `img_scale`, `mean`, `std`, `to_rgb` and `size_divisor` read from
        `cfg.data.test.pipeline` (`MultiScaleFlipAug` around `RotateResize` / `Normalize` / `Pad`); keywords override.  With
        `aug=True` the pipeline's `flip` and scale list become `views`, in `MultiScaleFlipAug`'s order: for each scale the plain
        view, then the flipped one if `flip`.  Raises ValueError for a pipeline this class does not reproduce: without `aug=True`,
        `flip=True` or more than one scale; always `keep_ratio=False`, an interpolation other than bilinear, a fixed-size `Pad`."""
        want_aug = bool(aug)
        aug = [t for t in cfg.data.test.pipeline if t['type'] == 'MultiScaleFlipAug']
        if len(aug) != 1:
            raise ValueError("SceneInference.from_config: the test pipeline must hold one MultiScaleFlipAug")
        aug = aug[0]
        scales = aug['img_scale'] if isinstance(aug['img_scale'], list) else [aug['img_scale']]
        flip = bool(aug.get('flip', False))
        if want_aug:
            got = dict(views=[(tuple(sc), f) for sc in scales for f in ((False, True) if flip else (False,))])
        else:
            if flip:
                raise ValueError("SceneInference.from_config: flip=True (test-time flip augmentation) is not reproduced")
            if len(scales) != 1:
                raise ValueError("SceneInference.from_config: %d test scales (multi-scale augmentation) are not reproduced" % len(scales))
            got = dict(img_scale=tuple(scales[0]))
        for t in aug['transforms']:
            if t['type'] in ('RotateResize', 'Resize', 'PolyResize'):
                if not t.get('keep_ratio', True):
                    raise ValueError("SceneInference.from_config: keep_ratio=False (a per-axis scale factor) is not reproduced")
                if t.get('interpolation', 'bilinear') != 'bilinear':
                    raise ValueError("SceneInference.from_config: interpolation=%r is not reproduced (bilinear only)" % (t['interpolation'],))
            elif t['type'] == 'Normalize':
                got.update(mean=tuple(t['mean']), std=tuple(t['std']), to_rgb=t.get('to_rgb', True))
            elif t['type'] == 'Pad':
                if t.get('size') is not None or t.get('size_divisor') is None:
                    raise ValueError("SceneInference.from_config: Pad to a fixed size is not reproduced")
                got.update(size_divisor=t['size_divisor'])
        got.update(kw)
        return cls(model, **got)

    # ---- the three stages of a call ------------------------------------------------------------------------------------------
    def tile_shapes(self, W, H):
        """Host-side planning of a W x H scene: per rate ((w, h) of the scaled scene, its patches' `_Shape` or None for the
        native-size route).  Raises the ValueError of a scene smaller than a tile when `img_scale` is None."""
        out = []
        for r, v in self.rates:
            w, h = (W, H) if v == 1.0 else scaled_size(W, H, v)
            if self.views is not None:
                out.append(((w, h), self._aug_shape(r, w, h)))
                continue
            if self.img_scale is None:
                if min(w, h) < self.subsize:
                    raise ValueError("SceneInference: the scene at rate %s is %d x %d, smaller than a %d tile (the reference "
                                     "would upscale such a patch: set img_scale)" % (r, w, h, self.subsize))
                out.append(((w, h), None))
                continue
            if min(w, h) < 1:
                raise ValueError("SceneInference: the scene at rate %s is empty" % r)
            src = (min(w, self.subsize), min(h, self.subsize))
            if src not in self._shapes:
                if len(self._shapes) >= 4:
                    self._shapes.pop(next(iter(self._shapes)))
                self._shapes[src] = _Shape(src, self.img_scale, self.size_divisor, self.batch)
            out.append(((w, h), self._shapes[src]))
        return out

    def _aug_shape(self, r, w, h):
        """The `_AugShape` of the patches of a w x h scaled scene (views of one scale share a `_Shape`)."""
        if min(w, h) < 1:
            raise ValueError("SceneInference: the scene at rate %s is empty" % r)
        if min(w, h) < self.subsize and any(sc is None for sc, _ in self.views):
            raise ValueError("SceneInference: the scene at rate %s is %d x %d, smaller than a %d tile (the reference would "
                             "upscale such a patch: give the native-size views an img_scale)" % (r, w, h, self.subsize))
        src = (min(w, self.subsize), min(h, self.subsize))
        if src not in self._aug_shapes:
            if len(self._aug_shapes) >= 4:
                self._aug_shapes.pop(next(iter(self._aug_shapes)))
            per_scale = {}
            for sc, _ in self.views:
                if sc not in per_scale:
                    per_scale[sc] = _Shape(src, sc, self.size_divisor, self.batch)
            self._aug_shapes[src] = _AugShape([per_scale[sc] for sc, _ in self.views], [f for _, f in self.views])
        return self._aug_shapes[src]

    def prepare(self, scene):
        """Upload (if needed), resample per rate, plan the tiles, capture the graphs on first use.  Returns the plan."""
        if isinstance(scene, np.ndarray):
            scene = torch.from_numpy(np.ascontiguousarray(scene))
        if scene.dtype != torch.uint8 or scene.dim() != 3 or scene.size(2) != 3:
            raise ValueError("SceneInference: scene must be uint8 [H, W, 3]")
        H, W = int(scene.size(0)), int(scene.size(1))
        planned = self.tile_shapes(W, H)
        sizes = [size for size, _ in planned]
        p = next(self.model.parameters())
        if not p.is_cuda:
            raise ValueError("SceneInference: the model must be on a GPU")
        dev = p.device
        scene = scene.to(dev)
        if scene.stride(2) != 1 or scene.stride(1) != 3:
            scene = scene.contiguous()
        plan = _Plan()
        for (r, v), (w, h) in zip(self.rates, sizes):
            plan.rates.append(v)
            plan.scenes.append(scene if (w, h) == (W, H) else self._resample(scene, w, h))
            if (w, h) not in self._origins:
                if len(self._origins) >= 16:
                    self._origins.pop(next(iter(self._origins)))
                host = split_origins(w, h, self.subsize, self.gap)
                padded = host + [host[-1]] * (-len(host) % self.batch)
                self._origins[(w, h)] = (host, torch.tensor(padded, dtype=torch.int32).to(dev))
            host, on_dev = self._origins[(w, h)]
            plan.origins.append(host)
            plan.origins_dev.append(on_dev)
        for _, shape in planned:
            plan.shapes.append(shape)
            if isinstance(shape, _AugShape):
                if shape.pipe is None:
                    imgs = [torch.zeros((self.batch, 3, sh.pad[1], sh.pad[0]), dtype=p.dtype, device=dev) for sh, _ in shape.views]
                    shape.pipe = PipelinedAugInference(self.model, imgs, shape.metas, depth=self.depth, rescale=True)
                for sh, _ in shape.views:                      # the axis tables' upload happens here, not in the tile loop
                    if not sh.native:
                        sh.tables = [resize_tables(a, b, dev) for a, b in zip(sh.src, sh.new)]
                continue
            if shape is None and self.pipe is None:
                img = torch.zeros((self.batch, 3, self.subsize, self.subsize), dtype=p.dtype, device=dev)
                self.pipe = PipelinedInference(self.model, img, self.metas, depth=self.depth)
            elif shape is not None and shape.pipe is None:
                img = torch.zeros((self.batch, 3, shape.pad[1], shape.pad[0]), dtype=p.dtype, device=dev)
                shape.pipe = PipelinedInference(self.model, img, shape.metas, depth=self.depth, rescale=True)
            if shape is not None and not shape.native:         # the axis tables' upload happens here, not in the tile loop
                shape.tables = [resize_tables(a, b, dev) for a, b in zip(shape.src, shape.new)]
        return plan

    def _fill(self, shape, scene, origins, static_img, flip=False):
        """The tiles at `origins` of `scene` into a detector input buffer (`_AugShape`: every view into its own buffer)."""
        if isinstance(shape, _AugShape):
            for (sh, f), buf in zip(shape.views, static_img):
                self._fill(sh, scene, origins, buf, f)
            return static_img
        if shape is None or shape.native:
            return (scene_tiles_flip if flip else scene_tiles)(scene, origins, static_img, self.mean, self.std, self.to_rgb)
        return (scene_tiles_resized_flip if flip else scene_tiles_resized)(scene, origins, shape.src, shape.new, static_img,
                                                                           self.mean, self.std, self.to_rgb)

    @staticmethod
    def _resample(scene, w, h):
        x = scene.permute(2, 0, 1)[None].float()
        y = F.interpolate(x, size=(h, w), mode='bicubic', align_corners=False)
        return y.round_().clamp_(0, 255).to(torch.uint8)[0].permute(1, 2, 0).contiguous()

    def run_tiles(self, plan):
        """Every tile of every rate through the captured graphs; the packed results land in plan.packed.  Nothing here waits
        for the device or copies to the host."""
        B = self.batch
        dev = plan.scenes[0].device
        shapes = plan.shapes or [None] * len(plan.scenes)
        pipes = []
        plan.packed = []
        for scene, on_dev, shape in zip(plan.scenes, plan.origins_dev, shapes):
            pipe = self.pipe if shape is None else shape.pipe
            pipes.append(pipe)
            rows = pipe.slots[0].packed[0].size(0)
            packed = torch.empty((on_dev.size(0), rows, 28), dtype=torch.float32, device=dev)
            plan.packed.append(packed)
            for i in range(0, on_dev.size(0), B):
                def fill(static_img, i=i):
                    self._fill(shape, scene, on_dev[i:i + B], static_img)

                def sink(outs, i=i):
                    for j, o in enumerate(outs):
                        packed[i + j].copy_(o, non_blocking=True)
                pipe.submit_device(fill, sink)
        cur = torch.cuda.current_stream(dev)
        for pipe in pipes:
            for s in pipe.streams:
                cur.wait_stream(s)
        return plan

    def merge(self, plan):
        """collect per rate -> concatenation per class across rates -> one batched merge NMS -> one gather, one D2H."""
        C = self.num_classes
        parts = [self._collect(plan, i) for i in range(len(plan.rates))]
        tables = torch.stack([t for _, t in parts]).cpu().numpy()            # the one D2H of the offsets and flags
        for i in np.nonzero(tables[:, C + 1])[0]:
            self._rerun_overflowed(plan, int(i))
            parts[i] = self._collect(plan, int(i))
            tables[i] = parts[i][1].cpu().numpy()
        if len(parts) == 1:
            n = int(tables[0, C])
            dets, seg = parts[0][0][:n], parts[0][1][:C + 1]
            sizes = np.diff(tables[0, :C + 1])
        else:
            pieces = [d[int(t[c]):int(t[c + 1])] for c in range(C) for (d, _), t in zip(parts, tables)]
            dets = torch.cat(pieces)
            sizes = np.diff(tables[:, :C + 1], axis=1).sum(axis=0)
            seg = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dets.device)
        n = int(sizes.sum())
        if n == 0:
            return [np.zeros((0, 9), np.float64) for _ in range(C)]
        keep, num = poly_nms_f64_batched_device(dets, seg, int(sizes.max()), self.nms_thresh, hbb_prefilter=True, presorted=False)
        # rows past a segment's count are unwritten: clamped, gathered with the rest and dropped on the host
        out = torch.cat([dets[keep.clamp(0, n - 1)].reshape(-1), num.to(torch.float64)]).cpu().numpy()
        rows, num = out[:n * 9].reshape(n, 9), out[n * 9:].astype(np.int64)
        off = np.concatenate([[0], np.cumsum(sizes)])
        return [rows[off[c]:off[c] + num[c]].copy() for c in range(C)]

    def __call__(self, scene):
        with torch.no_grad():
            return self.merge(self.run_tiles(self.prepare(scene)))

    # ---- helpers -------------------------------------------------------------------------------------------------------------
    def _collect(self, plan, i):
        T = len(plan.origins[i])
        dets, table, _ = scene_collect(plan.packed[i][:T], plan.origins_dev[i][:T], plan.rates[i], self.num_classes)
        return dets, table

    def _rerun_overflowed(self, plan, i):
        """Rate i has tiles whose packed result overflowed the static capacity: run their batches through
        `model.simple_test_batch` -- `model.aug_test` per tile with `views` -- (which take the dynamic path for them) and write
        the rows into the tiles' packed slots."""
        packed, on_dev, B = plan.packed[i], plan.origins_dev[i], self.batch
        T, m = len(plan.origins[i]), packed.size(1) - 1
        over = np.nonzero(packed[:T, m, 1].cpu().numpy())[0]
        redo = {}
        shape = plan.shapes[i] if plan.shapes else None
        inputs = (self.pipe if shape is None else shape.pipe).slots[0].inputs
        img = [torch.empty_like(v) for v in inputs] if isinstance(shape, _AugShape) else torch.empty_like(inputs)
        for b in sorted(set(int(t) // B for t in over)):
            self._fill(shape, plan.scenes[i], on_dev[b * B:(b + 1) * B], img)
            with torch.no_grad():
                if isinstance(shape, _AugShape):               # per class [k, 9]: no rep-points on this route, zeros in their place
                    results = [[np.concatenate([np.zeros((len(r), 18), np.float32), r], 1) for r in per_class]
                               for per_class in shape.pipe.slots[0].fallback(img)]
                elif shape is None:
                    results = self.model.simple_test_batch(img, self.metas)
                else:
                    results = self.model.simple_test_batch(img, shape.metas, rescale=True)
            for t in over[over // B == b]:
                per_class = results[int(t) - b * B]
                rows = np.concatenate([np.concatenate([r[:, -27:], np.full((len(r), 1), c, np.float32)], 1)
                                       for c, r in enumerate(per_class)]).astype(np.float32)
                redo[int(t)] = rows
        self.fallback_tiles += len(redo)
        need = max([m] + [len(r) for r in redo.values()])
        if need > m:                                   # static_capacity below max_per_img: the slots grow to the longest result
            grown = torch.zeros((packed.size(0), need + 1, 28), dtype=torch.float32, device=packed.device)
            grown[:, :m] = packed[:, :m]
            grown[:, need] = packed[:, m]
            plan.packed[i] = packed = grown
        for t, rows in redo.items():
            slot = np.zeros((packed.size(1), 28), np.float32)
            slot[:len(rows)] = rows
            slot[-1, 0] = len(rows)
            packed[t].copy_(torch.from_numpy(slot))

    def write_task1(self, dstpath, name, per_class, classes=DOTA_CLASSES):
        """Append `name score x1 y1 .. x4 y4` lines to dstpath/Task1_<class>.txt, one per kept detection, formatted as
        `mergesingle` formats them (`str()` of Python floats, score first).  Classes without detections get no file."""
        os.makedirs(dstpath, exist_ok=True)
        for cls, rows in zip(classes, per_class):
            if len(rows) == 0:
                continue
            with open(os.path.join(dstpath, 'Task1_' + cls + '.txt'), 'a') as f:
                for det in np.asarray(rows, np.float64).tolist():
                    f.write(name + ' ' + str(det[-1]) + ' ' + ' '.join(map(str, det[0:-1])) + '\n')
