"""A train pipeline with its image half on the device.  `DeviceTrainPipeline.from_config(train_pipeline)` splits the configs'
`train_pipeline` in two:

  `.host`     runs in the loader workers and never touches the GPU: it loads the image and the annotations, makes every random
              draw and does the box half (scale, flip, rotate, `poly2rbox`, `filter_border`, `rbox2poly`) and the meta keys
              exactly as the host classes of pipelines.py do -- it calls their own `plan` methods -- and returns the raw uint8
              image with the plan of what is to be done to it.  A seeded `.host` and a seeded host `Compose` make the same draws.
  `.collate`  runs in the process that owns the GPU: one pinned upload of the batch's images, one of its tables, one
              `train_images` call (mmdet_ops/train_image_ops.py), and returns what `DefaultFormatBundle`, `Collect` and mmcv's
              collate hand the detector.

What the device half cannot do is refused at construction with a ValueError that names the step, so the caller keeps the host
pipeline."""
import numpy as np

from . import imops
from . import pipelines as P

_LOADERS = ('LoadImageFromFile', 'LoadAnnotations', 'CorrectBox', 'CorrectRBBox')
_RESIZES = ('RotateResize', 'PolyResize')
_FLIPS = ('RotateRandomFlip', 'PolyRandomFlip')
# the order the image steps must stand in: the kernels resize, flip, rotate, then normalise and pad
_STAGE = {'RotateResize': 1, 'PolyResize': 1, 'RotateRandomFlip': 2, 'PolyRandomFlip': 2, 'HSVAugment': 3, 'PolyRandomRotate': 4,
          'Normalize': 5, 'Pad': 5, 'DefaultFormatBundle': 6, 'Collect': 7}


def _refuse(step, why):
    raise ValueError("DeviceTrainPipeline: %s: %s (keep the host pipeline)" % (step, why))


class HostHalf(object):
    """The `Compose`-compatible host half (`DotaDataset(pipeline=[dp.host])`): results dict -> dict(img=raw uint8 HWC,
    plan=..., img_meta=..., gt_bboxes=..., gt_labels=...) or None where the host pipeline returns None."""

    def __init__(self, loaders, planned, collect):
        self.loaders, self.planned, self.collect = loaders, planned, collect

    def __call__(self, results):
        for t in self.loaders:
            results = t(results)
            if results is None:
                return None
        if isinstance(results, list):
            _refuse('mosaic', 'a list of images is not one image')
        img = results['img']
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("DeviceTrainPipeline: the image must be uint8 [h, w, 3], not %s %s" % (img.dtype, img.shape))
        inv = None
        for t in self.planned:
            results = t.plan(results)
            if results is None:
                return None
            if isinstance(t, P.PolyRandomRotate) and results['rotate']:
                inv = imops.invert_affine(t.rm_image)
        flip = P.RotateRandomFlip.direction_of(results) if results.get('flip') else None
        data = self.collect(results)                                   # the raw image rides along under 'img'
        data['plan'] = dict(src=tuple(img.shape[:2]), new=tuple(results['img_shape'][:2]), pad=tuple(results['pad_shape'][:2]),
                            flip=flip, inv=inv)
        return data


class DeviceTrainPipeline(object):
    def __init__(self, host, mean, std, to_rgb, pad_before_normalize, device):
        self.host = host
        self.mean, self.std, self.to_rgb = mean, std, to_rgb
        self.pad_before_normalize, self.device = pad_before_normalize, device

    @classmethod
    def from_config(cls, train_pipeline_cfg, device='cuda'):
        """train_pipeline_cfg: the list of step dicts of a config's `train_pipeline` (`cfg.data.train.pipeline`)."""
        loaders, planned, collect, norm, stage, pad_first = [], [], None, None, 0, None
        seen = set()
        for step in train_pipeline_cfg:
            step = dict(step)
            name = step.get('type')
            name = name if isinstance(name, str) else getattr(name, '__name__', repr(name))
            if name in _LOADERS:
                if planned:
                    _refuse(name, 'a loading step behind an image step')
                if name == 'LoadImageFromFile' and step.get('to_float32', False):
                    _refuse(name, 'to_float32=True (the kernels read uint8)')
                loaders.append(P.build_pipeline(step))
                continue
            if name not in _STAGE:
                _refuse(name, 'a step the device pipeline does not know')
            kind = 'resize' if name in _RESIZES else 'flip' if name in _FLIPS else name
            if kind in seen:
                _refuse(name, 'a second step of its kind')
            seen.add(kind)
            if _STAGE[name] < stage:
                _refuse(name, 'out of the order resize, flip, rotate, normalize / pad')
            stage = _STAGE[name]
            if name in _RESIZES:
                if not step.get('keep_ratio', True):
                    _refuse(name, 'keep_ratio=False')
                if step.get('interpolation', 'bilinear') != 'bilinear':
                    _refuse(name, 'interpolation=%r (bilinear only)' % step['interpolation'])
            if name == 'PolyRandomRotate' and step.get('auto_bound', False):
                _refuse(name, 'auto_bound=True')
            if name == 'Pad':
                if step.get('size') is not None or step.get('pad_val', 0) != 0:
                    _refuse(name, 'a fixed size or a pad value other than 0')
                pad_first = norm is None
            t = P.build_pipeline(step)
            if name == 'Normalize':
                norm = t
            if name == 'Collect':
                collect = t
            elif name != 'DefaultFormatBundle':                        # (its tensors are made on the device, in collate)
                planned.append(t)
        for kind, name in (('resize', 'RotateResize'), ('flip', 'RotateRandomFlip'), ('Normalize', 'Normalize'), ('Pad', 'Pad'),
                           ('Collect', 'Collect')):
            if kind not in seen:
                _refuse(name, 'the pipeline has no such step')
        if not loaders or not isinstance(loaders[0], P.LoadImageFromFile):
            _refuse('LoadImageFromFile', 'the pipeline must begin with it')
        if sorted(collect.keys) != ['gt_bboxes', 'gt_labels', 'img']:
            _refuse('Collect', "keys other than ['img', 'gt_bboxes', 'gt_labels']")
        return cls(HostHalf(loaders, planned, collect), norm.mean, norm.std, bool(norm.to_rgb), bool(pad_first), device)

    # ---- the device half -----------------------------------------------------------------------------------------------
    def upload(self, samples):
        """The host work of `collate` and its two uploads: the plan, the images and the tables (descriptors, matrices, axis
        tables, boxes, labels) in two pinned buffers, each copied to the device without blocking."""
        import torch
        from ..mmdet_ops.train_image_ops import TrainImagePlan
        boxes = [np.asarray(s['gt_bboxes'], np.float32).reshape(-1, 8) for s in samples]
        labels = [np.asarray(s['gt_labels'], np.int64).reshape(-1) for s in samples]
        plan = TrainImagePlan([s['plan'] for s in samples], self.mean, self.std, self.to_rgb, self.pad_before_normalize,
                              extras=dict(gt_bboxes=np.concatenate(boxes), gt_labels=np.concatenate(labels)))
        if plan.out_shape[3] % 4 != 0:
            raise ValueError("DeviceTrainPipeline: the batch's width %d is no multiple of 4" % plan.out_shape[3])
        dev = torch.device(self.device)
        pinned_images = torch.empty(plan.images_bytes, dtype=torch.uint8, pin_memory=True)
        plan.pack_images([s['img'] for s in samples], pinned_images)
        pinned_table = torch.empty(plan.table.size, dtype=torch.uint8, pin_memory=True)
        pinned_table.numpy()[:] = plan.table
        images = pinned_images.to(dev, non_blocking=True)
        table = pinned_table.to(dev, non_blocking=True)
        return dict(plan=plan, images=images, table=table, counts=[len(b) for b in boxes],
                    img_metas=[s['img_meta'] for s in samples])

    def run(self, staged):
        """The device work of `collate`: one `train_images` call; boxes and labels are views of the uploaded table."""
        import torch
        from ..mmdet_ops.train_image_ops import train_images
        plan, table = staged['plan'], staged['table']
        img = torch.empty(plan.out_shape, dtype=torch.float32, device=table.device)
        train_images(staged['images'], table, plan, img)
        all_boxes = plan.section(table, 'gt_bboxes', torch.float32).view(-1, 8)
        all_labels = plan.section(table, 'gt_labels', torch.int64)
        gt_bboxes, gt_labels, at = [], [], 0
        for n in staged['counts']:
            gt_bboxes.append(all_boxes[at:at + n])
            gt_labels.append(all_labels[at:at + n])
            at += n
        return dict(img=img, img_metas=staged['img_metas'], gt_bboxes=gt_bboxes, gt_labels=gt_labels)

    def collate(self, samples):
        """samples: what `.host` returned for the images of a batch -> dict(img=[B, 3, H, W] float32 device tensor,
        img_metas=[...], gt_bboxes=[float32 [n, 8] device tensors], gt_labels=[int64 [n] device tensors]); H, W are the
        maxima of the samples' pad shapes."""
        return self.run(self.upload(samples))
