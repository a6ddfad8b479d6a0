"""Thin wrapper of the training image kernels (csrc/orp_train_images.hip): `train_images` turns the raw uint8 HWC images of a
batch into the padded, normalised, collated [B, 3, H, W] float32 tensor -- the train pipelines' resize (keep_ratio, bilinear),
flip (horizontal / vertical), rotation (`PolyRandomRotate`, auto_bound=False), `Normalize` and `Pad` in either order and the
collate's zeros, each sample with its own geometry, in one launch (two when a sample rotates).  `TrainImagePlan` is the host
half: it lays the images, the descriptor table of include/orp_hip.h, the inverse matrices and the axis tables out in two flat
buffers, one upload each.  Only enqueues work on PyTorch's current stream."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .scene_ops import resize_axis

# orp_train_image_desc of include/orp_hip.h, 64 bytes
DESC_DTYPE = np.dtype(_lib.struct("orp_train_image_desc"))
assert DESC_DTYPE.itemsize == 64

FLIP_CODES = {None: 0, 'horizontal': 1, 'vertical': 2}

_axis_cache = {}


def axis_table(n_in, n_out):
    """`scene_ops.resize_axis(n_in, n_out)` on the host, cached per (n_in, n_out)."""
    key = (int(n_in), int(n_out))
    t = _axis_cache.get(key)
    if t is None:
        t = resize_axis(*key)
        if len(_axis_cache) >= 4096:
            _axis_cache.pop(next(iter(_axis_cache)))
        _axis_cache[key] = t
    return t


def _align(v, a=16):
    return (int(v) + a - 1) // a * a


def scratch_image_bytes(new_w, new_h):
    """Bytes of one rotating sample's scratch image (`orp_train_images_scratch_bytes`)."""
    return int(_lib.lib().orp_train_images_scratch_bytes(int(new_w), int(new_h)))


class TrainImagePlan(object):
    """The host side of one `train_images` call.  samples: one dict per image with `src`, `new`, `pad` as (h, w), `flip`
    (None / 'horizontal' / 'vertical') and `inv` (None: the sample does not rotate; else the 2 x 3 float64 inverse matrix of
    `imops.invert_affine`).  `extras`: {name: numpy array} carried along in the table buffer (16-byte aligned), for what else
    the batch needs on the device.  Builds `desc`, `table` (uint8: descriptors, matrices, axis tables, extras), the images'
    byte offsets, `out_shape` = (B, 3, max pad_h, max pad_w) and `scratch_bytes`."""

    def __init__(self, samples, mean, std, to_rgb=True, pad_before_normalize=False, extras=None):
        B = len(samples)
        if B < 1 or B > 65535:
            raise ValueError("a batch holds 1 to 65535 images, not %d" % B)
        self.mean = np.asarray(mean, np.float32).reshape(3).copy()
        self.std = np.asarray(std, np.float32).reshape(3).copy()
        self.to_rgb, self.pad_before_normalize = bool(to_rgb), bool(pad_before_normalize)
        desc = np.zeros(B, DESC_DTYPE)
        inv = np.zeros((B, 6), np.float64)
        i0_parts, w1_parts, where, n_axis = [], [], {}, 0

        def table_of(n_in, n_out):
            nonlocal n_axis
            key = (int(n_in), int(n_out))
            if key not in where:
                i0, w1 = axis_table(*key)
                where[key] = n_axis
                i0_parts.append(i0)
                w1_parts.append(w1)
                n_axis += len(i0)
            return where[key]
        img_off, scr_off = 0, 0
        for b, s in enumerate(samples):
            (sh, sw), (nh, nw), (ph, pw) = [tuple(int(v) for v in s[k][:2]) for k in ('src', 'new', 'pad')]
            if min(sh, sw, nh, nw) <= 0:
                raise ValueError("sample %d: sizes must be positive (src %s, new %s)" % (b, (sh, sw), (nh, nw)))
            if ph < nh or pw < nw:
                raise ValueError("sample %d: pad shape %s is smaller than the resized shape %s" % (b, (ph, pw), (nh, nw)))
            if s.get('flip') not in FLIP_CODES:
                raise ValueError("sample %d: flip must be None, 'horizontal' or 'vertical', not %r" % (b, s.get('flip')))
            d = desc[b]
            d['src_offset'], d['src_h'], d['src_w'] = img_off, sh, sw
            d['new_h'], d['new_w'], d['pad_h'], d['pad_w'] = nh, nw, ph, pw
            d['flip'] = FLIP_CODES[s.get('flip')]
            d['x_table'], d['y_table'] = table_of(sw, nw), table_of(sh, nh)
            img_off = _align(img_off + sh * sw * 3)
            if s.get('inv') is not None:
                m = np.asarray(s['inv'], np.float64)
                if m.shape != (2, 3):
                    raise ValueError("sample %d: inv must be a 2 x 3 matrix" % b)
                inv[b] = m.reshape(6)
                d['rotate'], d['scratch_offset'] = 1, scr_off
                scr_off += scratch_image_bytes(nw, nh)
        self.desc, self.inv = desc, inv
        self.num_images, self.images_bytes, self.scratch_bytes, self.axis_len = B, img_off, scr_off, n_axis
        self.any_rotate = bool(desc['rotate'].any())
        self.out_shape = (B, 3, int(desc['pad_h'].max()), int(desc['pad_w'].max()))
        parts = [('desc', desc), ('inv', inv), ('axis_i0', np.concatenate(i0_parts).astype(np.int32)),
                 ('axis_w1', np.concatenate(w1_parts).astype(np.float32))]
        parts += [(k, np.ascontiguousarray(v)) for k, v in (extras or {}).items()]
        self.sections, off = {}, 0
        for name, a in parts:
            self.sections[name] = (off, a.nbytes)
            off = _align(off + a.nbytes)
        self.table = np.zeros(max(off, 16), np.uint8)
        for name, a in parts:
            o, n = self.sections[name]
            self.table[o:o + n] = a.reshape(-1).view(np.uint8)

    def pack_images(self, images, dst=None):
        """The images (uint8 [h, w, 3] arrays of the planned source sizes) at their offsets in one flat uint8 array (or torch
        tensor) `dst` of `images_bytes`."""
        if len(images) != self.num_images:
            raise ValueError("the plan holds %d images, not %d" % (self.num_images, len(images)))
        if dst is None:
            dst = np.zeros(self.images_bytes, np.uint8)
        flat = dst.numpy() if isinstance(dst, torch.Tensor) else dst
        for d, img in zip(self.desc, images):
            if img.dtype != np.uint8 or img.shape != (d['src_h'], d['src_w'], 3):
                raise ValueError("an image is %s %s, the plan has uint8 %s" % (img.dtype, img.shape, (d['src_h'], d['src_w'], 3)))
            o = int(d['src_offset'])
            flat[o:o + img.size] = img.reshape(-1)
        return dst

    def section(self, table, name, dtype):
        """The named section of the uploaded table as a flat tensor of `dtype`."""
        o, n = self.sections[name]
        return table[o:o + n].view(dtype)


def train_images(images, table, plan, out, scratch=None):
    """images: flat uint8 CUDA tensor of `plan.pack_images`; table: flat uint8 CUDA tensor, the upload of `plan.table`;
    out: contiguous float32 CUDA [B, 3, H, W] with H, W >= every sample's pad shape and W % 4 == 0 (`plan.out_shape` is the
    collate's).  Per sample b: out[b, :, :new_h, :new_w] = the resized, flipped, rotated, normalised image; the rest of its pad
    shape 0 (`Normalize` before `Pad`) or (0 - mean[c]) / std[c] (`Pad` before `Normalize`); beyond the pad shape 0.  Every
    element of out is written once.  scratch: uint8 CUDA buffer of `plan.scratch_bytes` for the rotating samples (taken from
    the per-stream workspace when None).  Returns out."""
    _lib.require_cuda(images, "images")
    _lib.require_cuda(table, "table")
    _lib.require_cuda(out, "out")
    if not isinstance(plan, TrainImagePlan):
        raise TypeError("plan must be a TrainImagePlan")
    if images.dtype != torch.uint8 or images.dim() != 1 or not images.is_contiguous() or images.numel() < plan.images_bytes:
        raise ValueError("images must be a flat uint8 tensor of at least %d bytes" % plan.images_bytes)
    if table.dtype != torch.uint8 or table.dim() != 1 or not table.is_contiguous() or table.numel() != plan.table.size:
        raise ValueError("table must be the flat uint8 upload of plan.table (%d bytes)" % plan.table.size)
    if out.dtype != torch.float32 or out.dim() != 4 or out.size(0) != plan.num_images or out.size(1) != 3 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 [%d, 3, H, W] tensor" % plan.num_images)
    if out.size(3) % 4 != 0:
        raise ValueError("out's width (%d) must be a multiple of 4" % out.size(3))
    if out.size(2) < plan.out_shape[2] or out.size(3) < plan.out_shape[3]:
        raise ValueError("out (%d x %d) is smaller than a sample's pad shape (%d x %d)"
                         % (out.size(3), out.size(2), plan.out_shape[3], plan.out_shape[2]))
    if images.device != out.device or table.device != out.device:
        raise ValueError("images, table and out must be on one device")
    if plan.any_rotate:
        if scratch is None:
            scratch = _lib.workspace(out.device, plan.scratch_bytes)
        _lib.require_cuda(scratch, "scratch")
        if scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < plan.scratch_bytes:
            raise ValueError("scratch must be a contiguous uint8 tensor of at least %d bytes" % plan.scratch_bytes)
    base = table.data_ptr()
    at = lambda name: ctypes.c_void_p(base + plan.sections[name][0])                               # noqa: E731
    m = (ctypes.c_float * 3)(*[float(v) for v in plan.mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in plan.std])
    _lib.call("orp_train_images", out.device, _lib.ptr(images), images.numel(), ctypes.c_void_p(plan.desc.ctypes.data), at('desc'),
              plan.num_images, at('inv'), at('axis_i0'), at('axis_w1'), plan.axis_len, m, s, int(plan.to_rgb),
              int(plan.pad_before_normalize), _lib.ptr(out), out.size(2), out.size(3), _lib.ptr(scratch) if plan.any_rotate else None,
              scratch.numel() if plan.any_rotate else 0, _lib.stream_of(out))
    return out
