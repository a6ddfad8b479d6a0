"""Thin wrappers of the whole-scene kernels (csrc/orp_scene.hip): `scene_tiles` crops, channel-swaps, normalises and converts
T tiles of a uint8 scene on the device; `scene_tiles_resized` resamples every patch first (the test pipeline's `RotateResize`)
and pads behind it; `scene_tiles_flip` / `scene_tiles_resized_flip` mirror the patch as the pipeline's `RandomFlip` does (the
flipped views of test-time augmentation); `scene_collect` turns the packed per-tile detections into the per-class fp64
segments `poly_nms_f64_batched_device` takes.  All only enqueue work on PyTorch's current stream."""
import ctypes

import numpy as np
import torch

from .. import _lib

_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def scene_tiles(scene, origins, out, mean, std, to_rgb=True, _entry="orp_scene_tiles"):
    """scene uint8 [H, W, 3] CUDA (any row stride; pixels contiguous), origins int32 [T, 2] CUDA (left, up),
    out [T, 3, S, S] contiguous CUDA float32 / float16 / bfloat16: out[t] = `imnormalize(scene[up:up+S, left:left+S], mean,
    std, to_rgb)` as CHW, rounded once to out's type; pixels outside the scene are 0.  Returns out."""
    _lib.require_cuda(scene, "scene")
    _lib.require_cuda(origins, "origins")
    _lib.require_cuda(out, "out")
    if scene.dtype != torch.uint8 or scene.dim() != 3 or scene.size(2) != 3 or scene.stride(2) != 1 or scene.stride(1) != 3:
        raise ValueError("scene must be uint8 [H, W, 3] with contiguous pixels (a row stride is allowed)")
    if origins.dtype != torch.int32 or origins.dim() != 2 or origins.size(1) != 2 or not origins.is_contiguous():
        raise ValueError("origins must be a contiguous int32 [T, 2] tensor")
    if out.dtype not in _DTYPES or out.dim() != 4 or out.size(1) != 3 or out.size(2) != out.size(3) or not out.is_contiguous():
        raise ValueError("out must be a contiguous [T, 3, S, S] float32 / float16 / bfloat16 tensor")
    if out.size(0) != origins.size(0):
        raise ValueError("out holds %d tiles, origins %d" % (out.size(0), origins.size(0)))
    m = (ctypes.c_float * 3)(*[float(v) for v in np.asarray(mean, np.float32).reshape(3)])
    s = (ctypes.c_float * 3)(*[float(v) for v in np.asarray(std, np.float32).reshape(3)])
    _lib.call(_entry, out.device, ctypes.c_void_p(scene.data_ptr()), scene.size(0), scene.size(1), scene.stride(0), _lib.ptr(origins),
              origins.size(0), out.size(2), m, s, int(bool(to_rgb)), _DTYPES[out.dtype], _lib.ptr(out), _lib.stream_of(out))
    return out


def scene_tiles_flip(scene, origins, out, mean, std, to_rgb=True):
    """`scene_tiles` with the test pipeline's horizontal `RandomFlip` in front of the normalisation: out[t, :, y, x] =
    scene_tiles(...)[t, :, y, S - 1 - x], bit for bit."""
    return scene_tiles(scene, origins, out, mean, std, to_rgb, _entry="orp_scene_tiles_flip")


def resize_axis(n_in, n_out):
    """The bilinear axis table of `orp_scene_tiles_resized` for `n_in` source and `n_out` output pixels (align_corners=False, what
    `imops.imresize` follows), in numpy fp32 with every operation rounded on its own: src = max(scale * (d + 0.5) - 0.5, 0),
    i0 = min(int(src), n_in - 1), w1 = src - i0.  Returns (i0 int32 [n_out], w1 float32 [n_out])."""
    half = np.float32(0.5)
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.maximum(scale * (np.arange(n_out, dtype=np.float32) + half) - half, np.float32(0))
    i0 = np.minimum(src.astype(np.int32), np.int32(n_in - 1))
    return i0, src - i0.astype(np.float32)


_axis_cache = {}


def resize_tables(n_in, n_out, device):
    """`resize_axis(n_in, n_out)` on `device`, cached per (n_in, n_out, device): the first use of a pair copies from the host
    (call it ahead of a loop that must not synchronise), later uses cost a dictionary look-up."""
    key = (int(n_in), int(n_out), torch.device(device))
    t = _axis_cache.get(key)
    if t is None:
        i0, w1 = resize_axis(key[0], key[1])
        t = (torch.from_numpy(i0).to(key[2]), torch.from_numpy(w1).to(key[2]))
        if len(_axis_cache) >= 64:
            _axis_cache.pop(next(iter(_axis_cache)))
        _axis_cache[key] = t
    return t


def scene_tiles_resized(scene, origins, src_size, new_size, out, mean, std, to_rgb=True, _entry="orp_scene_tiles_resized"):
    """scene and origins as for `scene_tiles`; src_size = (src_w, src_h) of every patch, new_size = (new_w, new_h) it is resized
    to; out [T, 3, pad_h, pad_w] contiguous CUDA float32 / float16 / bfloat16 with pad >= new.  out[t, :, :new_h, :new_w] =
    `imnormalize(resize(scene[up:up+src_h, left:left+src_w]), mean, std, to_rgb)` as CHW, the rest 0 -- the test pipeline's
    `RotateResize(keep_ratio)` -> `Normalize` -> `Pad`.  The resize is bilinear with `align_corners=False`, rounded to uint8, in
    the fp32 arithmetic `include/orp_hip.h` fixes (`resize_axis` builds its tables); source pixels are clamped inside the
    patch, and a patch must lie inside the scene (one that hangs over is moved inside).  new_size == src_size gives
    `scene_tiles`' output.  Returns out."""
    _lib.require_cuda(scene, "scene")
    _lib.require_cuda(origins, "origins")
    _lib.require_cuda(out, "out")
    if scene.dtype != torch.uint8 or scene.dim() != 3 or scene.size(2) != 3 or scene.stride(2) != 1 or scene.stride(1) != 3:
        raise ValueError("scene must be uint8 [H, W, 3] with contiguous pixels (a row stride is allowed)")
    if origins.dtype != torch.int32 or origins.dim() != 2 or origins.size(1) != 2 or not origins.is_contiguous():
        raise ValueError("origins must be a contiguous int32 [T, 2] tensor")
    if out.dtype not in _DTYPES or out.dim() != 4 or out.size(1) != 3 or not out.is_contiguous():
        raise ValueError("out must be a contiguous [T, 3, pad_h, pad_w] float32 / float16 / bfloat16 tensor")
    if out.size(0) != origins.size(0):
        raise ValueError("out holds %d tiles, origins %d" % (out.size(0), origins.size(0)))
    (src_w, src_h), (new_w, new_h) = [int(v) for v in src_size], [int(v) for v in new_size]
    if min(src_w, src_h, new_w, new_h) <= 0 or src_w > scene.size(1) or src_h > scene.size(0):
        raise ValueError("patches of %d x %d do not fit a scene of %d x %d" % (src_w, src_h, scene.size(1), scene.size(0)))
    if new_h > out.size(2) or new_w > out.size(3):
        raise ValueError("out (%d x %d) is smaller than the resized patch (%d x %d)" % (out.size(3), out.size(2), new_w, new_h))
    x_i0, x_w1 = resize_tables(src_w, new_w, out.device)
    y_i0, y_w1 = resize_tables(src_h, new_h, out.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in np.asarray(mean, np.float32).reshape(3)])
    s = (ctypes.c_float * 3)(*[float(v) for v in np.asarray(std, np.float32).reshape(3)])
    _lib.call(_entry, out.device, ctypes.c_void_p(scene.data_ptr()), scene.size(0), scene.size(1), scene.stride(0), _lib.ptr(origins),
              origins.size(0), src_w, src_h, new_w, new_h, out.size(3), out.size(2), _lib.ptr(x_i0), _lib.ptr(x_w1), _lib.ptr(y_i0),
              _lib.ptr(y_w1), m, s, int(bool(to_rgb)), _DTYPES[out.dtype], _lib.ptr(out), _lib.stream_of(out))
    return out


def scene_tiles_resized_flip(scene, origins, src_size, new_size, out, mean, std, to_rgb=True):
    """`scene_tiles_resized` with the horizontal `RandomFlip` between the resize and the normalisation (Resize -> RandomFlip ->
    Normalize -> Pad): the mirror is inside the resized patch's own width, out[t, :, y, x] = scene_tiles_resized(...)[t, :, y,
    new_w - 1 - x] for x < new_w, zeros beyond new_w / new_h as there.  Bit for bit that mirror."""
    return scene_tiles_resized(scene, origins, src_size, new_size, out, mean, std, to_rgb, _entry="orp_scene_tiles_resized_flip")


def scene_collect(packed, origins, rate, num_classes):
    """packed float32 [T, m + 1, 28] CUDA (the per-tile results of `core.fused_postprocess`), origins int32 [T, 2] CUDA,
    rate: the scene's scale.  Returns (dets float64 [T * m, 9], table int32 [num_classes + 2], src int32 [T * m, 2]), all
    on the device: table[:num_classes + 1] are the class segments' offsets into dets / src (rows past table[num_classes]
    are unwritten), table[num_classes + 1] is non-zero if a tile reported overflow (its rows are left out)."""
    _lib.require_cuda(packed, "packed")
    _lib.require_cuda(origins, "origins")
    if packed.dtype != torch.float32 or packed.dim() != 3 or packed.size(2) != 28 or packed.size(1) < 2 or not packed.is_contiguous():
        raise ValueError("packed must be a contiguous float32 [T, m + 1, 28] tensor")
    T, m = packed.size(0), packed.size(1) - 1
    if origins.dtype != torch.int32 or tuple(origins.shape) != (T, 2) or not origins.is_contiguous():
        raise ValueError("origins must be a contiguous int32 [T, 2] tensor")
    dev, C = packed.device, int(num_classes)
    dets = torch.empty((T * m, 9), dtype=torch.float64, device=dev)
    src = torch.empty((T * m, 2), dtype=torch.int32, device=dev)
    table = torch.empty((C + 2,), dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = _lib.workspace(dev, L.orp_scene_collect_workspace_bytes(T, C))
    _lib.call("orp_scene_collect", dev, _lib.ptr(packed), T, m, _lib.ptr(origins), float(rate), C, T * m, _lib.ptr(dets), _lib.ptr(table),
              _lib.ptr(src), ctypes.c_void_p(table.data_ptr() + 4 * (C + 1)), _lib.ptr(ws), ws.numel(), _lib.stream_of(packed))
    return dets, table, src
