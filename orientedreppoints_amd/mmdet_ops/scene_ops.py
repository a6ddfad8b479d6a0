"""Thin wrappers of the whole-scene kernels (csrc/orp_scene.hip): `scene_tiles` crops, channel-swaps, normalises and converts
T tiles of a uint8 scene on the device; `scene_collect` turns the packed per-tile detections into the per-class fp64
segments `poly_nms_f64_batched_device` takes.  Both only enqueue work on PyTorch's current stream."""
import ctypes

import numpy as np
import torch

from .. import _lib

_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def scene_tiles(scene, origins, out, mean, std, to_rgb=True):
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
    with torch.cuda.device(out.device):
        rc = _lib.lib().orp_scene_tiles(ctypes.c_void_p(scene.data_ptr()), scene.size(0), scene.size(1), scene.stride(0),
                                        _lib.ptr(origins), origins.size(0), out.size(2), m, s, int(bool(to_rgb)),
                                        _DTYPES[out.dtype], _lib.ptr(out), _lib.stream_of(out))
    _lib.check(rc, "orp_scene_tiles")
    return out


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
    with torch.cuda.device(dev):
        rc = L.orp_scene_collect(_lib.ptr(packed), T, m, _lib.ptr(origins), float(rate), C, T * m, _lib.ptr(dets),
                                 _lib.ptr(table), _lib.ptr(src), ctypes.c_void_p(table.data_ptr() + 4 * (C + 1)),
                                 _lib.ptr(ws), ws.numel(), _lib.stream_of(packed))
    _lib.check(rc, "orp_scene_collect")
    return dets, table, src
