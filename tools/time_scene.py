"""Whole-scene merge timing: the segmented fp64 merge NMS (`orp_poly_nms_f64_batched`, all classes of a scene in one
launch sequence) against the current host route (per class: host sort + one `orp_poly_nms_f64` call, what
`dota_devkit/result_merge.py` runs), on the same detections, in the same process.

Detections per class: clustered oriented boxes of 8 - 64 px over a ~4000^2 scene (20 hubs), scores rounded to 3 decimals
as in Task1 files.  Both routes are timed from numpy to the kept index lists (host clock, device synchronised); the
batched call is also timed device-side (HIP events around the launch sequence on data already on the device), with
the rows already in visiting order (presorted) and in input order (the two stable radix sorts of the fp64 score and the
segment id run inside the call).

    python tools/time_scene.py [--classes 15] [--sizes 2000,10000,40000] [--reps 3]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from orientedreppoints_amd import synthetic as S  # noqa: E402
from orientedreppoints_amd.dota_devkit.result_merge import py_gpu_nms_poly  # noqa: E402
from orientedreppoints_amd.dota_devkit.result_merge_multi_process import py_gpu_nms_poly_fast_segments  # noqa: E402
from orientedreppoints_amd.mmdet_ops.nms_wrapper import poly_nms_f64_batched_device  # noqa: E402


def scene_dets(n, seed):
    d = S.gen_polys(n, seed, clustered=True, wh=(8.0, 64.0))
    cx, cy = d[:, 0:8:2].mean(1, keepdims=True), d[:, 1:8:2].mean(1, keepdims=True)
    d[:, 0:8:2] += 3.0 * cx                                  # centres x4, box sizes kept
    d[:, 1:8:2] += 3.0 * cy
    d[:, 8] = np.round(d[:, 8], 3)
    return d


def best_of(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), out


def device_ms(segs, thr, fast, reps, presorted=True):
    """HIP-event time of one batched launch sequence (data and offsets already on the device)."""
    dev = torch.device("cuda:0")
    orders = [d[:, 8].argsort()[::-1] if presorted else np.arange(len(d)) for d in segs]
    cat = torch.from_numpy(np.ascontiguousarray(np.concatenate([d[o] for d, o in zip(segs, orders)]))).to(dev)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(d) for d in segs])]).astype(np.int32)).to(dev)
    mx = max(len(d) for d in segs)
    poly_nms_f64_batched_device(cat, off, mx, thr, hbb_prefilter=fast, presorted=presorted)
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        poly_nms_f64_batched_device(cat, off, mx, thr, hbb_prefilter=fast, presorted=presorted)
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=15)
    ap.add_argument("--sizes", default="2000,10000,40000")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_scene.py measures on the GPU"
    from orientedreppoints_amd import _lib
    print("device: %s, torch %s, hip %s, library %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip,
                                                       _lib.lib().orp_version().decode()))
    print("| boxes / class | classes | host route, full, thr 0.3 (ms) | batched full, thr 0.3 (ms) | same keep lists | "
          "batched fast, thr 0.1 (ms) | device: batched full / fast (ms) | device: fast, unsorted input (ms) | kept full / fast |")
    print("|---|---|---|---|---|---|---|---|---|")
    for n in [int(x) for x in a.sizes.split(",")]:
        segs = [scene_dets(n, 1000 + c) for c in range(a.classes)]
        py_gpu_nms_poly(segs[0], 0.3)                                            # warm: workspace growth, first launches
        py_gpu_nms_poly_fast_segments(segs, 0.3, hbb_prefilter=False)
        py_gpu_nms_poly_fast_segments(segs, 0.1)
        t_host, k_host = best_of(lambda: [py_gpu_nms_poly(d, 0.3) for d in segs], a.reps)
        t_full, k_full = best_of(lambda: py_gpu_nms_poly_fast_segments(segs, 0.3, hbb_prefilter=False), a.reps)
        t_fast, k_fast = best_of(lambda: py_gpu_nms_poly_fast_segments(segs, 0.1), a.reps)
        dv_full = device_ms(segs, 0.3, False, a.reps)
        dv_fast = device_ms(segs, 0.1, True, a.reps)
        dv_sort = device_ms(segs, 0.1, True, a.reps, presorted=False)
        print("| %d | %d | %.1f | %.1f | %s | %.1f | %.1f / %.1f | %.1f | %d / %d |" % (
            n, a.classes, t_host, t_full, k_full == k_host, t_fast, dv_full, dv_fast, dv_sort,
            sum(len(k) for k in k_full), sum(len(k) for k in k_fast)), flush=True)


if __name__ == "__main__":
    main()
