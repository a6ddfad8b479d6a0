"""Whole-scene inference timing: `SceneInference` (scene uploaded once as uint8, tiles cut / normalised / collected / merged
on the device) against the route that existed before it, built from the same parts: per tile host crop + `imnormalize` +
H2D copy -> `PipelinedInference.submit` (same depth) -> per-tile result lists on the host -> host translation ->
`py_gpu_nms_poly_fast_segments`.  R-50 FPN, fp32, head calibrated as in bench.py, uniform-noise scenes, rate 1.

The two routes alternate in one process; after a warm-up run of each, every route is timed `--reps` times per scene (host
clock around work that ends in a device synchronise; the scene is a host array for both, so the scene route pays its one
upload inside the timed window).  The scene route is then run three more times stage by stage (a synchronise after each
stage, which the product path does not have).  Reported: median and min .. max of the wall time per scene, tiles/s at the median, the
parent route's host preparation alone (crop + imnormalize + H2D of one tile), and HIP-event times of `orp_scene_tiles` (one
tile per launch as SceneInference issues it, and 16 tiles per launch; GB/s = 15 bytes per pixel over that time) and of
`orp_scene_collect` on the scene's packed results.

`--img-scale W,H` (e.g. 1333,960, the R-101 / Swin-T configs' test scale) adds the resized routes, alternated with the
native-size ones in the same process: the host-tiled route then pays `imrescale` + `Pad` per tile and runs graphs captured
with `rescale=True`; the scene route is `SceneInference(img_scale=...)`.  One table row per scene and test scale, and the
HIP-event times of `orp_scene_tiles_resized` next to those of `orp_scene_tiles`.

    python tools/time_scene_inference.py [--sizes 4096,8192,16384] [--reps 5] [--depth 4] [--img-scale 1333,960]
"""
import argparse
import copy
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import MODELS, TEST_CFG, calibrate_head  # noqa: E402
from orientedreppoints_amd import _lib  # noqa: E402
from orientedreppoints_amd.dota_devkit.img_split import split_origins  # noqa: E402
from orientedreppoints_amd.dota_devkit.result_merge_multi_process import py_gpu_nms_poly_fast_segments  # noqa: E402
from orientedreppoints_amd.mmdet_datasets.imops import imnormalize, impad_to_multiple, imrescale, rescale_size  # noqa: E402
from orientedreppoints_amd.mmdet_models import ConfigDict, PipelinedInference, SceneInference, build_detector  # noqa: E402
from orientedreppoints_amd.mmdet_ops.scene_ops import scene_collect, scene_tiles, scene_tiles_resized  # noqa: E402

SUB, GAP = 1024, 200
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def host_tile(scene, left, up, dev, img_scale=None):
    """The test pipeline of one patch on the host: crop (-> RotateResize(keep_ratio)) -> Normalize (-> Pad(32)) -> H2D."""
    crop = scene[up:up + SUB, left:left + SUB]
    if img_scale is None:
        return torch.from_numpy(np.ascontiguousarray(imnormalize(crop, MEAN, STD, True).transpose(2, 0, 1))[None]).to(dev)
    img = impad_to_multiple(imnormalize(imrescale(crop, img_scale), MEAN, STD, True), 32)
    return torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))[None]).to(dev)


def parent_route(pipe, scene, origins, num_classes, dev, img_scale=None):
    """What a user had to write before SceneInference.  Returns the kept rows per class."""
    results = []
    for left, up in origins:
        r = pipe.submit(host_tile(scene, left, up, dev, img_scale))
        if r is not None:
            results.append(r[0])
    results += [r[0] for r in pipe.flush()]
    segs = []
    for c in range(num_classes):
        rows = []
        for (left, up), res in zip(origins, results):
            d = res[c][:, -9:].astype(np.float64)
            d[:, 0:8:2] += left
            d[:, 1:8:2] += up
            rows.append(d)
        segs.append(np.concatenate(rows))
    keeps = py_gpu_nms_poly_fast_segments(segs, 0.1)
    return [s[k] for s, k in zip(segs, keeps)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn, inner=20, reps=5):
    """Median HIP-event time of one call of fn, from `inner` back-to-back calls between two events."""
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--img-scale", default=None, help="W,H: also time the routes with the test resize, e.g. 1333,960")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_scene_inference.py measures on the GPU"
    dev = torch.device("cuda:0")
    print("device: %s, torch %s, hip %s, library %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip,
                                                       _lib.lib().orp_version().decode()))
    torch.manual_seed(0)
    model = build_detector(ConfigDict(MODELS['r50']), train_cfg=None, test_cfg=ConfigDict(copy.deepcopy(TEST_CFG))).to(dev).eval()
    rng = np.random.default_rng(0)
    first = rng.integers(0, 256, size=(SUB, SUB, 3), dtype=np.uint8)
    calibrate_head(model, host_tile(first, 0, 0, dev))
    C = model.bbox_head.num_classes - 1
    scales = [None] + ([tuple(int(v) for v in a.img_scale.split(","))] if a.img_scale else [])
    routes = []                                                          # (img_scale, host-tiled pipe, SceneInference)
    for img_scale in scales:
        x = host_tile(first, 0, 0, dev, img_scale)
        new_w, new_h, factor = (SUB, SUB, 1.0) if img_scale is None else rescale_size((SUB, SUB), img_scale)
        metas = [dict(img_shape=(new_h, new_w, 3), pad_shape=(x.size(2), x.size(3), 3), scale_factor=factor, flip=False)]
        routes.append((img_scale, PipelinedInference(model, x, metas, depth=a.depth, rescale=img_scale is not None),
                       SceneInference(model, subsize=SUB, gap=GAP, batch=1, depth=a.depth, img_scale=img_scale)))

    # the tile kernels alone: one tile per launch (what SceneInference issues) and 16 per launch
    probe = torch.from_numpy(rng.integers(0, 256, size=(4096, 4096, 3), dtype=np.uint8)).to(dev)
    po = torch.tensor(split_origins(4096, 4096, SUB, GAP)[:16], dtype=torch.int32).to(dev)
    out16 = torch.empty((16, 3, SUB, SUB), dtype=torch.float32, device=dev)
    t1 = event_ms(lambda: scene_tiles(probe, po[:1], out16[:1], MEAN, STD, True))
    t16 = event_ms(lambda: scene_tiles(probe, po, out16, MEAN, STD, True))
    tile_bytes = 15.0 * SUB * SUB
    print("orp_scene_tiles fp32 1024^2: 1 tile / launch %.1f us (%.0f GB/s); 16 tiles / launch %.1f us per tile (%.0f GB/s)" % (
        t1 * 1e3, tile_bytes / t1 / 1e6, t16 / 16 * 1e3, 16 * tile_bytes / t16 / 1e6))
    for img_scale in scales[1:]:
        new_w, new_h, _ = rescale_size((SUB, SUB), img_scale)
        o16 = torch.empty((16, 3, -(-new_h // 32) * 32, -(-new_w // 32) * 32), dtype=torch.float32, device=dev)
        r1 = event_ms(lambda: scene_tiles_resized(probe, po[:1], (SUB, SUB), (new_w, new_h), o16[:1], MEAN, STD, True))
        r16 = event_ms(lambda: scene_tiles_resized(probe, po, (SUB, SUB), (new_w, new_h), o16, MEAN, STD, True))
        print("orp_scene_tiles_resized fp32 1024^2 -> %d x %d (pad %d x %d): 1 tile / launch %.1f us; 16 tiles / launch %.1f us per tile" % (
            new_w, new_h, o16.size(3), o16.size(2), r1 * 1e3, r16 / 16 * 1e3))
        del o16
    del probe, out16

    print("| scene | test scale | tiles | parent route: median (min .. max) ms | tiles/s | scene route: median (min .. max) ms | tiles/s | "
          "parent / scene | scene route by stage: upload + plan / tiles / collect + merge + fetch (ms) | parent host prep per tile (ms) | orp_scene_collect (ms) | rows collected | kept parent / scene | fallback tiles |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for side in [int(x) for x in a.sizes.split(",")]:
        scene = rng.integers(0, 256, size=(side, side, 3), dtype=np.uint8)
        origins = split_origins(side, side, SUB, GAP)
        T = len(origins)
        before = [si.fallback_tiles for _, _, si in routes]
        for img_scale, pipe, si in routes:                                # warm-up of all (workspaces, first launches)
            parent_route(pipe, scene, origins, C, dev, img_scale)
            si(scene)
        tp, ts, kp, ks = [[] for _ in routes], [[] for _ in routes], [None] * len(routes), [None] * len(routes)
        for _ in range(a.reps):                                           # alternated: routes and test scales
            for k, (img_scale, pipe, si) in enumerate(routes):
                t, kp[k] = timed(lambda: parent_route(pipe, scene, origins, C, dev, img_scale))
                tp[k].append(t)
                t, ks[k] = timed(lambda: si(scene))
                ts[k].append(t)
        for k, (img_scale, pipe, si) in enumerate(routes):
            stages = []
            for _ in range(3):                                            # the scene route once more, stage by stage
                s0, plan = timed(lambda: si.prepare(scene))
                s1, _ = timed(lambda: si.run_tiles(plan))
                s2, _ = timed(lambda: si.merge(plan))
                stages.append((s0, s1, s2))
            stages = np.median(np.array(stages), axis=0)
            prep = float(np.median([timed(lambda: host_tile(scene, 824, 824, dev, img_scale))[0] for _ in range(9)]))
            plan = si.run_tiles(si.prepare(scene))
            packed, odev = plan.packed[0][:T], plan.origins_dev[0][:T]
            tc = event_ms(lambda: scene_collect(packed, odev, 1.0, C), inner=5)
            n = int(scene_collect(packed, odev, 1.0, C)[1][C])
            mp, ms = float(np.median(tp[k])), float(np.median(ts[k]))
            print("| %d^2 | %s | %d | %.0f (%.0f .. %.0f) | %.0f | %.0f (%.0f .. %.0f) | %.0f | %.2f | %.0f / %.0f / %.0f | %.1f | %.3f | %d | %d / %d | %d |" % (
                side, "native" if img_scale is None else "%d,%d" % img_scale, T, mp, min(tp[k]), max(tp[k]), T / mp * 1e3, ms, min(ts[k]),
                max(ts[k]), T / ms * 1e3, mp / ms, stages[0], stages[1], stages[2], prep, tc, n, sum(len(x) for x in kp[k]),
                sum(len(x) for x in ks[k]), (si.fallback_tiles - before[k]) // (a.reps + 5)), flush=True)
            del plan, packed
        del scene


if __name__ == "__main__":
    main()
