"""Whole-scene detection with test-time augmentation, timed two ways on one synthetic scene (4096 x 4096 by default, 1024 tiles
with a gap of 200: 25 tiles; views = two scales x (plain, flipped), the R-101 config's (1333, 960) and the R-50 config's
(1333, 1024)):

  (a) the route that existed before `SceneInference(views=...)`: per tile the plain tile operators (`scene_tiles_resized` /
      `scene_tiles`) plus `torch.flip` for the mirrored views, eager `model.aug_test` on its tensor-op route
      (`static_postprocess=False`: what `aug_test` was before the fused route), the rows written into packed slots on the host,
      the existing collect and merge; (a2), for information, is the same with today's `aug_test` (fused route, one D2H per tile);
  (b) `SceneInference(views=...)`: all views filled on the device, one augmented graph per tile batch, `depth` in flight.

    python tests/checks/time_scene_aug.py [--size 4096] [--pairs 3] [--batch 1] [--depth 4] [--out FILE.json]

Both sides are warmed up (one full scene each: graph capture, library algorithm selection, weight packing), then alternate
`pairs` times; every figure is a host clock around a whole scene, which ends in the merge's device-to-host copy.  Prints one
JSON line: the seconds per scene of every round, min / max, rows found, and whether (b) beats (a) by more than twice (a)'s
min-max range.  Both routes are latency- and launch-bound (tile fills and the post-processing move a few MB per tile); the
detector's forwards dominate either side."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SUB, GAP = 1024, 200
VIEWS = [((1333, 960), False), ((1333, 960), True), ((1333, 1024), False), ((1333, 1024), True)]


def synthetic_scene(size, seed=5):
    """8 x 8 blocks of random colour plus fine noise (uint8 BGR)."""
    rng = np.random.RandomState(seed)
    blocks = np.kron(rng.randint(0, 256, size=((size + 7) // 8, (size + 7) // 8, 3)), np.ones((8, 8, 1)))[:size, :size]
    return np.clip(blocks + rng.normal(0, 12, size=(size, size, 3)), 0, 255).astype(np.uint8)


def eager_route(model, si_plain, scene_dev, views, static):
    """Side (a) (static=False) or (a2).  si_plain: a single-view SceneInference, used for its normalisation constants and its
    collect + merge."""
    from orientedreppoints_amd.dota_devkit.img_split import split_origins
    from orientedreppoints_amd.mmdet_models.scene_inference import _Plan, _Shape
    from orientedreppoints_amd.mmdet_ops.scene_ops import scene_tiles, scene_tiles_resized
    dev = scene_dev.device
    origins = split_origins(scene_dev.size(1), scene_dev.size(0), SUB, GAP)
    shapes = [_Shape((SUB, SUB), sc, 32, 1) for sc, _ in views]
    metas = [[dict(sh.metas[0], flip=f)] for sh, (_, f) in zip(shapes, views)]
    m = int(model.test_cfg.max_per_img)
    packed = np.zeros((len(origins), m + 1, 28), np.float32)
    o_dev = torch.tensor(origins, dtype=torch.int32).to(dev)
    for i in range(len(origins)):
        bufs = []
        for sh, (sc, flip) in zip(shapes, views):
            buf = torch.empty((1, 3, sh.pad[1], sh.pad[0]), dtype=torch.float32, device=dev)
            if sh.native:
                scene_tiles(scene_dev, o_dev[i:i + 1], buf, si_plain.mean, si_plain.std, si_plain.to_rgb)
            else:
                scene_tiles_resized(scene_dev, o_dev[i:i + 1], sh.src, sh.new, buf, si_plain.mean, si_plain.std, si_plain.to_rgb)
            if flip:
                buf[..., :sh.new[0]] = buf[..., :sh.new[0]].flip(-1)
            bufs.append(buf)
        model.test_cfg['static_postprocess'] = static
        try:
            with torch.no_grad():
                per_class = model.aug_test(bufs, metas, rescale=True)
        finally:
            model.test_cfg['static_postprocess'] = True
        rows = np.concatenate([np.concatenate([np.zeros((len(r), 18), np.float32), r, np.full((len(r), 1), c, np.float32)], 1)
                               for c, r in enumerate(per_class)])
        packed[i, :len(rows)] = rows
        packed[i, m, 0] = len(rows)
    plan = _Plan()
    plan.rates, plan.origins, plan.origins_dev = [1.0], [origins], [o_dev]
    plan.packed = [torch.from_numpy(packed).to(dev)]
    return si_plain.merge(plan)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--target", type=int, default=800, help="(point, class) pairs above score_thr per view of the first tile")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_scene_aug.py needs a GPU")
    from bench import calibrate_head
    from orientedreppoints_amd.dota_configs import r50_model, test_cfg
    from orientedreppoints_amd.dota_devkit.img_split import split_origins
    from orientedreppoints_amd.mmdet_models import ConfigDict, SceneInference, build_detector
    from orientedreppoints_amd.mmdet_ops.scene_ops import scene_tiles
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_detector(ConfigDict(r50_model), train_cfg=None, test_cfg=ConfigDict(dict(test_cfg))).to(dev).eval()
    scene = synthetic_scene(args.size)
    scene_dev = torch.from_numpy(scene).to(dev)
    si_plain = SceneInference(model, subsize=SUB, gap=GAP)
    first = torch.empty((1, 3, SUB, SUB), dtype=torch.float32, device=dev)
    scene_tiles(scene_dev, torch.zeros((1, 2), dtype=torch.int32, device=dev), first, si_plain.mean, si_plain.std, si_plain.to_rgb)
    calibrate_head(model, first, args.target)
    si = SceneInference(model, subsize=SUB, gap=GAP, batch=args.batch, depth=args.depth, views=VIEWS)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()                                         # (ends in the merge's D2H copy: the device is idle when it returns)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    side_a = lambda: eager_route(model, si_plain, scene_dev, VIEWS, False)
    side_a2 = lambda: eager_route(model, si_plain, scene_dev, VIEWS, True)
    side_b = lambda: si(scene_dev)
    _, out_a = timed(side_a)                               # warm-up of every side
    timed(side_a2)
    _, out_b = timed(side_b)
    t_a, t_a2, t_b = [], [], []
    for _ in range(max(3, args.pairs)):
        t_a.append(timed(side_a)[0])
        t_a2.append(timed(side_a2)[0])
        t_b.append(timed(side_b)[0])
    row = dict(size=args.size, tiles=len(split_origins(args.size, args.size, SUB, GAP)), views=len(VIEWS),
               batch=args.batch, depth=args.depth, eager_s=[round(t, 4) for t in t_a], eager_fused_s=[round(t, 4) for t in t_a2], scene_views_s=[round(t, 4) for t in t_b],
               eager_min_max=[round(min(t_a), 4), round(max(t_a), 4)], scene_views_min_max=[round(min(t_b), 4), round(max(t_b), 4)],
               rows_eager=int(sum(len(c) for c in out_a)), rows_scene_views=int(sum(len(c) for c in out_b)),
               fallback_tiles=si.fallback_tiles,
               bar_met=bool(min(t_a) - max(t_b) > 2 * (max(t_a) - min(t_a))))
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
