"""The data side of a training run, timed two ways on 1024^2 sources in batches of two, for the R-50 and the Swin-T train
pipelines of the reference configs (scales drawn up to 1333 x 1280 per sample):

  (host)    the host `Compose`: every image step on the CPU (mmdet_datasets/imops.py), ending in CPU tensors -- the hand-over to
            the detector (collate, upload) is NOT counted, which favours this side;
  (device)  `DeviceTrainPipeline`: `.host` (draws and boxes) then `.collate` (two pinned uploads, one `train_images` call), ending in
            a device synchronise -- planning and H2D are counted.

    python tests/checks/time_train_pipeline.py [--batches 8] [--runs 3] [--host-only] [--out FILE.jsonl]

One process; both sides see the same seeds, so they make the same draws.  One run of each side is dropped (warm-up), then the
two sides alternate `runs` times; every figure is a host clock around `batches` batches.  Then the two kernels alone: a captured
graph of K `train_images` calls over K different buffer sets (more bytes than the last-level cache holds), replayed and timed
with device events, against the memory floor (source bytes in, 12 B per output pixel out, and for rotating samples 3 B per
resized pixel to scratch and back).  Prints one JSON line per configuration; `--host-only` needs no GPU."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
HEAD = [dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True),
        dict(type='CorrectBox', correct_rbbox=True, refine_rbbox=True)]
TAIL = [dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]
SCALES = dict(img_scale=[(1333, 768), (1333, 1280)], keep_ratio=True, multiscale_mode='range', clamp_rbbox=False)
PIPELINES = {
    'r50': HEAD + [dict(type='RotateResize', **SCALES), dict(type='RotateRandomFlip', flip_ratio=0.5),
                   dict(type='Normalize', **NORM), dict(type='Pad', size_divisor=32)] + TAIL,
    'swin_tiny': HEAD + [dict(type='PolyResize', **SCALES), dict(type='PolyRandomFlip', flip_ratio=0.5),
                         dict(type='HSVAugment', hgain=0.015, sgain=0.7, vgain=0.4),
                         dict(type='PolyRandomRotate', rotate_ratio=0.5, angles_range=180, auto_bound=False),
                         dict(type='Pad', size_divisor=32), dict(type='Normalize', **NORM)] + TAIL,
}
README_RATES = {'r50': (65, 77), 'swin_tiny': (45, 50)}          # images/s of `bench.py --mode train` (README)


def write_dataset(folder, n_img, size, seed=5):
    from orientedreppoints_amd.mmdet_datasets.dota import DotaDataset
    rng = np.random.RandomState(seed)
    images, anns, aid = [], [], 0
    for i in range(n_img):
        name = 'S%04d.npy' % i
        blocks = np.kron(rng.randint(0, 256, size=(size // 8, size // 8, 3)), np.ones((8, 8, 1)))
        np.save(os.path.join(folder, name), np.clip(blocks + rng.normal(0, 12, size=blocks.shape), 0, 255).astype(np.uint8))
        images.append(dict(id=i, file_name=name, width=size, height=size))
        for _ in range(40):
            cx, cy = rng.uniform(0.2 * size, 0.8 * size, 2)
            w, h, a = rng.uniform(16, 120), rng.uniform(16, 120), rng.uniform(-np.pi, np.pi)
            base = np.array([[-.5, -.5], [.5, -.5], [.5, .5], [-.5, .5]]) * [w, h]
            q = base.dot(np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])) + [cx, cy]
            anns.append(dict(id=aid, image_id=i, category_id=int(aid % 15 + 1), bbox=[float(v) for v in q.reshape(-1)],
                             iscrowd=0, area=1.0, segmentation=[]))
            aid += 1
    ann_file = os.path.join(folder, 'ann.json')
    with open(ann_file, 'w') as f:
        json.dump(dict(images=images, annotations=anns,
                       categories=[dict(id=i + 1, name=n) for i, n in enumerate(DotaDataset.CLASSES)]), f)
    return ann_file


def floor_bytes(plan):
    d = plan.desc
    src = int((d['src_h'].astype(np.int64) * d['src_w'] * 3).sum())
    out = 12 * plan.out_shape[0] * plan.out_shape[2] * plan.out_shape[3]
    rot = int((d['new_h'].astype(np.int64) * d['new_w'] * 3 * 2 * (d['rotate'] != 0)).sum())
    return src + out + rot


def time_kernels(name, dev, size, sets=8, replays=20):
    """Both kernels through the entry point, a fixed worst-case plan: two `size`^2 sources resized to 1280^2 (the largest the
    configs draw from a square source), for the Swin-T pipeline both rotating."""
    from orientedreppoints_amd.mmdet_datasets import imops
    from orientedreppoints_amd.mmdet_ops.train_image_ops import TrainImagePlan, train_images
    rotate = name == 'swin_tiny'
    inv = imops.invert_affine(imops.rotation_matrix_2d((1280 / 2 - 0.5, 1280 / 2 - 0.5), 37.3, 1)) if rotate else None
    plans = [dict(src=(size, size), new=(1280, 1280), pad=(1280, 1280), flip=f, inv=inv) for f in (None, 'horizontal')]
    plan = TrainImagePlan(plans, NORM['mean'], NORM['std'], True, rotate)
    table = torch.from_numpy(plan.table).to(dev)
    g = torch.Generator(device='cpu').manual_seed(1)
    bufs = [(torch.randint(0, 256, (plan.images_bytes,), dtype=torch.uint8, generator=g).to(dev),
             torch.empty(plan.out_shape, dtype=torch.float32, device=dev),
             torch.empty(max(plan.scratch_bytes, 16), dtype=torch.uint8, device=dev)) for _ in range(sets)]
    for imgs, out, scratch in bufs:
        train_images(imgs, table, plan, out, scratch=scratch)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for imgs, out, scratch in bufs:
            train_images(imgs, table, plan, out, scratch=scratch)
    graph.replay()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        per_call.append(a.elapsed_time(b) * 1e-3 / (replays * sets))
    fb = floor_bytes(plan)
    return dict(kernel_call_us=[round(t * 1e6, 1) for t in per_call], floor_bytes=fb, stage_b=rotate,
                achieved_GBps=[round(fb / t * 1e-9, 1) for t in per_call])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not args.host_only and not torch.cuda.is_available():
        raise SystemExit("time_train_pipeline.py needs a GPU (or --host-only)")
    from orientedreppoints_amd.mmdet_datasets import DeviceTrainPipeline, DotaDataset
    B = 2
    rows = []
    with tempfile.TemporaryDirectory() as folder:
        ann_file = write_dataset(folder, 4, args.size)
        for name, steps in PIPELINES.items():
            host_ds = DotaDataset(ann_file=ann_file, img_prefix=folder, pipeline=steps)
            n = args.batches * B

            def seed(run):
                np.random.seed(100 + run)
                random.seed(100 + run)

            def side_host(run):
                seed(run)
                t0 = time.perf_counter()
                for k in range(n):
                    host_ds[k % len(host_ds)]
                return n / (time.perf_counter() - t0)
            row = dict(config=name, size=args.size, batch=B, batches=args.batches, cpus=len(os.sched_getaffinity(0)),
                       torch_threads=torch.get_num_threads())
            if args.host_only:
                side_host(0)
                row['host_samples_per_s'] = [round(side_host(r), 2) for r in range(1, args.runs + 1)]
            else:
                dev = torch.device("cuda:0")
                dp = DeviceTrainPipeline.from_config(steps, device=dev)
                dev_ds = DotaDataset(ann_file=ann_file, img_prefix=folder, pipeline=[dp.host])

                def side_device(run):
                    seed(run)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for k in range(0, n, B):
                        batch = dp.collate([dev_ds[(k + j) % len(dev_ds)] for j in range(B)])
                    torch.cuda.synchronize()
                    del batch
                    return n / (time.perf_counter() - t0)
                side_host(0)
                side_device(0)
                t_h, t_d = [], []
                for r in range(1, args.runs + 1):
                    t_h.append(side_host(r))
                    t_d.append(side_device(r))
                row['host_samples_per_s'] = [round(t, 2) for t in t_h]
                row['device_samples_per_s'] = [round(t, 2) for t in t_d]
                row['worth_having'] = bool(min(t_d) > max(t_h))
                lo, hi = README_RATES[name]
                row['training_rate_images_per_s'] = [lo, hi]
                row['host_keeps_up'] = bool(min(t_h) >= hi)
                row['device_keeps_up'] = bool(min(t_d) >= hi)
                row.update(time_kernels(name, dev, args.size))
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.out:
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
