"""The device train pipeline without a GPU: `warp_oracle` (the rotation `orp_train_images` is held to) against
`imops.warp_affine`; the oracle of the whole image half against the host `Compose` of the three reference configs; the host
half of `DeviceTrainPipeline` draw for draw against the host classes; the configurations it refuses; and the new source's
register and scratch use when compiled for gfx950.

Observed while writing (this suite's shapes): see the prints of each test (`pytest -s`); the largest shares are recorded in
docs/notebook/round26.md."""
import copy
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from test_scene_resize import noise_image, smooth_image
from train_pipeline_oracle import (R101, R50, SWIN, image_half_oracle, rotation_inverse, same_value, seeded, small_train_pipeline,
                                   warp_oracle, write_dataset)

ANGLES = [0, 90, 180, 37.3, -151.9, 0.01]


@pytest.mark.parametrize("angle", ANGLES)
@pytest.mark.parametrize("w,h", [(131, 97), (64, 64)])
def test_warp_oracle_against_warp_affine(w, h, angle):
    """Equal at 0, 90 and 180 degrees; otherwise no pixel further than one grey level from `imops.warp_affine` and at most 1e-3
    of the pixels different (`test_resize_oracle_against_imresize`'s cap: a condition, not a measurement)."""
    from orientedreppoints_amd.mmdet_datasets import imops
    m = imops.rotation_matrix_2d((w / 2 - 0.5, h / 2 - 0.5), angle, 1)
    for img in (noise_image(w, h, 5 + w), smooth_image(w, h, 9 + w)):
        got = warp_oracle(img, imops.invert_affine(m))
        want = imops.warp_affine(img, m, (w, h))
        assert got.shape == want.shape == (h, w, 3) and got.dtype == want.dtype == np.uint8
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        print("warp %d x %d by %s: %d of %d pixels differ, max %d" % (w, h, angle, int((diff > 0).sum()), diff.size, int(diff.max())))
        if angle in (0, 90, 180):
            assert np.array_equal(got, want)
        if angle == 0:
            assert np.array_equal(got, img)
        assert diff.max() <= 1
        assert (diff > 0).sum() <= 1e-3 * diff.size


def _datasets(tmp_path, cfg, all_metas=False):
    from orientedreppoints_amd.mmdet_datasets import DeviceTrainPipeline, DotaDataset
    ann_file, arrays = write_dataset(str(tmp_path))
    steps = small_train_pipeline(cfg, all_metas)
    host = DotaDataset(ann_file=ann_file, img_prefix=str(tmp_path), pipeline=steps)
    dp = DeviceTrainPipeline.from_config(steps)
    dev = DotaDataset(ann_file=ann_file, img_prefix=str(tmp_path), pipeline=[dp.host])
    return host, dev, dp, arrays


# seeds chosen on the CPU so that the oracle alone is inside the caps below
IMAGE_SEEDS = {R50: range(0, 8), R101: range(8, 16), SWIN: range(16, 28)}


@pytest.mark.parametrize("name", [R50, R101, SWIN])
def test_image_half_oracle_against_the_host_compose(tmp_path, reference_configs, name):
    """Same seeds, the config's train pipeline (scales around 64 - 128): boxes, labels and metas equal; the oracle's image
    against the host's: without rotation at most 1e-3 of the pixels differ (one resampling), each by at most one grey level
    (1 / std[c] plus an ulp); with rotation at most 5e-3 differ (a one-level difference after the resize reaches at most four
    warp outputs, plus the warp's own 1e-3), each by at most two grey levels."""
    host, dev, dp, arrays = _datasets(tmp_path, reference_configs[name])
    rotated = flipped = 0
    for seed in IMAGE_SEEDS[name]:
        idx = seed % 3
        want, got = seeded(host, idx, seed), seeded(dev, idx, seed)
        assert (want is None) == (got is None)
        if want is None:
            continue
        assert same_value(want['img_meta'], got['img_meta'])
        assert np.array_equal(want['gt_bboxes'].numpy(), got['gt_bboxes']) and np.array_equal(want['gt_labels'].numpy(), got['gt_labels'])
        plan = got['plan']
        assert np.array_equal(got['img'], arrays[idx]) and got['img'].dtype == np.uint8
        img = image_half_oracle(got['img'], plan, dp.mean, dp.std, dp.to_rgb, dp.pad_before_normalize)
        ref = want['img'].numpy()
        assert img.shape == ref.shape and ref.dtype == np.float32
        new_h, new_w = plan['new']
        diff = np.abs(img - ref)
        inside = diff[:, :new_h, :new_w]
        outside = diff.copy()
        outside[:, :new_h, :new_w] = 0
        assert not outside.any(), "the padding must be equal"
        levels = 2 if plan['inv'] is not None else 1
        share = float((inside > 0).sum()) / inside.size
        print("%s seed %d: rotate %s flip %s, %d of %d differ (%.2e), max %.4f" % (
            name, seed, plan['inv'] is not None, plan['flip'], int((inside > 0).sum()), inside.size, share, float(inside.max())))
        # levels / std[c] (mean and std are per output channel, as the planes are) plus an ulp: the normalised values lie
        # inside (-4, 4), where the difference of two rounded quotients is off by at most one spacing of 4
        bound = np.float32(levels) / dp.std + np.spacing(np.float32(4.0))
        assert np.abs(ref).max() < 4
        assert np.all(inside <= bound[:, None, None])
        assert share <= (5e-3 if plan['inv'] is not None else 1e-3)
        rotated += plan['inv'] is not None
        flipped += plan['flip'] is not None
    assert flipped >= 1
    assert (rotated >= 2) if name == SWIN else (rotated == 0)


@pytest.mark.parametrize("name", [R50, R101, SWIN])
def test_host_half_makes_the_host_pipeline_s_draws(tmp_path, reference_configs, name):
    """200 seeded samples: the device pipeline's host half returns None exactly where the host `Compose` does, and otherwise
    the same boxes, labels and every meta key (draws included: scale, flip, direction, rotation, angle) -- and the state of
    both random generators afterwards is the same, so the next sample draws alike too.  It never initialises the GPU."""
    import random
    import torch
    host, dev, dp, arrays = _datasets(tmp_path, reference_configs[name], all_metas=True)
    nones = rotated = vertical = 0
    for seed in range(200):
        idx = seed % 4
        want = seeded(host, idx, 1000 + seed)
        state_np, state_py = np.random.get_state(), random.getstate()
        got = seeded(dev, idx, 1000 + seed)
        after = np.random.get_state()
        assert state_np[0] == after[0] and np.array_equal(state_np[1], after[1]) and state_np[2:] == after[2:]
        assert state_py == random.getstate()
        assert (want is None) == (got is None), seed
        if want is None:
            nones += 1
            continue
        assert same_value(want['img_meta'], got['img_meta']), (seed, want['img_meta'], got['img_meta'])
        assert got['gt_bboxes'].dtype == np.float32 and np.array_equal(want['gt_bboxes'].numpy(), got['gt_bboxes'])
        assert got['gt_labels'].dtype == np.int64 and np.array_equal(want['gt_labels'].numpy(), got['gt_labels'])
        meta, plan = got['img_meta'], got['plan']
        assert plan['src'] == arrays[idx].shape[:2] and plan['new'] == tuple(meta['img_shape'][:2])
        assert plan['pad'] == tuple(meta['pad_shape'][:2]) == tuple(want['img'].shape[1:])
        assert (plan['flip'] is not None) == bool(meta['flip'])
        assert (plan['inv'] is not None) == bool(meta.get('rotate', False))
        rotated += plan['inv'] is not None
        vertical += plan['flip'] == 'vertical'
    if name == SWIN:
        assert nones >= 1 and rotated >= 50 and vertical >= 10
    else:
        assert nones == 0 and rotated == 0 and vertical == 0
    assert not torch.cuda.is_initialized()


def test_refused_configurations(reference_configs):
    """What the device half cannot do is refused at construction, with the step's name."""
    from orientedreppoints_amd.mmdet_datasets import DeviceTrainPipeline

    def edited(name, step_type, **changes):
        steps = copy.deepcopy(small_train_pipeline(reference_configs[name]))
        for s in steps:
            if s['type'] == step_type:
                s.update(changes)
        return steps
    for name in (R50, R101, SWIN):
        dp = DeviceTrainPipeline.from_config(small_train_pipeline(reference_configs[name]))
        assert dp.pad_before_normalize == (name == SWIN) and dp.to_rgb is True
        assert np.array_equal(dp.mean, np.asarray((123.675, 116.28, 103.53), np.float32))
        assert np.array_equal(dp.std, np.asarray((58.395, 57.12, 57.375), np.float32))
    with pytest.raises(ValueError, match="RotateResize.*keep_ratio"):
        DeviceTrainPipeline.from_config(edited(R50, 'RotateResize', keep_ratio=False))
    with pytest.raises(ValueError, match="PolyResize.*interpolation"):
        DeviceTrainPipeline.from_config(edited(SWIN, 'PolyResize', interpolation='bicubic'))
    with pytest.raises(ValueError, match="PolyRandomRotate.*auto_bound"):
        DeviceTrainPipeline.from_config(edited(SWIN, 'PolyRandomRotate', auto_bound=True))
    with pytest.raises(ValueError, match="LoadImageFromFile.*to_float32"):
        DeviceTrainPipeline.from_config(edited(R50, 'LoadImageFromFile', to_float32=True))
    steps = small_train_pipeline(reference_configs[R50])
    with pytest.raises(ValueError, match="MosaicPipeline"):
        DeviceTrainPipeline.from_config(steps[:3] + [dict(type='MosaicPipeline', individual_pipeline=[], pad_val=114)] + steps[3:])
    with pytest.raises(ValueError, match="RotateRandomFlip.*order"):                     # Normalize in front of the flip
        DeviceTrainPipeline.from_config(steps[:4] + [steps[5], steps[4]] + steps[6:])
    with pytest.raises(ValueError, match="Pad"):
        DeviceTrainPipeline.from_config(edited(R50, 'Pad', size_divisor=None, size=(128, 128)))
    dp = DeviceTrainPipeline.from_config(steps)
    with pytest.raises(ValueError, match="mosaic"):                                      # a list of images reaching the host half
        dp.host.loaders[:] = [lambda r: [r, r]]
        dp.host(dict())


def test_kernels_compile_without_spills_or_scratch():
    """csrc/orp_train_images.hip with the library's flags: both kernels spill nothing and use no scratch memory."""
    from orientedreppoints_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not found")
    src = os.path.join(build.CSRC, "orp_train_images.hip")
    flags = dict(build.SOURCES)["orp_train_images.hip"]
    assert flags == ["-ffp-contract=off"]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC] + build.COMMON + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "t.o")]
        r = subprocess.run(cmd, cwd=build.CSRC, stderr=subprocess.PIPE, stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        def num(key):
            return int(re.search(re.escape(key) + r":\s+(\d+)", blk).group(1))
        seen[blk.split()[0]] = dict(vgprs=num("VGPRs"), scratch=num("ScratchSize [bytes/lane]"), sgpr_spill=num("SGPRs Spill"),
                                    vgpr_spill=num("VGPRs Spill"), lds=num("LDS Size [bytes/block]"))
    assert len(seen) == 2 and any("train_resize_kernel" in k for k in seen) and any("train_rotate_kernel" in k for k in seen), sorted(seen)
    for name, u in seen.items():
        print(name, u)
        assert u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0 and u["scratch"] == 0, (name, u)
        assert u["vgprs"] <= 128 and u["lds"] <= 8192, (name, u)
