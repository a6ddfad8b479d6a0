"""`SceneInference(views=...)`: flip and multi-scale test-time augmentation on the captured scene path, end to end against a
restatement from what existed before it -- the plain tile operators plus `torch.flip`, the eager static `aug_test` per tile, the
existing collect and merge --, with the overflow fallback and without host synchronisation in the tile loop.  Exact comparisons;
the fixture pattern is tests/test_gpu_scene_inference.py's (256 tiles with a gap of 64 over a 600 x 700 scene, calibrated R-50)."""
import numpy as np
import pytest
import torch

from test_gpu_scene_inference import GAP, MEAN, NUM_CLASSES, STD, SUB, _calibrate_head, _scene, tile_oracle

FLIP_ONLY = [(None, False), (None, True)]
TWO_SCALES = [((320, 320), False), ((320, 320), True), ((210, 210), False), ((210, 210), True)]     # factors 1.25 and 210 / 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def detector(dev):
    from orientedreppoints_amd.dota_configs import r50_model, test_cfg
    from orientedreppoints_amd.mmdet_models import ConfigDict, build_detector
    det_flag = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(0)
    model = build_detector(ConfigDict(r50_model), train_cfg=None, test_cfg=ConfigDict(dict(test_cfg))).to(dev).eval()
    scene = _scene()
    _calibrate_head(model, torch.from_numpy(tile_oracle(scene, 0, 0, SUB)[None]).to(dev), 300)
    yield model, scene
    torch.backends.cudnn.deterministic = det_flag


def restated(model, scene, views, batch, dev):
    """Per tile batch: every view from `scene_tiles` / `scene_tiles_resized` (+ `torch.flip` inside the resized width), the
    eager static aug_test on them (for a batch of two: its two steps, the views' forwards on the batch and
    `fused_postprocess_views` per tile), rows into packed slots, then the existing `scene_collect` and merge."""
    from orientedreppoints_amd.dota_devkit.img_split import split_origins
    from orientedreppoints_amd.mmdet_models import SceneInference
    from orientedreppoints_amd.mmdet_models.scene_inference import _Plan, _Shape
    from orientedreppoints_amd.mmdet_ops.scene_ops import scene_tiles, scene_tiles_resized
    scene_dev = torch.from_numpy(scene).to(dev)
    origins = split_origins(scene.shape[1], scene.shape[0], SUB, GAP)
    shapes = [_Shape((SUB, SUB), sc, 32, batch) for sc, _ in views]
    metas = [[dict(m, flip=f) for m in sh.metas] for sh, (_, f) in zip(shapes, views)]
    m = int(model.test_cfg.max_per_img)
    packed = np.zeros((len(origins), m + 1, 28), np.float32)
    for i in range(0, len(origins), batch):
        group = origins[i:i + batch]
        o_dev = torch.tensor(group + [group[-1]] * (batch - len(group)), dtype=torch.int32).to(dev)
        bufs = []
        for sh, (sc, flip) in zip(shapes, views):
            buf = torch.empty((batch, 3, sh.pad[1], sh.pad[0]), dtype=torch.float32, device=dev)
            if sc is None:
                scene_tiles(scene_dev, o_dev, buf, MEAN, STD, True)
            else:
                scene_tiles_resized(scene_dev, o_dev, sh.src, sh.new, buf, MEAN, STD, True)
            if flip:
                buf[..., :sh.new[0]] = buf[..., :sh.new[0]].flip(-1)
            bufs.append(buf)
        with torch.no_grad():
            if batch == 1:
                results = [model.aug_test(bufs, metas, rescale=True)]
            else:
                outs = [model.bbox_head(model.extract_feat(b)) for b in bufs]
                results = [model.aug_result_packed(model.aug_postprocess_static(outs, metas, True, j)) for j in range(batch)]
        for j in range(len(group)):
            rows = np.concatenate([np.concatenate([np.zeros((len(r), 18), np.float32), r, np.full((len(r), 1), c, np.float32)], 1)
                                   for c, r in enumerate(results[j])])
            packed[i + j, :len(rows)] = rows
            packed[i + j, m, 0] = len(rows)
    plan = _Plan()
    plan.rates, plan.origins = [1.0], [origins]
    plan.origins_dev = [torch.tensor(origins, dtype=torch.int32).to(dev)]
    plan.packed = [torch.from_numpy(packed).to(dev)]
    return SceneInference(model, subsize=SUB, gap=GAP).merge(plan), int(packed[:, m, 0].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("views", [FLIP_ONLY, TWO_SCALES], ids=["flip", "two_scales_flip"])
def test_scene_views_equal_the_restatement(dev, detector, views, batch):
    from orientedreppoints_amd.mmdet_models import SceneInference
    model, scene = detector
    want, rows = restated(model, scene, views, batch, dev)
    plain = SceneInference(model, subsize=SUB, gap=GAP, batch=batch, depth=2)(scene)
    assert sum(len(w) > 0 for w in want) >= 2 and rows > sum(len(p) for p in plain)     # (the views add detections)
    si = SceneInference(model, subsize=SUB, gap=GAP, batch=batch, depth=2, views=views)
    for source in (scene, torch.from_numpy(scene).to(dev)):              # the second call reuses the graphs
        got = si(source)
        assert len(got) == NUM_CLASSES
        for c in range(NUM_CLASSES):
            assert got[c].dtype == np.float64 and got[c].shape == want[c].shape, (c, got[c].shape, want[c].shape)
            assert np.array_equal(got[c], want[c]), c
    assert si.fallback_tiles == 0 and si.pipe is None and len(si._aug_shapes) == 1


@pytest.mark.gpu
def test_scene_views_overflow_takes_the_fallback(dev, detector):
    """static_capacity low enough that tiles overflow: they are re-run through model.aug_test, counted, and the result equals
    the run with ample capacity."""
    from orientedreppoints_amd.mmdet_models import SceneInference
    model, scene = detector
    want = SceneInference(model, subsize=SUB, gap=GAP, batch=1, depth=2, views=FLIP_ONLY)(scene)
    model.test_cfg['static_capacity'] = 64
    try:
        si = SceneInference(model, subsize=SUB, gap=GAP, batch=1, depth=2, views=FLIP_ONLY)
        got = si(scene)
    finally:
        model.test_cfg['static_capacity'] = 8192
    assert si.fallback_tiles >= 1, "no tile overflowed: the capacity is not low enough for this scene"
    assert sum(len(w) for w in want) > 0
    for c in range(NUM_CLASSES):
        assert np.array_equal(got[c], want[c]), c


@pytest.mark.gpu
def test_scene_views_tile_loop_does_not_synchronise(dev, detector):
    """torch's sync debug mode on "error" around the tile loop (flipped and resized views filled, augmented graphs replayed)."""
    from orientedreppoints_amd.mmdet_models import SceneInference
    model, scene = detector
    si = SceneInference(model, subsize=SUB, gap=GAP, batch=1, depth=3, views=TWO_SCALES)
    want = si(scene)
    plan = si.prepare(torch.from_numpy(scene).to(dev))
    assert len(plan.origins[0]) >= 6
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        si.run_tiles(plan)
        with pytest.raises(RuntimeError):                        # (the mode is live: a D2H copy of a device tensor raises)
            plan.packed[0][0, 0, 0].item()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    got = si.merge(plan)
    for c in range(NUM_CLASSES):
        assert np.array_equal(got[c], want[c])
