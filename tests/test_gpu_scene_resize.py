"""The config's test resize on the MI355X: `orp_scene_tiles_resized` against `resize_oracle` -> `imnormalize` -> zero pad (bit for
bit), `rescale=True` in the captured post-processing against the dynamic path, and `SceneInference(img_scale=...)` end to end
against the composition numpy crop -> `resize_oracle` -> `imnormalize` -> pad -> `simple_test_batch(rescale=True)` ->
translate -> CPU oracle merge.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from test_gpu_scene_inference import (MEAN, NUM_CLASSES, STD, _calibrate_head, _scene, detector, dev, oracle_merge,  # noqa: F401
                                      tile_oracle, translate_rows)
from test_scene_resize import SHAPE_PAIRS, resize_oracle


def pad_to(v, divisor=32):
    return -(-v // divisor) * divisor


def resized_tile_oracle(scene, left, up, src, new, pad, mean=MEAN, std=STD, to_rgb=True):
    """float32 [3, pad_h, pad_w]: the src patch at (left, up) resized to new, normalised, CHW, zeros behind (Pad after Normalize)."""
    from orientedreppoints_amd.mmdet_datasets.imops import imnormalize
    crop = scene[up:up + src[1], left:left + src[0]]
    assert crop.shape[:2] == (src[1], src[0]), "the patch must lie inside the scene"
    out = np.zeros((3, pad[1], pad[0]), np.float32)
    out[:, :new[1], :new[0]] = imnormalize(resize_oracle(crop, new[0], new[1]), mean, std, to_rgb).transpose(2, 0, 1)
    return out


def _check_tiles(dev, scene, scene_dev, origins, src, new, dtypes=(torch.float32, torch.float16, torch.bfloat16),
                 mean=MEAN, std=STD):
    from orientedreppoints_amd.mmdet_datasets.imops import imnormalize
    from orientedreppoints_amd.mmdet_ops.scene_ops import scene_tiles_resized
    pad = (pad_to(new[0]), pad_to(new[1]))
    o_dev = torch.tensor(origins, dtype=torch.int32).to(dev)
    resized = [resize_oracle(scene[u:u + src[1], l:l + src[0]], new[0], new[1]) for l, u in origins]
    for to_rgb in (True, False):
        want = np.zeros((len(origins), 3, pad[1], pad[0]), np.float32)
        for k, r in enumerate(resized):
            want[k, :, :new[1], :new[0]] = imnormalize(r, mean, std, to_rgb).transpose(2, 0, 1)
        for dtype in dtypes:
            out = torch.full((len(origins), 3, pad[1], pad[0]), 7.0, dtype=dtype, device=dev)
            scene_tiles_resized(scene_dev, o_dev, src, new, out, mean, std, to_rgb)
            got = out.cpu()
            assert torch.equal(got, torch.from_numpy(want).to(dtype)), (src, new, to_rgb, dtype)
            if dtype == torch.float32:
                assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))      # bits, signed zeros included
                if pad[0] > new[0]:
                    assert not got[:, :, :, new[0]:].any()
                if pad[1] > new[1]:
                    assert not got[:, :, new[1]:, :].any()


def _edge_origins(W, H, src):
    """The corner, an odd interior origin, and patches flush with the scene's right edge, bottom edge and both."""
    return [(0, 0), (min(13, W - src[0]), min(7, H - src[1])), (W - src[0], 1 if H > src[1] else 0),
            (3 if W > src[0] else 0, H - src[1]), (W - src[0], H - src[1])]


# ---- (4) the tile kernel, bit-exact -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("src,new", SHAPE_PAIRS)
def test_scene_tiles_resized_bit_exact(dev, src, new):
    """fp32 output array_equal (bit patterns) to resize_oracle -> imnormalize -> zero pad of the cropped patch, fp16 / bf16
    equal to torch's cast of that, to_rgb on and off, origins in the corner, at odd offsets and flush with the right and
    bottom edges of a contiguous scene (source pixels are clamped inside the patch: a tile does not see its neighbours)."""
    rng = np.random.RandomState(src[0] + new[0])
    H, W = src[1] + 77, src[0] + 213
    scene = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    _check_tiles(dev, scene, torch.from_numpy(scene).to(dev), _edge_origins(W, H, src), src, new)


@pytest.mark.gpu
def test_scene_tiles_resized_scene_layouts_and_patch_filling_the_scene(dev):
    """An odd-width scene, a strided view at an odd byte offset, and a patch that is the whole scene (what a scene smaller
    than a tile gives), for a small upscale and for the 1024^2 -> 960^2 of the configs."""
    rng = np.random.RandomState(11)
    big = rng.randint(0, 256, size=(1100, 1500 + 7, 3)).astype(np.uint8)
    big_dev = torch.from_numpy(big).to(dev)
    view, view_dev = big[:, 5:5 + 1500], big_dev[:, 5:5 + 1500]
    assert not view_dev.is_contiguous() and view_dev.data_ptr() % 2 == 1
    odd = rng.randint(0, 256, size=(1031, 1277, 3)).astype(np.uint8)
    odd_dev = torch.from_numpy(odd).to(dev)
    for src, new in (((517, 333), (1333, 859)), ((1024, 1024), (960, 960))):
        only32 = (torch.float32,) if src[0] == 1024 else (torch.float32, torch.float16, torch.bfloat16)
        _check_tiles(dev, view, view_dev, _edge_origins(1500, 1100, src)[1:], src, new, only32)
        _check_tiles(dev, odd, odd_dev, _edge_origins(1277, 1031, src)[2:], src, new, only32)
    whole = rng.randint(0, 256, size=(333, 517, 3)).astype(np.uint8)
    _check_tiles(dev, whole, torch.from_numpy(whole).to(dev), [(0, 0)], (517, 333), (1333, 859))


@pytest.mark.gpu
def test_scene_tiles_resized_other_mean_std(dev):
    """A second normalisation (no round numbers, a mean above 255): still numpy's bits."""
    rng = np.random.RandomState(3)
    scene = rng.randint(0, 256, size=(300, 333, 3)).astype(np.uint8)
    _check_tiles(dev, scene, torch.from_numpy(scene).to(dev), [(0, 0), (13, 11), (333 - 200, 300 - 120)], (200, 120), (333, 200),
                 mean=(0.1, 300.7, 127.5), std=(0.3, 255.0, 1.7))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [64, 1024])
def test_scene_tiles_resized_identity_is_scene_tiles(dev, S):
    """new == src: every weight is 0 or 1 and the output equals `scene_tiles`' bit for bit, in all three output types."""
    from orientedreppoints_amd.mmdet_ops.scene_ops import scene_tiles, scene_tiles_resized
    rng = np.random.RandomState(S)
    scene = rng.randint(0, 256, size=(S + 90, S + 301, 3)).astype(np.uint8)
    scene_dev = torch.from_numpy(scene).to(dev)
    origins = _edge_origins(S + 301, S + 90, (S, S))
    o_dev = torch.tensor(origins, dtype=torch.int32).to(dev)
    for to_rgb in (True, False):
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            a = torch.full((len(origins), 3, S, S), 7.0, dtype=dtype, device=dev)
            b = torch.full((len(origins), 3, S, S), 9.0, dtype=dtype, device=dev)
            scene_tiles(scene_dev, o_dev, a, MEAN, STD, to_rgb)
            scene_tiles_resized(scene_dev, o_dev, (S, S), (S, S), b, MEAN, STD, to_rgb)
            bits = torch.int32 if dtype == torch.float32 else torch.int16
            assert torch.equal(a.view(bits), b.view(bits)), (S, to_rgb, dtype)
    want = np.stack([tile_oracle(scene, l, u, S, to_rgb=False) for l, u in origins])
    assert np.array_equal(b.float().cpu().numpy(), torch.from_numpy(want).to(torch.bfloat16).float().numpy())


@pytest.mark.gpu
def test_scene_tiles_resized_argument_checks(dev):
    from orientedreppoints_amd.mmdet_ops.scene_ops import scene_tiles_resized
    scene = torch.zeros((100, 120, 3), dtype=torch.uint8, device=dev)
    origins = torch.zeros((2, 2), dtype=torch.int32, device=dev)
    out = torch.zeros((2, 3, 64, 96), device=dev)
    scene_tiles_resized(scene, origins, (120, 100), (77, 64), out, MEAN, STD)
    with pytest.raises(TypeError):
        scene_tiles_resized(scene.cpu(), origins, (120, 100), (77, 64), out, MEAN, STD)
    with pytest.raises(ValueError, match="uint8"):
        scene_tiles_resized(scene.float(), origins, (120, 100), (77, 64), out, MEAN, STD)
    with pytest.raises(ValueError, match="origins"):
        scene_tiles_resized(scene, origins.long(), (120, 100), (77, 64), out, MEAN, STD)
    with pytest.raises(ValueError, match="tiles"):
        scene_tiles_resized(scene, origins[:1], (120, 100), (77, 64), out, MEAN, STD)
    with pytest.raises(ValueError, match="do not fit"):
        scene_tiles_resized(scene, origins, (121, 100), (77, 64), out, MEAN, STD)
    with pytest.raises(ValueError, match="smaller than the resized patch"):
        scene_tiles_resized(scene, origins, (120, 100), (97, 64), out, MEAN, STD)
    with pytest.raises(ValueError, match="out must be"):
        scene_tiles_resized(scene, origins, (120, 100), (77, 64), out.double(), MEAN, STD)


# ---- (5) rescale in the static post-processing ------------------------------------------------------------------------------
def _same_results(got, want):
    assert len(got) == len(want)
    n = 0
    for g_img, w_img in zip(got, want):
        assert len(g_img) == len(w_img) == NUM_CLASSES
        for g, w in zip(g_img, w_img):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
            n += len(g)
    return n


def _tile_batch(scene, dev, batch, S=256):
    return torch.from_numpy(np.stack([tile_oracle(scene, 100 * j, 60 * j, S) for j in range(batch)])).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("scale_factor", [0.9375, 1333 / 1024, 1.0])
def test_graphed_inference_rescale_equals_the_dynamic_path(dev, detector, scale_factor):
    """`GraphedInference(model, img, metas, rescale=True)(img)` (boxes and rep-points divided inside the captured graph, before
    the NMS) array_equal to `simple_test_batch(img, metas, rescale=True)` on the dynamic path (no static post-processing);
    the tensor-op static path under capture and `PipelinedInference` give the same."""
    from orientedreppoints_amd.mmdet_models import GraphedInference, PipelinedInference
    model, scene = detector
    img = _tile_batch(scene, dev, 2)
    metas = [dict(img_shape=(256, 256, 3), pad_shape=(256, 256, 3), scale_factor=scale_factor, flip=False) for _ in range(2)]
    cfg = model.test_cfg
    cfg['static_postprocess'] = False
    try:
        with torch.no_grad():
            want = model.simple_test_batch(img, metas, rescale=True)
            plain = model.simple_test_batch(img, metas, rescale=False)
    finally:
        cfg['static_postprocess'] = True
    gi = GraphedInference(model, img, metas, rescale=True)
    assert _same_results(gi(img), want) > 0
    assert _same_results(gi(img), want) > 0                                     # a second replay of the same graph
    same_as_plain = all(w.shape == p.shape and np.array_equal(w, p) for w, p in zip(want[0], plain[0]))
    assert same_as_plain == (scale_factor == 1.0)                               # (the division does happen)
    cfg['fused_postprocess'] = False
    try:
        tensor_op = GraphedInference(model, img, metas, rescale=True)
    finally:
        cfg['fused_postprocess'] = True
    _same_results(tensor_op(img), want)
    pipe = PipelinedInference(model, img, metas, depth=2, rescale=True)
    assert pipe.submit(img) is None and pipe.submit(img) is None
    for res in pipe.flush():
        _same_results(res, want)


@pytest.mark.gpu
def test_graphed_inference_without_rescale_is_unchanged(dev, detector):
    """rescale=False (the default): the graph's results are those of the tensor-op static path and of the dynamic path, whatever
    scale factor the metas carry."""
    from orientedreppoints_amd.mmdet_models import GraphedInference
    model, scene = detector
    img = _tile_batch(scene, dev, 1)
    metas = [dict(img_shape=(256, 256, 3), pad_shape=(256, 256, 3), scale_factor=0.9375, flip=False)]
    cfg = model.test_cfg
    got = GraphedInference(model, img, metas)(img)
    cfg['fused_postprocess'] = False
    try:
        with torch.no_grad():
            tensor_op = model.simple_test_batch(img, metas)
    finally:
        cfg['fused_postprocess'] = True
    cfg['static_postprocess'] = False
    try:
        with torch.no_grad():
            dynamic = model.simple_test_batch(img, metas)
    finally:
        cfg['static_postprocess'] = True
    assert _same_results(got, tensor_op) > 0
    _same_results(got, dynamic)


# ---- (6), (7): SceneInference with img_scale ---------------------------------------------------------------------------------
IMG_SCALE = (1333, 960)


@pytest.fixture(scope="module")
def detector1024(dev):
    """An R-50 FPN detector with random weights, calibrated on a 1024^2 patch resized to 960^2 (about 400 (point, class) pairs
    above score_thr there); the library's convolutions in their reproducible mode for the module."""
    from orientedreppoints_amd.dota_configs import r50_model, test_cfg
    from orientedreppoints_amd.mmdet_models import ConfigDict, build_detector
    det_flag = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(0)
    model = build_detector(ConfigDict(r50_model), train_cfg=None, test_cfg=ConfigDict(dict(test_cfg))).to(dev).eval()
    first = resized_tile_oracle(_scene(5, 1024, 1024), 0, 0, (1024, 1024), (960, 960), (960, 960))
    _calibrate_head(model, torch.from_numpy(first[None]).to(dev), 400)
    yield model
    torch.backends.cudnn.deterministic = det_flag


def _expected_resized(model, scene, batch, dev, img_scale, subsize=1024, gap=200):
    """Per class the merged rows of: numpy crop -> resize_oracle -> imnormalize -> pad -> simple_test_batch(rescale=True) in the
    same tile batches -> translate -> CPU oracle merge.  Also returns the number of rows before the merge."""
    from orientedreppoints_amd.dota_devkit.img_split import split_origins
    from orientedreppoints_amd.mmdet_datasets.imops import rescale_size
    H, W = scene.shape[:2]
    src = (min(W, subsize), min(H, subsize))
    new_w, new_h, scale_factor = rescale_size(src, img_scale)
    pad = (pad_to(new_w), pad_to(new_h))
    metas = [dict(img_shape=(new_h, new_w, 3), pad_shape=(pad[1], pad[0], 3), scale_factor=scale_factor, flip=False)
             for _ in range(batch)]
    rows = [[] for _ in range(NUM_CLASSES)]
    origins = split_origins(W, H, subsize, gap)
    for i in range(0, len(origins), batch):
        group = origins[i:i + batch]
        padded = group + [group[-1]] * (batch - len(group))
        img = torch.from_numpy(np.stack([resized_tile_oracle(scene, l, u, src, (new_w, new_h), pad) for l, u in padded])).to(dev)
        with torch.no_grad():
            results = model.simple_test_batch(img, metas, rescale=True)
        for j, (left, up) in enumerate(group):
            for c in range(NUM_CLASSES):
                rows[c].append(translate_rows(results[j][c], left, up, 1.0))
    rows = [np.concatenate(r) for r in rows]
    return [oracle_merge(r)[0] for r in rows], sum(len(r) for r in rows), len(origins)


def _same_per_class(got, want):
    assert len(got) == len(want) == NUM_CLASSES
    for c in range(NUM_CLASSES):
        assert got[c].dtype == np.float64 and got[c].shape == want[c].shape, (c, got[c].shape, want[c].shape)
        assert np.array_equal(got[c], want[c]), c


@pytest.mark.gpu
@pytest.mark.parametrize("batch,depth", [(1, 1), (1, 3), (2, 1), (2, 3)])
def test_scene_inference_img_scale_end_to_end_exact(dev, detector1024, batch, depth):
    """`SceneInference(model, img_scale=(1333, 960))` on a scene of four 1024^2 tiles (each resized to 960^2, scale factor
    0.9375) and on a scene 700 rows high (two 1024 x 700 patches, upscaled to 1333 x 911 and padded to 1344 x 928):
    array_equal per class to the composition above.  One instance serves both scenes: graphs are kept per patch shape."""
    from orientedreppoints_amd.mmdet_models import SceneInference
    model = detector1024
    si = SceneInference(model, batch=batch, depth=depth, img_scale=IMG_SCALE)
    for scene, tiles, src, new, pad in ((_scene(5, 1250, 1400), 4, (1024, 1024), (960, 960), (960, 960)),
                                        (_scene(6, 700, 1300), 2, (1024, 700), (1333, 911), (1344, 928))):
        want, before, n_tiles = _expected_resized(model, scene, batch, dev, IMG_SCALE)
        assert n_tiles == tiles
        kept = sum(len(w) for w in want)
        assert sum(len(w) > 0 for w in want) >= 2 and 0 < kept < before, "the scene must detect in two classes and the merge must suppress"
        for source in (scene, torch.from_numpy(scene).to(dev)):          # a host array and a device tensor; the second call reuses the graphs
            _same_per_class(si(source), want)
        shape = si._shapes[src]
        assert shape.new == new and shape.pad == pad and not shape.native
        assert tuple(shape.pipe.slots[0].static_img.shape) == (batch, 3, pad[1], pad[0])
    assert len(si._shapes) == 2 and si.pipe is None and si.fallback_tiles == 0


@pytest.mark.gpu
def test_scene_inference_img_scale_overflow_fallback(dev, detector1024):
    """static_capacity low enough that tiles overflow: the fallback runs `simple_test_batch(img, metas, rescale=True)` on the
    resized tiles and the result is array_equal to the run with ample capacity."""
    from orientedreppoints_amd.mmdet_models import SceneInference
    model, scene = detector1024, _scene(5, 1250, 1400)
    want = SceneInference(model, batch=2, depth=2, img_scale=IMG_SCALE)(scene)
    model.test_cfg['static_capacity'] = 64
    try:
        si = SceneInference(model, batch=2, depth=2, img_scale=IMG_SCALE)
        got = si(scene)
    finally:
        model.test_cfg['static_capacity'] = 8192
    assert si.fallback_tiles >= 1, "no tile overflowed: the capacity is not low enough for this scene"
    assert sum(len(w) for w in want) > 0
    _same_per_class(got, want)


@pytest.mark.gpu
def test_scene_inference_img_scale_tile_loop_does_not_synchronise(dev, detector1024):
    """With torch's sync debug mode on "error" around the tile loop of the resized route (axis tables, scale factor and graphs
    are all in place after `prepare`) the tiles run without raising, and the mode does fire when something synchronises."""
    from orientedreppoints_amd.mmdet_models import SceneInference
    model, scene = detector1024, _scene(5, 1250, 1400)
    si = SceneInference(model, batch=1, depth=3, img_scale=IMG_SCALE)
    want = si(scene)
    plan = si.prepare(torch.from_numpy(scene).to(dev))
    assert len(plan.origins[0]) == 4 and plan.shapes[0].tables is not None
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        si.run_tiles(plan)
        with pytest.raises(RuntimeError):                        # (the mode is live: a D2H copy of a device tensor raises)
            plan.packed[0][0, 0, 0].item()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    _same_per_class(si.merge(plan), want)


@pytest.mark.gpu
def test_scene_inference_img_scale_identity_is_the_native_route(dev, detector1024):
    """On a scene of full 1024^2 tiles img_scale=(1333, 1024) resolves to scale factor 1.0: the tiles go through `scene_tiles`,
    the graphs divide by 1.0, and the arrays are those of img_scale=None."""
    from orientedreppoints_amd.mmdet_models import SceneInference
    model, scene = detector1024, _scene(5, 1250, 1400)
    want = SceneInference(model, batch=2, depth=2)(scene)
    si = SceneInference(model, batch=2, depth=2, img_scale=(1333, 1024))
    got = si(scene)
    assert si._shapes[(1024, 1024)].native and si._shapes[(1024, 1024)].scale_factor == 1.0
    assert sum(len(w) for w in want) > 0
    _same_per_class(got, want)
