"""The per-patch test resize of `SceneInference(img_scale=...)` without a GPU: `resize_oracle`, the numpy fp32 restatement of the
arithmetic `orp_scene_tiles_resized` is held to, against `imops.imresize`; the planning (`new`, `pad`, `scale_factor`) against
what the host pipeline writes into the metas; `from_config` on the reference's configs; the argument checks."""
import copy

import numpy as np
import pytest

from test_gpu_scene_inference import stub_model

# (src_w, src_h) -> (new_w, new_h): 1024^2 under (1333, 960), an upscale, a 640 x 1024 patch, a small odd patch, an identity
SHAPE_PAIRS = [((1024, 1024), (960, 960)), ((1024, 1024), (1333, 1333)), ((640, 1024), (833, 1333)), ((517, 333), (1333, 859)),
               ((300, 200), (300, 200))]


def resize_axis_oracle(n_in, n_out):
    """(i0, i1, w0, w1) of an axis of n_in -> n_out pixels, align_corners=False, every fp32 operation rounded on its own:
    scale = fp32(in) / fp32(out); src = max(scale * (d + 0.5) - 0.5, 0); i0 = min(int(src), in - 1); i1 = min(i0 + 1, in - 1);
    w1 = src - i0; w0 = 1 - w1."""
    f = np.float32
    scale = f(n_in) / f(n_out)
    src = np.maximum(scale * (np.arange(n_out, dtype=np.float32) + f(0.5)) - f(0.5), f(0))
    assert src.dtype == np.float32
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = src - i0.astype(np.float32)
    w0 = f(1) - w1
    assert w0.dtype == w1.dtype == np.float32
    return i0, i1, w0, w1


def resize_oracle(patch, new_w, new_h):
    """uint8 [h, w, 3] -> uint8 [new_h, new_w, 3]: top = w0x*a + w1x*b, bot = w0x*c + w1x*d, v = w0y*top + w1y*bot, each
    product and sum an fp32 numpy operation of its own (numpy does not contract), then rint (ties to even) and the clamp."""
    h, w = patch.shape[:2]
    x0, x1, wx0, wx1 = resize_axis_oracle(w, new_w)
    y0, y1, wy0, wy1 = resize_axis_oracle(h, new_h)
    src = patch.astype(np.float32)
    wx0, wx1 = wx0[None, :, None], wx1[None, :, None]
    wy0, wy1 = wy0[:, None, None], wy1[:, None, None]
    top = wx0 * src[y0][:, x0] + wx1 * src[y0][:, x1]
    bot = wx0 * src[y1][:, x0] + wx1 * src[y1][:, x1]
    v = wy0 * top + wy1 * bot
    assert v.dtype == np.float32
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def noise_image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def smooth_image(w, h, seed):
    """Double cumulative sum of N(0, 1) * 0.05 + 128, clipped: long gradients, where a resize's last-bit differences show."""
    g = np.random.RandomState(seed).normal(size=(h, w, 3))
    return np.clip(np.cumsum(np.cumsum(g, 0), 1) * 0.05 + 128, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("src,new", SHAPE_PAIRS)
def test_resize_oracle_against_imresize(src, new):
    """No pixel further than one grey level from `imops.imresize`, at most 1e-3 of the pixels different: the band in which
    torch's CPU resize differs from itself between thread counts (5.2e-4 on the smooth image, 1.3e-5 on noise).  A cap, not a
    measurement.  The identity pair is equal."""
    from orientedreppoints_amd.mmdet_datasets.imops import imresize
    images = [noise_image(src[0], src[1], 1 + src[0])]
    if (src, new) == SHAPE_PAIRS[0]:
        images.append(smooth_image(src[0], src[1], 7))
        assert images[1].std() > 5
    for img in images:
        got = resize_oracle(img, new[0], new[1])
        want = imresize(img, new)
        assert got.shape == want.shape == (new[1], new[0], 3) and got.dtype == want.dtype == np.uint8
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        print("resize %s -> %s: %d of %d pixels differ, max %d" % (src, new, int((diff > 0).sum()), diff.size, int(diff.max())))
        if src == new:
            assert np.array_equal(got, img) and np.array_equal(want, img)
        assert diff.max() <= 1
        assert (diff > 0).sum() <= 1e-3 * diff.size


def test_resize_axis_tables_are_the_oracle_s():
    """The tables the wrapper hands to the kernel are the restatement's i0 and w1, bit for bit; identity weights are 0."""
    from orientedreppoints_amd.mmdet_ops.scene_ops import resize_axis
    for n_in, n_out in [(1024, 960), (1024, 1333), (640, 833), (333, 859), (517, 1333), (200, 200), (1, 5), (7, 1)]:
        i0, w1 = resize_axis(n_in, n_out)
        o0, _, _, o1 = resize_axis_oracle(n_in, n_out)
        assert i0.dtype == np.int32 and w1.dtype == np.float32 and i0.shape == w1.shape == (n_out,)
        assert np.array_equal(i0, o0) and np.array_equal(w1.view(np.uint32), o1.view(np.uint32))
        assert i0.min() >= 0 and i0.max() <= n_in - 1 and w1.min() >= 0 and w1.max() < 1
    i0, w1 = resize_axis(200, 200)
    assert np.array_equal(i0, np.arange(200)) and not w1.any()


@pytest.mark.parametrize("img_scale", [(1333, 960), (1333, 1024)])
@pytest.mark.parametrize("patch", [(1024, 1024), (1024, 700), (517, 333)])
def test_planning_matches_the_host_pipeline(patch, img_scale):
    """`new`, `pad` and `scale_factor` of a patch are what RotateResize(keep_ratio=True) -> Normalize -> Pad(32) write into
    `img_shape`, `pad_shape` and `scale_factor`."""
    from orientedreppoints_amd.mmdet_datasets.pipelines import Compose
    from orientedreppoints_amd.mmdet_models import SceneInference
    host = Compose([dict(type='RotateResize', keep_ratio=True),
                    dict(type='Normalize', mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True),
                    dict(type='Pad', size_divisor=32)])
    res = host(dict(img=np.zeros((patch[1], patch[0], 3), np.uint8), scale=img_scale, flip=False))
    si = SceneInference(stub_model(), img_scale=img_scale, batch=2)
    # a scene that yields exactly this patch shape: as wide / high as the patch where that is below the tile size
    W = patch[0] if patch[0] < 1024 else 3000
    H = patch[1] if patch[1] < 1024 else 2500
    ((w, h), shape), = si.tile_shapes(W, H)
    assert (w, h) == (W, H) and shape.src == patch
    assert (shape.new[1], shape.new[0], 3) == tuple(res['img_shape'])
    assert (shape.pad[1], shape.pad[0], 3) == tuple(res['pad_shape']) == res['img'].shape
    assert shape.scale_factor == res['scale_factor'] and np.ndim(shape.scale_factor) == 0
    assert len(shape.metas) == 2
    for m in shape.metas:
        assert tuple(m['img_shape']) == tuple(res['img_shape']) and tuple(m['pad_shape']) == tuple(res['pad_shape'])
        assert m['scale_factor'] == res['scale_factor'] and m['flip'] is False
    if patch == (1024, 1024):
        assert shape.native == (img_scale == (1333, 1024))
        assert shape.new == ((960, 960) if img_scale == (1333, 960) else (1024, 1024))


def test_from_config_reads_the_reference_configs(reference_configs):
    from orientedreppoints_amd.mmdet_models import Config, SceneInference
    want = {'orientedrepoints_r50_demo.py': (1333, 1024), 'orientedrepoints_r101_demo.py': (1333, 960),
            'orientedrepoints_swin_tiny_demo.py': (1333, 960)}
    assert sorted(want) == sorted(reference_configs)
    for name, scale in want.items():
        si = SceneInference.from_config(stub_model(), reference_configs[name], batch=2, gap=100)
        assert si.img_scale == scale and si.size_divisor == 32 and si.to_rgb is True and si.batch == 2 and si.gap == 100
        assert np.array_equal(si.mean, np.asarray((123.675, 116.28, 103.53), np.float32))
        assert np.array_equal(si.std, np.asarray((58.395, 57.12, 57.375), np.float32))
        (_, shape), = si.tile_shapes(4096, 4096)
        assert shape.src == (1024, 1024)
        if scale == (1333, 1024):
            assert shape.scale_factor == 1.0 and shape.native
        else:
            assert shape.scale_factor == 0.9375 and shape.new == shape.pad == (960, 960)

    def edited(**changes):
        cfg = copy.deepcopy(dict(reference_configs['orientedrepoints_r101_demo.py']._cfg_dict))
        aug = cfg['data']['test']['pipeline'][1]
        assert aug['type'] == 'MultiScaleFlipAug' and aug['transforms'][0]['type'] == 'RotateResize'
        for k, v in changes.items():
            if k in ('flip', 'img_scale'):
                aug[k] = v
            else:
                aug['transforms'][0][k] = v
        return Config(cfg)
    assert SceneInference.from_config(stub_model(), edited()).img_scale == (1333, 960)
    with pytest.raises(ValueError, match="flip"):
        SceneInference.from_config(stub_model(), edited(flip=True))
    with pytest.raises(ValueError, match="scales"):
        SceneInference.from_config(stub_model(), edited(img_scale=[(1333, 960), (1333, 1024)]))
    with pytest.raises(ValueError, match="keep_ratio"):
        SceneInference.from_config(stub_model(), edited(keep_ratio=False))
    with pytest.raises(ValueError, match="interpolation"):
        SceneInference.from_config(stub_model(), edited(interpolation='bicubic'))


def test_img_scale_argument_checks():
    """img_scale=None keeps refusing a scene smaller than a tile; with img_scale set the same scene is planned."""
    from orientedreppoints_amd.mmdet_models import SceneInference
    scene = np.zeros((1023, 4000, 3), np.uint8)
    with pytest.raises(ValueError, match="smaller than a 1024 tile"):
        SceneInference(stub_model(), subsize=1024, gap=200)(scene)
    with pytest.raises(ValueError, match="smaller than a 1024 tile"):
        SceneInference(stub_model(), subsize=1024, gap=200).tile_shapes(4000, 1023)
    si = SceneInference(stub_model(), subsize=1024, gap=200, img_scale=(1333, 960))
    ((w, h), shape), = si.tile_shapes(4000, 1023)
    assert (w, h) == (4000, 1023) and shape.src == (1024, 1023) and not shape.native
    assert shape.new == (961, 960) and shape.pad == (992, 960)
    with pytest.raises(AttributeError):                      # past the planning: the stub has no parameters to find a device by
        si(scene)
    for bad in ((1333,), (1333, 0), (1333, 960, 3)):
        with pytest.raises(ValueError, match="img_scale"):
            SceneInference(stub_model(), img_scale=bad)
    with pytest.raises(ValueError, match="size_divisor"):
        SceneInference(stub_model(), img_scale=(1333, 960), size_divisor=12)


def test_rescale_needs_one_scale_factor_per_image():
    """The captured path takes `rescale=True` with a scalar scale factor only; the per-axis 4-vector of keep_ratio=False is
    refused before anything is captured."""
    import torch
    from orientedreppoints_amd import dota_configs
    from orientedreppoints_amd.mmdet_models import ConfigDict, GraphedInference, build_detector
    from orientedreppoints_amd.mmdet_models.core import is_scalar_scale
    assert is_scalar_scale(0.9375) and is_scalar_scale(1) and is_scalar_scale(np.float32(1.3))
    assert not is_scalar_scale(np.array([1.3, 1.2, 1.3, 1.2], np.float32)) and not is_scalar_scale(torch.tensor(1.0))
    model = build_detector(ConfigDict(dota_configs.r50_model), train_cfg=None, test_cfg=ConfigDict(dota_configs.test_cfg)).eval()
    metas = [dict(img_shape=(64, 64, 3), pad_shape=(64, 64, 3), scale_factor=np.array([1.3, 1.2, 1.3, 1.2], np.float32), flip=False)]
    with pytest.raises(ValueError, match="one scale factor per image"):
        GraphedInference(model, torch.zeros(1, 3, 64, 64), metas, rescale=True)
