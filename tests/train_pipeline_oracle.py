"""A numpy oracle of the image half of the train pipelines, the arithmetic `orp_train_images` is held to bit for bit:
`resize_oracle` (tests/test_scene_resize.py), index flips, `warp_oracle` (the rotation of include/orp_hip.h, line by line),
`imnormalize`, and the three padding regions.  Shared by the CPU and the GPU tests; nothing here needs a device."""
import json
import os

import numpy as np

from test_scene_resize import resize_oracle


def rotation_inverse(w, h, angle):
    """The inverse matrix `PolyRandomRotate` warps a w x h image with for `angle` degrees (about (w/2 - 0.5, h/2 - 0.5))."""
    from orientedreppoints_amd.mmdet_datasets import imops
    return imops.invert_affine(imops.rotation_matrix_2d((w / 2 - 0.5, h / 2 - 0.5), angle, 1))


def warp_oracle(img, inv):
    """uint8 [h, w, 3] -> uint8 [h, w, 3].  For output pixel (x, y), in float64 with every operation rounded on its own:
    sx = (i00*x + i01*y) + i02, sy likewise; x0 = floor(sx), fx = (float)(sx - x0); y0, fy likewise.  Then in fp32 with every
    product and sum rounded on its own: top = (1 - fx)*a + fx*b, bot = (1 - fx)*c + fx*d, v = (1 - fy)*top + fy*bot; taps
    outside the image are 0; rint (ties to even), clamp to [0, 255]."""
    h, w = img.shape[:2]
    inv = np.asarray(inv, np.float64)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    sx = (inv[0, 0] * xs + inv[0, 1] * ys) + inv[0, 2]
    sy = (inv[1, 0] * xs + inv[1, 1] * ys) + inv[1, 2]
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0).astype(np.float32)[..., None], (sy - y0).astype(np.float32)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    src = img.astype(np.float32)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        v = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        v[~inside] = 0
        return v
    one = np.float32(1)
    top = (one - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1)
    bot = (one - fx) * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1)
    v = (one - fy) * top + fy * bot
    assert fx.dtype == fy.dtype == top.dtype == bot.dtype == v.dtype == np.float32
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def resized_oracle(img, plan):
    """The uint8 image after the resize, the flip and the rotation of `plan` (dict: src, new, pad as (h, w); flip None /
    'horizontal' / 'vertical'; inv None or the 2 x 3 inverse matrix)."""
    new_h, new_w = plan['new']
    assert tuple(img.shape[:2]) == tuple(plan['src'])
    r = resize_oracle(img, new_w, new_h)
    if plan.get('flip') == 'horizontal':
        r = r[:, ::-1]
    elif plan.get('flip') == 'vertical':
        r = r[::-1]
    else:
        assert plan.get('flip') is None
    if plan.get('inv') is not None:
        r = warp_oracle(np.ascontiguousarray(r), plan['inv'])
    return r


def image_half_oracle(img, plan, mean, std, to_rgb, pad_before_normalize, out_hw=None):
    """float32 [3, H, W] (H, W = out_hw, the sample's pad shape when None): the normalised image in [:new_h, :new_w]; the
    rest of the pad shape 0 (`Normalize` before `Pad`) or the normalised zero byte (`Pad` before `Normalize`); 0 beyond."""
    from orientedreppoints_amd.mmdet_datasets.imops import imnormalize
    (new_h, new_w), (pad_h, pad_w) = plan['new'], plan['pad']
    H, W = (pad_h, pad_w) if out_hw is None else out_hw
    out = np.zeros((3, H, W), np.float32)
    if pad_before_normalize:
        out[:, :pad_h, :pad_w] = imnormalize(np.zeros((1, 1, 3), np.uint8), mean, std, to_rgb).reshape(3, 1, 1)
    out[:, :new_h, :new_w] = imnormalize(resized_oracle(img, plan), mean, std, to_rgb).transpose(2, 0, 1)
    return out


def batch_oracle(images, plans, mean, std, to_rgb, pad_before_normalize, out_hw=None):
    """float32 [B, 3, H, W]; H, W are the maxima of the pad shapes when out_hw is None (the collate)."""
    if out_hw is None:
        out_hw = (max(p['pad'][0] for p in plans), max(p['pad'][1] for p in plans))
    return np.stack([image_half_oracle(i, p, mean, std, to_rgb, pad_before_normalize, out_hw) for i, p in zip(images, plans)])


# ---- the reference configs' train pipelines on a small dataset ---------------------------------------------------------------
R50, R101, SWIN = 'orientedrepoints_r50_demo.py', 'orientedrepoints_r101_demo.py', 'orientedrepoints_swin_tiny_demo.py'
SMALL_SCALES = [(128, 64), (128, 120)]                      # in place of [(1333, 768), (1333, 1280)]: seconds, not minutes
ALL_META_KEYS = ('filename', 'ori_shape', 'img_shape', 'pad_shape', 'scale_factor', 'flip', 'flip_direction', 'img_norm_cfg',
                 'scale', 'scale_idx', 'keep_ratio', 'rotate', 'rotate_angle', 'pad_fixed_size', 'pad_size_divisor')


def small_train_pipeline(cfg, all_metas=False):
    """The config's `train_pipeline` as plain dicts, its scales replaced by SMALL_SCALES (and every meta key collected)."""
    steps = []
    for s in cfg.data.train.pipeline:
        s = dict(s)
        if s['type'] in ('RotateResize', 'PolyResize'):
            assert s['multiscale_mode'] == 'range' and len(s['img_scale']) == 2
            s['img_scale'] = list(SMALL_SCALES)
        if s['type'] == 'Collect' and all_metas:
            s['meta_keys'] = ALL_META_KEYS
        steps.append(s)
    return steps


def _rect(cx, cy, w, h, a):
    c, s = np.cos(a), np.sin(a)
    base = np.array([[-.5, -.5], [.5, -.5], [.5, .5], [-.5, .5]]) * [w, h]
    return (base.dot(np.array([[c, s], [-s, c]])) + [cx, cy]).reshape(-1)


SOURCE_SIZES = [(70, 90), (90, 70), (83, 77), (64, 96)]      # (h, w)


def write_dataset(tmp_path):
    """Four .npy images around 90 x 70 with a few boxes each; the last has one box in a corner, which a rotation drops
    (the pipeline's None case).  Returns (annotation file, the images)."""
    from orientedreppoints_amd.mmdet_datasets.dota import DotaDataset
    rng = np.random.RandomState(3)
    images, anns, arrays, aid = [], [], [], 0
    for i, (h, w) in enumerate(SOURCE_SIZES):
        name = 'T%04d.npy' % i
        arr = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        np.save(os.path.join(tmp_path, name), arr)
        arrays.append(arr)
        images.append(dict(id=20 + i, file_name=name, width=w, height=h))
        boxes = [_rect(8, 7, 9, 7, 0.3)] if i == 3 else \
            [_rect(rng.uniform(20, w - 20), rng.uniform(20, h - 20), rng.uniform(8, 30), rng.uniform(8, 30), rng.uniform(-3, 3))
             for _ in range(4)]
        for q in boxes:
            anns.append(dict(id=aid, image_id=20 + i, category_id=int(aid % 15 + 1), bbox=[float(v) for v in np.float32(q)],
                             iscrowd=0, area=1.0, segmentation=[]))
            aid += 1
    cats = [dict(id=i + 1, name=n) for i, n in enumerate(DotaDataset.CLASSES)]
    ann_file = os.path.join(tmp_path, 'ann.json')
    with open(ann_file, 'w') as f:
        json.dump(dict(images=images, annotations=anns, categories=cats), f)
    return ann_file, arrays


def seeded(ds, idx, seed):
    """`ds.prepare_train_img(idx)` under `np.random.seed(seed)` and `random.seed(seed)`."""
    import random
    np.random.seed(seed)
    random.seed(seed)
    return ds.prepare_train_img(idx)


def same_value(a, b):
    """Equal, with types: dicts and sequences element by element, arrays by dtype, shape and value."""
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and sorted(a) == sorted(b) and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and \
            np.array_equal(a, b)
    return type(a) is type(b) and a == b
