"""Test-time augmentation on the detector and the captured graph: `fused_postprocess_views`, the static route of `aug_test`,
`GraphedAugInference` and the overflow fallback, on the three views of tests/test_gpu_parity.py's aug_test case (a 256^2 image:
original, mirrored, half size; R-50, random weights made to detect).  The library's convolutions run in their reproducible mode."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _views(img):
    meta = dict(img_shape=(256, 256, 3), pad_shape=(256, 256, 3), scale_factor=1.0, flip=False)
    half = torch.nn.functional.interpolate(img, scale_factor=0.5, mode='bilinear', align_corners=False)
    return ([img, img.flip(-1), half],
            [[meta], [dict(meta, flip=True)], [dict(img_shape=(128, 128, 3), pad_shape=(128, 128, 3), scale_factor=0.5, flip=False)]])


@pytest.fixture(scope="module")
def setup(dev):
    """(model, imgs, metas, outs, want, single): the views' head outputs computed ONCE and, from those same outputs, today's
    route -- get_bboxes(nms=False) per view, merge_aug_results, the dynamic multiclass_rnms -- as per-class arrays."""
    from orientedreppoints_amd.dota_configs import r50_model, test_cfg
    from orientedreppoints_amd.mmdet_models import ConfigDict, build_detector
    from orientedreppoints_amd.mmdet_models.core import multiclass_rnms, rbbox2result
    det_flag = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(0)
    model = build_detector(ConfigDict(r50_model), train_cfg=None, test_cfg=ConfigDict(dict(test_cfg))).to(dev).eval()
    head = model.bbox_head
    with torch.no_grad():
        head.reppoints_cls_out.weight.normal_(0, 0.05)
        head.reppoints_cls_out.bias.fill_(-3.3)
        head.reppoints_pts_init_out.bias.copy_(torch.tensor(
            [[-1, -1], [-1, 0], [-1, 1], [0, -1], [0, 0], [0, 1], [1, -1], [1, 0], [1, 1]],
            dtype=torch.float32, device=dev).reshape(-1) * 2.0)
        imgs, metas = _views(torch.randn(1, 3, 256, 256, device=dev))
        outs = [head(model.extract_feat(im)) for im in imgs]
        cand = [head.get_bboxes(*(tuple(o) + (m, model.test_cfg, False, False)))[0] for o, m in zip(outs, metas)]
        boxes, scores = model.merge_aug_results([c[0] for c in cand], [c[1] for c in cand], metas)
        det, lab = multiclass_rnms(boxes, scores, model.test_cfg.score_thr, model.test_cfg.nms, model.test_cfg.max_per_img)
        want = rbbox2result(det, lab, head.num_classes)
        single = model.simple_test(imgs[0], metas[0], rescale=True)
    yield model, imgs, metas, outs, want, single
    torch.backends.cudnn.deterministic = det_flag


def _equal(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.shape[1] == 9 and np.array_equal(a, b)


@pytest.mark.gpu
def test_fused_postprocess_views_equals_merge_and_dynamic_nms(dev, setup):
    """On the same head outputs: array_equal per class; the union detects more than the single view.  rescale=False is the
    rescale=True result times the first view's factor (half-size view first: 0.5)."""
    model, imgs, metas, outs, want, single = setup
    assert sum(len(c) for c in want) > sum(len(c) for c in single) > 20
    with torch.no_grad():
        got = model.aug_result_packed(model.aug_postprocess_static(outs, metas, True))
        rev_full = model.aug_result_packed(model.aug_postprocess_static(outs[::-1], metas[::-1], True))
        rev_half = model.aug_result_packed(model.aug_postprocess_static(outs[::-1], metas[::-1], False))
    _equal(got, want)
    assert sum(len(c) for c in rev_full) > 20
    for a, b in zip(rev_half, rev_full):
        assert np.array_equal(a[:, :8], b[:, :8] * np.float32(0.5)) and np.array_equal(a[:, 8], b[:, 8])


@pytest.mark.gpu
def test_aug_test_static_route_agrees_with_the_dynamic_route(dev, setup):
    """aug_test (static route) against aug_test under static_postprocess=False: equal row counts, rtol=1e-5 / atol=1e-4 -- both
    rerun the forwards, and the library's small-map convolutions are not bitwise reproducible between two runs."""
    model, imgs, metas, _, want, _ = setup
    with torch.no_grad():
        got = model.aug_test(imgs, metas, rescale=True)
        model.test_cfg['static_postprocess'] = False
        try:
            dyn = model.aug_test(imgs, metas, rescale=True)
        finally:
            model.test_cfg['static_postprocess'] = True
    assert sum(len(c) for c in got) == sum(len(c) for c in want)
    for a, b in zip(got, dyn):
        assert a.shape == b.shape and np.allclose(a, b, rtol=1e-5, atol=1e-4)


@pytest.mark.gpu
def test_graphed_aug_inference_replays_equal_eager_aug_test(dev, setup):
    """Three different images through one captured graph: each replay bit-equal to the eager static aug_test of that image, and
    two replays of one image bit-equal."""
    from orientedreppoints_amd.mmdet_models import GraphedAugInference
    model, imgs, metas, _, _, _ = setup
    g = GraphedAugInference(model, imgs, metas, rescale=True)
    torch.manual_seed(1)
    first = None
    for i in range(3):
        views, _ = _views(torch.randn(1, 3, 256, 256, device=dev))
        with torch.no_grad():
            eager = model.aug_test(views, metas, rescale=True)
        got = g(views)
        assert len(got) == 1 and sum(len(c) for c in got[0]) > 20
        _equal(got[0], eager)
        if i == 0:
            first = (views, got[0])
    _equal(g(first[0])[0], first[1])
    assert g.captures == 1


@pytest.mark.gpu
def test_overflowing_capacity_returns_the_dynamic_result(dev, setup):
    """static_capacity below the number of pairs: aug_test and the graph both return the dynamic route's result."""
    from orientedreppoints_amd.mmdet_models import GraphedAugInference
    model, imgs, metas, outs, want, _ = setup
    model.test_cfg['static_capacity'] = 32
    try:
        with torch.no_grad():
            assert model.aug_result_packed(model.aug_postprocess_static(outs, metas, True)) is None
            model.test_cfg['static_postprocess'] = False
            dyn = model.aug_test(imgs, metas, rescale=True)
            model.test_cfg['static_postprocess'] = True
            eager = model.aug_test(imgs, metas, rescale=True)
        graphed = GraphedAugInference(model, imgs, metas, rescale=True)(imgs)[0]
    finally:
        model.test_cfg['static_postprocess'] = True
        model.test_cfg['static_capacity'] = 8192
    assert sum(len(c) for c in dyn) == sum(len(c) for c in want) > 32
    for got in (eager, graphed):
        for a, b in zip(got, dyn):
            assert a.shape == b.shape and np.allclose(a, b, rtol=1e-5, atol=1e-4)
