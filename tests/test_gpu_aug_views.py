"""Test-time augmentation, kernel and operator level (no detector): `orp_pp_compact_views` against
`OrientedRepPointsDetector.merge_aug_results` on the same device tensors followed by the dynamic `multiclass_rnms`, and the
flipped tile kernels against the mirrored output of the plain ones.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

C = 15
THR = 0.05
IOU = 0.4
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ---- compact ---------------------------------------------------------------------------------------------------------------
def make_view(rng, m0, width, dev, hot=0.12):
    """Synthetic head results of one view: sig [C, n] sigmoid-like scores (a fraction `hot` of them above THR), cand [m0] int64
    distinct points, boxes [m0, 8] rotated rectangles inside a `width`-wide image, reppoints [m0, 18]."""
    n = m0 + 50
    sig = rng.uniform(0.0, THR * 0.99, size=(C, n))
    mask = rng.uniform(size=(C, n)) < hot
    sig[mask] = rng.uniform(THR * 1.01, 1.0, size=int(mask.sum()))
    cand = rng.permutation(n)[:m0].astype(np.int64)
    cx, cy = rng.uniform(20, width - 20, size=m0), rng.uniform(20, width - 20, size=m0)
    w, h, a = rng.uniform(8, 40, size=m0), rng.uniform(8, 40, size=m0), rng.uniform(0, np.pi, size=m0)
    dx = np.stack([-w, w, w, -w], 1) / 2
    dy = np.stack([-h, -h, h, h], 1) / 2
    x = cx[:, None] + dx * np.cos(a)[:, None] - dy * np.sin(a)[:, None]
    y = cy[:, None] + dx * np.sin(a)[:, None] + dy * np.cos(a)[:, None]
    boxes = np.stack([x, y], 2).reshape(m0, 8)
    rep = rng.uniform(0, width, size=(m0, 18))
    f = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)
    return f(sig), torch.from_numpy(cand).to(dev), f(boxes), f(rep)


def run_views(views, cap, dev):
    """`compact_views` + `rnms_batched_device`.  views: (sig, cand, boxes, rep, flip, width, scale)."""
    from orientedreppoints_amd.mmdet_models.core import compact_views
    from orientedreppoints_amd.mmdet_ops.nms_wrapper import rnms_batched_device
    m_all = sum(v[1].numel() for v in views)
    out = dict(boxes_all=torch.full((m_all, 8), 7.0, device=dev), rep_all=torch.full((m_all, 18), 7.0, device=dev),
               dets=torch.full((cap, 9), 7.0, device=dev), sel_cand=torch.full((cap,), 7, dtype=torch.int32, device=dev),
               sel_label=torch.full((cap,), 7, dtype=torch.int32, device=dev),
               seg=torch.full((2,), 7, dtype=torch.int32, device=dev), total=torch.full((1,), 7, dtype=torch.int32, device=dev))
    compact_views(views, C, THR, cap, out['boxes_all'], out['rep_all'], out['dets'], out['sel_cand'], out['sel_label'],
                  out['seg'], out['total'])
    out['keep'], out['num'] = rnms_batched_device(out['dets'], out['seg'], cap, IOU)
    return out


def expected(views, dev):
    """merge_aug_results on the views' device tensors (host-scalar scale factors) + the steps of the dynamic multiclass_rnms."""
    from orientedreppoints_amd.mmdet_models.core import multiclass_rnms
    from orientedreppoints_amd.mmdet_models.detector import OrientedRepPointsDetector as D
    det = D.__new__(D)                                         # merge_aug_results reads no module state
    metas = [[dict(img_shape=(w, w, 3), scale_factor=s, flip=f)] for _, _, _, _, f, w, s in views]
    scores = [torch.cat([sig.new_zeros(cand.numel(), 1), sig[:, cand].t()], 1) for sig, cand, _, _, _, _, _ in views]
    boxes, scores = D.merge_aug_results(det, [v[2] for v in views], scores, metas)
    # (rbbox_flip takes rows of 8k coordinates: the 18 of a rep-point row are padded to 24 and cut back, x / y parity kept)
    rep = D.merge_aug_results(det, [torch.cat([v[3], v[3][:, :6]], 1) for v in views], None, metas)[:, :18]
    valid = scores[:, 1:] > THR
    idx = valid.nonzero()
    e = dict(boxes_all=boxes, rep_all=rep, total=int(idx.size(0)), sel_cand=idx[:, 0], sel_label=idx[:, 1])
    if idx.size(0):
        b = boxes[:, None].expand(-1, C, 8)[valid]
        offs = idx[:, 1].to(b) * (b.max() + 1)
        e['dets'] = torch.cat([b + offs[:, None], scores[:, 1:][valid][:, None]], 1)
    e['nms'] = multiclass_rnms(boxes, scores, THR, dict(type='rnms', iou_thr=IOU), 10 ** 6)
    return e


CASES = {
    # m0 per view, flips, widths, scales
    "three": ((1, 37, 300), (False, True, False), (128, 333, 128), (1.0, 0.5, np.float32(1333 / 1024))),
    "quiet_first": ((64, 64), (True, True), (333, 128), (0.9375, 1.5)),
    "empty_between": ((37, 0, 300), (True, False, True), (128, 128, 333), (np.float32(1333 / 1024), 1.0, 0.9375)),
    "all_empty": ((0, 0), (False, True), (128, 333), (1.0, 0.5)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_compact_views_equals_merge_aug_results_and_dynamic_nms(dev, case):
    """boxes_all / reppoints_all bit-equal to merge_aug_results (flips mixed, widths 128 and 333, scales with exact and inexact
    reciprocals); dets, sel_cand, sel_label, seg, total equal to multiclass_rnms' own intermediate tensors; the rows kept by
    rnms_batched_device equal to multiclass_rnms' result.  Views of 1, 37, 300 candidates (more than one block), a view with
    nothing above the threshold, an empty view between two others, all views empty."""
    m0s, flips, widths, scales = CASES[case]
    rng = np.random.RandomState(len(case))
    views = []
    for i, (m0, f, w, s) in enumerate(zip(m0s, flips, widths, scales)):
        sig, cand, boxes, rep = make_view(rng, m0, w, dev, hot=0.0 if (case == "quiet_first" and i == 0) else 0.12)
        views.append((sig, cand, boxes, rep, f, w, s))
    cap = 8192
    got, want = run_views(views, cap, dev), expected(views, dev)
    n = want['total']
    assert (n > 50) == (case != "all_empty")
    assert np.array_equal(_bits(got['boxes_all']), _bits(want['boxes_all']))
    assert np.array_equal(_bits(got['rep_all']), _bits(want['rep_all']))
    assert int(got['total'].item()) == n and got['seg'].tolist() == [0, n]
    assert torch.equal(got['sel_cand'][:n].long(), want['sel_cand']) and torch.equal(got['sel_label'][:n].long(), want['sel_label'])
    if n:
        assert np.array_equal(_bits(got['dets'][:n]), _bits(want['dets']))
    assert (got['dets'][n:, 8] == float('-inf')).all() and (got['dets'][n:, :8] == 0).all()
    k = int(got['num'][0].item())
    keep = got['keep'][:k]
    w_det, w_lab = want['nms']
    assert k == w_det.size(0) and (k > 0) == (n > 0)
    rows = got['sel_cand'][keep].long()
    assert np.array_equal(_bits(got['boxes_all'][rows]), _bits(w_det[:, :8]))
    assert np.array_equal(_bits(got['dets'][keep, 8]), _bits(w_det[:, 8]))
    assert torch.equal(got['sel_label'][keep].long(), w_lab)


@pytest.mark.gpu
def test_compact_views_overflow_sets_the_packed_flag(dev):
    """total > capacity: total reports every pair, seg stops at the capacity and orp_pp_pack's tail row carries the flag."""
    from orientedreppoints_amd import _lib
    rng = np.random.RandomState(1)
    views = [make_view(rng, 37, 128, dev) + (False, 128, 1.0), make_view(rng, 64, 128, dev) + (True, 128, 0.5)]
    cap, m = 16, 16
    got = run_views(views, cap, dev)
    assert int(got['total'].item()) > cap and got['seg'].tolist() == [0, cap]
    packed = torch.full((m + 1, 28), 7.0, device=dev)
    _lib.check(_lib.lib().orp_pp_pack(_lib.ptr(got['keep']), _lib.ptr(got['num']), _lib.ptr(got['dets']), _lib.ptr(got['sel_cand']),
                                      _lib.ptr(got['sel_label']), _lib.ptr(got['boxes_all']), _lib.ptr(got['rep_all']),
                                      _lib.ptr(got['total']), cap, m, _lib.ptr(packed), _lib.stream_of(packed)), "orp_pp_pack")
    assert packed[m, 1].item() == 1.0
    ample = run_views(views, 8192, dev)
    assert int(ample['total'].item()) == int(got['total'].item())


@pytest.mark.gpu
def test_one_plain_view_equals_orp_pp_compact_bit_for_bit(dev):
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    rng = np.random.RandomState(2)
    sig, cand, boxes, rep = make_view(rng, 300, 333, dev)
    cap = 4096
    got = run_views([(sig, cand, boxes, rep, False, 333, 1.0)], cap, dev)
    dets = torch.full((cap, 9), 7.0, device=dev)
    sel_cand, sel_label = torch.empty((cap,), dtype=torch.int32, device=dev), torch.empty((cap,), dtype=torch.int32, device=dev)
    seg, total = torch.empty((2,), dtype=torch.int32, device=dev), torch.empty((1,), dtype=torch.int32, device=dev)
    scratch = torch.empty((L.orp_pp_compact_scratch_bytes(300),), dtype=torch.uint8, device=dev)
    _lib.check(L.orp_pp_compact(_lib.ptr(sig), _lib.ptr(cand), 300, sig.size(1), C, _lib.ptr(boxes), THR, cap, _lib.ptr(dets),
                                _lib.ptr(sel_cand), _lib.ptr(sel_label), _lib.ptr(seg), _lib.ptr(total), _lib.ptr(scratch),
                                scratch.numel(), _lib.stream_of(sig)), "orp_pp_compact")
    assert int(total.item()) > 100
    assert np.array_equal(_bits(got['dets']), _bits(dets))
    assert torch.equal(got['sel_cand'], sel_cand) and torch.equal(got['sel_label'], sel_label)
    assert torch.equal(got['seg'], seg) and torch.equal(got['total'], total)
    assert np.array_equal(_bits(got['boxes_all']), _bits(boxes)) and np.array_equal(_bits(got['rep_all']), _bits(rep))


@pytest.mark.gpu
def test_nine_views_are_refused(dev):
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_models.core import PpView
    L = _lib.lib()
    sig, cand, boxes, rep = make_view(np.random.RandomState(3), 4, 128, dev)
    arr = (PpView * 9)()
    for a in arr:
        a.sig_all, a.cand, a.boxes, a.reppoints = sig.data_ptr(), cand.data_ptr(), boxes.data_ptr(), rep.data_ptr()
        a.m0, a.n, a.flip, a.img_width, a.scale = 4, sig.size(1), 0, 128, 1.0
    cap = 64
    out8, out18, dets = torch.empty((36, 8), device=dev), torch.empty((36, 18), device=dev), torch.empty((cap, 9), device=dev)
    i32 = lambda n: torch.empty((n,), dtype=torch.int32, device=dev)
    sel_cand, sel_label, seg, total = i32(cap), i32(cap), i32(2), i32(1)
    scratch = torch.empty((L.orp_pp_compact_views_scratch_bytes(36),), dtype=torch.uint8, device=dev)
    args = [C, THR, cap, _lib.ptr(out8), _lib.ptr(out18), _lib.ptr(dets), _lib.ptr(sel_cand), _lib.ptr(sel_label), _lib.ptr(seg),
            _lib.ptr(total), _lib.ptr(scratch), scratch.numel(), _lib.stream_of(dets)]
    assert L.orp_pp_compact_views(arr, 9, *args) == _lib.ORP_EINVAL
    assert L.orp_pp_compact_views(arr, 0, *args) == _lib.ORP_EINVAL
    assert L.orp_pp_compact_views(arr, 8, *args) == _lib.ORP_OK
    torch.cuda.synchronize()


# ---- flipped tiles ---------------------------------------------------------------------------------------------------------
def _scene(rng, H, W, dev):
    return torch.from_numpy(rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("S,dtype", [(32, torch.float32), (64, torch.float16), (64, torch.bfloat16)])
def test_flipped_native_tiles_are_the_mirrored_plain_tiles(dev, S, dtype):
    """Origins inside the scene, at odd lefts and hanging over the right and bottom edges (the zeros are mirrored too)."""
    from orientedreppoints_amd.mmdet_ops.scene_ops import scene_tiles, scene_tiles_flip
    scene = _scene(np.random.RandomState(S), 150, 201, dev)
    origins = torch.tensor([(0, 0), (13, 7), (201 - S, 150 - S), (201 - S // 2 - 1, 150 - S // 3), (200, 149)], dtype=torch.int32).to(dev)
    for to_rgb in (True, False):
        plain = torch.full((5, 3, S, S), 7.0, dtype=dtype, device=dev)
        flipped = torch.full((5, 3, S, S), 7.0, dtype=dtype, device=dev)
        scene_tiles(scene, origins, plain, MEAN, STD, to_rgb)
        scene_tiles_flip(scene, origins, flipped, MEAN, STD, to_rgb)
        assert plain.float().abs().max() > 1 and (plain[3][:, :, -1] == 0).all()
        assert torch.equal(flipped.view(torch.int16 if dtype != torch.float32 else torch.int32),
                           plain.flip(-1).view(torch.int16 if dtype != torch.float32 else torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("src,new,pad", [((50, 37), (45, 33), (64, 64)), ((64, 64), (64, 64), (64, 64)), ((50, 37), (50, 37), (64, 64))])
def test_flipped_resized_tiles_mirror_inside_the_resized_width(dev, src, new, pad):
    """A 50 x 37 patch to 45 x 33 (new_w odd, no multiple of 4) in a 64 x 64 pad, and identity resizes (padded and not):
    out[.., x] = plain[.., new_w - 1 - x] for x < new_w bit for bit, exactly zero beyond new_w and new_h."""
    from orientedreppoints_amd.mmdet_ops.scene_ops import scene_tiles_resized, scene_tiles_resized_flip
    scene = _scene(np.random.RandomState(7), 150, 201, dev)
    origins = torch.tensor([(0, 0), (13, 7), (201 - src[0], 150 - src[1])], dtype=torch.int32).to(dev)
    for dtype, as_int in ((torch.float32, torch.int32), (torch.float16, torch.int16), (torch.bfloat16, torch.int16)):
        plain = torch.full((3, 3, pad[1], pad[0]), 7.0, dtype=dtype, device=dev)
        flipped = torch.full((3, 3, pad[1], pad[0]), 7.0, dtype=dtype, device=dev)
        scene_tiles_resized(scene, origins, src, new, plain, MEAN, STD, True)
        scene_tiles_resized_flip(scene, origins, src, new, flipped, MEAN, STD, True)
        assert plain.float().abs().max() > 1
        assert torch.equal(flipped[..., :new[0]].contiguous().view(as_int), plain[..., :new[0]].flip(-1).contiguous().view(as_int))
        assert (flipped[..., new[0]:].contiguous().view(as_int) == 0).all() and (flipped[:, :, new[1]:].contiguous().view(as_int) == 0).all()


@pytest.mark.gpu
def test_flipped_tiles_refuse_a_misaligned_pad(dev):
    """The plain kernels' alignment rules: a float32 row of 62 and a float16 row of 60 columns are ORP_EINVAL."""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.scene_ops import scene_tiles_flip, scene_tiles_resized_flip
    scene = _scene(np.random.RandomState(9), 150, 201, dev)
    origins = torch.tensor([(0, 0)], dtype=torch.int32).to(dev)
    for dtype, width in ((torch.float32, 62), (torch.float16, 60)):
        with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
            scene_tiles_resized_flip(scene, origins, (50, 37), (45, 33), torch.empty((1, 3, 64, width), dtype=dtype, device=dev),
                                     MEAN, STD)
        with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
            scene_tiles_flip(scene, origins, torch.empty((1, 3, width, width), dtype=dtype, device=dev), MEAN, STD)
