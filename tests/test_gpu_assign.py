"""GPU: the four operators of csrc/orp_assign.hip (through orientedreppoints_amd/mmdet_ops/apaa.py) on every case of
tests/assign_cases.py -- every route of the launch code (column maximum for k <= 256 and k > 256, the one-thread arg-max
assignment, both formulations of the selection) and every tie rule the file's header fixes.

The three decision operators are compared EXACTLY with the plain numpy references of tests/assign_cases.py; the feature
dissimilarity within 1e-4 absolute of a float64 reference (the project's bar for loss floats).  Each operator is also called
twice on the same input and must return the same result: the order in which atomicMin / atomicAdd slots are taken must not show.
That the cases hold the ties and sit on the intended side of every route boundary is asserted without a GPU in
tests/test_assign_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import assign_cases as A  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- point assign -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_num", A.POINT_POS_NUMS)
@pytest.mark.parametrize("case", A.POINT_CASES, ids=lambda c: c.name)
def test_point_assign_is_the_reference(dev, case, pos_num):
    """gt_inds equal the reference's: equal distance -> the smaller point index, equal distance to two gts -> the earlier gt
    keeps the point, levels clamped at both ends, zero-extent gts, pos_num beyond the points of a level."""
    from orientedreppoints_amd.mmdet_ops import apaa
    pts, gts = A.point_case(case)
    want = A.ref_point_assign(pts, gts, A.POINT_SCALE, pos_num)
    p, g = _t(pts, dev), _t(gts, dev)
    got = apaa.point_assign(p, g, A.POINT_SCALE, pos_num)
    again = apaa.point_assign(p, g, A.POINT_SCALE, pos_num)
    assert got.dtype == torch.int64 and got.shape == (pts.shape[0],)
    bad = np.nonzero(got.cpu().numpy() != want)[0]
    assert bad.size == 0, "%s pos_num %d: %d points differ, first %s: got %s want %s" % (
        case.name, pos_num, bad.size, bad[:8], got.cpu().numpy()[bad[:8]], want[bad[:8]])
    assert torch.equal(got, again)


# ---- max-IoU assign ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", A.MAXIOU_SHAPES, ids=lambda v: str(v))
def test_max_iou_assign_is_the_reference(dev, k, n):
    """gt_inds and max_overlaps equal the reference's, NaN positions included, for a (lo, hi) and a scalar negative range,
    min_pos_iou 0 and 0.25, gt_max_assign_all both ways (False up to n = 1000)."""
    from orientedreppoints_amd.mmdet_ops import apaa
    ov = A.maxiou_case(k, n)
    d = _t(ov, dev)
    for neg, mp, aa in A.maxiou_runs(n):
        want_gi, want_mo = A.ref_max_iou_assign(ov, A.MAXIOU_POS, neg, mp, aa)
        gi, mo = apaa.max_iou_assign(d, A.MAXIOU_POS, neg, mp, aa)
        gi2, mo2 = apaa.max_iou_assign(d, A.MAXIOU_POS, neg, mp, aa)
        gi_h, mo_h = gi.cpu().numpy(), mo.cpu().numpy()
        what = "k %d n %d neg %s min_pos %s assign_all %s" % (k, n, neg, mp, aa)
        bad = np.nonzero(gi_h != want_gi)[0]
        assert bad.size == 0, "%s: %d rows differ, first %s: got %s want %s" % (what, bad.size, bad[:8], gi_h[bad[:8]], want_gi[bad[:8]])
        assert np.array_equal(mo_h, want_mo, equal_nan=True), what
        assert torch.equal(gi, gi2) and np.array_equal(mo_h, mo2.cpu().numpy(), equal_nan=True), what


# ---- select -------------------------------------------------------------------------------------------------------------------------
def _select(case, dev):
    from orientedreppoints_amd.mmdet_ops import apaa
    return apaa.apaa_select(_t(case.q, dev), _t(case.gt, dev), _t(case.lvl, dev), case.num_gt, case.num_level, case.k, case.ratio)


@pytest.mark.parametrize("case", A.SELECT_CASES, ids=lambda c: c.name)
def test_apaa_select_is_the_reference(dev, case):
    """keep flags equal the reference's under the order (NaN last, -0 == +0, level, index), in the counting formulation (at
    most kSelCap = 1024 positives of a gt) and the sequential one (more), side by side in the big cases."""
    want = A.ref_apaa_select(case.q, case.gt, case.lvl, case.num_gt, case.num_level, case.k, case.ratio)
    got = _select(case, dev)
    again = _select(case, dev)
    assert got.dtype == torch.bool and got.shape == want.shape
    got_h = got.cpu().numpy()
    bad = np.nonzero(got_h != want)[0]
    assert bad.size == 0, "%s: %d flags differ; first (index, gt, level, Q bits, got, want): %s" % (
        case.name, bad.size, [(int(i), int(case.gt[i]), int(case.lvl[i]), hex(int(case.q.view(np.uint32)[i])), bool(got_h[i]), bool(want[i]))
                              for i in bad[:8]])
    assert torch.equal(got, again)


def test_apaa_select_special_values_by_hand(dev):
    """The two cases of the issue, written out: per_level_topk = 1 keeps the +0.0 at index 0 of [+0.0, -0.0], and the 1.0 of
    [1.0, NaN with the sign bit set] -- in the counting formulation and, with the gt padded past kSelCap, in the sequential one."""
    for name in ("hand_level_cut", "hand_level_cut_sequential"):
        kept = np.nonzero(_select(A.SELECT_BY_NAME[name], dev).cpu().numpy()[:A.HAND_LEVEL_CUT.q.size])[0].tolist()
        assert kept == A.HAND_LEVEL_CUT_KEPT, (name, kept)
    for name in ("hand_final_cut", "hand_final_cut_sequential"):
        case = A.SELECT_BY_NAME[name]
        want = A.ref_apaa_select(case.q, case.gt, case.lvl, case.num_gt, case.num_level, case.k, case.ratio)
        kept = np.nonzero(_select(case, dev).cpu().numpy())[0].tolist()
        assert kept == np.nonzero(want)[0].tolist(), (name, kept)
        if name == "hand_final_cut":
            assert kept == A.HAND_FINAL_CUT_KEPT


# ---- feature dissimilarity --------------------------------------------------------------------------------------------------------
_feat_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report_feature_dissimilarity():
    yield
    import conftest
    for C, worst in sorted(_feat_worst.items()):
        conftest.REPORT.append("apaa_feature_dissimilarity vs float64 grid_sample reference, C = %3d: largest |difference| %.3g "
                               "(bar 1e-4)" % (C, worst))


@pytest.mark.parametrize("P", A.FEAT_PS)
@pytest.mark.parametrize("C", A.FEAT_CS)
def test_feature_dissimilarity_vs_float64_reference(dev, C, P):
    """Within 1e-4 absolute of the float64 reference on maps with H != W, C below, at and above one trip of the 64-lane
    channel loop, every (image, level) pair, points inside, on every border and outside; exactly 1 on the all-zero map."""
    from orientedreppoints_amd.mmdet_ops import apaa
    feats, pts, img, lvl = A.feat_case(C, P)
    want = A.ref_feature_dissimilarity(feats, A.FEAT_STRIDES, pts, img, lvl)
    args = ([_t(f, dev) for f in feats], list(A.FEAT_STRIDES), _t(pts, dev), _t(img, dev), _t(lvl, dev))
    got = apaa.apaa_feature_dissimilarity(*args)
    again = apaa.apaa_feature_dissimilarity(*args)
    assert got.dtype == torch.float32 and got.shape == (P,)
    got_h = got.cpu().numpy().astype(np.float64)
    diff = np.abs(got_h - want)
    print("C %d P %d: largest |difference| %.3g at positive %d" % (C, P, diff.max(), int(diff.argmax())))
    _feat_worst[C] = max(_feat_worst.get(C, 0.0), float(diff.max()))
    assert diff.max() <= 1e-4, "C %d P %d: positive %d (image %d, level %d) got %r want %r" % (
        C, P, diff.argmax(), img[diff.argmax()], lvl[diff.argmax()], got_h[diff.argmax()], want[diff.argmax()])
    zero = (img == A.FEAT_ZERO_MAP[0]) & (lvl == A.FEAT_ZERO_MAP[1])
    assert np.all(got_h[zero] == 1.0)
    assert torch.equal(got, again)
