"""CPU: the references of tests/assign_cases.py against the CPU oracle on every case of the tables, and the properties of the
generated data that keep tests/test_gpu_assign.py from passing vacuously -- that the ties it is about do occur, that every gt
of a select case is on the intended side of kSelCap, that the shape lists contain the route boundaries of the launch code.
No GPU, no kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assign_cases as A  # noqa: E402


# ---- point assign -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.POINT_CASES, ids=lambda c: c.name)
def test_point_assign_reference_is_the_oracle_and_the_ties_occur(case, oracle):
    """Every table and pos_num: the numpy reference equals oracle.point_assign.  The level expression of every gt is an exact
    integer or far enough from one (0.29; after clamping, for the zero-extent gts) that no case rests on the last bit of log2f.
    From the reference alone: with more than one gt, some point is contested by two gts at exactly the same distance, and some
    top-pos_num cut runs between two equal distances."""
    pts, gts = A.point_case(case)
    assert pts.shape == (1364 if len(case.strides) == 5 else 1280, 3) and gts.shape == (case.k, 8)
    lo, hi = int(np.log2(min(case.strides))), int(np.log2(max(case.strides)))
    e = A.point_level_expression(gts, A.POINT_SCALE)
    clamp = lambda v: np.clip(np.trunc(v), lo, hi)                        # noqa: E731
    assert np.all((e == np.round(e)) | (clamp(e - 0.29) == clamp(e + 0.29)) | (np.abs(e - np.round(e)) >= 0.29))
    if case.k >= 40:
        lv = np.trunc(e)
        assert (lv < lo).any() and (lv > hi).any() and ((lv >= lo) & (lv <= hi)).any(), "levels below, inside and above the grid's"
        ext = np.stack([gts[:, 0::2].max(1) - gts[:, 0::2].min(1), gts[:, 1::2].max(1) - gts[:, 1::2].min(1)], 1)
        assert ((ext[:, 0] == 0) & (ext[:, 1] > 0)).any() and ((ext[:, 0] == 0) & (ext[:, 1] == 0)).any()
        assert any(np.array_equal(gts[i], gts[j]) for i in range(case.k) for j in range(i)), "no duplicated gt"
    for pos_num in A.POINT_POS_NUMS:
        stats = {}
        want = A.ref_point_assign(pts, gts, A.POINT_SCALE, pos_num, stats)
        assert np.array_equal(want, oracle.point_assign(pts, gts, A.POINT_SCALE, pos_num)), (case.name, pos_num)
        assert want.min() >= 0 and want.max() <= case.k and (want > 0).any()
        assert stats.get("cut_ties", 0) > 0, "no top-pos_num cut through equal distances"
        if case.k > 1:
            assert stats.get("contested_equal", 0) > 0, "no point contested at equal distance"


def test_point_assign_reference_on_random_tie_heavy_cases(oracle):
    """300 small random cases of the same family (duplicated gts, pos_num 1, 3, 9, both grids): reference == oracle."""
    rng = np.random.RandomState(5)
    grids = [A.grid_points(256, (8, 16, 32, 64, 128)), A.grid_points(256, (8, 16)), A.grid_points(64, (8, 16, 32))]
    for it in range(300):
        pts = grids[it % 3]
        gts = A.point_gts(int(rng.randint(1, 30)), 9000 + it, size=256 if it % 3 < 2 else 64)
        pn = (1, 3, 9)[rng.randint(0, 3)]
        assert np.array_equal(A.ref_point_assign(pts, gts, 4, pn), oracle.point_assign(pts, gts, 4, pn)), it


def test_point_assign_pos_num_beyond_the_level(oracle):
    """pos_num = 9 onto the four points of the stride-128 level: all four are taken, nothing else."""
    pts = A.grid_points(256, (8, 16, 32, 64, 128))
    gts = np.asarray([[0, 0, 1024, 0, 1024, 1024, 0, 1024]], np.float32)          # level 8 -> clamped to 7
    want = A.ref_point_assign(pts, gts, 4, 9)
    assert np.array_equal(np.nonzero(want)[0], np.arange(1360, 1364))
    assert any(np.trunc(A.point_level_expression(A.point_case(c)[1], 4)).max() >= 7 for c in A.POINT_CASES)


# ---- max-IoU assign ---------------------------------------------------------------------------------------------------------------
def test_max_iou_shape_list_contains_the_route_boundaries():
    """k: 256 is the last size of the single-pass column maximum and 257 the first of the per-gt one; 255 / 23 / 100 / 300 do
    not divide 256.  n: 4096 = 64 blocks x 64 rows is where the block count stops growing; 63 / 64 / 65 surround one block.
    Every k and every n of the lists is used, and the one-thread arg-max kernel is kept to n <= 1000 on both sides of k = 256."""
    assert {255, 256, 257} <= set(A.MAXIOU_KS) and {1, 63, 64, 65, 4095, 4096, 4097} <= set(A.MAXIOU_NS)
    assert {k for k, _ in A.MAXIOU_SHAPES} == set(A.MAXIOU_KS) and {n for _, n in A.MAXIOU_SHAPES} == set(A.MAXIOU_NS)
    assert max(n * k for k, n in A.MAXIOU_SHAPES) == 4097 * 300
    small = [(k, n) for k, n in A.MAXIOU_SHAPES if n <= A.MAXIOU_ARGMAX_MAX_N]
    assert {k for k, _ in small} >= {1, 2, 23, 100, 255, 256, 257, 300}
    for k, n in A.MAXIOU_SHAPES:
        runs = A.maxiou_runs(n)
        assert any(aa for _, _, aa in runs) and (n > A.MAXIOU_ARGMAX_MAX_N) == (not any(not aa for _, _, aa in runs))
        assert {neg if isinstance(neg, float) else "pair" for neg, _, _ in runs} == {0.375, "pair"}
        assert {mp for _, mp, _ in runs} == {0.0, 0.25}


@pytest.mark.parametrize("k,n", A.MAXIOU_SHAPES, ids=lambda v: str(v))
def test_max_iou_reference_is_the_oracle_and_the_ties_occur(k, n, oracle):
    """Every shape and threshold combination: gt_inds and max_overlaps of the numpy reference equal the oracle's, NaN positions
    included.  The data: values exactly on every threshold; rows and columns whose maximum is attained more than once; the
    all-zero column takes every all-zero-maximum row at min_pos_iou = 0 (pinned) and none at 0.25; the NaN column takes none."""
    ov = A.maxiou_case(k, n)
    assert ov.shape == (n, k) and ov.dtype == np.float32
    fin = ov[~np.isnan(ov)]
    assert np.array_equal(fin * 8, np.round(fin * 8)) and fin.min() >= 0 and fin.max() <= 1
    special = A.maxiou_special_columns(k)
    nan_col = special[1] if special else None
    plain = ov[:, [g for g in range(k) if g != nan_col]]
    if n * k >= 4096:
        assert set(np.unique(fin)) >= {0.0, 0.125, 0.25, 0.375, 0.5}
        assert 0 < np.isnan(plain).any(1).sum() <= 5 and 0 < np.isnan(plain).any(0).sum() <= 5        # the scattered NaN
        if nan_col is None:
            clean = plain[~np.isnan(plain).any(1)]
            assert k == 1 or ((clean == clean.max(1)[:, None]).sum(1) > 1).any(), "no row whose maximum ties"
            assert set(np.unique(clean.max(1))) >= {0.0, 0.125, 0.25, 0.375, 0.5, 0.625}       # on and around every threshold
    if n >= 63 and k >= 3:
        cols = plain[:, ~np.isnan(plain).any(0)]
        assert ((cols == cols.max(0)[None, :]).sum(0) > 1).any(), "no column whose maximum ties"
    results = {}
    for neg, mp, aa in A.maxiou_runs(n):
        gi, mo = A.ref_max_iou_assign(ov, A.MAXIOU_POS, neg, mp, aa)
        ogi, omo = oracle.max_iou_assign(ov, A.MAXIOU_POS, neg, mp, aa)
        assert np.array_equal(gi, ogi), (k, n, neg, mp, aa)
        assert np.array_equal(mo, omo, equal_nan=True)
        assert gi.min() >= -1 and gi.max() <= k
        results[(neg, mp, aa)] = (gi, mo)
    if special:
        zero = special[0]
        assert (ov[:, zero] == 0).all()
        for (neg, mp, aa), (gi, mo) in results.items():
            if nan_col is not None:
                assert np.isnan(ov[:, nan_col]).all() and np.isnan(mo).all(), "an all-NaN column makes every row maximum NaN"
                assert not (gi == nan_col + 1).any(), "the all-NaN column took a row"
            if mp == 0.25:
                assert not (gi == zero + 1).any()
        gi = results[(0.375, 0.0, True)][0]
        if zero == k - 1:
            assert np.all(gi == k), "min_pos_iou = 0: every row equals the zero column's maximum and takes that gt"
        else:
            later = ov[:, zero + 1:]
            with np.errstate(invalid="ignore"):
                overwritten = (later == later.max(0)[None, :]).any(1)
            assert np.all(gi[~overwritten] == zero + 1)


def test_max_iou_special_columns_cover_both_placements_and_every_route():
    zeros = {A.maxiou_special_columns(k)[0] == k - 1 for k in A.MAXIOU_KS if k >= 3}
    assert zeros == {True, False}
    with_nan = [k for k in A.MAXIOU_KS if k >= 3 and A.maxiou_special_columns(k)[1] is not None]
    assert any(256 // k > 1 for k in with_nan) and any(128 < k <= 256 for k in with_nan) and any(k > 256 for k in with_nan)
    without = [k for k in A.MAXIOU_KS if k >= 3 and A.maxiou_special_columns(k)[1] is None]
    assert any(k > 256 for k in without) and any(k <= 256 and 256 % k for k in without)


# ---- select -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.SELECT_CASES, ids=lambda c: c.name)
def test_select_reference_and_case_properties(case, oracle):
    """Every case: some positives kept, some dropped, none kept that has gt 0, a gt above num_gt or a level out of range; the
    reference equals oracle.apaa_select, on the cases with NaN and -0.0 too (the oracle ranks with the same total order)."""
    keep = A.ref_apaa_select(case.q, case.gt, case.lvl, case.num_gt, case.num_level, case.k, case.ratio)
    assert keep.dtype == bool and keep.any() and not keep.all()
    bad = (case.gt < 1) | (case.gt > case.num_gt) | (case.lvl < 0) | (case.lvl >= case.num_level)
    assert not keep[bad].any()
    assert case.k * case.num_level <= 64
    has_special = bool(np.isnan(case.q).any() or (np.signbit(case.q) & (case.q == 0)).any())
    assert has_special == case.special
    want = oracle.apaa_select(case.q, case.gt, case.lvl, case.num_gt, case.num_level, case.k, case.ratio).astype(bool)
    assert np.array_equal(keep, want)


def test_select_reference_on_random_cases(oracle):
    """200 random cases: quantised Q, levels out of range, gt 0, gts above num_gt, every (num_level, k, ratio) of the tables."""
    rng = np.random.RandomState(17)
    for it in range(200):
        nl, k = [(1, 6), (5, 6), (10, 6), (16, 4), (3, 1)][rng.randint(0, 5)]
        ratio = (0.4, 1.0, 0.01, 0.5)[rng.randint(0, 4)]
        P, G = int(rng.randint(1, 400)), int(rng.randint(1, 9))
        q = (rng.randint(-4, 12, P) / 4.0).astype(np.float32)
        q[q == 0] = 0.0
        gt = rng.randint(0, G + 3, P)
        lvl = rng.randint(-1, nl + 1, P)
        want = oracle.apaa_select(q, gt, lvl, G, nl, k, ratio).astype(bool)
        assert np.array_equal(A.ref_apaa_select(q, gt, lvl, G, nl, k, ratio), want), it


def test_select_cases_cover_what_they_claim():
    """The small cases: num_level 1 / 5 / 10 at per_level_topk 6 and 16 at 4, ratios 0.4 / 1.0 / 0.01, quantised and
    continuous Q, num_gt above and below the largest gt present, levels -1 and num_level and gt 0 present, a gt with exactly one
    positive, and every gt below kSelCap.  The big cases: gt 1 at exactly kSelCap (fast formulation), gt 2 at kSelCap + 1 with
    the same (Q, level) pairs permuted plus one that is never kept -- so the two formulations must keep the same (Q, level)
    multiset --, gt 3 at 3000, the rest a few dozen.  The padded cases: every gt above kSelCap."""
    small = [c for c in A.SELECT_CASES if c.name.startswith(("quant_l", "cont_l"))]
    assert {(c.num_level, c.k) for c in small} == {(1, 6), (5, 6), (10, 6), (16, 4)}
    assert {c.ratio for c in small} == {0.4, 1.0, 0.01}
    for c in small:
        assert A.select_counts(c.gt, c.lvl, c.num_gt, c.num_level).max() <= 100
        assert (c.lvl == -1).any() and (c.lvl == c.num_level).any() and (c.gt == 0).any()
        assert int((c.gt == 7).sum()) == 1 and c.num_gt >= 7
        quantised = np.array_equal(c.q * 4, np.round(c.q * 4))
        assert quantised == c.name.startswith("quant")
    assert any(c.num_gt > c.gt.max() for c in small) and any(c.num_gt < c.gt.max() for c in small)
    for c in (A.SELECT_BY_NAME["big_quant"], A.SELECT_BY_NAME["big_cont"]):
        cnt = A.select_counts(c.gt, c.lvl, c.num_gt, c.num_level)
        # 1024 = kSelCap (csrc/orp_assign.hip): the largest list the counting formulation holds
        assert cnt[0] == 1024 == A.SEL_CAP and cnt[1] == 1025 and cnt[2] == 3000
        assert cnt[3:].max() <= 100 and cnt[3:].min() >= 10 and 5500 <= c.q.size <= 6500
        keep = A.ref_apaa_select(c.q, c.gt, c.lvl, c.num_gt, c.num_level, c.k, c.ratio)
        pairs = lambda g: sorted(zip(c.q[(c.gt == g)].tolist(), c.lvl[(c.gt == g)].tolist()))      # noqa: E731
        kept = lambda g: sorted(zip(c.q[keep & (c.gt == g)].tolist(), c.lvl[keep & (c.gt == g)].tolist()))      # noqa: E731
        extra = (7.5, 2)
        assert pairs(2) == sorted(pairs(1) + [extra]) and max(q for q, _ in pairs(1)) < 7.5
        assert kept(1) == kept(2) and len(kept(1)) == 12                      # ceil(0.4 * 30)
        assert not np.array_equal(c.q[c.gt == 1], c.q[c.gt == 2][:1024])       # permuted
    for c in A.SELECT_CASES:
        cnt = A.select_counts(c.gt, c.lvl, c.num_gt, c.num_level)
        if c.name.endswith("_sequential"):
            assert cnt.min() > A.SEL_CAP, c.name
        elif not c.name.startswith("big"):
            assert cnt.max() <= A.SEL_CAP, c.name


def test_select_special_values_follow_the_stated_order():
    """The hand cases, from the reference: the kept indices written out in tests/assign_cases.py.  The padding of the
    *_sequential twins (NaN with the sign bit clear at higher indices on a level of its own) does not change which of the
    original positives of the per-level case are kept.  The palette cases hold both zeros, both NaN, +inf and negative
    values."""
    for case, kept in ((A.HAND_LEVEL_CUT, A.HAND_LEVEL_CUT_KEPT), (A.HAND_FINAL_CUT, A.HAND_FINAL_CUT_KEPT)):
        keep = A.ref_apaa_select(case.q, case.gt, case.lvl, case.num_gt, case.num_level, case.k, case.ratio)
        assert np.nonzero(keep)[0].tolist() == kept
        bits = case.q.view(np.uint32)
        assert {0x00000000, 0x80000000, 0x7FC00000, 0xFFC00000, 0x7F800000} <= set(bits.tolist()) and (case.q < 0).any()
    c, p = A.HAND_LEVEL_CUT, A.SELECT_BY_NAME["hand_level_cut_sequential"]
    keep = A.ref_apaa_select(p.q, p.gt, p.lvl, p.num_gt, p.num_level, p.k, p.ratio)
    assert np.nonzero(keep[:c.q.size])[0].tolist() == A.HAND_LEVEL_CUT_KEPT and keep[c.q.size:].sum() == c.num_gt
    # 0.0 at index 0 and -0.0 at index 1 of one level; 1.0 and the sign-set NaN on the next
    assert c.q.view(np.uint32)[:4].tolist() == [0x00000000, 0x80000000, 0x3F800000, 0xFFC00000]
    for name in ("palette_k1_r10", "palette_k6_r04", "palette_k2_r001"):
        bits = set(A.SELECT_BY_NAME[name].q.view(np.uint32).tolist())
        assert {0x00000000, 0x80000000, 0x7FC00000, 0xFFC00000, 0x7F800000, 0xBFC00000} <= bits


# ---- feature dissimilarity --------------------------------------------------------------------------------------------------------
def _oracle_dissimilarity(oracle, feats, pts, img, lvl):
    want = np.empty(pts.shape[0], np.float32)
    for i in range(pts.shape[0]):
        s = oracle.sample_points(feats[lvl[i]][img[i]], A.FEAT_STRIDES[lvl[i]], pts[i:i + 1])
        want[i] = oracle.feature_dissimilarity(s)[0]
    return want


@pytest.mark.parametrize("P", A.FEAT_PS)
@pytest.mark.parametrize("C", A.FEAT_CS)
def test_feature_dissimilarity_reference_vs_oracle(C, P, oracle):
    """The float64 grid_sample reference agrees with oracle.sample_points -> oracle.feature_dissimilarity (fp32) within the
    project's bar for loss floats, 1e-4 absolute.  The data: H != W on every level; P = 501 uses every (image, level) pair; the
    all-zero map gives exactly 1; every norm of the scaled map is under the 1e-2 clamp; points fall inside, across every border
    and more than a pixel outside; and the case is well conditioned -- moving every coordinate by a few fp32 ulps moves the
    reference by far less than the bar (the operator is discontinuous where a sampled vector vanishes)."""
    feats, pts, img, lvl = A.feat_case(C, P)
    assert all(f.shape == (A.FEAT_BATCH, C, h, w) and h != w for f, (h, w) in zip(feats, A.FEAT_LEVELS))
    ref = A.ref_feature_dissimilarity(feats, A.FEAT_STRIDES, pts, img, lvl)
    assert ref.shape == (P,) and np.isfinite(ref).all() and ref.min() >= -1e-12 and ref.max() <= 2 + 1e-12
    assert np.max(np.abs(ref - _oracle_dissimilarity(oracle, feats, pts, img, lvl))) <= 1e-4
    moved = (pts.astype(np.float64) * (1 + 2.0 ** -21)).astype(np.float32)
    assert np.max(np.abs(ref - A.ref_feature_dissimilarity(feats, A.FEAT_STRIDES, moved, img, lvl))) <= 1e-5
    zero = (img == A.FEAT_ZERO_MAP[0]) & (lvl == A.FEAT_ZERO_MAP[1])
    assert np.all(ref[zero] == 1.0)
    if P == 501:
        assert len(set(zip(img.tolist(), lvl.tolist()))) == A.FEAT_BATCH * len(A.FEAT_LEVELS) and zero.sum() > 10
        small = (img == A.FEAT_SMALL_MAP[0]) & (lvl == A.FEAT_SMALL_MAP[1])
        f = feats[A.FEAT_SMALL_MAP[1]][A.FEAT_SMALL_MAP[0]].astype(np.float64)
        assert small.sum() > 10 and np.sqrt((f * f).sum(0)).max() < 1e-2 and f.any()
        assert np.abs(ref[small] - 1).max() > 1e-3                           # ... and the result is still a cosine, not the constant 1
        h = np.asarray([A.FEAT_LEVELS[l][0] * A.FEAT_STRIDES[l] for l in lvl], np.float64)[:, None]
        w = np.asarray([A.FEAT_LEVELS[l][1] * A.FEAT_STRIDES[l] for l in lvl], np.float64)[:, None]
        s = np.asarray([A.FEAT_STRIDES[l] for l in lvl], np.float64)[:, None]
        x, y = pts[:, 0::2].astype(np.float64), pts[:, 1::2].astype(np.float64)
        for frac in ((x < -1.5 * s), (x > w + 1.5 * s), (y < -1.5 * s), (y > h + 1.5 * s),                  # all four taps invalid
                     (x > -0.5 * s) & (x < 0.5 * s), (x > w - 0.5 * s) & (x < w + 0.5 * s),                    # one column of taps invalid
                     (y > -0.5 * s) & (y < 0.5 * s), (y > h - 0.5 * s) & (y < h + 0.5 * s),
                     (x > s) & (x < w - s) & (y > s) & (y < h - s)):
            assert frac.mean() >= 0.01
        assert np.all(ref[4] == 1.0)                                         # the hand-placed positive whose nine points are all outside
        assert (x[1, :5] == 0).all() and (y[1, 5:] == 0).all() and (x[2, :5] == w[2]).all() and (y[2, 5:] == h[2]).all()
