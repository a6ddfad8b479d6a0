"""Helper of the assigner / APAA selection tests (not a conftest, no tests in here): seeded case tables for the four operators of
csrc/orp_assign.hip and a plain numpy / torch-CPU reference of each, written from the semantics stated in that file's header
and kernel comments -- not from the CPU oracle (oracle/orp_oracle4.c), which tests/test_assign_cases.py compares them with.

The decision operators (point assign, max-IoU assign, select) are compared EXACTLY, so their cases are built from values on
which every tie rule fires: gt centres on a 4-px lattice against a stride-8 grid, overlaps that are multiples of 1/8 landing on
every threshold, quality values that are multiples of 1/4, zeros of both signs and NaN of both signs.  The shapes are the
smallest that reach each route of the launch code (k <= 256 / k > 256, n < 4096 / n >= 4096, more than kSelCap = 1024 positives
of one gt, ...).  tests/test_assign_cases.py asserts without a GPU that the data has these properties; tests/test_gpu_assign.py
runs the kernels.

Nothing here calls an orp_* entry point."""
import collections
import math

import numpy as np
import torch

F32 = np.float32
NAN_POS = np.array([0x7FC00000], np.uint32).view(np.float32)[0]      # quiet NaN, sign bit clear
NAN_NEG = np.array([0xFFC00000], np.uint32).view(np.float32)[0]      # quiet NaN, sign bit set
SEL_CAP = 1024            # kSelCap of apaa_select_kernel: a gt with more positives than this takes the sequential formulation


# ---- PointAssigner ----------------------------------------------------------------------------------------------------------------
def ref_point_assign(points, gts, scale, pos_num, stats=None):
    """points [N, 3] (x, y, stride), gts [K, 8] -> gt_inds [N] int64 (0 background, else 1-based gt).  fp32 throughout, one
    rounding per operation (the kernel is built without contraction).  Per gt in order: centre and extent of the axis-aligned
    hull with the extent clamped at 1e-6, level = truncated mean of the two log2(extent / scale) clamped to the levels the
    points have, the pos_num smallest (distance, point index) of that level; a point changes owner only on a STRICTLY smaller
    distance.  `stats` (a dict) receives counts a test needs to know that the ties happened: "contested_equal" = a selected
    point already owned at exactly the same distance, "cut_ties" = top-pos_num cuts between two equal distances."""
    p = np.asarray(points, F32).reshape(-1, 3)
    g = np.asarray(gts, F32).reshape(-1, 8)
    n = p.shape[0]
    out = np.zeros(n, np.int64)
    if n == 0 or g.shape[0] == 0:
        return out
    plvl = np.trunc(np.log2(p[:, 2])).astype(np.int64)
    lo, hi = int(plvl.min()), int(plvl.max())
    owner_d = np.full(n, np.inf, F32)
    two, sc, eps = F32(2), F32(scale), F32(1e-6)
    for gi in range(g.shape[0]):
        xs, ys = g[gi, 0::2], g[gi, 1::2]
        cx, cy = (xs.min() + xs.max()) / two, (ys.min() + ys.max()) / two
        w, h = np.maximum(xs.max() - xs.min(), eps), np.maximum(ys.max() - ys.min(), eps)
        lvl = int(np.trunc((np.log2(w / sc) + np.log2(h / sc)) / two))
        lvl = max(lo, min(hi, lvl))
        idx = np.nonzero(plvl == lvl)[0]
        dx, dy = (p[idx, 0] - cx) / w, (p[idx, 1] - cy) / h
        d = np.sqrt(dx * dx + dy * dy).astype(F32)
        ok = ~np.isnan(d)
        idx, d = idx[ok], d[ok]
        order = np.lexsort((idx, d))                       # by distance, then by point index
        if stats is not None and order.size > pos_num and d[order[pos_num - 1]] == d[order[pos_num]]:
            stats["cut_ties"] = stats.get("cut_ties", 0) + 1
        for o in order[:pos_num]:
            i = idx[o]
            if stats is not None and out[i] != 0 and d[o] == owner_d[i]:
                stats["contested_equal"] = stats.get("contested_equal", 0) + 1
            if d[o] < owner_d[i]:
                out[i] = gi + 1
                owner_d[i] = d[o]
    return out


def grid_points(size, strides):
    """The point grid of a size x size image: per stride s the (size / s)^2 cell origins, level-major, [N, 3] fp32."""
    pts = []
    for s in strides:
        f = size // s
        ys, xs = np.meshgrid(np.arange(f) * s, np.arange(f) * s, indexing="ij")
        pts.append(np.stack([xs.ravel(), ys.ravel(), np.full(f * f, s)], 1))
    return np.concatenate(pts, 0).astype(F32)


def _box(cx, cy, w, h):
    x0, x1, y0, y1 = cx - w / 2.0, cx + w / 2.0, cy - h / 2.0, cy + h / 2.0
    return [x0, y0, x1, y0, x1, y1, x0, y1]


# (w, h) in units of 2^l: squares of side 4 and 6 and the 2:1 rectangles of short side 4.  Level expression: l, l + 0.585,
# l + 0.5 -- an exact integer or at least 0.29 from one (the 2:1 rectangle of short side 6 would sit at l + 1.085: left out).
_POINT_SHAPES = ((4.0, 4.0), (6.0, 6.0), (8.0, 4.0), (4.0, 8.0))


def point_gts(k, seed, size=256):
    """k gts: axis-aligned boxes of the shapes above at l in 0 .. 8, centres on the 4-px lattice of the image.  From the fifth
    on, every eighth gt is an exact duplicate of an earlier one; with k >= 8, gt 5 has zero width and gt 6 zero area."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(k):
        if i >= 4 and i % 8 == 4:
            out.append(list(out[rng.randint(0, i)]))
            continue
        l = rng.randint(0, 9)
        w, h = _POINT_SHAPES[rng.randint(0, len(_POINT_SHAPES))]
        w, h = w * 2.0 ** l, h * 2.0 ** l
        if k >= 8 and i == 5:
            w, h = 0.0, 64.0
        if k >= 8 and i == 6:
            w, h = 0.0, 0.0
        cx, cy = 4.0 * rng.randint(0, size // 4), 4.0 * rng.randint(0, size // 4)
        out.append(_box(cx, cy, w, h))
    return np.asarray(out, F32).reshape(k, 8)


def point_level_expression(gts, scale):
    """float64 value of the level expression of every gt (before truncation and clamping), for the premise check."""
    g = np.asarray(gts, np.float64).reshape(-1, 8)
    w = np.maximum(g[:, 0::2].max(1) - g[:, 0::2].min(1), 1e-6)
    h = np.maximum(g[:, 1::2].max(1) - g[:, 1::2].min(1), 1e-6)
    return (np.log2(w / scale) + np.log2(h / scale)) / 2


PointCase = collections.namedtuple("PointCase", "name strides k seed")
POINT_CASES = [
    PointCase("k1", (8, 16, 32, 64, 128), 1, 101),
    PointCase("k40", (8, 16, 32, 64, 128), 40, 102),
    PointCase("k300", (8, 16, 32, 64, 128), 300, 103),
    PointCase("k40_two_levels", (8, 16), 40, 104),          # levels 3 and 4 only: clamping has something to do at the top
]
POINT_POS_NUMS = (1, 3, 9)
POINT_SCALE = 4


def point_case(case):
    """-> (points [N, 3], gts [K, 8]) fp32."""
    return grid_points(256, case.strides), point_gts(case.k, case.seed)


# ---- MaxIoUAssigner ---------------------------------------------------------------------------------------------------------------
def _max_nan_wins(a, axis):
    """torch.max semantics along `axis` of a 2-D array: (values, indices); NaN wins, the first index on ties."""
    isn = np.isnan(a)
    has = isn.any(axis)
    arg = np.where(has, isn.argmax(axis), np.where(isn, -np.inf, a).argmax(axis))
    val = np.take_along_axis(a, np.expand_dims(arg, axis), axis).squeeze(axis)
    return val, arg


def ref_max_iou_assign(ov, pos, neg, min_pos, assign_all):
    """ov [N, K] fp32 point-major -> (gt_inds [N] int64 in {-1, 0, 1 .. K}, max_overlaps [N] fp32).  `neg` is a scalar (the
    range [0, neg)) or a (lo, hi) pair.  Row maximum with torch.max semantics; -1 -> 0 where lo <= max < hi -> arg + 1 where
    max >= pos; then per gt in order, if its column maximum is >= min_pos (false for NaN): assign_all -> EVERY row equal to the
    column maximum takes the gt (a later gt overwrites), else only the first arg-max row does."""
    ov = np.asarray(ov, F32)
    n, k = ov.shape
    lo, hi = (F32(neg[0]), F32(neg[1])) if isinstance(neg, (tuple, list)) else (F32(0), F32(neg))
    if k == 0:
        return np.zeros(n, np.int64), np.zeros(n, F32)
    m, arg = _max_nan_wins(ov, 1)
    gt_inds = np.full(n, -1, np.int64)
    with np.errstate(invalid="ignore"):
        gt_inds[(m >= lo) & (m < hi)] = 0
        sel = m >= F32(pos)
        gt_inds[sel] = arg[sel] + 1
        gm, garg = _max_nan_wins(ov, 0)
        for g in range(k):
            if not gm[g] >= F32(min_pos):
                continue
            if assign_all:
                gt_inds[ov[:, g] == gm[g]] = g + 1
            else:
                gt_inds[garg[g]] = g + 1
    return gt_inds, m


# k <= 256 takes gt_max_rows_kernel + gt_max_finish_kernel (rows per pass 256 // k: 1 from k = 129 on, idle tail threads unless
# k divides 256), k > 256 takes gt_max_kernel; n < 4096 launches ceil(n / 64) row blocks, n >= 4096 launches 64.
MAXIOU_KS = (1, 2, 23, 100, 255, 256, 257, 300)
MAXIOU_NS = (1, 63, 64, 65, 4095, 4096, 4097)
MAXIOU_SHAPES = [(1, 1), (2, 63), (23, 64), (100, 65), (255, 4095), (256, 4096), (257, 4097), (300, 4097),
                 (256, 63), (257, 1), (300, 64), (255, 65), (1, 4097), (23, 4096), (100, 4095), (2, 4096), (257, 65)]
MAXIOU_POS = 0.5
MAXIOU_NEGS = ((0.125, 0.375), 0.375)
MAXIOU_MIN_POS = (0.0, 0.25)
MAXIOU_ARGMAX_MAX_N = 1000           # gt_max_assign_all=False is one thread: keep it to small n


MAXIOU_NAN_COLUMN_KS = (23, 256, 257)     # one k per column-maximum route: several rows per pass, one row per pass, gt_max_kernel


def maxiou_special_columns(k):
    """(all-zero column, all-NaN column or None) of maxiou_case, or None for k < 3.  The zero column is the LAST gt for odd k
    (nothing overwrites it: at min_pos_iou = 0 every row takes it) and gt 2 for even k (later gts overwrite most rows).  An
    all-NaN column makes EVERY row maximum NaN, so only the k of MAXIOU_NAN_COLUMN_KS have one; the row arg-max and its ties
    are tested by the other k."""
    return None if k < 3 else ((k - 1 if k % 2 else 1), (k - 2 if k in MAXIOU_NAN_COLUMN_KS else None))


def maxiou_case(k, n):
    """[n, k] fp32 overlaps, multiples of 1/8 in [0, 1] capped per column and per row (so column and row maxima differ and land
    on every threshold, whatever k and n).  With n * k >= 64 five scattered NaN; with k >= 3 the columns of maxiou_special_columns."""
    rng = np.random.RandomState(1000 * k + n)
    cap = rng.randint(1, 9, size=k)
    cap[0] = 8                                 # (so that k = 1 and k = 2 reach every value too)
    row_cap = rng.randint(0, 9, size=n)
    ov = np.minimum(np.minimum(rng.randint(0, 9, size=(n, k)), cap[None, :]), row_cap[:, None]).astype(F32) / F32(8)
    if n * k >= 64:
        for _ in range(5):
            ov[rng.randint(0, n), rng.randint(0, k)] = np.nan
    if k >= 3:
        zero, nan = maxiou_special_columns(k)
        ov[:, zero] = 0
        if nan is not None:
            ov[:, nan] = np.nan
    return ov


def maxiou_runs(n):
    """(neg, min_pos, assign_all) combinations a shape is run with."""
    return [(neg, mp, aa) for neg in MAXIOU_NEGS for mp in MAXIOU_MIN_POS for aa in (True, False)
            if aa or n <= MAXIOU_ARGMAX_MAX_N]


# ---- APAA selection ---------------------------------------------------------------------------------------------------------------
def ref_apaa_select(q, gt, lvl, num_gt, num_level, k, ratio):
    """-> keep [P] bool.  Total order of the quality values: NaN (either sign) last, -0 == +0, then level, then index.  Per gt
    1 .. num_gt: per level 0 .. num_level - 1 the k smallest, concatenated level-major; STABLE sort of the candidates by value;
    keep the first ceil(ratio * n) of n candidates, all of them if n < 2.  Positives of gt 0, of a gt above num_gt or of a level
    outside [0, num_level) are never kept."""
    q = np.asarray(q, F32)
    gt = np.asarray(gt, np.int64)
    lvl = np.asarray(lvl, np.int64)
    isn = np.isnan(q)
    val = np.where(isn | (q == 0), F32(0), q)              # -0 -> +0; NaN carried by `isn`
    keep = np.zeros(q.shape[0], bool)
    for g in range(1, int(num_gt) + 1):
        cand = []
        for lv in range(int(num_level)):
            idx = np.nonzero((gt == g) & (lvl == lv))[0]
            order = np.lexsort((idx, val[idx], isn[idx]))
            cand.extend(idx[order[:k]].tolist())
        cand = np.asarray(cand, np.int64)
        n = cand.size
        if n < 2:
            keep[cand] = True
            continue
        order = np.lexsort((np.arange(n), val[cand], isn[cand]))          # stable by (NaN last, value)
        keep[cand[order[:int(math.ceil(float(n) * float(ratio)))]]] = True
    return keep


def select_counts(gt, lvl, num_gt, num_level):
    """Positives per gt 1 .. num_gt that the kernel lists (level in range): which formulation each gt takes."""
    gt, lvl = np.asarray(gt, np.int64), np.asarray(lvl, np.int64)
    ok = (lvl >= 0) & (lvl < num_level) & (gt >= 1) & (gt <= num_gt)
    return np.bincount(gt[ok], minlength=num_gt + 1)[1:]


SelectCase = collections.namedtuple("SelectCase", "name q gt lvl num_gt num_level k ratio special")
# special: the case holds NaN or -0.0


def _select_small(name, seed, quantised, num_level, k, ratio, num_gt_delta):
    """About 600 positives of gts 0 .. 13 (gt 0 = none) on levels -1 .. num_level (both ends out of range); gt 7 has exactly one
    positive.  num_gt = 12 + num_gt_delta: +3 leaves gts with no positive, -2 leaves positives of gts that are not asked for."""
    rng = np.random.RandomState(seed)
    P = 600
    gt = rng.randint(0, 14, P).astype(np.int64)
    gt[gt == 7] = 8
    gt[rng.randint(0, P)] = 7
    lvl = rng.randint(-1, num_level + 1, P).astype(np.int32)
    lvl[gt == 7] = num_level - 1
    q = (rng.randint(0, 20, P) / 4.0 if quantised else rng.uniform(0, 5, P)).astype(F32)
    return SelectCase(name, q, gt, lvl, 12 + num_gt_delta, num_level, k, ratio, False)


def _select_big(name, seed, quantised):
    """Both formulations in one call: gt 1 has exactly SEL_CAP positives, gt 2 the SAME (Q, level) pairs in another order plus
    one more with a Q above all of them (SEL_CAP + 1: sequential), gt 3 has 3000, gts 4 .. 23 a few dozen each; all shuffled
    together.  P is about 6000."""
    rng = np.random.RandomState(seed)
    draw = lambda m: (rng.randint(0, 20, m) / 4.0 if quantised else rng.uniform(0, 5, m)).astype(F32)      # noqa: E731
    q1, l1 = draw(SEL_CAP), rng.randint(0, 5, SEL_CAP)
    perm = rng.permutation(SEL_CAP)
    q2, l2 = np.concatenate([q1[perm], [F32(7.5)]]), np.concatenate([l1[perm], [2]])
    q3, l3 = draw(3000), rng.randint(0, 5, 3000)
    m = 950
    q4, l4, g4 = draw(m), rng.randint(-1, 6, m), rng.randint(4, 24, m)
    q = np.concatenate([q1, q2, q3, q4]).astype(F32)
    lvl = np.concatenate([l1, l2, l3, l4]).astype(np.int32)
    gt = np.concatenate([np.full(SEL_CAP, 1), np.full(SEL_CAP + 1, 2), np.full(3000, 3), g4]).astype(np.int64)
    mix = rng.permutation(q.size)
    return SelectCase(name, q[mix], gt[mix], lvl[mix], 23, 5, 6, 0.4, False)


def _pad(case, name, per_gt):
    """The same case with `per_gt` more positives of every gt 1 .. num_gt, appended (higher indices), all NaN with the sign bit
    clear -- the top of the order, after every tie -- on one more level: every gt then takes the sequential formulation while
    the ranking among the original positives is unchanged."""
    g = np.repeat(np.arange(1, case.num_gt + 1), per_gt).astype(np.int64)
    return SelectCase(name, np.concatenate([case.q, np.full(g.size, NAN_POS, F32)]), np.concatenate([case.gt, g]),
                      np.concatenate([case.lvl, np.full(g.size, case.num_level, np.int32)]), case.num_gt, case.num_level + 1,
                      case.k, case.ratio, True)


def _select_hand_level_cut():
    """per_level_topk = 1, top_ratio = 1: the per-level cut alone decides.  gt 1, one pair or triple per level:
    level 0: +0.0, -0.0        -> the +0.0 (equal values: the smaller index)          index 0
    level 1: 1.0, NaN(sign set) -> the 1.0 (NaN above everything)                      index 2
    level 2: NaN(sign clear), +inf -> the +inf                                         index 5
    level 3: -0.0, -2.0, +0.0  -> the -2.0                                             index 7
    gt 2, level 0: NaN(sign clear), NaN(sign set) -> the first (all NaN are equal)     index 9"""
    q = np.array([0.0, -0.0, 1.0, NAN_NEG, NAN_POS, np.inf, -0.0, -2.0, 0.0, NAN_POS, NAN_NEG], F32)
    gt = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2], np.int64)
    lvl = np.array([0, 0, 1, 1, 2, 2, 3, 3, 3, 0, 0], np.int32)
    return SelectCase("hand_level_cut", q, gt, lvl, 2, 4, 1, 1.0, True), [0, 2, 5, 7, 9]


def _select_hand_final_cut():
    """per_level_topk = 6, top_ratio = 0.25: all four positives of a gt are candidates, the final cut keeps one.
    gt 1, level 0: +0.0, -0.0, 1.0, NaN(sign set)        -> the +0.0                   index 0
    gt 2, level 1: NaN(sign set), 2.0, -3.0, NaN(clear)  -> the -3.0                   index 6
    gt 3, levels 1, 0: +0.0 on level 1, -0.0 on level 0, +inf, NaN -> the -0.0 (equal values: the lower LEVEL)   index 9"""
    q = np.array([0.0, -0.0, 1.0, NAN_NEG, NAN_NEG, 2.0, -3.0, NAN_POS, 0.0, -0.0, np.inf, NAN_POS], F32)
    gt = np.array([1] * 4 + [2] * 4 + [3] * 4, np.int64)
    lvl = np.array([0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1], np.int32)
    return SelectCase("hand_final_cut", q, gt, lvl, 3, 2, 6, 0.25, True), [0, 6, 9]


_PALETTE = np.array([0.0, -0.0, NAN_POS, NAN_NEG, np.inf, -1.5, -0.25, 0.25, 1.0, 0.0, -0.0], F32)


def _select_palette(name, seed, k, ratio):
    """700 positives of gts 1 .. 8 on levels 0 .. 4 whose Q is drawn from a palette of eleven values, four of them zeros and two
    NaN: nearly every cut runs through equal values."""
    rng = np.random.RandomState(seed)
    P = 700
    return SelectCase(name, _PALETTE[rng.randint(0, _PALETTE.size, P)], rng.randint(1, 9, P).astype(np.int64),
                      rng.randint(0, 5, P).astype(np.int32), 8, 5, k, ratio, True)


HAND_LEVEL_CUT, HAND_LEVEL_CUT_KEPT = _select_hand_level_cut()
HAND_FINAL_CUT, HAND_FINAL_CUT_KEPT = _select_hand_final_cut()
SELECT_CASES = [
    _select_small("quant_l5_r04", 201, True, 5, 6, 0.4, 0),
    _select_small("cont_l5_r10", 202, False, 5, 6, 1.0, 3),
    _select_small("quant_l1_r10", 203, True, 1, 6, 1.0, -2),
    _select_small("cont_l1_r001", 204, False, 1, 6, 0.01, 0),
    _select_small("quant_l10_r001", 205, True, 10, 6, 0.01, 3),
    _select_small("cont_l10_r04", 206, False, 10, 6, 0.4, -2),
    _select_small("quant_l16_k4_r04", 207, True, 16, 4, 0.4, 0),       # per_level_topk * num_level = 64: the cap exactly
    _select_small("cont_l16_k4_r10", 208, False, 16, 4, 1.0, -2),
    _select_big("big_quant", 211, True),
    _select_big("big_cont", 212, False),
    HAND_LEVEL_CUT,
    _pad(HAND_LEVEL_CUT, "hand_level_cut_sequential", SEL_CAP + 6),
    HAND_FINAL_CUT,
    _pad(HAND_FINAL_CUT, "hand_final_cut_sequential", SEL_CAP + 6),
    _select_palette("palette_k1_r10", 221, 1, 1.0),
    _select_palette("palette_k6_r04", 222, 6, 0.4),
    _select_palette("palette_k2_r001", 223, 2, 0.01),
    _pad(_select_palette("palette_k1_r10", 221, 1, 1.0), "palette_k1_r10_sequential", SEL_CAP + 1),
    _pad(_select_palette("palette_k6_r04", 222, 6, 0.4), "palette_k6_r04_sequential", SEL_CAP + 1),
]
SELECT_BY_NAME = {c.name: c for c in SELECT_CASES}
assert len(SELECT_BY_NAME) == len(SELECT_CASES)


# ---- APAA feature dissimilarity ---------------------------------------------------------------------------------------------------
def ref_feature_dissimilarity(feats, strides, pts18, img, lvl):
    """feats: list of [B, C, H, W] arrays, pts18 [P, 18] image-space points, img / lvl [P] -> [P] float64.  Everything in
    float64: F.grid_sample (bilinear, zeros, align_corners=False) of the point's (image, level) map at its nine points, the mean
    of the nine, each vector divided by its norm clamped at 1e-2, CosineSimilarity(eps=1e-6) of the two, and the largest
    1 - cosine of the nine."""
    pts = torch.from_numpy(np.asarray(pts18, np.float64)).reshape(-1, 9, 2)
    img, lvl = np.asarray(img, np.int64), np.asarray(lvl, np.int64)
    out = torch.empty(pts.shape[0], dtype=torch.float64)
    for l, (feat, s) in enumerate(zip(feats, strides)):
        f = torch.from_numpy(np.asarray(feat, np.float64))
        B, C, H, W = f.shape
        for b in range(B):
            sel = np.nonzero((img == b) & (lvl == l))[0]
            if sel.size == 0:
                continue
            p = pts[sel]
            grid = torch.stack([p[..., 0] / (W * float(s) / 2) - 1, p[..., 1] / (H * float(s) / 2) - 1], -1)[None]    # [1, P', 9, 2]
            smp = torch.nn.functional.grid_sample(f[b:b + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=False)
            smp = smp[0].permute(1, 2, 0)                                                    # [P', 9, C]
            mean = smp.mean(1, keepdim=True)
            u = smp / smp.norm(dim=2, keepdim=True).clamp(min=1e-2)
            v = mean / mean.norm(dim=2, keepdim=True).clamp(min=1e-2)
            cos = (u * v).sum(2) / (u.norm(dim=2).clamp(min=1e-6) * v.norm(dim=2).clamp(min=1e-6))
            out[sel] = (1 - cos).max(1)[0]
    return out.numpy()


FEAT_LEVELS = ((12, 20), (6, 10), (3, 5))         # H != W
FEAT_STRIDES = (8, 16, 32)
FEAT_BATCH = 3
FEAT_CS = (1, 64, 96, 256)                        # the lane loop strides by 64: less than one trip, one, one and a half, four
FEAT_PS = (1, 5, 501)
FEAT_ZERO_MAP = (1, 2)                            # (image, level): all zero -> the result is exactly 1
FEAT_SMALL_MAP = (2, 1)                           # (image, level): scaled by 1e-4 -> every norm under the 1e-2 clamp
FEAT_HAND_POINTS = 6


def feat_case(C, P):
    """-> (feats [3 x [B, C, H, W] fp32], pts18 [P, 18] fp32, img [P] int32, lvl [P] int32).  Points are uniform from two strides
    outside the map to two strides past its far edge; positive i sits on (image, level) pair i % 9 (rotated by C so that P = 1
    and P = 5 do not always use the same pairs).  With P >= 9 the first FEAT_HAND_POINTS positives are hand-placed: on pixel
    centres, on each of the four borders, and two strides outside (all four taps invalid)."""
    rng = np.random.RandomState(7000 + 10 * C + P)
    feats = [rng.normal(size=(FEAT_BATCH, C, h, w)).astype(F32) for h, w in FEAT_LEVELS]
    feats[FEAT_ZERO_MAP[1]][FEAT_ZERO_MAP[0]] = 0
    feats[FEAT_SMALL_MAP[1]][FEAT_SMALL_MAP[0]] *= F32(1e-4)
    pair = (np.arange(P) + C) % (FEAT_BATCH * len(FEAT_LEVELS))
    img, lvl = (pair % FEAT_BATCH).astype(np.int32), (pair // FEAT_BATCH).astype(np.int32)
    pts = np.empty((P, 9, 2))
    for i in range(P):
        (h, w), s = FEAT_LEVELS[lvl[i]], FEAT_STRIDES[lvl[i]]
        pts[i, :, 0] = rng.uniform(-2 * s, (w + 2) * s, 9)
        pts[i, :, 1] = rng.uniform(-2 * s, (h + 2) * s, 9)
    if P >= 9:
        for i in range(FEAT_HAND_POINTS):
            (h, w), s = FEAT_LEVELS[lvl[i]], FEAT_STRIDES[lvl[i]]
            ex, ey = w * s, h * s
            if i == 0:        # pixel centres
                pts[i, :, 0] = (rng.randint(0, w, 9) + 0.5) * s
                pts[i, :, 1] = (rng.randint(0, h, 9) + 0.5) * s
            elif i == 1:      # left border, then top border
                pts[i, :5, 0] = 0
                pts[i, 5:, 1] = 0
            elif i == 2:      # right border, then bottom border
                pts[i, :5, 0] = ex
                pts[i, 5:, 1] = ey
            elif i == 3:      # the four corners of the map
                pts[i, :4] = [[0, 0], [ex, 0], [0, ey], [ex, ey]]
            elif i == 4:      # every point two strides outside: nine zero vectors
                pts[i, :, 0] = -2 * s
                pts[i, :, 1] = rng.uniform(0, ey, 9)
            else:             # some points outside on each side, the rest inside
                pts[i, 0], pts[i, 1], pts[i, 2], pts[i, 3] = [-2 * s, ey / 2], [ex + 2 * s, ey / 2], [ex / 2, -2 * s], [ex / 2, ey + 2 * s]
    return feats, pts.reshape(P, 18).astype(F32), img, lvl
