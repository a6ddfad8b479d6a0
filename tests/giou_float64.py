"""Helper of the convex GIoU gradient tests (not a conftest): a float64 GIoU written from the definition, its difference
quotients, a row classifier that looks at the inputs and at that float64 function only, and seeded input families.

GIoU(hull(9 points), gt quad) = I / U - (C - U) / C with A = area of the hull, B = area of the gt, I = area of their
intersection, U = A + B - I and C = area of the hull of both.  Here: monotone-chain hull, Sutherland-Hodgman clip, shoelace
area, Python floats (float64), no epsilon anywhere.  Nothing in this file is taken from csrc/orp_convex_giou.hip, from the
oracle's restatement or from the reference's kernel: they march, clip triangle fans against the origin and compare against
1E-8, this file does none of that.

Classes of a row (`classify`):
  TOUCHING  a hull vertex lies within 1e-8 of a gt vertex or of a gt edge (segment).  The function has a kink there whose
            one-sided derivatives the reference's gradient does not respect (it drops coincident vertices and clip crossings
            "equal" to a vertex): only the reference itself is an authority for these rows.
  SMOOTH    the forward and the backward difference quotient of each of the 18 coordinates agree: a derivative exists, the
            analytic gradient must equal the central quotient.
  KINK      they do not (a point enters or leaves the hull, ties, duplicates, ...): every gradient component must lie
            between the two one-sided quotients, which is all the math says at a kink.  (Central quotients at two step
            sizes agree at a kink -- both return the average -- so "smooth" has to be one-sided agreement.)

Exact copies of a point are moved TOGETHER by the quotients, and it is the SUM of the gradient over the copies that is held
against them.  Moved one at a time, a copy that sits on a hull vertex can only add a vertex next to the one its twin keeps:
GIoU is then neither a maximum nor a minimum of smooth pieces (I / U grows with the hull, (C - U) / C mixes signs), and the
limit of the true gradients of the nearby smooth inputs -- everything to one copy, nothing to the others, which is what the
reference, the oracle and the kernel emit -- need not lie between the one-sided quotients of a single copy (measured: 84 of
300 rows of the `duplicates` family up to 0.92 x row scale outside, while the summed gradient equals the quotient of the
distinct points to 6e-8).  Which copy carries the gradient is the reference's convention (the first in input order) and is
held against the oracle and the reference only.  For rows without exact copies nothing changes.

  POINT     all 9 points are the same point.  The hull is no polygon, and the reference's convention is NO gradient: all 18
            components are exactly 0, also where the point lies outside the gt and moving it changes C (the summed
            quotient is not 0 there: measured on 75 of 300 rows, up to the whole row scale).  Like TOUCHING this is a
            convention of the reference that stays; unlike it, it can be written down, so these rows are held to exactly
            0 instead of to the quotients.  Only the `coincident` family may contain such rows.
"""
import collections
import functools

import numpy as np

from orientedreppoints_amd import synthetic as S

SMOOTH, KINK, TOUCHING, POINT = 0, 1, 2, 3
CLASS_NAMES = ("smooth", "kink", "touching", "point")
TOUCH_EPS = 1e-8
# one-sided quotients "agree" below this fraction of the row's scale (largest |central quotient| of the row).  Of the
# reference alone: for a smooth row fwd - bwd = h f'' ~ (h / size) x scale, at most a few 1e-5 with the steps below.
SMOOTH_TOL = 1e-4
# slack of the bracket check, in units of the row scale: the one-sided quotients carry O(h f'') themselves, i.e. as much as
# two quotients that count as agreeing may differ.  (1e-3 was the starting point, with 6e-4 measured on exact grids at
# step 2^-13; at the steps below the float64 function's own worst case is 1.3e-5, on the exact grids at 2^-15.)
BRACKET_SLACK = 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# float64 GIoU from the definition
# ---------------------------------------------------------------------------------------------------------------------
def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull(points):
    """Monotone chain; counter-clockwise, collinear points dropped; fewer than 3 vertices when the set is degenerate."""
    p = sorted(set(points))
    if len(p) <= 2:
        return p
    lower, upper = [], []
    for q in p:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], q) <= 0:
            lower.pop()
        lower.append(q)
    for q in reversed(p):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], q) <= 0:
            upper.pop()
        upper.append(q)
    return lower[:-1] + upper[:-1]


def area(poly):
    """Shoelace, signed (positive = counter-clockwise)."""
    s = 0.0
    n = len(poly)
    for i in range(n):
        a, b = poly[i], poly[(i + 1) % n]
        s += a[0] * b[1] - a[1] * b[0]
    return 0.5 * s


def clip(subject, clipper):
    """Sutherland-Hodgman: `subject` cut by each edge of the convex counter-clockwise `clipper`."""
    out = subject
    n = len(clipper)
    for i in range(n):
        a, b = clipper[i], clipper[(i + 1) % n]
        src, out = out, []
        if not src:
            break
        p = src[-1]
        cp = _cross(a, b, p)
        for q in src:
            cq = _cross(a, b, q)
            if (cp >= 0) != (cq >= 0):
                t = cp / (cp - cq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
            if cq >= 0:
                out.append(q)
            p, cp = q, cq
    return out


def _ccw(quad):
    return quad if area(quad) >= 0 else quad[::-1]


def giou_one(points, gt_ccw, gt_area):
    """(GIoU, IoU) of the hull of `points` (list of (x, y)) and the convex counter-clockwise quad `gt_ccw`."""
    h = hull(points)
    a = area(h) if len(h) >= 3 else 0.0
    i = abs(area(clip(h, gt_ccw))) if len(h) >= 3 else 0.0
    u = a + gt_area - i
    c = area(hull(points + gt_ccw))
    return i / u - (c - u) / c, i / u


def giou_f64(pts, gts):
    """pts [n,18], gts [n,8] -> (giou[n], iou[n]) float64."""
    pts = np.asarray(pts, np.float64).reshape(-1, 9, 2)
    gts = np.asarray(gts, np.float64).reshape(-1, 4, 2)
    out = np.empty((pts.shape[0], 2))
    for r in range(pts.shape[0]):
        g = _ccw([tuple(v) for v in gts[r].tolist()])
        out[r] = giou_one([tuple(v) for v in pts[r].tolist()], g, area(g))
    return out[:, 0], out[:, 1]


# ---------------------------------------------------------------------------------------------------------------------
# difference quotients and the classifier
# ---------------------------------------------------------------------------------------------------------------------
Quotients = collections.namedtuple("Quotients", "value iou fwd bwd cen cen_half scale noise cls same")


def step_is_exact(pts, h):
    """x + h, x - h, x + h/2, x - h/2 are float32 numbers for every coordinate (the perturbed inputs are inputs the kernel
    could be given, and the quotients' denominators are exact)."""
    x = np.asarray(pts, np.float32).astype(np.float64)
    return all(np.array_equal((x + d).astype(np.float32).astype(np.float64), x + d) for d in (h, -h, h / 2, -h / 2))


def _touching(points, gt_ccw):
    for v in hull(points):
        for k in range(4):
            a, b = gt_ccw[k], gt_ccw[(k + 1) % 4]
            ex, ey = b[0] - a[0], b[1] - a[1]
            t = ((v[0] - a[0]) * ex + (v[1] - a[1]) * ey) / (ex * ex + ey * ey)
            t = min(1.0, max(0.0, t))
            dx, dy = v[0] - (a[0] + t * ex), v[1] - (a[1] + t * ey)
            if dx * dx + dy * dy <= TOUCH_EPS * TOUCH_EPS:
                return True
    return False


def quotients(pts, gts, h):
    """Value, forward / backward / central quotients at step h, central at h / 2, row scale (largest |central|), the
    quotient's own noise |central(h) - central(h/2)| (row maximum), the class of every row and same[n,9,9] (point i is an
    exact copy of point j; copies move together).  Float64 throughout; sees nothing but the inputs."""
    assert step_is_exact(pts, h), "step %g is not exact in float32 at these coordinates" % h
    P = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 9, 2)
    G = np.asarray(gts, np.float32).astype(np.float64).reshape(-1, 4, 2)
    n = P.shape[0]
    value, iou = np.empty(n), np.empty(n)
    f = np.empty((4, n, 18))                       # f(x + h), f(x - h), f(x + h/2), f(x - h/2)
    cls = np.empty(n, np.int64)
    for r in range(n):
        g = _ccw([tuple(v) for v in G[r].tolist()])
        ga = area(g)
        base = [tuple(v) for v in P[r].tolist()]
        value[r], iou[r] = giou_one(base, g, ga)
        for k in range(18):
            i, c = divmod(k, 2)
            for j, d in enumerate((h, -h, h / 2, -h / 2)):
                q = [((v[0] + d, v[1]) if c == 0 else (v[0], v[1] + d)) if v == base[i] else v for v in base]
                f[j, r, k] = giou_one(q, g, ga)[0]
        cls[r] = POINT if len(set(base)) == 1 else TOUCHING if _touching(base, g) else SMOOTH
    fwd = (f[0] - value[:, None]) / h
    bwd = (value[:, None] - f[1]) / h
    cen = (f[0] - f[1]) / (2 * h)
    cen_half = (f[2] - f[3]) / h
    scale = np.abs(cen).max(1)
    noise = np.abs(cen - cen_half).max(1)
    kink = (np.abs(fwd - bwd) > SMOOTH_TOL * scale[:, None]).any(1)
    cls[(cls == SMOOTH) & kink] = KINK
    same = (P[:, :, None, :] == P[:, None, :, :]).all(3)
    return Quotients(value, iou, fwd, bwd, cen, cen_half, scale, noise, cls, same)


def central_bar(q):
    """Per row: how close an analytic gradient has to be to the central quotient on a smooth row -- the quotient's own
    noise, from the float64 function alone: max(1e-6 x row scale, 10 x |central(h) - central(h/2)|)."""
    return np.maximum(1e-6 * q.scale, 10.0 * q.noise)


# one float ulp at 1: |GIoU| <= 1, the outputs are float64 values rounded once to float (half an ulp), and the 1E-8 sign
# thresholds of the kernels may move an area by ~1e-8 of its size
VALUE_BAR = 2.0 ** -23


def check_against_math(out19, q):
    """The checks a [n,19] output (18 gradient components + GIoU) has to pass against the float64 function.  Returns
    (measurements, failures): measurements = dict of the maxima, failures = list of strings (empty = pass)."""
    out19 = np.asarray(out19, np.float64)
    val = out19[:, 18]
    grad = np.einsum("nij,njc->nic", q.same.astype(np.float64), np.nan_to_num(out19[:, :18]).reshape(-1, 9, 2)).reshape(-1, 18)
    fails = []
    if not np.isfinite(out19).all():
        fails.append("%d rows with a non-finite output" % int((~np.isfinite(out19)).any(1).sum()))
    dv = np.abs(val - q.value)
    bad = np.nonzero(~(dv <= VALUE_BAR))[0]
    if bad.size:
        fails.append("value: %d rows off the float64 GIoU by more than %.3g (worst row %d: %.3g)"
                     % (bad.size, VALUE_BAR, int(bad[np.argmax(dv[bad])]), float(np.nanmax(dv[bad]))))
    sm = q.cls == SMOOTH
    dc = np.abs(grad - q.cen).max(1)
    bar = central_bar(q)
    bad = np.nonzero(sm & ~(dc <= bar))[0]
    if bad.size:
        w = int(bad[np.argmax(dc[bad] / np.maximum(bar[bad], 1e-300))])
        fails.append("smooth rows: %d off the central quotient (worst row %d: |d| = %.3g, bar %.3g, scale %.3g)"
                     % (bad.size, w, dc[w], bar[w], q.scale[w]))
    lo, hi = np.minimum(q.fwd, q.bwd), np.maximum(q.fwd, q.bwd)
    out = np.maximum(lo - grad, grad - hi).max(1)                 # how far outside the bracket (<= 0: inside)
    checked = (q.cls == SMOOTH) | (q.cls == KINK)
    bad = np.nonzero((q.cls == POINT) & (out19[:, :18] != 0).any(1))[0]
    if bad.size:
        fails.append("point rows: %d with a gradient that is not exactly 0 (first: row %d)" % (bad.size, int(bad[0])))
    bad = np.nonzero(checked & ~(out <= BRACKET_SLACK * q.scale))[0]
    if bad.size:
        w = int(bad[np.argmax(out[bad] / np.maximum(q.scale[bad], 1e-300))])
        fails.append("bracket: %d rows outside [backward, forward] (worst row %d: %.3g outside, scale %.3g)"
                     % (bad.size, w, out[w], q.scale[w]))
    pos = q.scale > 0
    m = dict(value=float(np.nanmax(dv)) if dv.size else 0.0,
             smooth_rel=float(np.max(dc[sm & pos] / q.scale[sm & pos])) if (sm & pos).any() else 0.0,
             bracket_rel=float(max(0.0, np.max(out[checked & pos] / q.scale[checked & pos]))) if (checked & pos).any() else 0.0,
             counts=tuple(int((q.cls == c).sum()) for c in (SMOOTH, KINK, TOUCHING, POINT)))
    return m, fails


# ---------------------------------------------------------------------------------------------------------------------
# seeded input families
# ---------------------------------------------------------------------------------------------------------------------
GRID = np.array([[x, y] for y in (-1.0, 0.0, 1.0) for x in (-1.0, 0.0, 1.0)])      # 9 x 2


def _rot(xy, th):
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    return np.stack([c * xy[..., 0] - s * xy[..., 1], s * xy[..., 0] + c * xy[..., 1]], axis=-1)


def _rects(rng, n, lo, hi, wh, aligned=False, integer=False):
    """[n,8] rectangles: centres U(lo, hi), sides U(wh), random angle (0 when `aligned`)."""
    c = rng.uniform(lo, hi, size=(n, 2))
    w, h = rng.uniform(wh[0], wh[1], size=n), rng.uniform(wh[0], wh[1], size=n)
    if integer:
        c, w, h = np.round(c), 2 * np.ceil(w / 2), 2 * np.ceil(h / 2)
    th = np.zeros(n) if aligned else rng.uniform(-np.pi / 2, np.pi / 2, size=n)
    return S._corners(c[:, 0], c[:, 1], w, h, th)


def _pack(pts, gts):
    return np.asarray(pts, np.float64).reshape(-1, 18), np.asarray(gts, np.float64).reshape(-1, 8)


def gen_existing(n, seed):
    """What the suite checked so far: synthetic.gen_pointsets within N(0, 15) of the gt's centre."""
    gts = S.gen_gts(n, seed)
    ctr = gts.reshape(-1, 4, 2).mean(1) + np.random.RandomState(seed + 1).normal(0, 15, (n, 2))
    return _pack(S.gen_pointsets(n, seed + 2, around=ctr), gts)


def gen_cluster(n, seed):
    """9 points within sigma = 0.08 px of each other, inside the gt (the head's first iterations)."""
    rng = np.random.RandomState(seed)
    gts = S.gen_gts(n, seed)
    q = gts.reshape(-1, 4, 2)
    ctr = q.mean(1) + 0.25 * rng.uniform(-1, 1, (n, 1)) * (q[:, 1] - q[:, 0]) + 0.25 * rng.uniform(-1, 1, (n, 1)) * (q[:, 3] - q[:, 0])
    return _pack(ctr[:, None, :] + rng.normal(0, 0.08, (n, 9, 2)), gts)


def gen_enclosing(n, seed):
    """The hull encloses the gt: a jittered, rotated 3 x 3 grid about 6 x the gt's size."""
    rng = np.random.RandomState(seed)
    gts = S.gen_gts(n, seed)
    q = gts.reshape(-1, 4, 2)
    r = np.linalg.norm(q - q.mean(1, keepdims=True), axis=2).max(1)
    half = rng.uniform(2.5, 3.5, (n, 1, 2)) * r[:, None, None]
    p = _rot(GRID[None] * half + rng.normal(0, 0.05, (n, 9, 2)) * r[:, None, None], rng.uniform(-np.pi, np.pi, n))
    return _pack(q.mean(1)[:, None, :] + p + rng.normal(0, 0.2, (n, 1, 2)) * r[:, None, None], gts)


def gen_disjoint(n, seed):
    """Point sets at least 300 px away from their gt."""
    rng = np.random.RandomState(seed)
    gts = S.gen_gts(n, seed)
    ctr = gts.reshape(-1, 4, 2).mean(1)
    th = rng.uniform(-np.pi, np.pi, n)
    far = ctr + (500 + rng.uniform(0, 200, n))[:, None] * np.stack([np.cos(th), np.sin(th)], 1)
    pts, gts = _pack(S.gen_pointsets(n, seed + 2, around=far), gts)
    gap = np.linalg.norm(pts.reshape(-1, 9, 1, 2) - gts.reshape(-1, 1, 4, 2), axis=3).min((1, 2))
    assert gap.min() >= 300
    return pts, gts


def gen_tiny(n, seed):
    """gts of 0.3 - 2 px with point sets of their size, at small coordinates (fine float32 grid)."""
    rng = np.random.RandomState(seed)
    gts = _rects(rng, n, 6.0, 26.0, (0.3, 2.0))
    q = gts.reshape(-1, 4, 2)
    half = rng.uniform(0.15, 1.0, (n, 1, 2))
    p = _rot(GRID[None] * half + rng.normal(0, 0.04, (n, 9, 2)), rng.uniform(-np.pi, np.pi, n))
    return _pack(q.mean(1)[:, None, :] + p + rng.normal(0, 0.3, (n, 1, 2)), gts)


def gen_large(n, seed):
    """The existing generator moved to coordinates around 16 000."""
    pts, gts = gen_existing(n, seed)
    return _pack(pts + 15000.0, gts + 15000.0)


def gen_negative(n, seed):
    """The existing generator moved so that most coordinates are negative."""
    pts, gts = gen_existing(n, seed)
    sh = np.array([-1500.0, -700.0])
    return _pack(pts.reshape(-1, 9, 2) + sh, gts.reshape(-1, 4, 2) + sh)


def gen_orientation(n, seed):
    """gts given clockwise (odd rows) and counter-clockwise (even rows), starting at any of their corners."""
    rng = np.random.RandomState(seed)
    pts, gts = gen_existing(n, seed)
    q = gts.reshape(-1, 4, 2).copy()
    for r in range(n):
        g = np.roll(q[r], rng.randint(4), axis=0)
        ccw = area([tuple(v) for v in g.tolist()]) > 0
        q[r] = g if ccw == (r % 2 == 0) else g[::-1]
    return _pack(pts, q)


def _int_grids(rng, n, lo, hi):
    c = np.round(rng.uniform(lo, hi, (n, 1, 2)))
    step = rng.randint(1, 12, (n, 1, 2)).astype(np.float64)
    return c + GRID[None] * step


def gen_exact_grid(n, seed):
    """Exact integer 3 x 3 grids (every hull edge carries a collinear point, equal x / y everywhere) on rotated gts."""
    rng = np.random.RandomState(seed)
    gts = _rects(rng, n, 60.0, 190.0, (4.0, 40.0))
    ctr = gts.reshape(-1, 4, 2).mean(1)
    p = np.round(ctr)[:, None, :] + np.round(rng.normal(0, 4, (n, 1, 2))) + GRID[None] * rng.randint(1, 12, (n, 1, 2))
    return _pack(p, gts)


def gen_near_tie(n, seed):
    """The exact grids with every coordinate moved by +-1e-7 ... 1e-3 (below and above the kernels' 1E-8 and float32's
    resolution: some ties stay exact, some are broken by one ulp, some by much more)."""
    rng = np.random.RandomState(seed)
    pts, gts = gen_exact_grid(n, seed)
    d = 10.0 ** rng.uniform(-7, -3, (n, 18)) * rng.choice([-1.0, 1.0], (n, 18))
    return _pack(pts + d, gts)


def gen_axis_aligned(n, seed):
    """Integer grids on integer axis-aligned gts: hull vertices on gt edges and corners do occur."""
    rng = np.random.RandomState(seed)
    gts = _rects(rng, n, 60.0, 190.0, (4.0, 24.0), aligned=True, integer=True)
    ctr = gts.reshape(-1, 4, 2).mean(1)
    p = ctr[:, None, :] + np.round(rng.normal(0, 3, (n, 1, 2))) + GRID[None] * rng.randint(1, 10, (n, 1, 2))
    return _pack(p, gts)


def gen_shared_corners(n, seed):
    """The first 4 points are the gt's corners, the other 5 lie inside: GIoU = 1, every hull vertex touches."""
    rng = np.random.RandomState(seed)
    gts = S.gen_gts(n, seed)
    q = gts.reshape(-1, 4, 2)
    u, v = rng.uniform(0.1, 0.9, (n, 5, 1)), rng.uniform(0.1, 0.9, (n, 5, 1))
    inner = q[:, :1] + u * (q[:, 1:2] - q[:, :1]) + v * (q[:, 3:4] - q[:, :1])
    return _pack(np.concatenate([q, inner], axis=1), gts)


def gen_duplicates(n, seed):
    """3 to 9 distinct points, the rest exact copies of them, shuffled: hulls of 3 to 9 vertices at most."""
    rng = np.random.RandomState(seed)
    pts, gts = gen_existing(n, seed)
    p = pts.reshape(-1, 9, 2).copy()
    for r in range(n):
        k = 3 + r % 7
        src = np.concatenate([np.arange(k), rng.randint(0, k, 9 - k)])
        p[r] = p[r, rng.permutation(9)][src][rng.permutation(9)]
    return _pack(p, gts)


def gen_coincident(n, seed):
    """All 9 points are the same point: inside the gt (even rows) or up to 60 px away from its centre (odd rows)."""
    rng = np.random.RandomState(seed)
    gts = S.gen_gts(n, seed)
    q = gts.reshape(-1, 4, 2)
    inside = q[:, 0] + rng.uniform(0.2, 0.8, (n, 1)) * (q[:, 1] - q[:, 0]) + rng.uniform(0.2, 0.8, (n, 1)) * (q[:, 3] - q[:, 0])
    away = q.mean(1) + rng.normal(0, 30, (n, 2))
    c = np.where((np.arange(n) % 2 == 0)[:, None], inside, away)
    return _pack(np.repeat(c[:, None, :], 9, axis=1), gts)


def gen_collinear(n, seed):
    """9 exactly collinear points (integer start, integer direction, integer multiples) across or next to rotated gts."""
    rng = np.random.RandomState(seed)
    gts = _rects(rng, n, 60.0, 190.0, (4.0, 40.0))
    ctr = gts.reshape(-1, 4, 2).mean(1)
    d = rng.randint(-4, 5, (n, 2))
    d[(d == 0).all(1)] = (1, 2)
    t = np.stack([rng.permutation(9) - 4 for _ in range(n)])
    p = np.round(ctr + rng.normal(0, 6, (n, 2)))[:, None, :] + t[:, :, None] * d[:, None, :]
    return _pack(p, gts)


# The `> 1` rule (GIoULossFuction, giou_rows_kernel): a row with any gradient component > 1 gets 1e-6 in all 18.
# d GIoU / d x ~ 1 / size, so the family is gts of 0.1 - 1 px; on top of the random rows, hand-made ones on the
# 0.25 px square gt (0, 0) .. (0.25, 0.25) (area 1/16) with the hull strictly inside it, where GIoU = A / B and
# d / d v = ((y_next - y_prev) / 2, (x_prev - x_next) / 2) / B in exact binary fractions:
#   square of side 1/8        -> every hull component is exactly +-1.0f: must NOT fire
#   the same, 1/64 wider      -> 1.125 in two components: fires
#   triangle, height 7/32     -> one component -1.75, the largest +0.875: must NOT fire
_RULE_ROWS = (
    ("exactly_one", [(0.0625, 0.0625), (0.1875, 0.0625), (0.1875, 0.1875), (0.0625, 0.1875)]),
    ("just_above", [(0.0625, 0.0625), (0.203125, 0.0625), (0.203125, 0.1875), (0.0625, 0.1875)]),
    ("large_negative", [(0.0625, 0.125), (0.15625, 0.015625), (0.15625, 0.234375)]),
)
RULE_HANDMADE = len(_RULE_ROWS)


def gen_rule(n, seed):
    """Rows on which the `> 1` rule fires and rows on which it does not; the first RULE_HANDMADE rows are _RULE_ROWS."""
    rng = np.random.RandomState(seed)
    gts = _rects(rng, n, 6.0, 26.0, (0.1, 1.0))
    q = gts.reshape(-1, 4, 2)
    half = rng.uniform(0.05, 0.4, (n, 1, 2))
    p = _rot(GRID[None] * half + rng.normal(0, 0.02, (n, 9, 2)), rng.uniform(-np.pi, np.pi, n))
    p = q.mean(1)[:, None, :] + p + rng.normal(0, 0.15, (n, 1, 2))
    for r, (_, verts) in enumerate(_RULE_ROWS[:n]):
        sh = np.array([4.0 + r, 9.0])                               # integer shifts keep the binary fractions exact
        inner = [(0.125 - 0.00390625 * k, 0.125 + 0.001953125 * k) for k in range(9 - len(verts))]   # strictly inside each hull
        p[r] = np.array(verts + inner)[np.roll(np.arange(9), r)] + sh
        q[r] = np.array([(0.0, 0.0), (0.25, 0.0), (0.25, 0.25), (0.0, 0.25)]) + sh
    return _pack(p, q)


Family = collections.namedtuple("Family", "gen step generic may_touch tie positive_area")
# step: exact in float32 at the family's coordinates (generate() puts them on the grid of h / 2, quotients() asserts it)
FAMILIES = collections.OrderedDict([
    ("existing",       Family(gen_existing,       2.0 ** -12, True,  False, False, True)),
    ("cluster",        Family(gen_cluster,        2.0 ** -12, True,  False, False, True)),
    ("enclosing",      Family(gen_enclosing,      2.0 ** -12, True,  False, False, True)),
    ("disjoint",       Family(gen_disjoint,       2.0 ** -11, True,  False, False, True)),
    ("tiny_gt",        Family(gen_tiny,           2.0 ** -18, True,  False, False, True)),
    ("large_coords",   Family(gen_large,          2.0 ** -9,  True,  False, False, True)),
    ("negative",       Family(gen_negative,       2.0 ** -12, True,  False, False, True)),
    ("orientation",    Family(gen_orientation,    2.0 ** -12, True,  False, False, True)),
    ("exact_grid",     Family(gen_exact_grid,     2.0 ** -15, False, False, True,  True)),
    ("near_tie",       Family(gen_near_tie,       2.0 ** -15, False, False, True,  True)),
    ("axis_aligned",   Family(gen_axis_aligned,   2.0 ** -15, False, True,  False, True)),
    ("shared_corners", Family(gen_shared_corners, 2.0 ** -12, False, True,  False, True)),
    ("duplicates",     Family(gen_duplicates,     2.0 ** -12, False, False, False, True)),
    ("coincident",     Family(gen_coincident,     2.0 ** -12, False, False, False, False)),
    ("collinear",      Family(gen_collinear,      2.0 ** -15, False, False, False, False)),
    ("rule",           Family(gen_rule,           2.0 ** -18, False, False, False, True)),
])

SAMPLE_ROWS = 300                  # rows per family that get the float64 quotients (about 4 s per family)


def family_seed(name):
    return 1000 + 17 * list(FAMILIES).index(name)


def generate(name, n, seed=None):
    """(pts [n,18], gts [n,8]) float32 of family `name`; all values finite.  Every coordinate is a multiple of half the
    family's step (and far below 2^24 of them), so that x +- h and x +- h / 2 are float32 numbers too."""
    pts, gts = FAMILIES[name].gen(n, family_seed(name) if seed is None else seed)
    q = FAMILIES[name].step / 2
    pts, gts = np.round(pts / q) * q, np.round(gts / q) * q
    assert max(np.abs(pts).max(), np.abs(gts).max()) + 2 * q < 2.0 ** 24 * q
    pts, gts = np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(gts, np.float32)
    assert pts.shape == (n, 18) and gts.shape == (n, 8) and np.isfinite(pts).all() and np.isfinite(gts).all()
    return pts, gts


@functools.lru_cache(maxsize=None)
def sample(name):
    """(pts, gts, Quotients) of the family's SAMPLE_ROWS-row sample (computed once per process)."""
    pts, gts = generate(name, SAMPLE_ROWS)
    return pts, gts, quotients(pts, gts, FAMILIES[name].step)


def class_caps(name, q):
    """The conditions the issue puts on the classifier's output, as a list of violated ones (empty = fine)."""
    fam = FAMILIES[name]
    n = q.cls.size
    smooth, touching = int((q.cls == SMOOTH).sum()), int((q.cls == TOUCHING).sum())
    bad = []
    if fam.generic and smooth < 0.8 * n:
        bad.append("%s: only %d of %d rows are smooth (generic families: at least 80 %%)" % (name, smooth, n))
    if not fam.may_touch and touching:
        bad.append("%s: %d touching rows (allowed in the axis-aligned and shared-corner families only)" % (name, touching))
    if name != "coincident" and (q.cls == POINT).any():
        bad.append("%s: %d rows whose 9 points all coincide" % (name, int((q.cls == POINT).sum())))
    return bad
