"""GPU: csrc/orp_convex_giou.hip (the gradient of both regression losses) held to the oracle row by row on every input
family of tests/giou_float64.py, to the float64 math directly, and to itself bit for bit; convex_iou's diagonal against the
float64 I / U; the `> 1` rule of GIoULoss / _SegmentGIoULoss on rows where it fires.

Bars
  kernel vs oracle, gradient   |d| <= 2^-22 x the row's largest oracle component.  Derived: kernel and oracle evaluate the
                               same fp64 expressions (contraction is off on both sides) and round once to float, so two
                               results differ by at most one float ulp of the larger, 2^-23 relative, i.e. 2^-22 of the
                               row's largest component at the most.  Measured (MI355X, 20 000 rows per family): 0 in all
                               16 families -- every component bit-equal.
  kernel vs oracle, value      <= 1 float ulp of the oracle's value (floor 2^-50: the fp64 values carry ~1e-16 absolute,
                               a GIoU below 1e-8 has a smaller ulp than that).  Measured: 0, bit-equal.
  kernel vs float64            the bars of tests/test_giou_gradient_math.py, taken from the float64 function alone; they
                               are NOT re-derived from the kernel's output.
  convex_iou vs float64 I / U  2^-23: an IoU is in [0, 1], fp64 internals rounded once to float (2^-25 .. 2^-24) plus
                               the 1E-8 sign thresholds of the clip.
TOUCHING rows (a hull vertex on a gt vertex or edge) and POINT rows (all 9 points coincide) follow conventions of the
reference, not the derivative (giou_float64's docstring): the kernel is held to the oracle on them like on any other row,
and the oracle to the reference in tests/test_oracle_vs_ref.py."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest  # noqa: E402
import giou_float64 as G  # noqa: E402

ROWS = 20000                      # per family, kernel vs oracle


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()            # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _kernel(pts, gts, dev):
    """[n,19] float32 straight out of orp_convex_giou."""
    from orientedreppoints_amd.mmdet_ops.iou_wrapper import convex_giou_cuda
    out = convex_giou_cuda.convex_giou(_t(pts, dev), _t(gts, dev))
    return out.reshape(-1, 19).cpu().numpy()


@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_kernel_equals_the_oracle_row_by_row(dev, oracle, family):
    pts, gts = G.generate(family, ROWS)
    want, flags = oracle.convex_giou(pts, gts, return_flags=True)
    got = _kernel(pts, gts, dev)
    assert got.shape == want.shape == (ROWS, 19)
    assert np.isfinite(want).all(), "the oracle itself is not finite on %s" % family
    finite = np.isfinite(got).all(1)
    scale = np.abs(want[:, :18]).max(1).astype(np.float64)
    dg = np.abs(got[:, :18].astype(np.float64) - want[:, :18]).max(1)
    dv = np.abs(got[:, 18].astype(np.float64) - want[:, 18])
    ulp = np.maximum(np.spacing(np.abs(want[:, 18])).astype(np.float64), 2.0 ** -50)
    rel = dg[finite & (scale > 0)] / scale[finite & (scale > 0)]
    bits = (got.view(np.uint32) != want.view(np.uint32)).any(1)
    conftest.REPORT.append("giou kernel vs oracle, %-14s %d rows: gradient |d| / row scale %.3g (bar 2^-22 = %.3g), value %.3g ulp, "
                           "%d rows not bit-equal, %d flagged, largest component %.3g"
                           % (family, ROWS, rel.max() if rel.size else 0.0, 2.0 ** -22, float(np.nanmax(dv / ulp)), int(bits.sum()),
                              int(flags.sum()), float(scale.max())))
    assert finite.all(), "%s: %d rows with a non-finite output, first %d" % (family, (~finite).sum(), np.nonzero(~finite)[0][0])
    bad = np.nonzero(~(dg <= 2.0 ** -22 * scale))[0]
    assert bad.size == 0, "%s: %d rows off the oracle's gradient, worst row %d: |d| = %.3g at row scale %.3g" % (
        family, bad.size, bad[np.argmax(dg[bad])], dg[bad].max(), scale[bad[np.argmax(dg[bad])]])
    bad = np.nonzero(~(dv <= ulp))[0]
    assert bad.size == 0, "%s: %d rows off the oracle's value, worst %.3g" % (family, bad.size, dv[bad].max())


@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_kernel_gradient_is_the_derivative_of_the_float64_giou(dev, family):
    """The checks of tests/test_giou_gradient_math.py on the kernel's own output: an error that kernel and oracle share
    is still caught."""
    pts, gts, q = G.sample(family)
    m, fails = G.check_against_math(_kernel(pts, gts, dev), q)
    conftest.REPORT.append(
        "giou math, kernel, %-14s smooth/kink/touching/point %s  value %.2g  smooth |g - central| / scale %.2g  outside bracket / "
        "scale %.2g" % (family, "/".join(str(c) for c in m["counts"]), m["value"], m["smooth_rel"], m["bracket_rel"]))
    assert not G.class_caps(family, q), G.class_caps(family, q)
    assert not fails, "%s: %s" % (family, "; ".join(fails))


def _mixed(rows_per_family=200):
    parts = [G.generate(name, rows_per_family) for name in G.FAMILIES]
    return np.concatenate([p for p, _ in parts]), np.concatenate([g for _, g in parts])


def test_results_do_not_depend_on_the_batch_the_order_or_the_stream(dev):
    """Bit for bit: the same call twice; rows permuted; a row alone; the first 63 / 64 / 65 rows (the wave size and its
    neighbours); a non-default stream."""
    from orientedreppoints_amd.mmdet_ops.iou_wrapper import convex_giou_cuda
    pts, gts = _mixed()
    n = pts.shape[0]
    tp, tg = _t(pts, dev), _t(gts, dev)
    run = lambda a, b: convex_giou_cuda.convex_giou(a, b).reshape(-1, 19)                        # noqa: E731
    base = run(tp, tg)
    eq = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))                      # noqa: E731
    assert torch.isfinite(base).all()
    assert eq(run(tp, tg), base)
    perm = torch.from_numpy(np.random.RandomState(0).permutation(n)).to(dev)
    assert eq(run(tp[perm].contiguous(), tg[perm].contiguous()), base[perm])
    for k in (63, 64, 65):
        assert eq(run(tp[:k].contiguous(), tg[:k].contiguous()), base[:k]), k
    for r in range(0, n, n // 48):                                        # 3 rows of every family, each alone
        assert eq(run(tp[r:r + 1].contiguous(), tg[r:r + 1].contiguous()), base[r:r + 1]), r
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = run(tp, tg)
    side.synchronize()
    assert eq(other, base)


def test_convex_iou_diagonal_is_the_float64_iou(dev):
    """convex_iou(points, gts)[i, i] against I / U of the float64 reference, on the families whose hull and gt both have
    positive area."""
    from orientedreppoints_amd.mmdet_ops import convex_iou
    for name, fam in G.FAMILIES.items():
        if not fam.positive_area:
            continue
        pts, gts, q = G.sample(name)
        got = convex_iou(_t(pts, dev), _t(gts, dev)).diagonal().cpu().numpy().astype(np.float64)
        d = np.abs(got - q.iou)
        conftest.REPORT.append("convex_iou diagonal vs float64 I / U, %-14s largest |d| %.3g (bar %.3g)" % (name, np.nanmax(d), G.VALUE_BAR))
        assert np.isfinite(got).all(), name
        assert (d <= G.VALUE_BAR).all(), (name, float(d.max()), int(np.argmax(d)))


def _rule_rows(oracle, n=2000):
    pts, gts = G.generate("rule", n)
    want = oracle.convex_giou(pts, gts)
    names = [k for k, _ in G._RULE_ROWS]
    assert want[names.index("exactly_one"), :18].max() == np.float32(1.0)          # exactly 1.0f: must not fire
    neg = want[names.index("large_negative"), :18]
    assert neg.min() < -1.5 and neg.max() <= 1.0                                     # large negative component: must not fire
    return pts, gts, want


def _assert_rule_counts(fire, near):
    assert fire.sum() >= 10, "the `> 1` rule fires on %d rows only" % fire.sum()
    assert (~fire).sum() >= 10, "the `> 1` rule leaves %d rows only" % (~fire).sum()
    # apart from the hand-made row at exactly 1.0f no row sits within rounding of the threshold (one float rounding of
    # difference between kernel and oracle cannot change which rows fire)
    assert not near[G.RULE_HANDMADE:].any()


def test_rule_fires_in_giou_loss_module(dev, oracle):
    """GIoULoss on the rule-firing family.  Expected gradient from the oracle's rows as test_giou_loss_module builds it --
    weight first, then `any component > 1 -> 1e-6 in all 18`, then -g / P x loss_weight, all in float -- with the rule
    active.  Bar per row: 1e-6 x the row's largest expected component (2^-22 kernel vs oracle + four float roundings: the
    weight, the division by P -- a multiplication by a rounded 1 / P on the device --, loss_weight)."""
    from orientedreppoints_amd.mmdet_models.losses import GIoULoss
    pts, gts, want = _rule_rows(oracle)
    P = pts.shape[0]
    wn = np.tile(np.array([1.0, 0.5, 2.0, 0.0], np.float32), P // 4 + 1)[:P]
    wn[:G.RULE_HANDMADE] = 1.0
    gref = want[:, :18] * wn[:, None]
    fire = (gref > 1).any(1)
    _assert_rule_counts(fire, np.abs(np.abs(gref).max(1) - 1) < 1e-5)
    assert not fire[0] and fire[1] and not fire[2]                      # exactly 1.0f / 1.125 / -1.75 with +0.875
    gref[fire] = np.float32(1e-6)
    gref = -gref / np.float32(P) * np.float32(0.375)
    pred = _t(pts, dev).requires_grad_(True)
    loss = GIoULoss(loss_weight=0.375)(pred, _t(gts, dev), _t(wn, dev))
    loss.backward()
    assert abs(float(loss.detach()) - 0.375 * np.mean((1 - want[:, 18].astype(np.float64)) * wn)) <= 1e-6
    got = pred.grad.cpu().numpy()
    d = np.abs(got.astype(np.float64) - gref).max(1)
    conftest.REPORT.append("`> 1` rule, GIoULoss: fires on %d of %d rows; largest |d| / row scale %.3g"
                           % (fire.sum(), P, np.max(d[wn > 0] / np.abs(gref[wn > 0]).max(1))))
    assert (d <= 1e-6 * np.abs(gref).max(1)).all(), (int(np.argmax(d)), float(d.max()))
    assert (got[fire] == got[fire][:, :1]).all()                                # fired rows: one constant in all 18


def test_rule_fires_in_segment_giou_loss(dev, oracle):
    """train_ops._SegmentGIoULoss (giou_rows_kernel) on the rule-firing family: the rule looks at the kernel's own
    components (weights are 0 / 1 there), the row is then ((-g) x (w / max(denom[seg], 1))) x loss_weight in float."""
    from orientedreppoints_amd.mmdet_ops import train_ops
    pts, gts, want = _rule_rows(oracle)
    P, nseg = pts.shape[0], 3
    rng = np.random.RandomState(3)
    wn = (rng.rand(P) > 0.2).astype(np.float32)
    wn[:G.RULE_HANDMADE] = 1.0
    seg = rng.randint(0, nseg, P)
    denom = np.array([0.5, 40.0, 700.0], np.float32)
    g = want[:, :18].copy()
    fire = (g > 1).any(1)
    _assert_rule_counts(fire & (wn > 0), np.abs(np.abs(g).max(1) - 1) < 1e-5)
    assert not fire[0] and fire[1] and not fire[2]
    g[fire] = np.float32(1e-6)
    t = wn / np.maximum(denom[seg], np.float32(1.0))
    for lw in (0.375, 1.0):
        gref = ((-g) * t[:, None]) * np.float32(lw)
        pred = _t(pts, dev).requires_grad_(True)
        loss = train_ops._SegmentGIoULoss.apply(pred, _t(gts, dev), _t(wn, dev), _t(seg, dev), nseg, _t(denom, dev), lw)
        loss.sum().backward()
        for s in range(nseg):
            ref = lw * np.sum(((1 - want[:, 18].astype(np.float64)) * wn)[seg == s]) / max(float(denom[s]), 1.0)
            assert abs(float(loss[s]) - ref) <= 1e-5 * max(1.0, abs(ref)), (s, float(loss[s]), ref)
        got = pred.grad.cpu().numpy()
        d = np.abs(got.astype(np.float64) - gref).max(1)
        conftest.REPORT.append("`> 1` rule, _SegmentGIoULoss (loss_weight %g): fires on %d of %d weighted rows; largest |d| / row scale %.3g"
                               % (lw, (fire & (wn > 0)).sum(), int((wn > 0).sum()), np.max(d[wn > 0] / np.abs(gref[wn > 0]).max(1))))
        assert (d <= 1e-6 * np.abs(gref).max(1)).all(), (lw, int(np.argmax(d)), float(d.max()))
        assert np.array_equal(got[fire], gref[fire])
