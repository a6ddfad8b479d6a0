"""CPU: the oracle's convex GIoU (oracle/orp_oracle3.c: values in the reference's operation order, gradient restated in
reverse mode) against the MATH -- a float64 GIoU written from the definition and its difference quotients
(tests/giou_float64.py) -- on every input family of that module: the generator the suite used so far, tight clusters, hulls
that enclose their gt, disjoint pairs, tiny gts, large and negative coordinates, both orientations, exact and nearly exact
ties, hull vertices on the gt's edges and corners, duplicated, coincident and collinear points, and rows on which the
`> 1` rule fires.

Per family (300 rows):
  * every output is finite;
  * the value equals the float64 GIoU to one float ulp at 1 (2^-23);
  * smooth rows: every gradient component equals the central quotient to the quotient's own noise,
    max(1e-6 x row scale, 10 x |central(h) - central(h / 2)|), both terms of the float64 function alone;
  * smooth and kink rows: every component lies between the backward and the forward quotient (slack 1e-4 x row scale);
  * touching rows (a hull vertex within 1e-8 of a gt vertex or edge) are exempt from both gradient checks and counted: the
    reference treats a vertex "equal" to another and a crossing at a vertex by rules of its own (1E-8 sign thresholds,
    dropped crossings), its gradient there is a convention that only tests/test_oracle_vs_ref.py can hold;
  * rows whose 9 points all coincide get exactly 0 in all 18 components (the reference's convention for a hull that is no
    polygon); exact copies of a point are moved together (giou_float64's docstring says why);
  * rows the oracle flags (the reference's scratch arrays would overflow) get NO exemption -- the restatement has no such
    limit -- and are counted;
  * the classes fulfil the caps: >= 80 % smooth and no touching row in the generic families, touching rows in the
    axis-aligned and shared-corner families only.
The measured maxima go into the run's report."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest  # noqa: E402
import giou_float64 as G  # noqa: E402


@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_oracle_gradient_is_the_derivative_of_the_float64_giou(oracle, family):
    pts, gts, q = G.sample(family)
    out, flags = oracle.convex_giou(pts, gts, return_flags=True)
    m, fails = G.check_against_math(out, q)
    conftest.REPORT.append(
        "giou math, oracle, %-14s smooth/kink/touching/point %s  flagged %d  value %.2g  smooth |g - central| / scale %.2g  "
        "outside bracket / scale %.2g" % (family, "/".join(str(c) for c in m["counts"]), int(flags.sum()), m["value"],
                                          m["smooth_rel"], m["bracket_rel"]))
    assert not G.class_caps(family, q), G.class_caps(family, q)
    assert not fails, "%s: %s" % (family, "; ".join(fails))
    if G.FAMILIES[family].tie:
        assert m["counts"][0] + m["counts"][1] == q.cls.size          # every row got the bracket check


def test_float64_giou_on_hand_computed_cases():
    """The float64 function itself on cases computed by hand: a unit square against itself (1), against its right half
    shifted (I = 1/2, U = 3/2, C = 3/2 -> 1/3), against a disjoint unit square two to the right (I = 0, U = 2, C = 3 ->
    -1/3), and a single point at a corner of the gt's hull-to-be (I = 0, U = 1, C = 1 -> 0)."""
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
    nine = lambda quad, fill: quad + [fill] * 5                                                  # noqa: E731
    assert G.giou_one(nine(sq, (0.5, 0.5)), sq, 1.0) == (1.0, 1.0)
    half = [(x + 0.5, y) for x, y in sq]
    assert abs(G.giou_one(nine(half, (1.0, 0.5)), sq, 1.0)[0] - 1.0 / 3) < 1e-15
    far = [(x + 2.0, y) for x, y in sq]
    assert abs(G.giou_one(nine(far, (2.5, 0.5)), sq, 1.0)[0] + 1.0 / 3) < 1e-15
    assert G.giou_one([(0.25, 0.25)] * 9, sq, 1.0) == (0.0, 0.0)
    assert G.giou_one(nine(sq, (0.5, 0.5)), sq[::-1][::-1], 1.0)[1] == 1.0
    # the classifier: a hull vertex on a gt corner / edge touches, one 1e-6 away does not
    assert G._touching(nine(sq, (0.5, 0.5)), sq)
    assert G._touching([(0.5, 0.0), (0.7, 0.3), (0.3, 0.3)] * 3, sq)
    assert not G._touching([(0.5, 1e-6), (0.7, 0.3), (0.3, 0.3)] * 3, sq)


def test_rule_family_fires_and_does_not_fire(oracle):
    """What the GPU test of the `> 1` rule relies on, checked with the oracle: at the GPU test's size the family has at
    least 10 rows with a component > 1 and at least 10 without, a row whose largest component is exactly 1.0f and a row
    with a component below -1 and none above 1."""
    import numpy as np
    pts, gts = G.generate("rule", 2000)
    g = oracle.convex_giou(pts, gts)[:, :18]
    fire = (g > 1).any(1)
    assert fire.sum() >= 10 and (~fire).sum() >= 10
    names = [n for n, _ in G._RULE_ROWS]
    one, above, neg = (g[names.index(n)] for n in ("exactly_one", "just_above", "large_negative"))
    assert one.max() == np.float32(1.0) and not fire[names.index("exactly_one")]
    assert above.max() == np.float32(1.125) and fire[names.index("just_above")]
    assert neg.min() == np.float32(-1.75) and neg.max() == np.float32(0.875) and not fire[names.index("large_negative")]
