"""CPU: the premises under which tests/test_gpu_dcn_bwd_exact.py may compare the MFMA DeformConv backward BIT FOR BIT with a
float64 reference, the conventions of that reference at the sampler's border classes, and the conditions that keep the
comparison from passing vacuously -- on the generated data of every case of tests/dcn_bwd_cases.py.  No GPU, no kernel.

Premise: for every gradient the sum of the ABSOLUTE values of the terms of any output element (per corner, and for grad_offset /
grad_mask without the bilinear factors, so the kernels' intermediate channel sums are covered too) stays below 2^24 units (1/8 for
grad_input / grad_weight under modulation, 1/4 otherwise).  Every partial sum is then an fp32 number in any order.  Measured with
|grad_out| <= 3, |w| <= 7, |x| <= 15: the tightest is grad_offset / grad_mask of the DCNv2 cases at 2^22.7 of these (conservative)
units (test_premises_and_expected_gradients prints every figure); |grad_out| <= 7 would leave less than one bit.

The reference (dcn_bwd_cases.reference_backward) is held from two sides on three small cases (borders, stride 2, DCNv2): it
EQUALS torch.autograd.grad through dcn_half_cases.reference_level in float64, and it EQUALS the CPU oracle's column formulation
(oracle.dcn_backward / dcn_v2_backward, fp32 column kernels) -- exactly, not to 1e-6: on this data the oracle's fp32 arithmetic
does not round either."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_half_cases as D  # noqa: E402
import dcn_bwd_cases as B  # noqa: E402

GRADS = ("grad_input", "grad_offset", "grad_weight", "grad_mask")


def _flat(want, name):
    v = want[name]
    if v is None:
        return None
    return torch.cat([t.reshape(-1) for t in (v if isinstance(v, list) else [v])])


@pytest.mark.parametrize("case", B.ALL_CASES, ids=lambda c: c.name)
def test_premises_and_expected_gradients(case):
    """Every bound of premise_bounds is below 2^24 units, every expected gradient is an fp32 number and a multiple of its unit,
    and grad_input, grad_offset and grad_weight are non-zero -- or all zero, in the cases built for that."""
    data, gos, want = B.expected(case, "cpu")
    assert all(float(g.abs().max()) <= B.META[case.name].go_max and torch.equal(g, torch.round(g)) for g in gos)
    bounds = B.premise_bounds(case, data, gos)
    print(case.name, " ".join("%s 2^%.1f" % (k, np.log2(max(v, 1.0))) for k, (v, _) in bounds.items()))
    for k, (v, unit) in bounds.items():
        assert v < 2.0 ** 24, "%s: a partial sum of %s may reach %.0f units of %g (2^%.2f)" % (case.name, k, v, unit, np.log2(v))
    for name in GRADS:
        v = _flat(want, name)
        assert (v is None) == (name == "grad_mask" and not case.mask)
        if v is None:
            continue
        assert torch.equal(v.float().double(), v), "%s: an expected %s is not an fp32 number" % (case.name, name)
        q = v / bounds[name][1]
        assert torch.equal(q, torch.round(q)), "%s: an expected %s is not a multiple of its unit" % (case.name, name)
        if case.name in B.ZERO_CASES:
            assert not v.any(), "%s: %s should be all zero" % (case.name, name)
        elif name != "grad_mask":
            assert bool(v.any()), "%s: %s is all zero" % (case.name, name)


def _autograd(case, data, gos):
    xs = [x.clone().requires_grad_(True) for x in data["xs"]]
    offs = [o.clone().requires_grad_(True) for o in data["offs"]]
    masks = [m.clone().requires_grad_(True) for m in data["masks"]] if case.mask else None
    w = data["weight"].clone().requires_grad_(True)
    loss = 0.0
    for i in range(len(case.levels)):
        out = D.reference_level(case, xs[i], offs[i], masks[i] if case.mask else None, w, None)
        loss = loss + (out * gos[i]).sum()
    leaves = xs + offs + [w] + (masks if case.mask else [])
    g = torch.autograd.grad(loss, leaves)
    n = len(xs)
    return dict(grad_input=list(g[:n]), grad_offset=list(g[n:2 * n]), grad_weight=g[2 * n],
                grad_mask=list(g[2 * n + 1:]) if case.mask else None)


CROSS_CASES = ("bord_9x11_v1", "geo_3x3_s2", "bord_9x11_v2")


@pytest.mark.parametrize("name", CROSS_CASES)
def test_reference_equals_autograd_and_the_oracle(name, oracle):
    """reference_backward against float64 autograd through the forward helper (equality) and against the CPU oracle's column
    formulation (equality too: its fp32 column kernels do not round on this data).  Pins the conventions at the border classes:
    zero at or beyond -1 / H / W, per-corner predicates, the right-sided slope at integer coordinates."""
    case = B.BY_NAME[name]
    data, gos, want = B.expected(case, "cpu")
    auto = _autograd(case, data, gos)
    for k in GRADS:
        if want[k] is None:
            continue
        assert torch.equal(_flat(auto, k), _flat(want, k)), "%s: %s differs from autograd at %d elements" % (
            name, k, int((_flat(auto, k) != _flat(want, k)).sum()))
    gw = np.zeros(tuple(data["weight"].shape))
    for i in range(len(case.levels)):
        x, off, go = (t.numpy() for t in (data["xs"][i], data["offs"][i], gos[i]))
        if case.mask:
            o = oracle.dcn_v2_backward(x, off, data["masks"][i].numpy(), data["weight"].numpy(), go, case.stride, case.pad, case.dil)
            pairs = (("grad_input", o[0]), ("grad_offset", o[1]), ("grad_mask", o[2]))
            gw += o[3].astype(np.float64)
        else:
            o = oracle.dcn_backward(x, off, data["weight"].numpy(), go, case.stride, case.pad, case.dil)
            pairs = (("grad_input", o[0]), ("grad_offset", o[1]))
            gw += o[2].astype(np.float64)
        for k, got in pairs:
            assert np.array_equal(got.astype(np.float64), want[k][i].numpy()), "%s level %d: the oracle's %s differs at %d elements" % (
                name, i, k, int((got.astype(np.float64) != want[k][i].numpy()).sum()))
    assert np.array_equal(gw, want["grad_weight"].numpy())


def test_a_flipped_corner_predicate_is_caught(monkeypatch):
    """The cross-check is not decoration: with `high <= N - 1` turned into `high < N - 1` in the coordinate derivative the
    reference no longer equals autograd on a borders case."""
    case = B.BY_NAME["bord_9x11_v1"]
    data, gos, _ = B.expected(case, "cpu")

    def flipped(case, h, w, H, W):
        valid = (h > -1) & (w > -1) & (h < H) & (w < W)
        h0, w0 = torch.floor(h), torch.floor(w)
        t_ok, b_ok, l_ok, r_ok = h0 >= 0, h0 + 1 < H - 1, w0 >= 0, w0 + 1 < W - 1
        return valid, torch.stack([valid & t_ok & l_ok, valid & t_ok & r_ok, valid & b_ok & l_ok, valid & b_ok & r_ok], 1)
    monkeypatch.setattr(B, "corner_predicates", flipped)
    wrong = B.reference_backward(case, data, gos)
    auto = _autograd(case, data, gos)
    assert torch.equal(_flat(auto, "grad_input"), _flat(wrong, "grad_input"))          # (the scatter does not use the predicates)
    assert int((_flat(auto, "grad_offset") != _flat(wrong, "grad_offset")).sum()) >= 20


@pytest.mark.parametrize("case", B.BORDER_CASES, ids=lambda c: c.name)
def test_border_cases_reach_every_sample_class(case):
    """Every class of SAMPLE_CLASSES holds at least 20 samples on rows with a non-zero grad_out (here: every row is non-zero)."""
    data, gos, _ = B.expected(case, "cpu")
    for go in gos:
        assert bool((B._rows(go) != 0).any(dim=1).all()), "a grad_out row of a borders case is zero"
    counts, total = D.sample_class_counts(case, data)
    for k in D.SAMPLE_CLASSES:
        assert counts[k] >= 20, "%s: sampling class %r holds %d of %d samples" % (case.name, k, counts[k], total)


def test_region_cases_reach_the_list_structure():
    """Over the regions family the per-region list lengths contain 0, a value in 1..15, exactly 64, exactly 65, a value above
    1024 and a value that is no multiple of 16; the map sizes and region counts are the ones the family claims."""
    lengths = {}
    for case in B.REGION_CASES:
        data, gos, _ = B.expected(case, "cpu")
        lengths[case.name] = torch.cat([t.reshape(-1) for t in B.region_list_lengths(case, data, gos)]).tolist()
    every = [n for v in lengths.values() for n in v]
    assert 0 in every and 64 in every and 65 in every
    assert any(1 <= n <= 15 for n in every) and any(n > 1024 for n in every) and any(n % 16 for n in every)
    assert lengths["reg_one_64"] == [64] and sorted(lengths["reg_one_65"]) == [0, 65]
    assert sorted(lengths["reg_pileup"]) == [0] * 8 + [19 * 21 * 9]
    assert not any(lengths["reg_outside"])
    assert {c.levels for c in B.REGION_CASES if len(c.levels) == 1} >= {((1, 1),), ((7, 9),), ((8, 8),), ((9, 8),), ((16, 17),), ((19, 21),)}
    nreg = {c.name: len(lengths[c.name]) for c in B.REGION_CASES}
    assert 1 in nreg.values() and {2, 6, 18, 42} <= set(nreg.values())
    # the same rule on the geometry that existing tests use: lists in a dense 3 x 3 call hold roughly 9 entries per pixel
    assert all(n > 0 for n in lengths["reg_19x21"])


def test_chunk_cases_reach_the_chunk_structure():
    """Level sizes of 1, 31, 32, 33 and 65 positions, a chunk across two images, eight levels, and 1, 7, 8, 9 and 17 active
    chunks (the active list is cut into 8 slabs of (n + 7) >> 3)."""
    sizes = B.BY_NAME["chunk_sizes"]
    assert [n for _, _, n in B.level_chunks(sizes)] == [1, 31, 32, 33, 65]
    st = B.BY_NAME["chunk_straddle"]
    assert st.batch == 3 and D.positions(st) == 75 and B.straddling_chunks(st) == [0, 1]
    assert len(B.BY_NAME["chunk_8levels"].levels) == 8
    counts = {}
    for case in B.CHUNK_CASES:
        _, gos, _ = B.expected(case, "cpu")
        act = B.active_chunks(case, gos)
        assert act == sorted(set(act))
        counts[case.name] = len(act)
    assert [counts["active_%d" % n] for n in (1, 7, 8, 9, 17)] == [1, 7, 8, 9, 17]
    total = sum(n for _, n, _ in B.level_chunks(B.BY_NAME["active_17"]))
    assert total == 17 and B.straddling_chunks(B.BY_NAME["active_9"])
    for n in (7, 8, 9):                                                  # the first and the last (partial) chunk take part
        _, gos, _ = B.expected(B.BY_NAME["active_%d" % n], "cpu")
        act = B.active_chunks(B.BY_NAME["active_%d" % n], gos)
        assert act[0] == 0 and act[-1] == total - 1


def test_sparsity_patterns_are_what_they_claim():
    by = {B.META[c.name].pattern: c for c in B.SPARSITY_CASES}
    assert set(by) == {"dense", "rows", "level_zero", "image_zero", "channel_edge", "zero"}
    g = {p: B.expected(c, "cpu")[1] for p, c in by.items()}
    assert all(1 <= int((B._rows(t) != 0).any(1).sum()) <= 3 for t in g["rows"])
    assert not g["level_zero"][1].any() and g["level_zero"][0].any() and g["level_zero"][2].any()
    assert all(not t[0].any() and t[1].any() for t in g["image_zero"])
    assert not any(t.any() for t in g["zero"])
    for t in g["channel_edge"]:
        r = B._rows(t)
        assert int((r != 0).sum(1).max()) == 1 and not r[:, 1:255].any() and r[:, 0].any() and r[:, 255].any()
    total = sum(n for _, n, _ in B.level_chunks(by["rows"]))
    assert len(B.active_chunks(by["rows"], g["rows"])) < total           # inactive chunks exist: their grad_offset rows are zeros


def test_geometry_and_subset_lists():
    geo = {(c.kh, c.kw, c.stride, c.pad, c.dil) for c in B.GEOMETRY_CASES}
    assert geo == {(3, 3, 2, 1, 1), (3, 3, 1, 2, 2), (3, 3, 1, 0, 1), (1, 1, 1, 0, 1), (1, 3, 1, 0, 1), (3, 1, 1, 0, 1), (2, 2, 1, 0, 1)}
    assert all(len(c.levels) == 2 and c.batch == 2 for c in B.GEOMETRY_CASES)
    assert not B.BY_NAME["geo_1x1"].mask                                 # DCNv1 with one tap: the exact-fp32 weight kernel
    assert all(n in B.BY_NAME for n in B.SUBSET)
    assert all(max(max(l) for l in c.levels) <= 40 for c in B.ALL_CASES)
    for case in B.HALF_CASES:                                            # finite in fp16, with room
        _, _, want = B.expected(case, "cpu")
        for k in GRADS:
            if want[k] is not None:
                assert float(_flat(want, k).abs().max()) < 65504 / 2, (case.name, k)
