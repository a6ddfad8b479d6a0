"""CPU: the premises under which tests/test_gpu_dcn_half.py may compare the fp16 / bf16 DeformConv forward BIT FOR BIT with a
float64 reference, and the conditions that keep such a comparison from passing vacuously -- asserted on the generated data of
every case (tests/dcn_half_cases.py) with the float64 helper and the CPU oracle's im2col.  No GPU, no kernel.

Premises (T = fp16 and bf16; unit = 2^x_exp / 8):
  1. every modulated bilinear weight is exact in fp16; every product weight x neighbour is a multiple of the unit and the four
     |products| of a sample add up to less than 256 units, so every partial product and every partial sum of the combine, in any
     association order, has at most 8 significand bits: exact in both types (the fp16 kernel combines in packed half arithmetic,
     the bf16 kernel in fp32).  The sample itself round-trips through T, and equals the oracle's column entry;
  2. every operand and sample is a NORMAL fp16 number or zero (the range cases scale x by 2^-8 and the weight by 2^-4);
  3. every term of the contraction is a multiple of unit x 2^w_exp, and sum |sample| |weight| + |bias| < 2^24 of those: every
     partial sum, in any order, is exact in fp32.
So the only rounding of the operator is the final conversion to T."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_half_cases as D  # noqa: E402

FP16_MIN_NORMAL = 2.0 ** -14
FP16_MAX = 65504.0


def _is_multiple(v, unit):
    q = v / unit
    return bool((q == torch.round(q)).all())


def check_premises(case, data, oracle):
    """Raises AssertionError if the case's data breaks a premise.  Returns the float64 outputs (all levels, flattened)."""
    unit = 2.0 ** case.x_exp / 8
    unit_out = unit * 2.0 ** case.w_exp
    taps = case.kh * case.kw
    w = data["weight"]
    assert _is_multiple(w, 2.0 ** case.w_exp)
    if case.bias:
        assert _is_multiple(data["bias"], unit_out)
    outs = []
    for i, (x, off) in enumerate(zip(data["xs"], data["offs"])):
        mask = data["masks"][i] if case.mask else None
        table = x.permute(0, 2, 3, 1).reshape(-1, case.cin)
        if case.mask:
            ocol = oracle.dcn_v2_im2col(x.numpy(), off.numpy(), mask.numpy(), case.kh, case.kw, case.pad, case.stride, case.dil)
        else:
            ocol = oracle.dcn_im2col(x.numpy(), off.numpy(), case.kh, case.kw, case.pad, case.stride, case.dil)
        ocol = torch.from_numpy(ocol).reshape(case.cin, taps, -1)                     # [C, tap, B * Ho * Wo]
        bound = torch.zeros((ocol.shape[2], case.cout), dtype=torch.float64)
        out = torch.zeros_like(bound)
        for tap in range(taps):
            idx, wgt, _, _ = D.tap_samples(case, x, off, mask, tap)
            assert D.representable(wgt, torch.float16).all(), "premise 1: a modulated bilinear weight is not exact in fp16"
            assert ((wgt == 0) | (wgt.abs() >= FP16_MIN_NORMAL)).all()
            spread = torch.zeros((idx.shape[0], case.cin), dtype=torch.float64)
            for k in range(4):
                term = wgt[:, k, None] * table[idx[:, k]]
                assert _is_multiple(term, unit), "premise 1: a weighted neighbour is not a multiple of the unit"
                assert ((term == 0) | (term.abs() >= FP16_MIN_NORMAL)).all(), "premise 2: a subnormal fp16 partial product"
                spread += term.abs()
            assert float(spread.max()) < 256 * unit, "premise 1: a partial sum of the combine may need more than 8 bits"
            col = D.tap_columns(x, idx, wgt)
            for dt in (torch.float16, torch.bfloat16):
                assert D.representable(col, dt).all(), "premise 1: a sample does not round-trip through %s" % dt
            assert ((col == 0) | (col.abs() >= FP16_MIN_NORMAL)).all(), "premise 2: a subnormal fp16 sample"
            assert torch.equal(ocol[:, tap, :].t().double(), col), "the helper's samples differ from the oracle's columns"
            wt = w[:, :, tap // case.kw, tap % case.kw].t()
            bound += spread @ wt.abs()                 # (spread >= |col|: bounds the products whichever way the combine went)
            out += col @ wt
        if case.bias:
            bound += data["bias"].abs()[None, :]
            out += data["bias"][None, :]
        assert float(bound.max()) < 2.0 ** 24 * unit_out, "premise 3: a partial sum of the contraction may exceed 2^24 units"
        assert _is_multiple(out, unit_out)
        assert D.representable(out, torch.float32).all()
        out = out.reshape(x.shape[0], off.shape[2], off.shape[3], case.cout).permute(0, 3, 1, 2)       # NCHW, as reference()
        outs.append(out.clamp_min(0.0) if case.relu else out)
    x_all = torch.cat([x.reshape(-1) for x in data["xs"]] + [w.reshape(-1)])
    assert ((x_all == 0) | (x_all.abs() >= FP16_MIN_NORMAL)).all(), "premise 2: a subnormal fp16 operand"
    return torch.cat([o.reshape(-1) for o in outs])


@pytest.fixture(scope="module")
def tile_rows():
    from orientedreppoints_amd import build
    from orientedreppoints_amd.mmdet_ops.deform_conv import half_tile_rows
    build.build_hip()
    return half_tile_rows


@pytest.mark.parametrize("case", D.ALL_CASES, ids=lambda c: c.name)
def test_exact_case_premises_and_conditions(case, oracle, tile_rows):
    """Every case: the premises above; the tile height the case claims, by the library's own query; and the conditions that keep
    the bitwise comparison from being vacuous -- at least 25 % of the outputs are NOT representable in T before the final
    rounding (both types), every border class of the sampler holds at least 1 % of the (position, tap) samples, a ReLU case
    has at least 10 % clipped and 10 % unclipped outputs, and fp16 overflow happens in the saturation case only."""
    data = D.generate(case)
    out = check_premises(case, data, oracle)
    ref = torch.cat([r.reshape(-1) for r in D.reference(case, data)])
    assert torch.equal(ref, out), "reference() and the per-tap contraction of this test disagree"
    assert tile_rows(D.positions(case), len(case.levels)) == case.rows
    for dt in (torch.float16, torch.bfloat16):
        inexact = 1.0 - float(D.representable(out, dt).double().mean())
        assert inexact >= 0.25, "%s: only %.1f %% of the outputs round in the final conversion to %s" % (case.name, 100 * inexact, dt)
    counts, total = D.sample_class_counts(case, data)
    for k, n in counts.items():
        assert n >= 0.01 * total, "%s: sampling class %r holds %d of %d samples" % (case.name, k, n, total)
    if case.relu:
        clipped = float((out == 0).double().mean())
        assert 0.10 <= clipped <= 0.90, clipped
    over = float((out.abs() > FP16_MAX).double().mean())
    if case in D.SATURATION_CASES:
        assert 0.01 <= over <= 0.5, over
        assert torch.isinf(out.to(torch.float16)).any() and not torch.isinf(out.to(torch.bfloat16)).any()
    else:
        assert over == 0.0 and float(out.abs().max()) < FP16_MAX - 32, "fp16 overflow outside the saturation case"


def test_case_list_covers_what_it_claims(tile_rows):
    """Structure of the list: each tile height has single-level cases whose position count is no multiple of the tile and whose
    tile counts are 1, 3 and 7 (mod 8) (idle workgroups of the 8-way remapped grid); a launch where a tile straddles two images;
    levels smaller than one tile; the depths and geometries of the issue; the scaled cases carry the same integers."""
    for rows in (32, 64, 96):
        cs = [c for c in D.TILE_CASES if c.rows == rows]
        assert all(len(c.levels) == 1 and D.positions(c) % rows != 0 for c in cs)
        assert {-(-D.positions(c) // rows) % 8 for c in cs} >= {1, 3, 7}
        assert all(tile_rows(D.positions(c), 1) == rows for c in cs)
    assert {c.rows for c in D.ALL_CASES} == {32, 64, 96}
    for c in D.SEAM_CASES + [D.BY_NAME["head_b2"]]:
        per_image = [D.out_size(h, c, c.kh) * D.out_size(w, c, c.kw) for h, w in c.levels]
        assert c.batch > 1 and any(n > c.rows and n % c.rows for n in per_image), "no tile straddles two images"
    for c in D.SEAM_CASES:
        assert len(c.levels) >= 3 and (2, 3) in c.levels
        assert any(c.batch * h * w < c.rows for h, w in c.levels)
    assert any((1, 1) in c.levels for c in D.SEAM_CASES) and any((1, 1) not in c.levels for c in D.SEAM_CASES)
    assert D.BY_NAME["head_b1"].levels == ((128, 128), (64, 64), (32, 32), (16, 16), (8, 8)) and D.positions(D.BY_NAME["head_b1"]) == 21824
    assert {c.cin for c in D.ALL_CASES} >= {256, 512, 1024}
    assert {c.cout for c in D.ALL_CASES} >= {64, 128, 192, 256, 320, 512}
    geo = {(c.kh, c.kw, c.stride, c.pad, c.dil) for c in D.ALL_CASES}
    assert geo >= {(3, 3, 2, 1, 1), (3, 3, 1, 2, 2), (1, 1, 1, 0, 1), (1, 3, 1, 0, 1), (3, 1, 1, 0, 1), (2, 2, 1, 0, 1)}
    assert any(c.mask and c.bias and c.relu and len(c.levels) > 1 for c in D.ALL_CASES)
    assert any(not c.mask and c.bias and len(c.levels) > 1 for c in D.ALL_CASES)
    unit, down, up = (D.generate(D.BY_NAME[n]) for n in ("range_unit", "range_down", "range_up"))
    assert (D.BY_NAME["range_down"].x_exp, D.BY_NAME["range_down"].w_exp, D.BY_NAME["range_up"].x_exp) == (-8, -4, 4)
    for a, b, c in zip(unit["xs"], down["xs"], up["xs"]):
        assert torch.equal(a, b * 2.0 ** 8) and torch.equal(a * 2.0 ** 4, c)
    assert torch.equal(unit["weight"], down["weight"] * 2.0 ** 4) and torch.equal(unit["weight"], up["weight"])
    for a, b in zip(unit["offs"] + unit["masks"], down["offs"] + down["masks"]):
        assert torch.equal(a, b)


def test_premise_check_fails_when_a_range_is_widened(oracle, monkeypatch):
    """The premise test is not decoration: with |x| <= 22 (one past the 21 that 256 units / (3/2) allows) a partial sum of the
    combine can need 9 bits, and with |w| <= 127 at c_in = 1024 the contraction can pass 2^24 units: both must be reported."""
    case = D.BY_NAME["depth_1024_320"]
    check_premises(case, D.generate(case), oracle)
    monkeypatch.setattr(D, "X_MAX", 22)
    wide = case._replace(x_max=22)
    with pytest.raises(AssertionError, match="premise 1"):
        check_premises(wide, D.generate(wide), oracle)
    monkeypatch.setattr(D, "X_MAX", 15)
    monkeypatch.setattr(D, "W_MAX", 127)
    with pytest.raises(AssertionError, match="premise 3"):
        check_premises(case, D.generate(case), oracle)


def test_half_path_ok_boundary(tile_rows):
    """orp_dcn_half_path_ok at its edges: c_in a multiple of 256, c_out a multiple of 64 (at least 64), at most 9 taps,
    groups = deformable_groups = 1.  And the tile-rows query's own argument check."""
    from orientedreppoints_amd import _lib
    ok = _lib.lib().orp_dcn_half_path_ok
    assert [ok(c, 256, 3, 3, 1, 1) for c in (128, 256, 384, 512)] == [0, 1, 0, 1]
    assert [ok(256, c, 3, 3, 1, 1) for c in (0, 32, 64, 96, 128, 320)] == [0, 0, 1, 0, 1, 1]
    assert [ok(256, 256, kh, kw, 1, 1) for kh, kw in ((3, 3), (1, 9), (2, 5), (5, 2), (1, 1))] == [1, 1, 0, 0, 1]
    assert ok(256, 256, 3, 3, 2, 1) == 0 and ok(512, 256, 3, 3, 2, 1) == 0 and ok(256, 256, 3, 3, 1, 2) == 0
    L = _lib.lib()
    assert L.orp_dcn_forward_h_tile_rows(0, 1) == _lib.ORP_EINVAL and L.orp_dcn_forward_h_tile_rows(100, 0) == _lib.ORP_EINVAL
    assert L.orp_dcn_forward_h_tile_rows(100, 9) == _lib.ORP_EINVAL
    with pytest.raises(_lib.OrpHipError):
        tile_rows(0, 1)
    assert np.all(np.isin([tile_rows(p, n) for p in (1, 31, 8000, 9000, 20000, 10 ** 7) for n in (1, 5, 8)], (32, 64, 96)))
