"""CPU: the premises under which tests/test_gpu_head_convs_exact.py may compare the small-level 3x3 convolution, the head's 1x1
output convolution and the DeformConv pair with fused 1x1 heads BIT FOR BIT with float64, and the conditions that keep such a
comparison from passing vacuously -- asserted on the generated data of every case of tests/head_conv_cases.py.  No GPU, no kernel.

Premises (unit = 1/8):
  1. every input is an fp32 number, and a multiple of the unit (features, weights and residuals are integers);
  2. at every output the sum of the terms' magnitudes -- sum |x||w| + |bias| + |residual|, for the heads
     sum_c relu(d_c) |wh_kc| + |b_k| + |r| on top of the DeformConv's own sum |sample||w| -- is below 2^24 units: every partial sum,
     in any order, is an fp32 number.
So nothing rounds, and the float64 result's .float() is THE result."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_half_cases as D  # noqa: E402
import head_conv_cases as HC  # noqa: E402


def _is_multiple(v, unit):
    q = v / unit
    return bool((q == torch.round(q)).all())


def _exact_input(t, unit=1.0):
    return HC.is_fp32(t) and _is_multiple(t, unit)


# ---- small-level 3x3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HC.CONV3_CASES, ids=lambda c: c.name)
def test_conv3_exact_case_premises(case):
    """integers |x| <= 15, |w| <= 7; sum |x||w| < 2^24 at every output of every level set and batch; the result is an fp32 number"""
    w = HC.conv3_weight(case)
    assert _exact_input(w) and float(w.abs().max()) == HC.W_MAX
    for levels in HC.conv3_level_sets(case):
        for B in HC.BATCHES:
            for x in HC.conv3_inputs(case.cin, levels, B, case.seed + B):
                assert _exact_input(x) and float(x.abs().max()) <= HC.X_MAX
                if x.size(2) * x.size(3) > 64 and B > 1:
                    continue                                  # (the bound does not depend on the batch: big levels once)
                assert float(HC.conv64(x, w, case.stride, magnitudes=True).max()) < 2.0 ** 24
                assert HC.is_fp32(HC.conv64(x, w, case.stride))


@pytest.mark.parametrize("case", HC.CONV3_CASES, ids=lambda c: c.name)
def test_conv3_cases_are_not_vacuous(case):
    """over a case's level sets every border class of the 3 x 3 window occurs; every level whose image is no whole number of
    32-position tiles has a tile that straddles an image seam when B > 1, and such levels exist next to whole-tile ones; the
    routing edge holds a 1024-position level (HIP) beside a 1025-position one (library)"""
    sets = HC.conv3_level_sets(case)
    seen = set()
    for levels in sets:
        for h, w in levels:
            seen |= HC.window_classes(h, w, case.stride)
    assert seen == HC.ALL_WINDOW_CLASSES, sorted(HC.ALL_WINDOW_CLASSES - seen)
    ragged = whole = 0
    for levels in sets:
        for i in HC.routed_small(levels):
            ho, wo = HC.out_hw(levels[i][0], levels[i][1], case.stride)
            for B in (2, 3):
                n = HC.straddling_tiles(B, ho * wo, HC.TILE_POSITIONS)
                if (ho * wo) % HC.TILE_POSITIONS:
                    assert n >= 1, (levels[i], B)
                    ragged += 1
                else:
                    assert n == 0
                    whole += 1
    assert ragged >= 4 and whole >= 2
    if case.stride == 1:
        assert [h * w for h, w in HC.LEVELS_EDGE] == [1023, 1024, 1025] and HC.routed_small(HC.LEVELS_EDGE) == [0, 1]
    assert all(len(HC.routed_small(lv)) == len(lv) for lv in (HC.LEVELS_S1, HC.LEVELS_S2, HC.LEVELS_P6, HC.LEVELS_THIN))


def test_conv3_case_list_reaches_the_paths_it_names():
    """the K geometry each case is built for: chunks per wave, N blocks, and the grid-level K slices after the launcher's rule"""
    by = HC.CONV3_BY_NAME
    assert [(c.cin, c.cout, c.stride, c.split_k) for c in HC.CONV3_CASES] == [
        (128, 64, 1, False), (256, 256, 1, False), (384, 64, 1, False), (128, 192, 1, False), (2048, 256, 2, True),
        (256, 256, 2, True), (256, 128, 2, False)]
    assert 9 * (128 // 8) // 8 == 18 and 18 > 128 // 8          # more chunks per wave than per tap: every wave spans two taps
    assert by["c128_192"].cout // 64 == 3
    p6, p7 = by["c2048_256_s2_split"], by["c256_256_s2_split"]
    assert HC.ksplit_of(HC.LEVELS_P6, [2], 1, p6.cin, p6.cout) == 8
    assert HC.ksplit_of(HC.LEVELS_P6, [2], 1, p6.cin, p6.cout, slices_that_fit=2) == 2       # the workspace fallback's case
    assert HC.ksplit_of(HC.LEVELS_S2, [2] * 5, 1, p7.cin, p7.cout) == 2
    assert {HC.ksplit_of(HC.LEVELS_S2, [2] * 5, B, p6.cin, p6.cout) for B in HC.BATCHES} == {4, 2, 1}
    assert HC.ksplit_of(HC.LEVELS_S2, [2] * 5, 3, p7.cin, p7.cout) == 1                       # too many workgroups: no split


# ---- 1x1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", HC.CONV1_CINS)
def test_conv1_exact_case_premises(cin):
    """integer x, w and residuals, bias and sub multiples of 1/8; sum |x||w| + |b| + |r| < 2^24 units; y and z = y - sub are fp32
    numbers; the ReLU clips some outputs and not others"""
    for cout in HC.CONV1_COUTS:
        for levels in (HC.CONV1_LEVELS, HC.CONV1_LEVELS8):
            for B in HC.CONV1_BATCHES:
                d = HC.conv1_data(cin, cout, levels, B, 7 * cin + cout + B)
                assert _exact_input(d["weight"]) and _exact_input(d["bias"], HC.UNIT) and _exact_input(d["sub"], HC.UNIT)
                assert not _is_multiple(d["bias"], 1.0) or cout == 1
                for x, r in zip(d["xs"], d["residuals"]):
                    assert _exact_input(x) and _exact_input(r)
                    assert float(HC.conv1_magnitude(x, d["weight"], d["bias"], r).max()) < HC.LIMIT
                    y, z = HC.conv1_reference(x, d["weight"], d["bias"], r, True, d["sub"])
                    assert HC.is_fp32(y) and HC.is_fp32(z) and _is_multiple(y, HC.UNIT)
                clipped = torch.cat([HC.conv1_reference(x, d["weight"], d["bias"], r)[0].reshape(-1)
                                     for x, r in zip(d["xs"], d["residuals"])]) < 0
                assert 0.2 <= float(clipped.double().mean()) <= 0.8


def test_conv1_case_list_covers_the_edges():
    assert [c // 8 for c in HC.CONV1_CINS] == [1, 32, 33] and (264 // 8) % 8 != 0
    assert set(HC.CONV1_COUTS) >= {1, 16, 17, 18, 19, 32}
    assert [h * w for h, w in HC.CONV1_LEVELS] == [1, 63, 64, 65, 1517]
    assert len(HC.CONV1_LEVELS8) == 8 and len(HC.CONV1_FORMS) == 16


# ---- heads ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tile_rows():
    from orientedreppoints_amd import build
    from orientedreppoints_amd.mmdet_ops.deform_conv import half_tile_rows
    build.build_hip()
    return half_tile_rows


@pytest.mark.parametrize("hc", HC.HEADS_CASES, ids=lambda c: c.name)
def test_heads_exact_case_premises_and_conditions(hc, tile_rows):
    """Both DeformConv layers: the sum of |sample||w| is below 2^24 units and the result a multiple of the unit.  Every head pair and
    epilogue form: sum_c relu(d_c)|wh_kc| + |b_k| + |r| < 2^24 units, the result an fp32 number.  Not vacuous: every border class
    of the sampler occurs, the ReLU zeroes between 20 % and 80 % of the DeformConv outputs, every level whose image is no whole
    number of tiles has a tile across an image seam when B > 1.  The tile height: the library's query answers what the case says,
    and the HEADS launch raises 32 rows to 64."""
    case = hc.dcn
    assert (case.cin, case.cout, case.kh, case.kw, case.stride, case.pad, case.dil) == (256, 256, 3, 3, 1, 1, 1)
    assert case.relu and not case.mask and not case.bias
    assert tile_rows(D.positions(case), len(case.levels)) == case.rows and hc.rows == max(64, case.rows)
    data = HC.heads_generate(hc)
    for i, (xa, xb) in enumerate(zip(data["xs_a"], data["xs_b"])):
        assert not torch.equal(xa, xb)
    assert not torch.equal(data["weight_a"], data["weight_b"])
    relu_d = []
    for layer in HC.heads_layers(data):
        assert all(_exact_input(t) for t in layer["xs"] + [layer["weight"]]) and all(_exact_input(o, 0.5) for o in layer["offs"])
        for x, off in zip(layer["xs"], layer["offs"]):
            assert float(HC.dcn_magnitude(case, x, off, layer["weight"]).max()) < HC.LIMIT
        d = D.reference(case, layer)
        assert all(_is_multiple(t, HC.UNIT) and HC.is_fp32(t) for t in d)
        zeroed = float(torch.cat([t.reshape(-1) for t in d]).eq(0).double().mean())
        assert 0.2 <= zeroed <= 0.8, zeroed
        relu_d.append(d)
        counts, total = D.sample_class_counts(case, layer)
        for k, n in counts.items():
            assert n >= 0.01 * total, "%s: sampling class %r holds %d of %d samples" % (hc.name, k, n, total)
    worst = 0.0
    for k_a, k_b in HC.HEAD_KS:
        hp = HC.head_params(k_a, k_b, case.seed + k_a)
        res = HC.heads_residuals(hc, k_b, case.seed + k_b)
        assert all(_exact_input(hp[n]) for n in ("weight_a", "weight_b")) and all(_exact_input(r) for r in res)
        assert all(_exact_input(hp[n], HC.UNIT) for n in ("bias_a", "bias_b"))
        assert float(hp["weight_a"].abs().max()) <= HC.HEAD_W_MAX and float(hp["weight_b"].abs().max()) <= HC.HEAD_W_MAX
        for lvl in range(len(case.levels)):
            for d, w, b, r in ((relu_d[0][lvl], hp["weight_a"], hp["bias_a"], None), (relu_d[1][lvl], hp["weight_b"], hp["bias_b"], res[lvl])):
                worst = max(worst, float(HC.head_magnitude(d, w, b, r).max()))
                y = HC.head64(d, w, b, r)
                assert HC.is_fp32(y) and _is_multiple(y, HC.UNIT)
    assert worst < HC.LIMIT, "a partial sum of a head may exceed 2^24 units (%.0f of %.0f)" % (worst, HC.LIMIT)
    per_image = [h * w for h, w in case.levels]
    for n in per_image:
        if case.batch > 1 and n % hc.rows:
            assert HC.straddling_tiles(case.batch, n, hc.rows) >= 1


def test_heads_case_list_covers_what_it_claims(tile_rows):
    by = HC.HEADS_BY_NAME
    assert by["seams_64"].dcn.levels == ((21, 19), (8, 8), (3, 5), (1, 1)) and by["seams_64"].dcn.batch == 2
    assert by["seams_64"].rows == 64 and any(2 * h * w < 64 for h, w in by["seams_64"].dcn.levels)
    assert by["wide_64"].rows == 64 and D.positions(by["wide_64"].dcn) > 8000 and by["wide_64"].dcn.rows == 64
    assert by["single_96"].dcn.levels == ((127, 129),) and by["single_96"].dcn.batch == 1 and by["single_96"].rows == 96
    assert tile_rows(127 * 129, 1) == 96 and (127 * 129) % 96 != 0
    m = by["multi_96"]
    assert m.rows == 96 and m.dcn.batch == 2 and len(m.dcn.levels) > 1
    assert sum(HC.straddling_tiles(2, h * w, 96) for h, w in m.dcn.levels) >= 2
    assert set(HC.HEAD_KS) == {(15, 18), (1, 20), (20, 4)} and len(HC.HEADS_FORMS) == 4


def test_premise_check_fails_when_a_range_is_widened():
    """the premise is not decoration: head weights of 2^12 on the seam case pass 2^24 units"""
    hc = HC.HEADS_BY_NAME["seams_64"]
    data = HC.heads_generate(hc)
    d = D.reference(hc.dcn, HC.heads_layers(data)[0])[0]
    hp = HC.head_params(15, 18, 1)
    assert float(HC.head_magnitude(d, hp["weight_a"], hp["bias_a"]).max()) < HC.LIMIT
    assert float(HC.head_magnitude(d, hp["weight_a"] * 2.0 ** 12, hp["bias_a"]).max()) >= HC.LIMIT


def test_random_cases():
    """shapes of the random cases; the heads' offsets are multiples of 2^-8, so the sampling coordinates are fp32 numbers"""
    assert HC.RANDOM_LEVELS == ((13, 16), (3, 5)) and HC.RANDOM_BATCH == 2
    r = HC.random_heads(1)
    assert all(_is_multiple(o.double(), 2.0 ** -8) and o.dtype == torch.float32 for o in r["offs"])
    assert all(float(o.abs().max()) > 3 for o in r["offs"][:1])
