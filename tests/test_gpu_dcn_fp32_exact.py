"""GPU: the exact fp32 MFMA DeformConv forward (csrc/orp_dcn.hip, split mode 0: the first-generation kernel for c_in % 256 != 0, the
second-generation kernel at tile heights 1 / 2 / 3, the pair launch) BIT FOR BIT against the float64 reference of
tests/dcn_half_cases.py.

Under the cases' premises (small-integer features and weights, offsets with fractional part 0 or 1/2, dyadic modulation values) every
bilinear weight, every weighted neighbour and every partial sum of the contraction is a multiple of one unit (2^(x_exp + w_exp) / 8) of
magnitude below 2^24 units: an fp32 number.  So nothing rounds in fp32 in ANY summation order, the kernels have no final rounding either,
and the expected bits are the float64 result's .to(torch.float32).  There is no tolerance: one wrong neighbour, weight, border
predicate, tap index or tile row changes bits.  tests/test_dcn_half_cases.py asserts the premises of the shared cases without a GPU;
the cases local to this file (depths the half path refuses) assert the one that matters here, `sum |sample| |w| + |bias| < 2^24
units`, before they launch."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_half_cases as D  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def exact_fp32_mode(dev):
    """Split mode 0 (the exact fp32 MFMA path, not fp32 by bf16 / fp16 pieces), as the `split` fixture of test_gpu_dcn_split.py
    sets it; back to the environment's choice afterwards."""
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    assert L.orp_dcn_set_split_mode(0) == 0 and L.orp_dcn_get_split_mode() == 0
    yield
    L.orp_dcn_set_split_mode(-1)


def _assert_exact(case, outs, want64, what):
    for level, (got, w64) in enumerate(zip(outs, want64)):
        want = w64.to(torch.float32)
        assert torch.equal(want.double(), w64), "%s level %d: an expected output is not an fp32 number" % (case.name, level)
        assert got.dtype == torch.float32 and got.shape == want.shape
        g, w = got.contiguous().reshape(-1), want.contiguous().reshape(-1)      # (NCHW order; flat, so that a 1 x 1 level has unit stride)
        bad = int((g.view(torch.int32) != w.view(torch.int32)).sum())           # (for the message)
        assert torch.equal(D.bits(g), D.bits(w)), "%s %s level %d (%dx%d): %d of %d outputs differ in their bits" % (
            case.name, what, level, case.levels[level][0], case.levels[level][1], bad, want.numel())


def _assert_premise(case, data, dev):
    """sum |sample| |w| + |bias| < 2^24 units at every output, with the helper's own samples: every partial sum of the
    contraction, in any order, is then an fp32 number."""
    unit = 2.0 ** (case.x_exp + case.w_exp) / 8
    w = data["weight"].to(dev)
    for i in range(len(case.levels)):
        x, off = data["xs"][i].to(dev), data["offs"][i].to(dev)
        mask = data["masks"][i].to(dev) if case.mask else None
        bound = torch.zeros((off.shape[0] * off.shape[2] * off.shape[3], case.cout), dtype=torch.float64, device=dev)
        for tap in range(case.kh * case.kw):
            idx, wgt, _, _ = D.tap_samples(case, x, off, mask, tap)
            bound += D.tap_columns(x.abs(), idx, wgt.abs()) @ w[:, :, tap // case.kw, tap % case.kw].abs().t()
        if case.bias:
            bound += data["bias"].to(dev).abs()[None, :]
        assert float(bound.max()) < 2.0 ** 24 * unit, "%s level %d: a partial sum may exceed 2^24 units" % (case.name, i)


def _run(case, data, want64, dev):
    from orientedreppoints_amd.mmdet_ops import deform_conv_forward_multi
    for channels_last in (False, True):
        t = D.device_inputs(case, data, torch.float32, dev, channels_last)
        outs = deform_conv_forward_multi(t["xs"], t["offs"], t["weight"], case.stride, case.pad, case.dil, masks=t["masks"],
                                         bias=t["bias"], relu=case.relu)
        for o in outs:
            assert o.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        _assert_exact(case, outs, want64, "channels-last" if channels_last else "NCHW")


# tile heights 1 / 2 / 3, level and image seams, two channel blocks per tap with a partial N block, stride 2, an even kernel, the
# DCNv2 epilogue (mask + bias + ReLU)
GEN2_CASES = ["mt1_t9", "mt2_t131", "mt3_t177", "seam_b3_1x2", "depth_512_320", "geo_3x3_s2", "geo_2x2", "v2_mask_bias_relu"]


@pytest.mark.parametrize("name", GEN2_CASES)
def test_second_generation_kernel_is_bitwise_the_float64_reference(dev, name):
    """c_in a multiple of 256: dcn_fwd_mfma2_kernel, NCHW and channels-last in / out.  The fp32 launcher takes its tile height
    from the same host function as the half launcher, whose query confirms the height the case claims."""
    from orientedreppoints_amd.mmdet_ops.deform_conv import half_tile_rows
    case = D.BY_NAME[name]
    assert case.cin % 256 == 0 and half_tile_rows(D.positions(case), len(case.levels)) == case.rows
    data, want64 = D.expected(case, dev)
    _run(case, data, want64, dev)


# c_in % 256 != 0: the first-generation kernel (32-position tiles, partial channel blocks, partial N blocks).  Local to this file:
# the half path refuses these depths.
_G1L = [(9, 11), (5, 5), (1, 2)]
GEN1_CASES = [
    D._c("g1_64_64", _G1L, batch=2, cin=64, cout=64, mask=True, bias=True, seed=101),
    D._c("g1_96_192", _G1L, batch=2, cin=96, cout=192, mask=True, bias=True, seed=102),
    D._c("g1_32_128", _G1L, batch=2, cin=32, cout=128, mask=True, bias=True, seed=103),
    D._c("g1_96_192_s2", _G1L, batch=2, cin=96, cout=192, stride=2, mask=True, bias=True, seed=104),
]


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in GEN1_CASES])
def test_first_generation_kernel_is_bitwise_the_float64_reference(dev, case):
    from orientedreppoints_amd.mmdet_ops.deform_conv import fast_path_ok
    assert case.cin % 256 != 0 and fast_path_ok(torch.empty((case.cout, case.cin, case.kh, case.kw)), 1, 1)
    data = D.generate(case)
    _assert_premise(case, data, dev)
    _run(case, data, D.reference(case, data, dev), dev)


def test_pair_launch_is_bitwise_the_float64_reference_of_each_layer(dev):
    """orp_dcn_forward_pair (two layers over the same offsets in one launch, one coefficient table per tile for both) on
    v1_plain's data with two different weight tensors: each output against its own reference."""
    from orientedreppoints_amd.mmdet_ops import deform_conv_forward_pair
    case = D.BY_NAME["v1_plain"]
    data, want_a = D.expected(case, dev)
    case_b = case._replace(name="v1_plain_second_weight", seed=case.seed + 1000)
    data_b = dict(data, weight=D.generate(case_b)["weight"])
    assert not torch.equal(data_b["weight"], data["weight"])
    _assert_premise(case_b, data_b, dev)
    want_b = D.reference(case_b, data_b, dev)
    for channels_last in (False, True):
        t = D.device_inputs(case, data, torch.float32, dev, channels_last)
        wb = data_b["weight"].to(dev).float()
        outs_a, outs_b = deform_conv_forward_pair(t["xs"], t["xs"], t["offs"], t["weight"], wb, case.stride, case.pad, case.dil)
        what = "pair, channels-last" if channels_last else "pair, NCHW"
        _assert_exact(case, outs_a, want_a, what + ", first layer")
        _assert_exact(case_b, outs_b, want_b, what + ", second layer")
