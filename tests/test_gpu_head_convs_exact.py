"""GPU: the three plain inference convolutions of the head and the FPN BIT FOR BIT against float64 --
  * orp_conv3x3_small_multi_strided (csrc/orp_conv_small.hip) through fused_norm.conv3x3_multi and through the C entry point,
  * orp_conv1x1_multi (csrc/orp_conv1x1.hip) through fused_norm.conv1x1_multi,
  * orp_dcn_forward_pair_heads (the HEADS instantiation of csrc/orp_dcn.hip) at its 64-row and its 96-row tile.

Under the premises that tests/test_head_conv_cases.py asserts on the same generated data (tests/head_conv_cases.py) nothing rounds in
fp32 in ANY summation order, so the expected bits are the float64 result's .float() and there is no tolerance: a wrong tap for one
wave's K slice, a lost residual on one level or a bias added twice changes bits.  Every launch is spied on the library's entry
point: exactly the expected entry ran, once, with the expected number of levels.  One random-data test per kernel holds the
worst |err| / bound against float64 to <= 1, with bounds derived from the number of roundings (head_conv_cases), and reports it."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_half_cases as D  # noqa: E402
import head_conv_cases as HC  # noqa: E402

SENTINEL = -12345.0625                    # no multiple of 1/8: no output of an exact case can equal it
CONV3_ENTRIES = ("orp_conv3x3_small_multi", "orp_conv3x3_small_multi_ex", "orp_conv3x3_small_multi_strided")
DCN_ENTRIES = ("orp_dcn_forward_pair_heads", "orp_dcn_forward_pair", "orp_dcn_forward_pair_amax", "orp_dcn_forward_multi_ex")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _spy(monkeypatch, *names):
    """calls: one (entry point, *arguments) tuple per call of one of the named entry points of the loaded library"""
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    calls = []
    for name in names:
        def spy(*args, _orig=getattr(L, name), _name=name):
            calls.append((_name,) + args)
            return _orig(*args)
        monkeypatch.setattr(L, name, spy)
    return calls


def _assert_bits(got, want64, what):
    want = want64.float()
    assert torch.equal(want.double(), want64), "%s: an expected output is not an fp32 number" % (what,)
    assert got.dtype == torch.float32 and got.shape == want.shape, what
    if not HC.same_bits(got, want):
        bad = int((got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum())
        raise AssertionError("%s: %d of %d outputs differ in their bits" % (what, bad, want.numel()))


def _conv3_module(case, dev, salt=0, stride=None):
    conv = torch.nn.Conv2d(case.cin, case.cout, 3, stride=stride or case.stride, padding=1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(HC.conv3_weight(case, salt).float())
    return conv.to(dev).eval()


def _strided_call(calls):
    """the arguments of the one launch that ran: (levels, weights, strides, nlevels, batch, c_in, c_out, workspace, bytes, stream)"""
    assert [c[0] for c in calls] == ["orp_conv3x3_small_multi_strided"], [c[0] for c in calls]
    return calls[0][1:]


# ---- the small-level 3x3 convolution ------------------------------------------------------------------------------------------------
def test_helper_agrees_with_the_library(dev):
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops import fused_norm
    assert fused_norm.SMALL_LEVEL_POSITIONS == HC.SMALL_LEVEL_POSITIONS
    ok = _lib.lib().orp_conv3x3_small_ok
    assert all(ok(c.cin, c.cout) == 1 for c in HC.CONV3_CASES) and ok(64, 64) == 0 and ok(128, 96) == 0


@pytest.mark.parametrize("B", HC.BATCHES)
@pytest.mark.parametrize("case", HC.CONV3_CASES, ids=lambda c: c.name)
def test_small_conv3x3_is_bitwise_the_float64_convolution(dev, monkeypatch, case, B):
    """conv3x3_multi on integer data, every level set of the case in one launch each: the launch is
    orp_conv3x3_small_multi_strided with exactly the levels of at most 1024 positions (the 1025-position level of the routing-edge
    set goes to the library and is held to the parity test's 1e-4 only), the case's stride and a workspace iff split_k"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv3x3_multi
    conv = _conv3_module(case, dev)
    w64 = conv.weight.detach().double()
    calls = _spy(monkeypatch, *CONV3_ENTRIES)
    for levels in HC.conv3_level_sets(case):
        xs64 = [x.to(dev) for x in HC.conv3_inputs(case.cin, levels, B, case.seed + B)]
        del calls[:]
        with torch.no_grad():
            got = conv3x3_multi([x.float() for x in xs64], conv, split_k=case.split_k)
        small = HC.routed_small(levels)
        a = _strided_call(calls)
        assert a[3] == len(small) and (a[4], a[5], a[6]) == (B, case.cin, case.cout)
        assert [(a[0][k].height, a[0][k].width) for k in range(a[3])] == [levels[i] for i in small]
        assert [a[2][k] for k in range(a[3])] == [case.stride] * len(small)
        assert (a[7] is not None and a[8] > 0) == case.split_k
        for i, (g, x64) in enumerate(zip(got, xs64)):
            want64 = HC.conv64(x64, w64, case.stride)
            what = "%s B=%d level %dx%d" % (case.name, B, levels[i][0], levels[i][1])
            if i in small:
                _assert_bits(g, want64, what)
            else:
                assert g.shape == want64.shape and float((g.double() - want64).abs().max()) <= 1e-4 * float(want64.abs().max()), what
        if levels is HC.LEVELS_EDGE:
            assert len(small) == 2 and len(levels) == 3


def test_small_conv3x3_sixteen_levels_with_a_module_per_tensor(dev, monkeypatch):
    """kMaxLevels tensors in one launch, eight distinct weight tensors each used by two of them (both towers' levels): every output
    against its own module's float64 convolution"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv3x3_multi
    case = HC.CONV3_BY_NAME["c256_256"]
    B = 2
    sizes = [(8, 8), (5, 7), (1, 1), (3, 3), (16, 16), (1, 33), (2, 5), (9, 4)] * 2
    mods = [_conv3_module(case, dev, salt=10 + k) for k in range(8)]
    convs = [mods[(3 * i) % 8] for i in range(16)]
    assert len({id(c) for c in convs}) == 8 and all(sum(c is m for c in convs) == 2 for m in mods)
    assert not torch.equal(mods[0].weight, mods[1].weight)
    xs64 = [x.to(dev) for x in HC.conv3_inputs(case.cin, sizes, B, 1601)]
    calls = _spy(monkeypatch, *CONV3_ENTRIES)
    with torch.no_grad():
        got = conv3x3_multi([x.float() for x in xs64], convs)
    a = _strided_call(calls)
    assert a[3] == 16 and len({a[1][k] for k in range(16)}) == 8
    for i in range(16):
        _assert_bits(got[i], HC.conv64(xs64[i], convs[i].weight.detach().double(), 1), "tensor %d (%dx%d)" % ((i,) + sizes[i]))


@pytest.mark.parametrize("split_k", [False, True])
def test_small_conv3x3_mixed_strides_in_one_launch(dev, monkeypatch, split_k):
    """strides 1 and 2 with per-tensor modules at 256 -> 256 in ONE launch (the API takes a stride per level)"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv3x3_multi
    case = HC.CONV3_BY_NAME["c256_256"]
    B = 2
    sizes = [(9, 11), (9, 11), (32, 32), (5, 7), (1, 1), (31, 17)]
    strides = [1, 2, 2, 1, 2, 1]
    m1, m2 = _conv3_module(case, dev, salt=21, stride=1), _conv3_module(case, dev, salt=22, stride=2)
    convs = [m1 if s == 1 else m2 for s in strides]
    xs64 = [x.to(dev) for x in HC.conv3_inputs(case.cin, sizes, B, 1701)]
    calls = _spy(monkeypatch, *CONV3_ENTRIES)
    with torch.no_grad():
        got = conv3x3_multi([x.float() for x in xs64], convs, split_k=split_k)
    a = _strided_call(calls)
    assert a[3] == 6 and [a[2][k] for k in range(6)] == strides and (a[7] is not None) == split_k
    for i in range(6):
        _assert_bits(got[i], HC.conv64(xs64[i], convs[i].weight.detach().double(), strides[i]),
                     "tensor %d (%dx%d, stride %d)" % (i, sizes[i][0], sizes[i][1], strides[i]))


def _carve(dev, shapes, gap=7):
    """(buffer, views, canary mask): one NaN-filled fp32 buffer, the views carved out of it in order with `gap` floats of SENTINEL before,
    between and behind them (an odd gap: the views are not 16-byte aligned)"""
    sizes = [int(torch.Size(s).numel()) for s in shapes]
    buf = torch.full((gap + sum(n + gap for n in sizes),), float('nan'), dtype=torch.float32, device=dev)
    canary = torch.zeros(buf.shape, dtype=torch.bool, device=dev)
    canary[:gap] = True
    pos, views = gap, []
    for s, n in zip(shapes, sizes):
        views.append(buf[pos:pos + n].view(s))
        canary[pos + n:pos + n + gap] = True
        pos += n + gap
    buf[canary] = SENTINEL
    return buf, views, canary


def _launch_strided(xs, outs, packs, strides, B, cin, cout, ws=None, ws_bytes=0, nlevels=None):
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import _norm_levels
    n = len(xs)
    levels = _norm_levels(xs, outs)
    wts = (ctypes.c_void_p * n)(*[p.data_ptr() if p is not None else None for p in packs])
    st = (ctypes.c_int * n)(*strides)
    with torch.cuda.device(xs[0].device):
        return _lib.lib().orp_conv3x3_small_multi_strided(levels, wts, st, n if nlevels is None else nlevels, B, cin, cout,
                                                          ctypes.c_void_p(ws.data_ptr()) if ws is not None else None, ws_bytes,
                                                          _lib.stream_of(xs[0]))


@pytest.mark.parametrize("name,sizes,B", [("c128_192", HC.LEVELS_S1, 3), ("c256_128_s2", HC.LEVELS_S2, 2)])
def test_small_conv3x3_entry_point_writes_every_output_and_nothing_else(dev, name, sizes, B):
    """the C entry point with outputs carved from one NaN-filled buffer, canaries between them: every output element is written
    (and is the float64 result), no canary is touched"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.deform_conv import _packed_weight
    case = HC.CONV3_BY_NAME[name]
    conv = _conv3_module(case, dev)
    packed = _packed_weight(conv.weight)
    xs64 = [x.to(dev) for x in HC.conv3_inputs(case.cin, sizes, B, 1801)]
    xs = [x.float().contiguous() for x in xs64]
    buf, outs, canary = _carve(dev, [(B, case.cout) + HC.out_hw(h, w, case.stride) for h, w in sizes])
    rc = _launch_strided(xs, outs, [packed] * len(xs), [case.stride] * len(xs), B, case.cin, case.cout)
    assert rc == _lib.ORP_OK
    torch.cuda.synchronize()
    assert bool((buf[canary] == SENTINEL).all()), "a canary between the outputs was overwritten"
    assert not bool(torch.isnan(buf).any()), "an output element was not written"
    for o, x64, (h, w) in zip(outs, xs64, sizes):
        _assert_bits(o, HC.conv64(x64, conv.weight.detach().double(), case.stride), "%s level %dx%d" % (name, h, w))


def test_small_conv3x3_workspace_smaller_than_the_split_it_would_pick(dev):
    """2048 -> 256, stride 2, one 32 x 32 image: the launcher picks 8 K slices; with a workspace that holds 2 partial images it has to
    fall back to 2, with one float less than that to none -- the same bits (the exact case does not depend on the order), and
    nothing written behind the workspace it was given"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.deform_conv import _packed_weight
    case = HC.CONV3_BY_NAME["c2048_256_s2_split"]
    B, sizes = 1, HC.LEVELS_P6
    assert HC.ksplit_of(sizes, [2], B, case.cin, case.cout) == 8
    conv = _conv3_module(case, dev)
    packed = _packed_weight(conv.weight)
    x64 = HC.conv3_inputs(case.cin, sizes, B, 1901)[0].to(dev)
    x = x64.float().contiguous()
    want64 = HC.conv64(x64, conv.weight.detach().double(), 2)
    out_floats = want64.numel()
    for slices, nbytes in ((16, 4 * 16 * out_floats), (2, 4 * 2 * out_floats), (1, 4 * 2 * out_floats - 4)):
        wsbuf = torch.full((nbytes // 4 + 1 + 64,), SENTINEL, dtype=torch.float32, device=dev)
        buf, outs, canary = _carve(dev, [tuple(want64.shape)])
        rc = _launch_strided([x], outs, [packed], [2], B, case.cin, case.cout, ws=wsbuf, ws_bytes=nbytes)
        assert rc == _lib.ORP_OK
        torch.cuda.synchronize()
        assert bool((wsbuf[-(-nbytes // 4):] == SENTINEL).all()), "written behind the workspace (%d slices fit)" % slices
        if slices == 1:
            assert bool((wsbuf == SENTINEL).all()), "no split fits, yet the workspace was written"
        else:
            assert not bool((wsbuf[:2 * out_floats] == SENTINEL).any()), "the partial images were not written"
        assert bool((buf[canary] == SENTINEL).all())
        _assert_bits(outs[0], want64, "workspace for %d slices" % slices)


def test_small_conv3x3_entry_point_refuses_what_it_cannot_run(dev):
    """ORP_EINVAL, outputs untouched: 17 levels, stride 3, input == output, Cin = 64, Cout = 96, a null weight"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.deform_conv import _packed_weight
    case = HC.CONV3_BY_NAME["c128_64"]
    B, n = 1, 17
    packed = _packed_weight(_conv3_module(case, dev).weight)
    xs = [x.to(dev).float().contiguous() for x in HC.conv3_inputs(case.cin, [(4, 4)] * n, B, 2001)]
    ys = [torch.full((B, case.cout, 4, 4), SENTINEL, dtype=torch.float32, device=dev) for _ in range(n)]
    ok = dict(xs=xs[:2], outs=ys[:2], packs=[packed] * 2, strides=[1, 1], B=B, cin=case.cin, cout=case.cout)
    bad = {
        "17 levels": dict(ok, xs=xs, outs=ys, packs=[packed] * n, strides=[1] * n),
        "stride 3": dict(ok, strides=[1, 3]),
        "input == output": dict(ok, outs=[ys[0], xs[1]]),
        "Cin = 64": dict(ok, cin=64),
        "Cout = 96": dict(ok, cout=96),
        "a null weight": dict(ok, packs=[packed, None]),
    }
    before = [x.clone() for x in xs]
    for what, kw in bad.items():
        assert _launch_strided(**kw) == _lib.ORP_EINVAL, what
        torch.cuda.synchronize()
        assert all(bool((y == SENTINEL).all()) for y in ys), what
        assert all(torch.equal(a, b) for a, b in zip(xs, before)), what
    assert _launch_strided(**ok) == _lib.ORP_OK                                     # (the valid call the bad ones differ from)
    torch.cuda.synchronize()
    assert not bool((ys[0] == SENTINEL).all()) and bool((ys[2] == SENTINEL).all())


@pytest.mark.parametrize("name", ["c256_256", "c256_256_s2_split"])
def test_small_conv3x3_inf_and_nan_reach_the_windows_that_read_them_and_no_other(dev, name):
    """one +Inf and one NaN in integer data: every output whose 3 x 3 window reads neither keeps the exact float64 bits, every
    output whose window reads one (all channels) is non-finite"""
    import torch.nn.functional as F
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv3x3_multi
    case = HC.CONV3_BY_NAME[name]
    B, sizes = 2, [(21, 19), (5, 7)]
    conv = _conv3_module(case, dev)
    clean = [x.to(dev) for x in HC.conv3_inputs(case.cin, sizes, B, 2101)]
    xs = [x.float() for x in clean]
    spots = [(0, 0, 3, 0, 5, float('inf')), (0, 1, 40, 16, 15, float('nan')), (1, 1, 255, 4, 6, float('inf'))]     # (level, b, c, y, x)
    read = [torch.zeros((B, 1, h, w), dtype=torch.float64, device=dev) for h, w in sizes]
    for lvl, b, c, yy, xx, v in spots:
        xs[lvl][b, c, yy, xx] = v
        read[lvl][b, 0, yy, xx] = 1.0
    with torch.no_grad():
        got = conv3x3_multi(xs, conv, split_k=case.split_k)
    ones = torch.ones((1, 1, 3, 3), dtype=torch.float64, device=dev)
    for g, x64, r in zip(got, clean, read):
        want = HC.conv64(x64, conv.weight.detach().double(), case.stride).float()
        t = (F.conv2d(r, ones, None, case.stride, 1) > 0).expand_as(want)
        assert int(t.sum()) > 0 and int((~t).sum()) > 0
        assert bool((~torch.isfinite(g[t])).all())
        assert HC.same_bits(g[~t], want[~t])


# ---- the 1x1 output convolution -------------------------------------------------------------------------------------------------------
def _conv1_modules(d, dev):
    cout, cin = d["weight"].shape[:2]
    mods = {}
    for with_bias in (False, True):
        m = torch.nn.Conv2d(cin, cout, 1, bias=with_bias)
        with torch.no_grad():
            m.weight.copy_(d["weight"].float())
            if with_bias:
                m.bias.copy_(d["bias"].float())
        mods[with_bias] = m.to(dev).eval()
    return mods


@pytest.mark.parametrize("cout", HC.CONV1_COUTS)
@pytest.mark.parametrize("cin", HC.CONV1_CINS)
def test_conv1x1_is_bitwise_the_float64_convolution_and_epilogue(dev, monkeypatch, cin, cout):
    """conv1x1_multi on integer data (bias and sub multiples of 1/8): five levels (hw = 1, 63, 64, 65, 1517) and eight levels in one
    launch, B = 1 and 3, every combination of bias x residual x ReLU x sub: y bit for bit the float64 result, z bit for bit y - sub"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_multi, conv1x1_ok
    calls = _spy(monkeypatch, "orp_conv1x1_multi")
    runs = 0
    for levels in (HC.CONV1_LEVELS, HC.CONV1_LEVELS8):
        for B in HC.CONV1_BATCHES:
            d = HC.conv1_data(cin, cout, levels, B, 7 * cin + cout + B)
            mods = _conv1_modules(d, dev)
            xs64 = [x.to(dev) for x in d["xs"]]
            xs = [x.float() for x in xs64]
            res64 = [r.to(dev) for r in d["residuals"]]
            res = [r.float() for r in res64]
            sub = d["sub"].to(dev).float().view(1, -1, 1, 1)
            assert conv1x1_ok(mods[True], xs[0])
            for with_bias, with_res, relu, with_sub in HC.CONV1_FORMS:
                del calls[:]
                with torch.no_grad():
                    out = conv1x1_multi(xs, mods[with_bias], relu=relu, residuals=res if with_res else None,
                                        sub=sub if with_sub else None)
                assert [c[0] for c in calls] == ["orp_conv1x1_multi"]
                a = calls[0][1:]
                assert (a[1], a[2], a[3], a[4], a[8]) == (len(levels), B, cin, cout, int(relu))
                assert (a[6] is not None) == with_bias and (a[7] is not None) == with_sub
                ys, zs = out if with_sub else (out, [None] * len(levels))
                for i in range(len(levels)):
                    y64, z64 = HC.conv1_reference(xs64[i], d["weight"], d["bias"] if with_bias else None,
                                                  res64[i] if with_res else None, relu, d["sub"] if with_sub else None)
                    what = "%d -> %d B=%d level %dx%d bias=%d residual=%d relu=%d sub=%d" % (
                        cin, cout, B, levels[i][0], levels[i][1], with_bias, with_res, relu, with_sub)
                    _assert_bits(ys[i], y64, "y, " + what)
                    if with_sub:
                        _assert_bits(zs[i], z64, "z, " + what)
                        assert HC.same_bits(zs[i], ys[i] - sub)
                runs += 1
    assert runs == 2 * len(HC.CONV1_BATCHES) * 16


def test_conv1x1_entry_point_refuses_what_it_cannot_run(dev):
    """ORP_EINVAL with the outputs untouched: 9 levels, Cout = 33, `output2` without `sub`"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import _BiasLevel, _packed_1x1_weight
    L = _lib.lib()
    B, cin, cout, n = 1, 256, 18, 9
    d = HC.conv1_data(cin, cout, [(3, 3)] * n, B, 2201)
    packed = _packed_1x1_weight(_conv1_modules(d, dev)[False].weight)
    xs = [x.to(dev).float().contiguous() for x in d["xs"]]
    ys = [torch.full((B, 33, 3, 3), SENTINEL, dtype=torch.float32, device=dev) for _ in range(n)]
    zs = [torch.full((B, 33, 3, 3), SENTINEL, dtype=torch.float32, device=dev) for _ in range(n)]
    sub = d["sub"].to(dev).float().contiguous()

    def launch(nlev, c_out, with_z, with_sub):
        levels = (_BiasLevel * n)()
        for i in range(n):
            levels[i] = _BiasLevel(xs[i].data_ptr(), None, ys[i].data_ptr(), zs[i].data_ptr() if with_z else None, 3, 3)
        with torch.cuda.device(dev):
            rc = L.orp_conv1x1_multi(levels, nlev, B, cin, c_out, _lib.ptr(packed), None, _lib.ptr(sub) if with_sub else None, 0,
                                     _lib.stream_of(xs[0]))
        torch.cuda.synchronize()
        return rc
    for what, args in (("9 levels", (9, cout, False, False)), ("Cout = 33", (8, 33, False, False)),
                       ("output2 without sub", (8, cout, True, False))):
        assert launch(*args) == _lib.ORP_EINVAL, what
        assert all(bool((t == SENTINEL).all()) for t in ys + zs), what
    assert launch(8, cout, True, True) == _lib.ORP_OK
    assert not bool((ys[7][:, :cout] == SENTINEL).any()) and bool((ys[8] == SENTINEL).all())


# ---- both DeformConvs + ReLU + the 1x1 heads ----------------------------------------------------------------------------------------
def _dcn_module(weight64, dev):
    from orientedreppoints_amd.mmdet_ops import DeformConv
    m = DeformConv(256, 256, 3, 1, 1)
    with torch.no_grad():
        m.weight.copy_(weight64.float())
    return m.to(dev).eval()


def _head_module(weight64, bias64, dev):
    m = torch.nn.Conv2d(256, weight64.size(0), 1, bias=bias64 is not None)
    with torch.no_grad():
        m.weight.copy_(weight64.float())
        if bias64 is not None:
            m.bias.copy_(bias64.float())
    return m.to(dev).eval()


@pytest.mark.parametrize("hc", HC.HEADS_CASES, ids=lambda c: c.name)
def test_pair_heads_launch_is_bitwise_head64_of_relu_of_dcn64(dev, monkeypatch, hc):
    """orp_dcn_forward_pair_heads at the tile height the case claims (the library's query; the launch raises 32 rows to 64), two
    layers with their own features and weights over one set of offsets: every head pair (15, 18) / (1, 20) / (20, 4), with and
    without residuals_b and head biases, against head64(relu(dcn64(x))) -- the DeformConv reference once per case, on the device"""
    from orientedreppoints_amd.mmdet_ops.deform_conv import deform_conv_forward_pair_heads, half_tile_rows, pair_heads_ok
    case = hc.dcn
    assert half_tile_rows(D.positions(case), len(case.levels)) == case.rows and hc.rows == max(64, case.rows)
    data, da, db = HC.heads_expected(hc, dev)
    ca, cb = _dcn_module(data["weight_a"], dev), _dcn_module(data["weight_b"], dev)
    xa, xb = [x.to(dev).float() for x in data["xs_a"]], [x.to(dev).float() for x in data["xs_b"]]
    offs = [o.to(dev).float() for o in data["offs"]]
    calls = _spy(monkeypatch, *DCN_ENTRIES)
    runs = 0
    for k_a, k_b in HC.HEAD_KS:
        hp = HC.head_params(k_a, k_b, case.seed + k_a)
        res64 = [r.to(dev) for r in HC.heads_residuals(hc, k_b, case.seed + k_b)]
        res = [r.float() for r in res64]
        for with_res, with_bias in HC.HEADS_FORMS:
            ba, bb = (hp["bias_a"], hp["bias_b"]) if with_bias else (None, None)
            ha, hb = _head_module(hp["weight_a"], ba, dev), _head_module(hp["weight_b"], bb, dev)
            assert pair_heads_ok(ca, cb, ha, hb, xa[0])
            del calls[:]
            with torch.no_grad():
                oa, ob = deform_conv_forward_pair_heads(xa, xb, offs, ca, cb, ha, hb, residuals_b=res if with_res else None)
            assert [c[0] for c in calls] == ["orp_dcn_forward_pair_heads"], [c[0] for c in calls]
            assert (calls[0][3], calls[0][4]) == (len(case.levels), case.batch)
            for i, (h, w) in enumerate(case.levels):
                what = "%s heads (%d, %d) residual=%d bias=%d level %dx%d" % (hc.name, k_a, k_b, with_res, with_bias, h, w)
                _assert_bits(oa[i], HC.head64(da[i], hp["weight_a"], ba), "first head, " + what)
                _assert_bits(ob[i], HC.head64(db[i], hp["weight_b"], bb, res64[i] if with_res else None), "second head, " + what)
            runs += 1
    assert runs == 12


# ---- random data: inside a derived bound, and the same bits twice -----------------------------------------------------------------------
def _worst(got, ref64, bound):
    return float(((got.double() - ref64).abs() / bound).max())


def test_small_conv3x3_random_data_inside_the_derived_bound(dev, monkeypatch):
    """N(0, 1) features, He-scale weights, 256 -> 256 at (2, 256, 13, 16) + a 3 x 5 level, stride 1 and stride 2 with the K split:
    |err| <= (9 Cin + 2) 2^-24 sum |x_k w_k| against float64 at every output; a second launch returns the same bits"""
    import conftest
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv3x3_multi
    calls = _spy(monkeypatch, *CONV3_ENTRIES)
    for stride, split_k in ((1, False), (2, True)):
        r = HC.random_conv(256, 256, 3, HC.RANDOM_LEVELS, HC.RANDOM_BATCH, 2301 + stride)
        conv = torch.nn.Conv2d(256, 256, 3, stride=stride, padding=1, bias=False)
        with torch.no_grad():
            conv.weight.copy_(r["weight"])
        conv = conv.to(dev).eval()
        xs = [x.to(dev) for x in r["xs"]]
        del calls[:]
        with torch.no_grad():
            got = conv3x3_multi(xs, conv, split_k=split_k)
            again = conv3x3_multi(xs, conv, split_k=split_k)
        assert [c[0] for c in calls] == ["orp_conv3x3_small_multi_strided"] * 2 and calls[0][4] == 2
        worst = max(_worst(g, HC.conv64(x, conv.weight.detach(), stride), HC.conv3_bound(x, conv.weight.detach(), stride))
                    for g, x in zip(got, xs))
        conftest.REPORT.append("small-level 3x3 convolution 256 -> 256, stride %d%s, N(0, 1) data: worst |err| / bound vs float64 %.2e"
                               % (stride, ", K split" if split_k else "", worst))
        assert worst <= 1.0
        assert all(HC.same_bits(a, b) for a, b in zip(got, again))


def test_conv1x1_random_data_inside_the_derived_bound(dev, monkeypatch):
    """N(0, 1) features, residuals and bias, He-scale weights, 256 -> 18 with bias + residual + ReLU + sub:
    |err| <= (Cin + 3) 2^-24 (sum |x_k w_k| + |b| + |r|); z is y - sub in fp32; a second launch returns the same bits"""
    import conftest
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_multi
    calls = _spy(monkeypatch, "orp_conv1x1_multi")
    r = HC.random_conv(256, 18, 1, HC.RANDOM_LEVELS, HC.RANDOM_BATCH, 2401)
    conv = torch.nn.Conv2d(256, 18, 1, bias=True)
    with torch.no_grad():
        conv.weight.copy_(r["weight"])
        conv.bias.copy_(r["bias"])
    conv = conv.to(dev).eval()
    xs, res = [x.to(dev) for x in r["xs"]], [t.to(dev) for t in r["residuals"]]
    sub = r["sub"].to(dev).view(1, -1, 1, 1)
    worst = 0.0
    for relu in (False, True):
        with torch.no_grad():
            ys, zs = conv1x1_multi(xs, conv, relu=relu, residuals=res, sub=sub)
            ys2, zs2 = conv1x1_multi(xs, conv, relu=relu, residuals=res, sub=sub)
        for y, z, x, t in zip(ys, zs, xs, res):
            y64, _ = HC.conv1_reference(x, conv.weight.detach(), conv.bias.detach(), t, relu)
            worst = max(worst, _worst(y, y64, HC.conv1_bound(x, conv.weight.detach(), conv.bias.detach(), t)))
            assert HC.same_bits(z, y - sub)
        assert all(HC.same_bits(a, b) for a, b in zip(ys + zs, ys2 + zs2))
    assert [c[0] for c in calls] == ["orp_conv1x1_multi"] * 4 and calls[0][2] == 2
    conftest.REPORT.append("1x1 output convolution 256 -> 18 + bias + residual (+ ReLU), N(0, 1) data: worst |err| / bound vs float64 %.2e"
                           % worst)
    assert worst <= 1.0


def test_pair_heads_random_data_inside_the_derived_bound(dev, monkeypatch):
    """N(0, 1) features, He-scale DeformConv and head weights, N(0, 2) offsets on a 2^-8 grid, heads (15, 18) with biases and
    residuals_b: |err| <= sum_c |wh_kc| e_c + (256 + 3) 2^-24 (sum_c relu(d_c) |wh_kc| + |b_k| + |r|) with the DeformConv's own
    bound e_c = (9 * 256 + 2) 2^-24 sum |sample w|"""
    import conftest
    from orientedreppoints_amd.mmdet_ops.deform_conv import deform_conv_forward_pair_heads
    case = HC.RANDOM_HEADS
    r = HC.random_heads(2501)
    hr = HC.random_conv(256, 15, 1, HC.RANDOM_LEVELS, HC.RANDOM_BATCH, 2502)
    hr2 = HC.random_conv(256, 18, 1, HC.RANDOM_LEVELS, HC.RANDOM_BATCH, 2503)
    ca, cb = _dcn_module(r["weight_a"], dev), _dcn_module(r["weight_b"], dev)
    ha, hb = _head_module(hr["weight"], hr["bias"], dev), _head_module(hr2["weight"], hr2["bias"], dev)
    xa, xb, offs = ([t.to(dev) for t in r[n]] for n in ("xs_a", "xs_b", "offs"))
    res = [t.to(dev) for t in hr2["residuals"]]
    calls = _spy(monkeypatch, *DCN_ENTRIES)
    with torch.no_grad():
        oa, ob = deform_conv_forward_pair_heads(xa, xb, offs, ca, cb, ha, hb, residuals_b=res)
    assert [c[0] for c in calls] == ["orp_dcn_forward_pair_heads"] and calls[0][3] == 2
    worst = 0.0
    for got, xs, conv, head, rs in ((oa, xa, ca, ha, None), (ob, xb, cb, hb, res)):
        w64, hw64, hb64 = conv.weight.detach().double(), head.weight.detach().double(), head.bias.detach().double()
        layer = dict(xs=[x.double() for x in xs], offs=[o.double() for o in offs], masks=None, weight=w64, bias=None)
        d = D.reference(case, layer, dev)
        for i in range(len(xs)):
            r64 = rs[i].double() if rs is not None else None
            bound = HC.heads_bound(case, layer["xs"][i], layer["offs"][i], w64, d[i], hw64, hb64, r64)
            worst = max(worst, _worst(got[i], HC.head64(d[i], hw64, hb64, r64), bound))
    conftest.REPORT.append("DeformConv pair + ReLU + 1x1 heads (15, 18), N(0, 1) data: worst |err| / bound vs float64 %.2e" % worst)
    assert worst <= 1.0
