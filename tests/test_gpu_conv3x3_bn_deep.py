"""GPU: stage 4's 512 -> 512 channel 3x3 convolution (stride 1 and 2) on the K-split fp16-pieces kernel with BatchNorm + ReLU in its
epilogue (orp_conv3x3_bn_deep).

Exact cases (small-integer activations and weights: every piece, product and partial sum is exact in any order, 9 * 512 * 15 * 7 < 2^24)
bit for bit against the float64 convolution cast to fp32 followed by the affine pass, over the smallest maps that reach every seam of
the 2 x 16 tile, both strides, the K-group seams (channels below / from 256, and the quarters), every tap, every input parity of the stride-2 halo and the
output-channel seams of the workgroups of a tile; random data against float64 inside the derived bound and within twice the
library path's ratio on the same inputs; the range edges, Inf / NaN, reproducibility, graph replay, the switch and the routing query.

Measured on MI355X (worst |err| / bound against float64, this file's random cases; docs/notebook/round23.md): stride 1 at 2 x 3 x 17
0.000151 against the library path's 0.000140, stride 2 at 2 x 7 x 35 0.000269 against 0.000151 (1.8 of the 2 allowed)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_conv1x1_bn as base  # noqa: E402

_bits, _same_bits, _conv64, _bound = base._bits, base._same_bits, base._conv64, base._bound
C = 512
# (stride, images, INPUT H, W).  Stride 1: 1 x 1, exactly one 2 x 16 tile, one more pixel each way (two images: the image seam), 1 x 40.
# Stride 2: 2 x 2, one output tile, one more pixel each way, 7 x 35 (4 x 18 outputs) and 3 x 3, whose last row and column are read by
# padding-adjacent taps only
LAYOUTS = [(1, 1, 1, 1), (1, 1, 2, 16), (1, 2, 3, 17), (1, 1, 1, 40),
           (2, 1, 2, 2), (2, 1, 4, 32), (2, 2, 5, 33), (2, 1, 7, 35), (2, 1, 3, 3)]
# the maps the backbone runs at a 1024^2 image (16 tile rows x 2 tile columns), two images: 512 and 256 workgroups
LAYOUTS += [(1, 2, 32, 32), (2, 2, 64, 64)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _conv3(dev, seed, stride=1, integer=False):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(C, C, 3, stride=stride, padding=1, bias=False)
    with torch.no_grad():
        if integer:
            conv.weight.copy_(torch.randint(-7, 8, (C, C, 3, 3), generator=g).float())
        else:
            conv.weight.copy_(torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5)      # He scale
    return conv.to(dev).eval()


@pytest.fixture(scope="module")
def exact(dev):
    """integer weights per stride and the salted BatchNorm (non-finite constants, signed zeros, a subnormal scale), made once"""
    return {1: _conv3(dev, 101, 1, integer=True), 2: _conv3(dev, 102, 2, integer=True)}, base._bn(C, dev, 7, salted=True)


def _range_bits(x):
    """max over the finite elements of |x| as float bits (orp_range.hpp: range_bits), a one-element int32 tensor"""
    a = x.detach().abs()
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    return a.max().reshape(1).contiguous().view(torch.int32)


def _spy(monkeypatch, name='orp_conv3x3_bn_deep'):
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    orig = getattr(L, name)
    calls = []

    def spy(*args):
        calls.append(args)
        return orig(*args)
    monkeypatch.setattr(L, name, spy)
    return calls


def _deep(x, conv, bn, relu=True, bits=None):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv3x3_bn_deep
    return conv3x3_bn_deep(x, conv, bn, relu=relu, force=True, range_bits=_range_bits(x) if bits is None else bits)


def _want(x, conv, bn, relu):
    """THE result of an exact case: the float64 convolution cast to fp32, then the affine pass (orp_affine.hpp's expression)"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act
    return bn_act(_conv64(x, conv).float().contiguous(), bn, relu=relu)


def _ref64(x, conv, bn, relu):
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine
    a, b = [t.double() for t in _bn_affine(bn)]
    y = _conv64(x, conv) * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


def _ints(shape, dev, seed):
    return torch.randint(-15, 16, shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)).float()


def _check(x, conv, bn, tag):
    for relu in (False, True):
        want = _want(x, conv, bn, relu)
        got = _deep(x, conv, bn, relu)
        assert got.is_contiguous() and got.data_ptr() != x.data_ptr()
        assert _same_bits(got, want), tag + (relu, int((_bits(got) != _bits(want)).sum()))


@pytest.mark.parametrize("stride,B,h,w", LAYOUTS)
def test_exact_cases_bit_for_bit(dev, monkeypatch, exact, stride, B, h, w):
    """integers |x| <= 15, |w| <= 7, every layout, ReLU off and on, salted BatchNorm constants"""
    calls = _spy(monkeypatch)
    convs, bn = exact
    with torch.no_grad():
        _check(_ints((B, C, h, w), dev, 7 * h + w + stride), convs[stride], bn, (stride, B, h, w))
    assert len(calls) == 2 and calls[0][6:12] == (B, C, C, h, w, stride)


@pytest.mark.parametrize("stride,h,w", [(1, 3, 17), (2, 7, 35)])
@pytest.mark.parametrize("lo,hi", [(0, 256), (256, 512), (0, 128), (128, 256), (256, 384), (384, 512)])
def test_each_k_group_alone(dev, exact, stride, h, w, lo, hi):
    """data that is non-zero only in input channels below 256 / from 256 on (the two K groups of stride 2), and in each quarter (the
    four of stride 1): one K group contributes, the others add exact zeros"""
    convs, bn = exact
    x = _ints((1, C, h, w), dev, 31 + lo // 128)
    x[:, :lo] = 0
    x[:, hi:] = 0
    with torch.no_grad():
        _check(x, convs[stride], bn, (stride, h, w, lo, hi))


@pytest.mark.parametrize("stride,h,w", [(1, 3, 17), (2, 5, 33)])
def test_single_tap_weights(dev, exact, stride, h, w):
    """the weight non-zero at one tap only, for each of the nine"""
    convs, bn = exact
    x = _ints((1, C, h, w), dev, 41)
    conv = _conv3(dev, 1, stride, integer=True)
    full = convs[stride].weight.detach()
    with torch.no_grad():
        for tap in range(9):
            conv.weight.zero_()
            conv.weight[:, :, tap // 3, tap % 3] = full[:, :, tap // 3, tap % 3]
            _check(x, conv, bn, (stride, tap))


@pytest.mark.parametrize("py,px", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_single_pixel_inputs_at_each_parity_stride2(dev, exact, py, px):
    """stride 2: one non-zero input pixel (all channels) at each (row parity, column parity) of the de-interleaved halo, next to a tile
    seam in both directions (7 x 35 input = 4 x 18 outputs: the pixel's window reaches two tile rows and two tile columns)"""
    convs, bn = exact
    x = torch.zeros((1, C, 7, 35), device=dev)
    x[0, :, 3 + py, 31 + px] = _ints((C,), dev, 51 + 2 * py + px)
    x[0, 0, 3 + py, 31 + px] = 15.0
    with torch.no_grad():
        _check(x, convs[2], bn, (py, px))


@pytest.mark.parametrize("stride,h,w", [(1, 2, 16), (2, 4, 32)])
def test_output_channels_at_the_workgroup_seams(dev, stride, h, w):
    """output channels 127 / 128, 255 / 256 and 383 / 384 (and 63 / 64 at stride 1) belong to different workgroups of a tile: each output channel o copies
    (o % 7 + 1) x input channel o, so that a value written to a neighbouring channel is a different value"""
    conv, bn = _conv3(dev, 1, stride, integer=True), base._bn(C, dev, 9)
    with torch.no_grad():
        conv.weight.zero_()
        o = torch.arange(C, device=dev)
        conv.weight[o, o, 1, 1] = (o % 7 + 1).float()
        x = _ints((1, C, h, w), dev, 61).abs() + 1
        for relu in (False, True):
            want, got = _want(x, conv, bn, relu), _deep(x, conv, bn, relu)
            for ch in (63, 64, 127, 128, 255, 256, 383, 384):
                assert _same_bits(got[:, ch], want[:, ch]), (stride, ch, relu)
            assert _same_bits(got, want)
        raw = _conv64(x, conv)
        for lo in (63, 127, 255, 383):
            assert bool((raw[:, lo] != raw[:, lo + 1]).any())


def test_unsupported_shapes_are_rejected(dev):
    """`_ok` refuses every pair but (512, 512) and every stride but 1 and 2; the launcher returns ORP_EINVAL and writes nothing"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import _packed_3x3_deep_planes
    L = _lib.lib()
    assert [L.orp_conv3x3_bn_deep_ok(C, C, s) for s in (0, 1, 2, 3, 4, -1)] == [0, 1, 1, 0, 0, 0]
    x = torch.randn(1, C, 8, 16, device=dev)
    conv = _conv3(dev, 2)
    packed, ab, bits = _packed_3x3_deep_planes(conv.weight), torch.ones(C, device=dev), _range_bits(x)
    assert packed.numel() == 4 * C * C * 9 + 16 == L.orp_conv3x3_bn_deep_packed_bytes(C, C)
    y = torch.full((1, C, 8, 16), 7.0, device=dev)
    args = [_lib.ptr(x), _lib.ptr(packed), _lib.ptr(ab), _lib.ptr(ab), _lib.ptr(bits), _lib.ptr(y)]
    for cin, cout in ((256, 256), (512, 256), (256, 512), (1024, 1024), (64, 64), (512, 2048)):
        for s in (1, 2):
            assert L.orp_conv3x3_bn_deep_ok(cin, cout, s) == 0 and L.orp_conv3x3_bn_deep_pays(cin, cout, 32, 32, s, 1) == 0
        assert L.orp_conv3x3_bn_deep_packed_bytes(cin, cout) == 0
        assert L.orp_conv3x3_bn_deep_pack_weight(_lib.ptr(conv.weight.detach()), cin, cout, _lib.ptr(packed), _lib.stream_of(x)) == _lib.ORP_EINVAL
        assert L.orp_conv3x3_bn_deep(*args, 1, cin, cout, 8, 16, 1, 1, _lib.stream_of(x)) == _lib.ORP_EINVAL
    for s in (0, 3, 4):
        assert L.orp_conv3x3_bn_deep(*args, 1, C, C, 8, 16, s, 1, _lib.stream_of(x)) == _lib.ORP_EINVAL
    for k in range(6):
        bad = list(args)
        bad[k] = None
        assert L.orp_conv3x3_bn_deep(*bad, 1, C, C, 8, 16, 1, 1, _lib.stream_of(x)) == _lib.ORP_EINVAL
    args[5] = _lib.ptr(x)
    assert L.orp_conv3x3_bn_deep(*args, 1, C, C, 8, 16, 1, 1, _lib.stream_of(x)) == _lib.ORP_EINVAL
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


@pytest.mark.parametrize("stride,B,h,w", [(1, 2, 3, 17), (2, 2, 7, 35)])
def test_random_data_inside_the_derived_bound(dev, stride, B, h, w):
    """N(0, 1) activations through a ReLU, He-scale weights, salted BatchNorm constants, against float64 conv + affine + ReLU inside
    (9 Cin + 2) 2^-24 (|a| sum |x_k w_k| + |b|), and the worst |err| / bound no more than twice the library path's (conv + bn_act) on
    the same inputs -- the library is the yardstick, the factor two is for the other summation order.  The ratios are taken over the
    outputs whose bound is a finite normal number and whose float64 value plus bound is inside fp32 (the salted channels with a
    non-finite constant, the subnormal scale and the overflowing scale have no such bound); on all others the result has to be
    non-finite exactly where the affine pass on the float64 convolution is."""
    import conftest
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine, bn_act
    conv, bn = _conv3(dev, 40 + stride, stride), base._bn(C, dev, 41, salted=True)
    g = torch.Generator(device=dev).manual_seed(C + stride)
    x = torch.relu(torch.randn((B, C, h, w), device=dev, generator=g))
    with torch.no_grad():
        a, b = [t.double() for t in _bn_affine(bn)]
        ref = _ref64(x, conv, bn, True)
        bound = _bound(x, conv, a, b, None)
        got = _deep(x, conv, bn, True)
        lib = bn_act(conv(x).contiguous(), bn, relu=True)
        aff = _want(x, conv, bn, True)
    ok = torch.isfinite(bound) & (bound >= 2.0 ** -126) & torch.isfinite(ref) & (ref.abs() + bound < 3.0e38)
    assert int(ok.sum()) >= ok.numel() * (C - 8) // C
    ours = float(((got.double() - ref).abs() / bound)[ok].max())
    theirs = float(((lib.double() - ref).abs() / bound)[ok].max())
    line = ("3x3 convolution + BatchNorm + ReLU 512 -> 512 stride %d at %d x %d x %d, worst |err| / bound vs float64: K-split fp16-pieces "
            "%.3g, library + pass %.3g" % (stride, B, h, w, ours, theirs))
    print(line)
    conftest.REPORT.append(line)
    assert ours <= 1.0
    assert ours <= 2.0 * theirs
    rest = ~ok
    assert bool((torch.isnan(got[rest]) == torch.isnan(aff[rest])).all())
    assert bool((torch.isinf(got[rest]) == torch.isinf(aff[rest])).all())


def _floor_term(x, conv, a):
    """|a| 2^-37 max|x| sum_k |w_k| per output channel: the fp16 subnormal floor of the activations' low pieces next to an outlier
    (test_gpu_conv3x3_bn.py)"""
    mx = float(x.abs().max())
    return (a.abs() * conv.weight.detach().double().abs().flatten(1).sum(1) * (2.0 ** -37 * mx)).view(1, -1, 1, 1)


@pytest.mark.parametrize("stride,h,w", [(1, 3, 17), (2, 5, 33)])
@pytest.mark.parametrize("case", ["outlier", "tiny", "huge"])
def test_range_edges_inside_the_bound(dev, case, stride, h, w):
    """as test_gpu_conv3x3_bn.py: one element 2^15 times the rest (the floor term is added to the bound, in this case only); maxima
    near 2^-120 and near 2^100 inside the plain bound.  BatchNorm without a shift, no ReLU"""
    import conftest
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine
    conv, bn = _conv3(dev, 60, stride), base._bn(C, dev, 61)
    with torch.no_grad():
        bn.running_mean.zero_(); bn.bias.zero_()                                                # shift = 0
    g = torch.Generator(device=dev).manual_seed(62)
    x = torch.relu(torch.randn((2, C, h, w), device=dev, generator=g)) + 0.01
    if case == "outlier":
        x[1, 300, h // 2, w // 2] = float(x.max()) * 2.0 ** 15
    elif case == "tiny":
        x = x * 2.0 ** -122
    else:
        x = x * 2.0 ** 98
    with torch.no_grad():
        a, b = [t.double() for t in _bn_affine(bn)]
        ref = _ref64(x, conv, bn, False)
        bound = _bound(x, conv, a, b, None)
        if case == "outlier":
            bound = bound + _floor_term(x, conv, a)
        got = _deep(x, conv, bn, False)
    assert bool(torch.isfinite(got).all())
    ratio = float(((got.double() - ref).abs() / bound).max())
    conftest.REPORT.append("3x3 K-split fp16-pieces convolution stride %d, range edge '%s' (max |x| %.3g): worst |err| / bound %.3f"
                           % (stride, case, float(x.abs().max()), ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("stride,h,w", [(1, 5, 19), (2, 9, 37)])
def test_inf_and_nan_reach_the_windows_that_read_them_and_no_other(dev, exact, stride, h, w):
    """one +Inf (channel below 256, at the top edge) and one NaN (channel above, across the tile seam) in integer data: the range word
    skips them, every output whose window reads neither is the exact result bit for bit, every output whose window reads one (all
    channels) is non-finite"""
    import torch.nn.functional as F
    conv, bn = exact[0][stride], base._bn(C, dev, 71)
    x = _ints((2, C, h, w), dev, 72)
    clean = x.clone()
    spots = [(0, 3, 0, 5, float('inf')), (1, 400, h - 2, w - 3, float('nan'))]
    mark = torch.zeros((2, 1, h, w), device=dev)
    for (b, ch, yy, xx, v) in spots:
        x[b, ch, yy, xx] = v
        mark[b, 0, yy, xx] = 1.0
    touched = F.conv2d(mark, torch.ones((1, 1, 3, 3), device=dev), stride=stride, padding=1) > 0
    assert int(_range_bits(x).item()) == int(_range_bits(clean).item())
    with torch.no_grad():
        want = _want(clean, conv, bn, False)
        got = _deep(x, conv, bn, False)
    t = touched.expand_as(got)
    assert int(t.sum()) > 0 and bool((~torch.isfinite(got[t])).all())
    assert np.array_equal(_bits(got[~t]), _bits(want[~t]))


@pytest.mark.parametrize("stride,h,w", [(1, 5, 33), (2, 9, 37)])
def test_same_launch_twice_gives_the_same_bits(dev, stride, h, w):
    conv, bn = _conv3(dev, 1, stride), base._bn(C, dev, 2)
    x = torch.relu(torch.randn((2, C, h, w), device=dev, generator=torch.Generator(device=dev).manual_seed(4)))
    with torch.no_grad():
        assert _same_bits(_deep(x, conv, bn), _deep(x, conv, bn))


def test_a_tile_does_not_depend_on_its_place_in_the_grid(dev):
    """an output's value does not depend on its tile or on the grid: a map's top-left tile computed alone (the map cropped to what
    that tile reads, the crop's border rows and columns zeroed like padding is) gives the bits it has inside the larger launch"""
    conv, bn = _conv3(dev, 3, 1), base._bn(C, dev, 4)
    x = torch.relu(torch.randn((1, C, 6, 40), device=dev, generator=torch.Generator(device=dev).manual_seed(5)))
    x[:, :, 2, :] = 0; x[:, :, :, 16] = 0                  # what lies below / right of the tile acts like padding
    with torch.no_grad():
        big = _deep(x, conv, bn)
        small = _deep(x[:, :, :2, :16].contiguous(), conv, bn, bits=_range_bits(x))
    assert _same_bits(big[:, :, :2, :16], small)


def _pin_the_library(monkeypatch):
    """what a block test compares bit for bit must not change from call to call: conv1 / conv3 on the fp32 kernel at every shape
    (test_gpu_conv1x1_bn.py: _force_fused) and the library's remaining convolutions held to its deterministic algorithms"""
    base._force_fused(monkeypatch)
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)


def _stage4_block(dev, stride):
    if stride == 1:
        return base._bottleneck(dev, 2048, 512), 2048
    ds = torch.nn.Sequential(torch.nn.Conv2d(1024, 2048, 1, stride=2, bias=False), torch.nn.BatchNorm2d(2048))
    return base._bottleneck(dev, 1024, 512, stride=2, downsample=ds), 1024


@pytest.mark.parametrize("stride,h,w", [(1, 6, 20), (2, 7, 35)])
def test_bottleneck_switch(dev, monkeypatch, stride, h, w):
    """a forced stage-4 block: with the switch on one new launch and none of the first route's; with it off no new launch and the bits of
    the library path (the parent's calls made by hand); `force_conv3x3` does not touch the new route"""
    from orientedreppoints_amd.mmdet_ops import fused_norm
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act
    _pin_the_library(monkeypatch)
    conv1x1_bn_act = fused_norm.conv1x1_bn_act
    calls, first = _spy(monkeypatch), _spy(monkeypatch, 'orp_conv3x3_bn_act')
    blk, cin = _stage4_block(dev, stride)
    x = torch.randn(2, cin, h, w, device=dev)
    with torch.no_grad():
        blk.force_conv3x3 = True
        blk(x.clone())
        assert len(calls) == 0 and len(first) == 0           # the table is closed around the timed maps, and this map is none
        del blk.force_conv3x3
        blk.force_conv3x3_deep = True
        on = blk(x.clone())
        assert len(calls) == 1 and len(first) == 0 and calls[0][6:12] == (2, C, C, h, w, stride)
        blk.fuse_conv3x3_deep = False
        assert not blk._conv3x3_deep_fusable()
        off = blk(x.clone())
        assert len(calls) == 1
        # the library path, by hand
        t = conv1x1_bn_act(x, blk.conv1, blk.bn1, relu=True)
        t = bn_act(blk.conv2(t).contiguous(), blk.bn2, relu=True)
        ds = blk.downsample
        if ds is not None:
            res, res_bn, r = ds[0](x).contiguous(), ds[1], ds[1](ds[0](x))
        else:
            res, res_bn, r = x.contiguous(), None, x
        hand = conv1x1_bn_act(t, blk.conv3, blk.bn3, residual=res, residual_bn=res_bn, relu=True)
        assert _same_bits(off, hand)
        del blk.fuse_conv3x3_deep
        assert blk._conv3x3_deep_fusable()                      # default: on
        # on and off agree inside the bounds carried through the block (test_gpu_conv3x3_bn.py)
        t1 = torch.relu(blk.bn1(blk.conv1(x)))
        t2 = torch.relu(blk.bn2(blk.conv2(t1)))
        d = 2 * base._stage_bound(x, blk.conv1, blk.bn1)
        d = d * base._gain(blk.conv2, blk.bn2) + 2 * base._stage_bound(t1, blk.conv2, blk.bn2)
        d = d * base._gain(blk.conv3, blk.bn3) + 2 * base._stage_bound(t2, blk.conv3, blk.bn3, r)
    diff = float((on - off).abs().max())
    assert 0.0 < diff <= d
    n0 = len(calls)
    with torch.enable_grad():
        stock = blk(x.clone())                                  # autograd on: the unfused module path
    assert len(calls) == n0 and stock.requires_grad


def test_routing_query_is_asked_before_conv1_and_force_bypasses_it(dev, monkeypatch):
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops import fused_norm
    L = _lib.lib()
    calls = _spy(monkeypatch)
    events, answer = [], [0]

    def pays(*args):
        events.append(('pays',) + args)
        return answer[0]
    monkeypatch.setattr(L, 'orp_conv3x3_bn_deep_pays', pays)
    conv1x1 = fused_norm.conv1x1_bn_act

    def conv1(*args, **kw):
        events.append(('conv1x1', bool(kw.get('want_range'))))
        return conv1x1(*args, **kw)
    monkeypatch.setattr(fused_norm, 'conv1x1_bn_act', conv1)
    conv, bn = _conv3(dev, 1), base._bn(C, dev, 2)
    x = torch.relu(torch.randn(2, C, 4, 24, device=dev))
    bits = _range_bits(x)
    with torch.no_grad():
        y = fused_norm.conv3x3_bn_deep(x, conv, bn, range_bits=bits)     # does not pay: library + pass
        assert events == [('pays', C, C, 4, 24, 1, 2)] and len(calls) == 0 and y.shape == x.shape
        answer[0] = 1
        fused_norm.conv3x3_bn_deep(x, conv, bn, range_bits=bits)         # pays: the new launch
        assert len(calls) == 1
        fused_norm.conv3x3_bn_deep(x, conv, bn)                          # the input's range is not known: library + pass
        assert len(calls) == 1
        answer[0] = 0
        n = len(events)
        fused_norm.conv3x3_bn_deep(x, conv, bn, force=True, range_bits=bits)   # forced: not asked
        assert len(events) == n and len(calls) == 2
        for stride, (h, w) in ((1, (4, 24)), (2, (7, 35))):
            blk, cin = _stage4_block(dev, stride)
            xin = torch.randn(2, cin, h, w, device=dev)
            del events[:]
            blk(xin)                                                     # asked in front of conv1, with conv2's input shape; no
            assert events[0] == ('pays', C, C, h, w, stride, 2) and events[1] == ('conv1x1', False)
            assert len(calls) == 2
            answer[0] = 1
            del events[:]
            blk(xin)                                                     # yes: conv1 leaves the range word, conv2 is the new launch
            assert events[0] == ('pays', C, C, h, w, stride, 2) and events[1] == ('conv1x1', True)
            assert len(calls) == 3
            calls.pop()
            answer[0] = 0


# the timed corners (INPUT map side at a 1024^2 image per stride): one image from the 1024^2 map to the 1536^2 map, two at the 1024^2 map
CORNERS = {1: 32, 2: 64}


def test_the_routing_table_is_closed():
    """nothing beyond the timed corners is routed: smaller or larger maps, more than two images, two images off the 1024^2 map, the timed
    area in another shape, the other stride's map"""
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    for s, side in CORNERS.items():
        big = side * 3 // 2
        routed = [L.orp_conv3x3_bn_deep_pays(C, C, side, side, s, 1), L.orp_conv3x3_bn_deep_pays(C, C, big, big, s, 1),
                  L.orp_conv3x3_bn_deep_pays(C, C, side, side, s, 2)]
        assert L.orp_conv3x3_bn_deep_pays(C, C, side - 1, side, s, 1) == 0
        assert L.orp_conv3x3_bn_deep_pays(C, C, big + 1, big, s, 1) == 0
        assert L.orp_conv3x3_bn_deep_pays(C, C, side, side, s, 3) == 0
        assert L.orp_conv3x3_bn_deep_pays(C, C, big, big, s, 2) == 0
        assert L.orp_conv3x3_bn_deep_pays(C, C, 1, side * side, s, 1) == 0
        assert L.orp_conv3x3_bn_deep_pays(C, C, side // 4, side * 4, s, 1) == 0
        assert L.orp_conv3x3_bn_deep_pays(C, C, side, side, 3 - s, 1) == 0
        assert L.orp_conv3x3_bn_deep_pays(C, C, side, side, 3, 1) == 0
        # between two timed corners that both paid a map is routed, and only there
        assert L.orp_conv3x3_bn_deep_pays(C, C, side, big, s, 1) == (1 if routed[0] and routed[1] else 0)
        assert routed == ROUTED[s]


# what the timing runs of docs/notebook/round23.md gave: (1024^2 map one image, 1536^2 map one image, 1024^2 map two images) per stride
ROUTED = {1: [1, 1, 1], 2: [1, 1, 1]}


@pytest.mark.parametrize("stride,h,w", [(1, 6, 20), (2, 7, 35)])
def test_captured_bottleneck_replays_the_eager_bits(dev, monkeypatch, stride, h, w):
    """a captured stage-4 block replays the eager bits for NEW input contents whose range is smaller than what the capture saw"""
    _pin_the_library(monkeypatch)
    calls = _spy(monkeypatch)
    blk, cin = _stage4_block(dev, stride)
    blk.force_conv3x3_deep = True
    xa = torch.randn(2, cin, h, w, device=dev) * 64
    xb = torch.randn(2, cin, h, w, device=dev) * 0.37
    with torch.no_grad():
        eager = {k: blk(v).clone() for k, v in (('a', xa), ('b', xb))}
        assert len(calls) == 2
        x = xa.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            blk(x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = blk(x)
        for k, v in (('a', xa), ('b', xb), ('a', xa), ('b', xb)):
            x.copy_(v)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert _same_bits(out, eager[k]), k
