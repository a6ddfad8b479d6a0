"""GPU: the stride-2 3x3 convolution of stage 2 / stage 3 block 0 (128 -> 128 and 256 -> 256 channels) on the narrow-pass fp16-pieces
kernel with BatchNorm + ReLU in its epilogue (orp_conv3x3_bn_s2).

Exact cases (small-integer activations and weights: every piece, product and partial sum is exact in any order, 9 * 256 * 15 * 7 < 2^24)
bit for bit against the float64 convolution cast to fp32 followed by the affine pass, over the smallest maps that reach every seam of
the 2 x 16 tile and both parities of height and width; the K-group and staging-pass seams (a workgroup's two K groups are the halves
of the input channels, a staging pass is 32 channels of each half), every tap, a single pixel at every parity of the de-interleaved
halo next to a tile seam and at the image border, the output-channel seams of the waves and workgroups; random data against float64
inside the derived bound and within twice the library path's share on the same inputs; the range edges, Inf / NaN, reproducibility,
graph replay, the switch, the routing query and the closed table.

The figures of the random cases on MI355X are in docs/notebook/round24.md."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_conv1x1_bn as base  # noqa: E402

_bits, _same_bits, _conv64, _bound = base._bits, base._same_bits, base._conv64, base._bound
CS = (128, 256)
# (images, INPUT H, W): 1 x 1 outputs (1 x 1 and 2 x 2 inputs), exactly one 2 x 16 tile (4 x 32 and 3 x 31), one output more each way
# (5 x 33 and 6 x 34 -> 3 x 17), one row and one column; heights and widths of both parities, one and three images
LAYOUTS = [(1, 1, 1), (3, 2, 2), (1, 4, 32), (3, 3, 31), (1, 5, 33), (3, 6, 34), (1, 1, 40), (1, 40, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _conv3(dev, C, seed, integer=False):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(C, C, 3, stride=2, padding=1, bias=False)
    with torch.no_grad():
        if integer:
            conv.weight.copy_(torch.randint(-7, 8, (C, C, 3, 3), generator=g).float())
        else:
            conv.weight.copy_(torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5)      # He scale
    return conv.to(dev).eval()


@pytest.fixture(scope="module")
def exact(dev):
    """integer weights and the salted BatchNorm (non-finite constants, signed zeros, a subnormal scale) per C, made once"""
    return {C: (_conv3(dev, C, 100 + C, integer=True), base._bn(C, dev, 7, salted=True)) for C in CS}


def _range_bits(x):
    """max over the finite elements of |x| as float bits (orp_range.hpp: range_bits), a one-element int32 tensor"""
    a = x.detach().abs()
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    return a.max().reshape(1).contiguous().view(torch.int32)


def _spy(monkeypatch, name='orp_conv3x3_bn_s2'):
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    orig = getattr(L, name)
    calls = []

    def spy(*args):
        calls.append(args)
        return orig(*args)
    monkeypatch.setattr(L, name, spy)
    return calls


def _s2(x, conv, bn, relu=True, bits=None):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv3x3_bn_s2
    return conv3x3_bn_s2(x, conv, bn, relu=relu, force=True, range_bits=_range_bits(x) if bits is None else bits)


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
        got = _s2(x, conv, bn, relu)
        assert got.shape == want.shape and got.is_contiguous() and got.data_ptr() != x.data_ptr()
        assert _same_bits(got, want), tag + (relu, int((_bits(got) != _bits(want)).sum()))


@pytest.mark.parametrize("B,h,w", LAYOUTS)
@pytest.mark.parametrize("C", CS)
def test_exact_cases_bit_for_bit(dev, monkeypatch, exact, C, B, h, w):
    """integers |x| <= 15, |w| <= 7, every layout, ReLU off and on, salted BatchNorm constants"""
    calls = _spy(monkeypatch)
    conv, bn = exact[C]
    with torch.no_grad():
        _check(_ints((B, C, h, w), dev, 7 * h + w + C), conv, bn, (C, B, h, w))
    assert len(calls) == 2 and calls[0][6:11] == (B, C, C, h, w)


def _channel_sets(C):
    """the input channels of each K group (the halves) and of each staging pass (32 channels of each half)"""
    half = C // 2
    sets = [("k%d" % g, [(g * half, (g + 1) * half)]) for g in range(2)]
    sets += [("pass%d" % s, [(32 * s, 32 * s + 32), (half + 32 * s, half + 32 * s + 32)]) for s in range(C // 64)]
    return sets


@pytest.mark.parametrize("C,name,spans", [(C, n, s) for C in CS for n, s in _channel_sets(C)])
def test_each_k_group_and_each_staging_pass_alone(dev, exact, C, name, spans):
    """data that is non-zero only in the input channels of one K group, and of one staging pass: the others add exact zeros"""
    conv, bn = exact[C]
    full = _ints((1, C, 7, 35), dev, 31 + len(name) + spans[0][0])
    x = torch.zeros_like(full)
    for lo, hi in spans:
        x[:, lo:hi] = full[:, lo:hi]
    with torch.no_grad():
        _check(x, conv, bn, (C, name))


@pytest.mark.parametrize("C", CS)
def test_single_tap_weights(dev, exact, C):
    """the weight non-zero at one tap only, for each of the nine"""
    full, bn = exact[C]
    x = _ints((1, C, 5, 33), dev, 41)
    conv = _conv3(dev, C, 1, integer=True)
    with torch.no_grad():
        for tap in range(9):
            conv.weight.zero_()
            conv.weight[:, :, tap // 3, tap % 3] = full.weight[:, :, tap // 3, tap % 3]
            _check(x, conv, bn, (C, tap))


@pytest.mark.parametrize("where", ["seam", "top-left", "bottom-right"])
@pytest.mark.parametrize("py,px", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("C", CS)
def test_single_pixel_inputs_at_each_parity(dev, exact, C, py, px, where):
    """one non-zero input pixel (all channels) at each (row parity, column parity) of the de-interleaved halo: next to a tile seam in
    both directions (7 x 35 input = 4 x 18 outputs: the pixel's window reaches two tile rows and two tile columns) and in the image's
    corners, where its windows also read the padding"""
    conv, bn = exact[C]
    yy, xx = {"seam": (3 + py, 31 + px), "top-left": (py, px), "bottom-right": (6 - py, 34 - px)}[where]
    x = torch.zeros((1, C, 7, 35), device=dev)
    x[0, :, yy, xx] = _ints((C,), dev, 51 + 2 * py + px)
    x[0, 0, yy, xx] = 15.0
    with torch.no_grad():
        _check(x, conv, bn, (C, py, px, where))


@pytest.mark.parametrize("C", CS)
def test_output_channels_at_the_wave_and_workgroup_seams(dev, C):
    """output channels 31 / 32, 63 / 64, 95 / 96 belong to different waves, 127 / 128 (C = 256) to different workgroups of a tile: each
    output channel o copies (o % 7 + 1) x input channel o, so that a value written to a neighbouring channel is a different value"""
    conv, bn = _conv3(dev, C, 1, integer=True), base._bn(C, dev, 9)
    seams = [s for s in (31, 63, 95, 127, 159, 191, 223) if s + 1 < C]
    with torch.no_grad():
        conv.weight.zero_()
        o = torch.arange(C, device=dev)
        conv.weight[o, o, 1, 1] = (o % 7 + 1).float()
        x = _ints((1, C, 4, 32), dev, 61).abs() + 1
        for relu in (False, True):
            want, got = _want(x, conv, bn, relu), _s2(x, conv, bn, relu)
            for lo in seams:
                assert _same_bits(got[:, lo], want[:, lo]) and _same_bits(got[:, lo + 1], want[:, lo + 1]), (C, lo, relu)
            assert _same_bits(got, want)
        raw = _conv64(x, conv)
        for lo in seams:
            assert bool((raw[:, lo] != raw[:, lo + 1]).any())


def test_unsupported_shapes_are_rejected(dev):
    """`_ok` refuses every pair but (128, 128) and (256, 256); the launcher returns ORP_EINVAL and writes nothing"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import _packed_3x3_s2_planes
    L = _lib.lib()
    C = 128
    x = torch.randn(1, C, 8, 16, device=dev)
    conv = _conv3(dev, C, 2)
    packed, ab, bits = _packed_3x3_s2_planes(conv.weight), torch.ones(C, device=dev), _range_bits(x)
    assert packed.numel() == 4 * C * C * 9 + 16 == L.orp_conv3x3_bn_s2_packed_bytes(C, C)
    y = torch.full((1, C, 4, 8), 7.0, device=dev)
    args = [_lib.ptr(x), _lib.ptr(packed), _lib.ptr(ab), _lib.ptr(ab), _lib.ptr(bits), _lib.ptr(y)]
    for cin, cout in ((64, 64), (128, 256), (256, 128), (512, 512), (192, 192), (0, 0), (-128, -128)):
        assert L.orp_conv3x3_bn_s2_ok(cin, cout) == 0 and L.orp_conv3x3_bn_s2_pays(cin, cout, 256, 256, 1) == 0
        assert L.orp_conv3x3_bn_s2_packed_bytes(cin, cout) == 0
        assert L.orp_conv3x3_bn_s2_pack_weight(_lib.ptr(conv.weight.detach()), cin, cout, _lib.ptr(packed), _lib.stream_of(x)) == _lib.ORP_EINVAL
        assert L.orp_conv3x3_bn_s2(*args, 1, cin, cout, 8, 16, 1, _lib.stream_of(x)) == _lib.ORP_EINVAL
    for b, h, w in ((0, 8, 16), (-1, 8, 16), (1, 0, 16), (1, 8, -2)):
        assert L.orp_conv3x3_bn_s2(*args, b, C, C, h, w, 1, _lib.stream_of(x)) == _lib.ORP_EINVAL
    for k in range(6):
        bad = list(args)
        bad[k] = None
        assert L.orp_conv3x3_bn_s2(*bad, 1, C, C, 8, 16, 1, _lib.stream_of(x)) == _lib.ORP_EINVAL
    args[5] = _lib.ptr(x)
    assert L.orp_conv3x3_bn_s2(*args, 1, C, C, 8, 16, 1, _lib.stream_of(x)) == _lib.ORP_EINVAL
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


@pytest.mark.parametrize("C", CS)
def test_random_data_inside_the_derived_bound(dev, C):
    """N(0, 1) activations through a ReLU, He-scale weights, salted BatchNorm constants, against float64 conv + affine + ReLU inside
    (9 Cin + 2) 2^-24 (|a| sum |x_k w_k| + |b|), and the worst |err| / bound no more than twice the library path's (conv + bn_act) on
    the same inputs -- the library is the yardstick, the factor two is for the other summation order (the project's rule, rounds 15
    and 23).  The shares are taken over the outputs whose bound is a finite normal number and whose float64 value plus bound is inside
    fp32; on all others the result has to be non-finite exactly where the affine pass on the float64 convolution is."""
    import conftest
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine, bn_act
    B, h, w = 2, 7, 35
    conv, bn = _conv3(dev, C, 40), base._bn(C, dev, 41, salted=True)
    g = torch.Generator(device=dev).manual_seed(C + 2)
    x = torch.relu(torch.randn((B, C, h, w), device=dev, generator=g))
    with torch.no_grad():
        a, b = [t.double() for t in _bn_affine(bn)]
        ref = _ref64(x, conv, bn, True)
        bound = _bound(x, conv, a, b, None)
        got = _s2(x, conv, bn, True)
        lib = bn_act(conv(x).contiguous(), bn, relu=True)
        aff = _want(x, conv, bn, True)
    ok = torch.isfinite(bound) & (bound >= 2.0 ** -126) & torch.isfinite(ref) & (ref.abs() + bound < 3.0e38)
    assert int(ok.sum()) >= ok.numel() * (C - 8) // C
    ours = float(((got.double() - ref).abs() / bound)[ok].max())
    theirs = float(((lib.double() - ref).abs() / bound)[ok].max())
    line = ("3x3 convolution + BatchNorm + ReLU %d -> %d stride 2 at %d x %d x %d, worst |err| / bound vs float64: narrow-pass fp16-pieces "
            "%.3g, library + pass %.3g" % (C, C, B, h, w, ours, theirs))
    print(line)
    conftest.REPORT.append(line)
    assert ours <= 1.0
    assert ours <= 2.0 * theirs
    rest = ~ok
    assert bool((torch.isnan(got[rest]) == torch.isnan(aff[rest])).all())
    assert bool((torch.isinf(got[rest]) == torch.isinf(aff[rest])).all())


def _floor_term(x, conv, a):
    """|a| 2^-37 max|x| sum_k |w_k| per output channel: the fp16 subnormal floor of the activations' low pieces next to an outlier
    (test_gpu_conv3x3_bn.py, round 15)"""
    mx = float(x.abs().max())
    return (a.abs() * conv.weight.detach().double().abs().flatten(1).sum(1) * (2.0 ** -37 * mx)).view(1, -1, 1, 1)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("case", ["outlier", "tiny", "huge"])
def test_range_edges_inside_the_bound(dev, case, C):
    """as test_gpu_conv3x3_bn.py: one element 2^15 times the rest (the floor term is added to the bound, in this case only); maxima
    near 2^-120 and near 2^100 inside the plain bound.  BatchNorm without a shift, no ReLU"""
    import conftest
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine
    h, w = 5, 33
    conv, bn = _conv3(dev, C, 60), base._bn(C, dev, 61)
    with torch.no_grad():
        bn.running_mean.zero_(); bn.bias.zero_()                                                # shift = 0
    g = torch.Generator(device=dev).manual_seed(62)
    x = torch.relu(torch.randn((2, C, h, w), device=dev, generator=g)) + 0.01
    if case == "outlier":
        x[1, C - 28, h // 2, w // 2] = float(x.max()) * 2.0 ** 15
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
        got = _s2(x, conv, bn, False)
    assert bool(torch.isfinite(got).all())
    ratio = float(((got.double() - ref).abs() / bound).max())
    line = ("3x3 narrow-pass fp16-pieces convolution %d channels stride 2, range edge '%s' (max |x| %.3g): worst |err| / bound %.3f"
            % (C, case, float(x.abs().max()), ratio))
    print(line)
    conftest.REPORT.append(line)
    assert ratio <= 1.0


@pytest.mark.parametrize("C", CS)
def test_inf_and_nan_reach_the_windows_that_read_them_and_no_other(dev, exact, C):
    """one +Inf (a channel of K group 0, at the top edge) and one NaN (a channel of K group 1, across the tile seam) in integer data: the
    range word skips them, every output whose window reads neither is the exact result bit for bit, every output whose window reads
    one (all channels) is non-finite"""
    import torch.nn.functional as F
    h, w = 9, 37
    conv, bn = exact[C][0], base._bn(C, dev, 71)
    x = _ints((2, C, h, w), dev, 72)
    clean = x.clone()
    spots = [(0, 3, 0, 5, float('inf')), (1, C - 20, h - 2, w - 3, float('nan'))]
    mark = torch.zeros((2, 1, h, w), device=dev)
    for (b, ch, yy, xx, v) in spots:
        x[b, ch, yy, xx] = v
        mark[b, 0, yy, xx] = 1.0
    touched = F.conv2d(mark, torch.ones((1, 1, 3, 3), device=dev), stride=2, padding=1) > 0
    assert int(_range_bits(x).item()) == int(_range_bits(clean).item())
    with torch.no_grad():
        want = _want(clean, conv, bn, False)
        got = _s2(x, conv, bn, False)
    t = touched.expand_as(got)
    assert int(t.sum()) > 0 and bool((~torch.isfinite(got[t])).all())
    assert np.array_equal(_bits(got[~t]), _bits(want[~t]))


@pytest.mark.parametrize("C", CS)
def test_same_launch_twice_gives_the_same_bits(dev, C):
    conv, bn = _conv3(dev, C, 1), base._bn(C, dev, 2)
    x = torch.relu(torch.randn((2, C, 9, 37), device=dev, generator=torch.Generator(device=dev).manual_seed(4)))
    with torch.no_grad():
        assert _same_bits(_s2(x, conv, bn), _s2(x, conv, bn))


@pytest.mark.parametrize("C", CS)
def test_a_tile_does_not_depend_on_its_place_in_the_grid_or_the_batch(dev, C):
    """an output's value does not depend on its tile, on the grid or on the batch: the top-left tile of the middle image of three,
    computed alone (the map cropped to the 3 x 31 inputs whose windows give that tile, what lies below / right of them zeroed like
    padding is), gives the bits it has inside the larger launch"""
    conv, bn = _conv3(dev, C, 3), base._bn(C, dev, 4)
    x = torch.relu(torch.randn((3, C, 9, 70), device=dev, generator=torch.Generator(device=dev).manual_seed(5)))
    x[:, :, 3, :] = 0; x[:, :, :, 31] = 0
    with torch.no_grad():
        big = _s2(x, conv, bn)
        small = _s2(x[1:2, :, :3, :31].contiguous(), conv, bn, bits=_range_bits(x))
        one = _s2(x[1:2].contiguous(), conv, bn, bits=_range_bits(x))
    assert small.shape[2:] == (2, 16)
    assert _same_bits(big[1:2, :, :2, :16], small)
    assert _same_bits(big[1:2], one)


def _pin_the_library(monkeypatch):
    """what a block test compares bit for bit must not change from call to call: conv1 / conv3 on the fp32 kernel at every shape
    (test_gpu_conv1x1_bn.py: _force_fused) and the library's remaining convolutions held to its deterministic algorithms"""
    base._force_fused(monkeypatch)
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)


def _block0(dev, C):
    """block 0 of stage 2 (C = 128) or stage 3 (C = 256): 2 C -> C -> 4 C channels, stride 2 in conv2 and the downsample"""
    ds = torch.nn.Sequential(torch.nn.Conv2d(2 * C, 4 * C, 1, stride=2, bias=False), torch.nn.BatchNorm2d(4 * C))
    return base._bottleneck(dev, 2 * C, C, stride=2, downsample=ds), 2 * C


@pytest.mark.parametrize("C", CS)
def test_bottleneck_switch(dev, monkeypatch, C):
    """a forced stride-2 block: with the switch on one new launch and none of the other routes'; with it off no new launch and the bits
    of the library path (the parent's calls made by hand); `force_conv3x3` / `force_conv3x3_deep` do not touch the new route"""
    from orientedreppoints_amd.mmdet_ops import fused_norm
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act
    _pin_the_library(monkeypatch)
    conv1x1_bn_act = fused_norm.conv1x1_bn_act
    calls, first, second = _spy(monkeypatch), _spy(monkeypatch, 'orp_conv3x3_bn_act'), _spy(monkeypatch, 'orp_conv3x3_bn_deep')
    blk, cin = _block0(dev, C)
    h, w = 7, 35
    x = torch.randn(2, cin, h, w, device=dev)
    with torch.no_grad():
        blk(x.clone())
        assert len(calls) == 0                                  # the table is closed around the timed maps, and this map is none
        blk.force_conv3x3 = True
        blk.force_conv3x3_deep = True
        blk(x.clone())
        assert len(calls) == 0 and len(first) == 0 and len(second) == 0
        del blk.force_conv3x3, blk.force_conv3x3_deep
        blk.force_conv3x3_s2 = True
        on = blk(x.clone())
        assert len(calls) == 1 and len(first) == 0 and len(second) == 0 and calls[0][6:11] == (2, C, C, h, w)
        blk.fuse_conv3x3_s2 = False
        assert not blk._conv3x3_s2_fusable()
        off = blk(x.clone())
        assert len(calls) == 1
        # the library path, by hand
        t = conv1x1_bn_act(x, blk.conv1, blk.bn1, relu=True)
        t = bn_act(blk.conv2(t).contiguous(), blk.bn2, relu=True)
        ds = blk.downsample
        res, res_bn, r = ds[0](x).contiguous(), ds[1], ds[1](ds[0](x))
        hand = conv1x1_bn_act(t, blk.conv3, blk.bn3, residual=res, residual_bn=res_bn, relu=True)
        assert _same_bits(off, hand)
        del blk.fuse_conv3x3_s2
        assert blk._conv3x3_s2_fusable()                        # default: on
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
    C = 128
    calls = _spy(monkeypatch)
    events, answer = [], [0]

    def pays(*args):
        events.append(('pays',) + args)
        return answer[0]
    monkeypatch.setattr(L, 'orp_conv3x3_bn_s2_pays', pays)
    conv1x1 = fused_norm.conv1x1_bn_act

    def conv1(*args, **kw):
        events.append(('conv1x1', bool(kw.get('want_range'))))
        return conv1x1(*args, **kw)
    monkeypatch.setattr(fused_norm, 'conv1x1_bn_act', conv1)
    conv, bn = _conv3(dev, C, 1), base._bn(C, dev, 2)
    x = torch.relu(torch.randn(2, C, 5, 24, device=dev))
    bits = _range_bits(x)
    with torch.no_grad():
        y = fused_norm.conv3x3_bn_s2(x, conv, bn, range_bits=bits)       # does not pay: library + pass
        assert events == [('pays', C, C, 5, 24, 2)] and len(calls) == 0 and y.shape == (2, C, 3, 12)
        answer[0] = 1
        fused_norm.conv3x3_bn_s2(x, conv, bn, range_bits=bits)           # pays: the new launch
        assert len(calls) == 1
        fused_norm.conv3x3_bn_s2(x, conv, bn)                            # the input's range is not known: library + pass
        assert len(calls) == 1
        answer[0] = 0
        n = len(events)
        fused_norm.conv3x3_bn_s2(x, conv, bn, force=True, range_bits=bits)   # forced: not asked
        assert len(events) == n and len(calls) == 2
        # a stride-1 convolution of the same channels is not this route's
        conv_s1 = torch.nn.Conv2d(C, C, 3, stride=1, padding=1, bias=False).to(dev).eval()
        assert not fused_norm.conv3x3_bn_s2_routed(x, conv_s1, bn, force=True)
        for Cb in CS:
            blk, cin = _block0(dev, Cb)
            h, w = 7, 35
            xin = torch.randn(2, cin, h, w, device=dev)
            del events[:]
            n = len(calls)
            blk(xin)                                                     # asked in front of conv1, with conv2's input shape; no
            assert events[0] == ('pays', Cb, Cb, h, w, 2) and events[1] == ('conv1x1', False)
            assert len(calls) == n
            answer[0] = 1
            del events[:]
            blk(xin)                                                     # yes: conv1 leaves the range word, conv2 is the new launch
            assert events[0] == ('pays', Cb, Cb, h, w, 2) and events[1] == ('conv1x1', True)
            assert len(calls) == n + 1
            answer[0] = 0


# the timed corners: INPUT map side of conv2 at a 1024^2 image per C (docs/notebook/round24.md); the 1536^2 image's is 3 / 2 of it
CORNERS = {128: 256, 256: 128}
# what the timing runs gave: (1024^2 map one image, 1536^2 map one image, 1024^2 map two images) per C
ROUTED = {128: [1, 1, 1], 256: [1, 1, 1]}


def test_the_routing_table_is_closed():
    """nothing beyond the timed corners is routed: smaller or larger maps, more than two images (batch 3), two images off the 1024^2
    map, the timed area in another (non-square) shape, the other C's map"""
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    for C, side in CORNERS.items():
        big = side * 3 // 2
        routed = [L.orp_conv3x3_bn_s2_pays(C, C, side, side, 1), L.orp_conv3x3_bn_s2_pays(C, C, big, big, 1),
                  L.orp_conv3x3_bn_s2_pays(C, C, side, side, 2)]
        assert L.orp_conv3x3_bn_s2_pays(C, C, side - 1, side, 1) == 0
        assert L.orp_conv3x3_bn_s2_pays(C, C, side, side - 1, 1) == 0
        assert L.orp_conv3x3_bn_s2_pays(C, C, big + 1, big, 1) == 0
        assert L.orp_conv3x3_bn_s2_pays(C, C, big, big + 1, 1) == 0
        assert L.orp_conv3x3_bn_s2_pays(C, C, side, side, 3) == 0
        assert L.orp_conv3x3_bn_s2_pays(C, C, big, big, 2) == 0
        assert L.orp_conv3x3_bn_s2_pays(C, C, 1, side * side, 1) == 0
        assert L.orp_conv3x3_bn_s2_pays(C, C, side // 4, side * 4, 1) == 0
        assert L.orp_conv3x3_bn_s2_pays(C, C, side * 2, side * 2, 1) == 0
        # between two timed corners that both paid a map is routed, and only there
        assert L.orp_conv3x3_bn_s2_pays(C, C, side, big, 1) == (1 if routed[0] and routed[1] else 0)
        assert routed == ROUTED[C]


@pytest.mark.parametrize("C", CS)
def test_captured_bottleneck_replays_the_eager_bits(dev, monkeypatch, C):
    """a captured stride-2 block replays the eager bits for NEW input contents whose range is smaller than what the capture saw"""
    _pin_the_library(monkeypatch)
    calls = _spy(monkeypatch)
    blk, cin = _block0(dev, C)
    blk.force_conv3x3_s2 = True
    h, w = 7, 35
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
