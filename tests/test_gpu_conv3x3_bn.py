"""GPU: the bottleneck 3x3 convolution on the fp16-pieces path with BatchNorm + ReLU in its epilogue (orp_conv3x3_bn_act).

Exact cases (small-integer activations and weights, power-of-two BatchNorm coefficients: every piece, product and sum is exact in any
order) bit for bit against float64, over every wave layout and tile, ragged maps, image seams and ReLU on / off; random data against
float64 inside the derived bound that the library path has to meet as well; the range edges (zero input, an outlier, tiny and huge
maxima, Inf / NaN, the range word the producers leave); the Bottleneck call site, the routing query, reproducibility and graph replay.

The helpers (_conv64, _bound, _bn, ...) are those of test_gpu_conv1x1_bn.py: `_bound` is (K + 2) 2^-24 (|a| sum |x_k w_k| + |b|) with
K = the weight's fan-in, 9 Cin here."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_conv1x1_bn as base  # noqa: E402

_bits, _same_bits, _conv64, _bound = base._bits, base._same_bits, base._conv64, base._bound

# channels -> (tile_h, tile_w, waves over positions, waves over channels)
LAYOUT = {64: (16, 16, 4, 2), 128: (4, 16, 2, 4), 256: (2, 16, 1, 8)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _conv3(c, dev, seed, integer=False, cout=None, **kw):
    g = torch.Generator().manual_seed(seed)
    cout = c if cout is None else cout
    kw.setdefault('padding', 1)
    kw.setdefault('bias', False)
    conv = torch.nn.Conv2d(c, cout, 3, **kw)
    with torch.no_grad():
        if integer:
            conv.weight.copy_(torch.randint(-7, 8, (cout, c, 3, 3), generator=g).float())
        else:
            conv.weight.copy_(torch.randn(cout, c, 3, 3, generator=g) * (2.0 / (9 * c)) ** 0.5)      # He scale
    return conv.to(dev).eval()


def _bn_pow2(c, dev, seed):
    """eval-mode BatchNorm whose folded (scale, shift) are signed powers of two / small multiples of 1/8 exactly: eps 0, variance 1,
    mean 0"""
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(c, eps=0.0)
    with torch.no_grad():
        e = torch.randint(-3, 3, (c,), generator=g).float()
        sign = torch.randint(0, 2, (c,), generator=g).float() * 2 - 1
        bn.weight.copy_(sign * torch.pow(torch.tensor(2.0), e))
        bn.bias.copy_(torch.randint(-64, 65, (c,), generator=g).float() / 8)
        bn.running_mean.zero_(); bn.running_var.fill_(1.0)
    return bn.to(dev).eval()


def _range_bits(x):
    """max over the finite elements of |x| as float bits (orp_range.hpp: range_bits), a one-element int32 tensor"""
    a = x.detach().abs()
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    return a.max().reshape(1).contiguous().view(torch.int32)


def _ref64(x, conv, bn, relu):
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine
    a, b = [t.double() for t in _bn_affine(bn)]
    y = _conv64(x, conv) * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


def _spy(monkeypatch, name='orp_conv3x3_bn_act'):
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    orig = getattr(L, name)
    calls = []

    def spy(*args):
        calls.append(args)
        return orig(*args)
    monkeypatch.setattr(L, name, spy)
    return calls


def _fused(x, conv, bn, relu=True, bits=None):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv3x3_bn_act
    return conv3x3_bn_act(x, conv, bn, relu=relu, force=True, range_bits=_range_bits(x) if bits is None else bits)


# (channels, images, H, W): the issue's shapes; 1 x 1, 1 x 40 and 40 x 1 maps; exactly one tile; one pixel more than a tile each way
EXACT = [(64, 3, 37, 35), (128, 2, 17, 50), (256, 1, 13, 16), (256, 1, 64, 64)]
for _c, (_th, _tw, _, _) in sorted(LAYOUT.items()):
    EXACT += [(_c, 1, 1, 1), (_c, 1, 1, 40), (_c, 1, 40, 1), (_c, 1, _th, _tw), (_c, 2, _th + 1, _tw + 1)]


@pytest.mark.parametrize("c,B,h,w", EXACT)
def test_exact_cases_bit_for_bit(dev, monkeypatch, c, B, h, w):
    """integers |x| <= 15, |w| <= 7 (9 * 256 * 105 < 2^24: the scaled pieces have no low part and every sum is exact), BatchNorm
    scale a signed power of two and shift a multiple of 1/8: float64 conv + affine (+ ReLU) cast to fp32 is THE result"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine, conv3x3_bn_act_tile
    assert conv3x3_bn_act_tile(c, c, h, w, B) == LAYOUT[c]
    calls = _spy(monkeypatch)
    conv, bn = _conv3(c, dev, 100 + c, integer=True), _bn_pow2(c, dev, 7 + c)
    a, b = _bn_affine(bn)
    assert bool((torch.frexp(a.abs())[0] == 0.5).all()) and bool((b * 8 == torch.round(b * 8)).all())
    g = torch.Generator(device=dev).manual_seed(c + 7 * h + w)
    x = torch.randint(-15, 16, (B, c, h, w), device=dev, generator=g).float()
    with torch.no_grad():
        for relu in (False, True):
            want = _ref64(x, conv, bn, relu).float()
            got = _fused(x, conv, bn, relu)
            assert got.is_contiguous() and got.data_ptr() != x.data_ptr()
            assert _same_bits(got, want), (c, B, h, w, relu, int((got != want).sum()))
    assert len(calls) == 2


def test_unsupported_shapes_are_rejected(dev):
    """the queries say no, and the launcher itself returns ORP_EINVAL for the channel counts (every pointer valid) and writes nothing"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import _packed_3x3_planes, conv3x3_bn_act_tile
    L = _lib.lib()
    assert [L.orp_conv3x3_bn_act_ok(c, c) for c in (64, 128, 256)] == [1, 1, 1]
    for cin, cout in ((512, 512), (64, 128), (32, 32), (96, 96), (256, 64)):
        assert L.orp_conv3x3_bn_act_ok(cin, cout) == 0 and conv3x3_bn_act_tile(cin, cout, 16, 16, 1) is None
        assert L.orp_conv3x3_bn_act_pays(cin, cout, 256, 256, 1) == 0
        conv = _conv3(cin, dev, 1, cout=cout)
        x = torch.randn(1, cin, 16, 16, device=dev)
        assert L.orp_conv3x3_bn_packed_bytes(cin, cout) == 0
        packed, ab = torch.zeros(4 * cin * cout * 9 + 16, dtype=torch.uint8, device=dev), torch.ones(cout, device=dev)
        assert L.orp_conv3x3_bn_pack_weight(_lib.ptr(conv.weight.detach()), cin, cout, _lib.ptr(packed), _lib.stream_of(x)) == _lib.ORP_EINVAL
        y = torch.full((1, cout, 16, 16), 7.0, device=dev)
        rc = L.orp_conv3x3_bn_act(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(ab), _lib.ptr(ab), _lib.ptr(_range_bits(x)), _lib.ptr(y),
                                  1, cin, cout, 16, 16, 1, _lib.stream_of(x))
        assert rc == _lib.ORP_EINVAL and bool((y == 7.0).all())
    x = torch.randn(1, 64, 16, 16, device=dev)                           # a supported shape with a missing pointer / y aliasing x
    conv = _conv3(64, dev, 2)
    packed, ab, bits = _packed_3x3_planes(conv.weight), torch.ones(64, device=dev), _range_bits(x)
    assert packed.numel() == 4 * 64 * 64 * 9 + 16
    args = [_lib.ptr(x), _lib.ptr(packed), _lib.ptr(ab), _lib.ptr(ab), _lib.ptr(bits), _lib.ptr(torch.empty_like(x))]
    for k in range(6):
        bad = list(args)
        bad[k] = None
        assert L.orp_conv3x3_bn_act(*bad, 1, 64, 64, 16, 16, 1, _lib.stream_of(x)) == _lib.ORP_EINVAL
    args[5] = _lib.ptr(x)
    assert L.orp_conv3x3_bn_act(*args, 1, 64, 64, 16, 16, 1, _lib.stream_of(x)) == _lib.ORP_EINVAL


RANDOM = [(64, 2, 37, 35), (128, 2, 17, 50), (256, 2, 13, 16)]


@pytest.mark.parametrize("c,B,h,w", RANDOM)
def test_random_data_inside_the_derived_bound(dev, c, B, h, w):
    """N(0, 1) activations through a ReLU, He-scale weights, against float64 conv + affine + ReLU inside
    (9 Cin + 2) 2^-24 (|a| sum |x_k w_k| + |b|); the library path (conv + bn_act) has to meet the same bound on the same inputs"""
    import conftest
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine, bn_act
    conv, bn = _conv3(c, dev, 40 + c), base._bn(c, dev, 41)
    g = torch.Generator(device=dev).manual_seed(c)
    x = torch.relu(torch.randn((B, c, h, w), device=dev, generator=g))
    with torch.no_grad():
        a, b = [t.double() for t in _bn_affine(bn)]
        ref = _ref64(x, conv, bn, True)
        bound = _bound(x, conv, a, b, None)
        got = _fused(x, conv, bn, True)
        lib = bn_act(conv(x).contiguous(), bn, relu=True)
    ours = float(((got.double() - ref).abs() / bound).max())
    theirs = float(((lib.double() - ref).abs() / bound).max())
    conftest.REPORT.append("3x3 convolution + BatchNorm + ReLU %d -> %d at %d x %d x %d, worst |err| / bound vs float64: fp16-pieces fused "
                           "%.3f, library + pass %.3f" % (c, c, B, h, w, ours, theirs))
    assert ours <= 1.0
    assert theirs <= 1.0


def test_all_zero_input(dev):
    """range word 0 -> scale 1; every output is relu?(shift[c]) exactly"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine
    conv, bn = _conv3(64, dev, 1), base._bn(64, dev, 2)
    x = torch.zeros((2, 64, 17, 19), device=dev)
    with torch.no_grad():
        b = _bn_affine(bn)[1].view(1, -1, 1, 1)
        for relu in (False, True):
            want = (torch.relu(b) if relu else b).expand(2, 64, 17, 19).contiguous()
            assert _same_bits(_fused(x, conv, bn, relu), want)


def _floor_term(x, conv, a):
    """|a| 2^-37 max|x| sum_k |w_k| per output channel: what the fp16 subnormal floor of the activations' low pieces can add when one
    element is far above the rest (the low piece of an element near the bottom of the high piece's range is rounded to a multiple of
    2^-24 in scaled units)"""
    mx = float(x.abs().max())
    return (a.abs() * conv.weight.detach().double().abs().flatten(1).sum(1) * (2.0 ** -37 * mx)).view(1, -1, 1, 1)


@pytest.mark.parametrize("case", ["outlier", "tiny", "huge"])
def test_range_edges_inside_the_bound(dev, case):
    """one element 2^15 times the rest (everything else lands near the bottom of the high piece: the floor term is added to the
    bound, in this case only); all data scaled so that the maximum is near 2^-120 (the scale clamps) and near 2^100, inside the
    plain bound.  BatchNorm without a shift, no ReLU, so that the bound is the contraction's alone"""
    import conftest
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine
    c = 128
    conv, bn = _conv3(c, dev, 60), base._bn(c, dev, 61)
    with torch.no_grad():
        bn.running_mean.zero_(); bn.bias.zero_()                                                # shift = 0
    g = torch.Generator(device=dev).manual_seed(62)
    x = torch.relu(torch.randn((2, c, 17, 50), device=dev, generator=g)) + 0.01
    if case == "outlier":
        x[1, 5, 9, 20] = float(x.max()) * 2.0 ** 15
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
        got = _fused(x, conv, bn, False)
    assert bool(torch.isfinite(got).all())
    ratio = float(((got.double() - ref).abs() / bound).max())
    conftest.REPORT.append("3x3 fp16-pieces convolution, range edge '%s' (max |x| %.3g): worst |err| / bound %.3f"
                           % (case, float(x.abs().max()), ratio))
    assert ratio <= 1.0


def test_inf_and_nan_reach_the_windows_that_read_them_and_no_other(dev):
    """one +Inf and one NaN in integer data: the range word skips them (range_bits), so every output whose 3 x 3 window reads
    neither is the exact float64 result, bit for bit; every output whose window reads one (all channels) is non-finite"""
    c, B, h, w = 64, 2, 21, 19
    conv, bn = _conv3(c, dev, 70, integer=True), _bn_pow2(c, dev, 71)
    g = torch.Generator(device=dev).manual_seed(72)
    x = torch.randint(-15, 16, (B, c, h, w), device=dev, generator=g).float()
    clean = x.clone()
    spots = [(0, 3, 0, 5, float('inf')), (1, 40, 16, 15, float('nan'))]      # (at the top edge; across the 16 x 16 tile seam)
    touched = torch.zeros((B, 1, h, w), dtype=torch.bool, device=dev)
    for (b, ch, yy, xx, v) in spots:
        x[b, ch, yy, xx] = v
        touched[b, 0, max(yy - 1, 0):yy + 2, max(xx - 1, 0):xx + 2] = True
    assert int(_range_bits(x).item()) == int(_range_bits(clean).item())
    with torch.no_grad():
        want = _ref64(clean, conv, bn, False).float()
        got = _fused(x, conv, bn, False)
    t = touched.expand(B, c, h, w)
    assert bool((~torch.isfinite(got[t])).all())
    assert np.array_equal(_bits(got[~t]), _bits(want[~t]))


@pytest.mark.parametrize("h,w", [(7, 9), (33, 31), (16, 16)])
def test_producers_leave_the_range_word(dev, monkeypatch, h, w):
    """orp_conv1x1_bn_act_range and orp_affine_act_range leave max range_bits(y) -- ragged tiles, three images, Inf / NaN in y"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, conv1x1_bn_act
    calls = _spy(monkeypatch, 'orp_conv1x1_bn_act_range')
    conv, bn = base._conv(256, 64, dev, 80), base._bn(64, dev, 81)
    g = torch.Generator(device=dev).manual_seed(82 + h)
    x = torch.randn((3, 256, h, w), device=dev, generator=g)
    x[2, 7, h - 1, w - 1] = 300.0                       # the maximum sits in the last, ragged tile
    x[0, 0, 0, 0] = float('inf'); x[1, 3, h // 2, 0] = float('nan')
    with torch.no_grad():
        for relu in (True, False):
            y, bits = conv1x1_bn_act(x, conv, bn, relu=relu, force=True, want_range=True)
            assert _same_bits(y, conv1x1_bn_act(x, conv, bn, relu=relu, force=True))
            assert int((~torch.isfinite(y)).sum()) > 0
            assert int(bits.item()) == int(_range_bits(y).item()) and int(bits.item()) > 0
            raw = conv(x).contiguous()
            want = bn_act(raw.clone(), bn, relu=relu)
            y2, bits2 = bn_act(raw.clone(), bn, relu=relu, want_range=True)
            assert _same_bits(y2, want) and int(bits2.item()) == int(_range_bits(y2).item())
    assert len(calls) == 2


def test_same_launch_twice_gives_the_same_bits(dev):
    conv, bn = _conv3(128, dev, 1), base._bn(128, dev, 2)
    x = torch.relu(torch.randn((2, 128, 33, 31), device=dev, generator=torch.Generator(device=dev).manual_seed(4)))
    with torch.no_grad():
        assert _same_bits(_fused(x, conv, bn), _fused(x, conv, bn))


def _force(blk, on=True):
    blk.force_conv3x3 = on


def _stage_bound(x, conv, bn):
    return base._stage_bound(x, conv, bn)


def test_bottleneck_switch_at_a_forced_supported_shape(dev, monkeypatch):
    """fuse_conv3x3 off / on at 256 -> 64 -> 64 -> 256, the bound of test_gpu_conv1x1_bn.py::test_bottleneck_switch_at_a_supported_shape
    with K = 9 Cin at conv2: both sides are within the bound of float64 at conv1 (the library may pick its algorithm per call), so
    within twice the bound of each other; a difference d of a stage's inputs grows by at most max_c |a_c| sum |w_c| through the next
    convolution + BatchNorm, and each later stage adds twice its own bound"""
    calls = _spy(monkeypatch)
    blk = base._bottleneck(dev, 256, 64)
    _force(blk)
    x = torch.randn(2, 256, 30, 22, device=dev)
    outs = {}
    with torch.no_grad():
        for flag in (False, True):
            blk.fuse_conv3x3 = flag
            assert blk._conv3x3_fusable() == flag
            n0 = len(calls)
            outs[flag] = blk(x.clone())
            assert len(calls) - n0 == (1 if flag else 0)
        del blk.fuse_conv3x3
        assert blk._conv3x3_fusable()                   # default: on
        t1 = torch.relu(blk.bn1(blk.conv1(x)))
        t2 = torch.relu(blk.bn2(blk.conv2(t1)))
        d = 2 * _stage_bound(x, blk.conv1, blk.bn1)
        d = d * base._gain(blk.conv2, blk.bn2) + 2 * _stage_bound(t1, blk.conv2, blk.bn2)
        d = d * base._gain(blk.conv3, blk.bn3) + 2 * base._stage_bound(t2, blk.conv3, blk.bn3, x)
    diff = float((outs[True] - outs[False]).abs().max())
    assert 0.0 < diff <= d
    n0 = len(calls)
    with torch.enable_grad():
        stock = blk(x.clone())                          # autograd on: the unfused module path
    assert len(calls) == n0 and stock.requires_grad


def test_unsupported_conv2_takes_the_library_path(dev, monkeypatch):
    """stride 2, 512 channels, a bias: library convolution + pass even when forced (within twice the bound of the same call made
    directly -- the library may pick its algorithm per call)"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine, bn_act, conv3x3_bn_act
    calls = _spy(monkeypatch)
    cases = [_conv3(64, dev, 3, stride=2), _conv3(512, dev, 4), _conv3(64, dev, 5, bias=True), _conv3(64, dev, 6, cout=128)]
    with torch.no_grad():
        for conv in cases:
            cin, cout = conv.weight.size(1), conv.weight.size(0)
            bn = base._bn(cout, dev, 9)
            x = torch.relu(torch.randn(1, cin, 12, 16, device=dev))
            got = conv3x3_bn_act(x, conv, bn, force=True, range_bits=_range_bits(x))
            want = bn_act(conv(x).contiguous(), bn, relu=True)
            a, b = [t.double() for t in _bn_affine(bn)]
            assert got.shape == want.shape
            assert float((got - want).abs().max()) <= 2 * float(_bound(x, conv, a, b, None).max())
    # the stride-2 block of a stage and a stage-4 block: no fused launch with the switch on and forced
    ds = torch.nn.Sequential(torch.nn.Conv2d(256, 512, 1, stride=2, bias=False), torch.nn.BatchNorm2d(512))
    for blk, cin in ((base._bottleneck(dev, 256, 128, stride=2, downsample=ds), 256), (base._bottleneck(dev, 2048, 512), 2048)):
        _force(blk)
        with torch.no_grad():
            blk(torch.randn(1, cin, 12, 16, device=dev))
    assert len(calls) == 0


def test_routing_query_is_consulted_and_force_bypasses_it(dev, monkeypatch):
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, conv3x3_bn_act
    L = _lib.lib()
    calls = _spy(monkeypatch)
    asked, answer = [], [0]

    def pays(*args):
        asked.append(args)
        return answer[0]
    monkeypatch.setattr(L, 'orp_conv3x3_bn_act_pays', pays)
    conv, bn = _conv3(64, dev, 1), base._bn(64, dev, 2)
    x = torch.relu(torch.randn(2, 64, 16, 24, device=dev))
    bits = _range_bits(x)
    with torch.no_grad():
        y = conv3x3_bn_act(x, conv, bn, range_bits=bits)                 # does not pay: library + pass
        assert asked == [(64, 64, 16, 24, 2)] and len(calls) == 0 and y.shape == x.shape
        answer[0] = 1
        conv3x3_bn_act(x, conv, bn, range_bits=bits)                     # pays: the fused launch
        assert asked[1:] == [(64, 64, 16, 24, 2)] and len(calls) == 1
        conv3x3_bn_act(x, conv, bn)                                      # the input's range is not known: library + pass
        assert len(calls) == 1
        answer[0] = 0
        conv3x3_bn_act(x, conv, bn, force=True, range_bits=bits)         # forced: not asked
        assert len(asked) == 2 and len(calls) == 2
        # the Bottleneck asks before conv1 runs, with conv2's input shape
        blk = base._bottleneck(dev, 256, 64)
        blk(torch.randn(2, 256, 16, 24, device=dev))
        assert asked[2:] == [(64, 64, 16, 24, 2)] and len(calls) == 2
        answer[0] = 1
        blk(torch.randn(2, 256, 16, 24, device=dev))
        assert len(calls) == 3


def test_the_routing_table_is_closed():
    """nothing beyond the timed corners is routed: maps smaller than a 1024^2 image's or larger than a 1536^2 image's, more than
    two images, two images off the 1024^2 map"""
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    for c, side in ((64, 256), (128, 128), (256, 64)):
        big = side * 3 // 2
        assert L.orp_conv3x3_bn_act_pays(c, c, side - 1, side, 1) == 0
        assert L.orp_conv3x3_bn_act_pays(c, c, big + 1, big, 1) == 0
        assert L.orp_conv3x3_bn_act_pays(c, c, side, side, 3) == 0
        assert L.orp_conv3x3_bn_act_pays(c, c, big, big, 2) == 0
        assert L.orp_conv3x3_bn_act_pays(c, c, 1, side * side, 1) == 0          # the timed area, not a timed map
        assert L.orp_conv3x3_bn_act_pays(c, c, side // 4, side * 4, 1) == 0
        assert L.orp_conv3x3_bn_act_pays(c, c, side, big, 1) == 1 and L.orp_conv3x3_bn_act_pays(c, c, side, side, 2) == 1


def test_captured_bottleneck_replays_the_eager_bits(dev, monkeypatch):
    """a captured block replays the eager bits for NEW input contents whose range is smaller than what the capture saw: the range
    word is reset inside the graph (a stale, larger word would scale the pieces differently)"""
    calls = _spy(monkeypatch)
    blk = base._bottleneck(dev, 256, 64)
    _force(blk)
    xa = torch.randn(2, 256, 30, 22, device=dev) * 64
    xb = torch.randn(2, 256, 30, 22, device=dev) * 0.37
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
