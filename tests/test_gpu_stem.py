"""GPU: the ResNet stem as one launch (orp_stem_conv_bn_relu_pool): 7x7 / stride 2 / padding 3 convolution 3 -> 64 on the exact fp32 MFMA,
BatchNorm + ReLU + 3x3 / stride 2 / padding 1 max-pool in its epilogue, and the same launch in raw mode (the convolution alone).

Raw mode, exact cases (small-integer pixels and weights: every product and partial sum is exact in any order, 147 * 15 * 7 < 2^24) bit for
bit against the float64 convolution cast to fp32, over the smallest inputs that reach every seam of the 4 x 16 pooled tile (8 x 32 conv
outputs, a 16 x 64 input) and both parities of height and width; each of the 147 taps alone (a wrong K order or a padding tap that
reads a pixel shows at once); a single pixel at each parity of the de-interleaved patch next to a tile seam and in two image corners;
the seam between the two output-channel blocks.  Fused mode bit for bit against bn_relu_maxpool of the raw-mode output (salted
BatchNorm constants, inputs salted with non-finite values and signed zeros).  Random data against float64 inside the derived bound and
within twice the library convolution's share of it.  Tile / batch independence, repeatability, graph replay, the switch, the `force`
attribute, the closed table and the refused arguments.

The figures of the random case on MI355X are in docs/notebook/round25.md."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_conv1x1_bn as base  # noqa: E402

_bits, _same_bits, _conv64 = base._bits, base._same_bits, base._conv64
# (images, H, W) of the INPUT: 1 x 1 and 7 x 7; exactly one tile (16 x 64 and, odd, 15 x 63); one pixel / one conv output more in each
# direction (17 x 65 odd, 18 x 66 even: 9 x 33 conv outputs, 5 x 17 pooled, two tiles each way); the strips; one and three images
LAYOUTS = [(1, 1, 1), (3, 7, 7), (1, 16, 64), (3, 15, 63), (1, 17, 65), (3, 18, 66), (1, 1, 80), (1, 80, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _conv7(dev, seed, integer=False):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
    with torch.no_grad():
        if integer:
            conv.weight.copy_(torch.randint(-7, 8, (64, 3, 7, 7), generator=g).float())
        else:
            conv.weight.copy_(torch.randn(64, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5)      # He scale
    return conv.to(dev).eval()


@pytest.fixture(scope="module")
def exact(dev):
    """integer weights and the salted BatchNorm (non-finite constants, signed zeros, a subnormal scale), made once"""
    return _conv7(dev, 164, integer=True), base._bn(64, dev, 7, salted=True)


def _ints(shape, dev, seed):
    return torch.randint(-15, 16, shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)).float()


def _spy(monkeypatch, name='orp_stem_conv_bn_relu_pool'):
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    orig = getattr(L, name)
    calls = []

    def spy(*args):
        calls.append(args)
        return orig(*args)
    monkeypatch.setattr(L, name, spy)
    return calls


def _raw(x, conv):
    from orientedreppoints_amd.mmdet_ops.fused_norm import stem_conv_raw
    return stem_conv_raw(x, conv)


def _fused(x, conv, bn):
    from orientedreppoints_amd.mmdet_ops.fused_norm import stem_conv_bn_relu_maxpool
    return stem_conv_bn_relu_maxpool(x, conv, bn)


def _pool_of_raw(x, conv, bn):
    """THE result of the fused mode: the two-launch epilogue (orp_affine_relu_maxpool) on the raw-mode output"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_relu_maxpool
    return bn_relu_maxpool(_raw(x, conv), bn)


def _check(x, conv, bn, tag):
    """raw mode against float64, fused mode against the pass on the raw output, both bit for bit"""
    want = _conv64(x, conv).float()
    got = _raw(x, conv)
    assert got.shape == want.shape and got.is_contiguous()
    assert _same_bits(got, want), tag + ('raw', int((_bits(got) != _bits(want)).sum()))
    fused, pooled = _fused(x, conv, bn), _pool_of_raw(x, conv, bn)
    assert fused.shape == pooled.shape and fused.is_contiguous()
    assert _same_bits(fused, pooled), tag + ('fused', int((_bits(fused) != _bits(pooled)).sum()))


@pytest.mark.parametrize("B,h,w", LAYOUTS)
def test_exact_cases_bit_for_bit(dev, monkeypatch, exact, B, h, w):
    """integers |x| <= 15, |w| <= 7, every layout"""
    calls = _spy(monkeypatch)
    conv, bn = exact
    with torch.no_grad():
        _check(_ints((B, 3, h, w), dev, 7 * h + w), conv, bn, (B, h, w))
    assert len(calls) == 3 and calls[0][5:14] == (B, 3, 64, h, w, 7, 2, 3, 0) and calls[1][13] == 1


def test_single_tap_weights(dev, exact):
    """the weight non-zero at one tap of one output channel only, for each of the 147 taps, on a map of two tiles each way"""
    full, _bn = exact
    x = _ints((1, 3, 17, 67), dev, 41)
    conv = _conv7(dev, 1, integer=True)
    xp = torch.nn.functional.pad(x.double(), (3, 3, 3, 3))
    ho, wo = 9, 34
    with torch.no_grad():
        for k in range(147):
            c, ky, kx = k // 49, (k % 49) // 7, k % 7
            o = (5 * k + 3) % 64
            conv.weight.zero_()
            conv.weight[o, c, ky, kx] = float(k % 7 + 1)
            got = _raw(x, conv)
            want = torch.zeros((1, 64, ho, wo), dtype=torch.float64, device=dev)
            want[0, o] = xp[0, c, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2] * (k % 7 + 1)
            assert _same_bits(got, want.float()), (k, c, ky, kx, o)
    assert full.weight.shape == conv.weight.shape


@pytest.mark.parametrize("where", ["seam", "top-left", "bottom-right"])
@pytest.mark.parametrize("py,px", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_single_pixel_inputs_at_each_parity(dev, exact, py, px, where):
    """one non-zero pixel (all channels) at each (row parity, column parity): next to the tile seam in both directions (19 x 70 input =
    10 x 35 conv outputs; the seams are between conv rows 7 | 8 and columns 31 | 32, i.e. input rows 15 | 16 and columns 63 | 64, and the
    pixel's windows reach both sides) and in the image's corners, where its windows also read the padding"""
    conv, bn = exact
    h, w = 19, 70
    yy, xx = {"seam": (15 + py, 63 + px), "top-left": (py, px), "bottom-right": (h - 1 - py, w - 1 - px)}[where]
    x = torch.zeros((1, 3, h, w), device=dev)
    x[0, :, yy, xx] = torch.tensor([15.0, -7.0, 4.0], device=dev)
    with torch.no_grad():
        _check(x, conv, bn, (py, px, where))


def test_output_channels_at_the_block_seam(dev):
    """output channels 31 / 32 belong to different channel blocks (waves): output channel o copies (o % 7 + 1) x input channel o % 3
    through its centre tap, so that a value written to a neighbouring channel is a different value"""
    conv, bn = _conv7(dev, 1, integer=True), base._bn(64, dev, 9)
    with torch.no_grad():
        conv.weight.zero_()
        o = torch.arange(64, device=dev)
        conv.weight[o, o % 3, 3, 3] = (o % 7 + 1).float()
        x = _ints((1, 3, 16, 64), dev, 61).abs() + 1
        want, got = _conv64(x, conv).float(), _raw(x, conv)
        for ch in (30, 31, 32, 33):
            assert _same_bits(got[:, ch], want[:, ch]), ch
        assert bool((want[:, 31] != want[:, 32]).any())
        _check(x, conv, bn, ('seam',))


def test_fused_mode_equals_the_pass_on_the_raw_output_with_salted_data(dev, exact):
    """random and integer inputs salted with +-Inf, NaN, signed zeros and magnitudes that underflow, salted BatchNorm constants: the
    fused launch gives the bits of orp_affine_relu_maxpool on the raw-mode output, on a map with partial tiles on both sides"""
    bn = exact[1]
    for conv, x in ((exact[0], _ints((2, 3, 21, 75), dev, 3)), (_conv7(dev, 5), torch.randn(2, 3, 21, 75, device=dev))):
        x = base._salt(x.clone(), 11)
        with torch.no_grad():
            fused, pooled = _fused(x, conv, bn), _pool_of_raw(x, conv, bn)
        assert fused.shape == (2, 64, 6, 19)
        assert _same_bits(fused, pooled), int((_bits(fused) != _bits(pooled)).sum())


def test_inf_and_nan_reach_the_windows_that_read_them_and_no_other(dev, exact):
    """one +Inf (top edge, next to the tile seam) and one NaN (bottom right corner) in integer data: every raw output whose window reads
    neither is the exact result bit for bit -- the padding tap and the dropped columns read no pixel -- and every one whose window
    reads one is non-finite, in all 64 channels"""
    import torch.nn.functional as F
    h, w = 19, 70
    conv = exact[0]
    x = _ints((2, 3, h, w), dev, 72)
    clean = x.clone()
    mark = torch.zeros((2, 1, h, w), device=dev)
    for (b, ch, yy, xx, v) in [(0, 1, 0, 64, float('inf')), (1, 2, h - 1, w - 1, float('nan'))]:
        x[b, ch, yy, xx] = v
        mark[b, 0, yy, xx] = 1.0
    touched = F.conv2d(mark, torch.ones((1, 1, 7, 7), device=dev), stride=2, padding=3) > 0
    with torch.no_grad():
        want = _conv64(clean, conv).float()
        got = _raw(x, conv)
    t = touched.expand_as(got)
    assert int(t.sum()) > 0 and bool((~torch.isfinite(got[t])).all())
    assert np.array_equal(_bits(got[~t]), _bits(want[~t]))


def test_random_data_inside_the_derived_bound(dev):
    """N(0, 1) pixels, He-scale weights, raw mode against the float64 convolution: worst |err| as a share of (147 + 2) 2^-24 sum |x w|
    (147 products and sums of the fp32 chain, one rounding of at most 2^-24 each relative to a partial result that the sum of magnitudes
    bounds), no more than twice the library convolution's share on the same inputs -- the library is the yardstick, the factor two is
    for the other summation order (the project's rule, rounds 15, 23 and 24)"""
    import conftest
    B, h, w = 2, 37, 131
    conv = _conv7(dev, 40)
    x = torch.randn((B, 3, h, w), device=dev, generator=torch.Generator(device=dev).manual_seed(42))
    with torch.no_grad():
        ref = _conv64(x, conv)
        bound = (147 + 2) * 2.0 ** -24 * _conv64(x, conv, magnitudes=True)
        got = _raw(x, conv)
        lib = conv(x)
    assert bool((bound > 0).all())
    ours = float(((got.double() - ref).abs() / bound).max())
    theirs = float(((lib.double() - ref).abs() / bound).max())
    line = ("stem 7x7 convolution 3 -> 64 stride 2 at %d x %d x %d, worst |err| / bound vs float64: fp32 MFMA kernel %.3g, library %.3g"
            % (B, h, w, ours, theirs))
    print(line)
    conftest.REPORT.append(line)
    assert ours <= 1.0
    assert ours <= 2.0 * theirs


def test_a_tile_does_not_depend_on_its_place_in_the_grid_or_the_batch(dev):
    """the top-left tile of the middle image of three, computed alone (the image cropped to the 16 x 64 pixels of that tile, what its
    windows read below / right of them zeroed like padding is), and that image alone, give the bits they have inside the larger launch"""
    conv, bn = _conv7(dev, 3), base._bn(64, dev, 4)
    x = torch.randn((3, 3, 19, 70), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    x[:, :, 16:19, :] = 0
    x[:, :, :, 64:67] = 0
    crop = x[1:2, :, :16, :64].contiguous()
    with torch.no_grad():
        for fn, th, tw in ((lambda t: _raw(t, conv), 8, 32), (lambda t: _fused(t, conv, bn), 4, 16)):
            big, small, one = fn(x), fn(crop), fn(x[1:2].contiguous())
            assert small.shape[2:] == (th, tw)
            assert _same_bits(big[1:2, :, :th, :tw], small)
            assert _same_bits(big[1:2], one)


def test_same_launch_twice_gives_the_same_bits(dev):
    conv, bn = _conv7(dev, 1), base._bn(64, dev, 2)
    x = torch.randn((2, 3, 21, 75), device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    with torch.no_grad():
        assert _same_bits(_raw(x, conv), _raw(x, conv))
        assert _same_bits(_fused(x, conv, bn), _fused(x, conv, bn))


def _stem_net(dev):
    """a ResNet whose forward is its stem alone"""
    from orientedreppoints_amd.mmdet_models.resnet import ResNet
    torch.manual_seed(8)
    net = ResNet(50, num_stages=1, out_indices=(0,))
    net.layer1 = torch.nn.Identity()
    net = net.to(dev)
    net.eval()
    net.bn1.load_state_dict(base._bn(64, dev, 9).state_dict())
    return net


def test_captured_stem_replays_the_eager_bits(dev, monkeypatch):
    """a captured stem replays the eager bits for NEW input contents"""
    calls = _spy(monkeypatch)
    net = _stem_net(dev)
    net.force_stem_conv = True
    xa = torch.randn(2, 3, 37, 75, device=dev) * 64
    xb = torch.randn(2, 3, 37, 75, device=dev) * 0.37
    with torch.no_grad():
        eager = {k: net(v)[0].clone() for k, v in (('a', xa), ('b', xb))}
        assert len(calls) == 2
        x = xa.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net(x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(x)[0]
        for k, v in (('a', xa), ('b', xb), ('a', xa), ('b', xb)):
            x.copy_(v)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert _same_bits(out, eager[k]), k


def test_switch_force_and_routing_query(dev, monkeypatch):
    """ResNet.forward: outside the table the stem keeps its launches; `force_stem_conv` routes it through the one launch (the bits of the
    fused mode, close to the library path); `fuse_stem_conv = False` switches it off again (the bits of before), `fuse_stem_pool` is not
    consulted; a yes of `orp_stem_pays` routes without force; autograd, a ceil-mode pool, a training-mode BatchNorm and a convolution
    with a bias keep the module path"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops import fused_norm
    L = _lib.lib()
    calls = _spy(monkeypatch)
    net = _stem_net(dev)
    x = torch.randn(1, 3, 76, 68, device=dev)
    with torch.no_grad():
        before = net(x)[0]
        assert len(calls) == 0                                  # the table is closed around the timed images, and this is none
        net.force_stem_conv = True
        on = net(x)[0]
        assert len(calls) == 1 and calls[0][5:14] == (1, 3, 64, 76, 68, 7, 2, 3, 1)
        assert _same_bits(on, _fused(x, net.conv1, net.bn1))
        net.fuse_stem_pool = False                              # the other switch is not consulted
        assert _same_bits(net(x)[0], on) and len(calls) == 3
        del net.fuse_stem_pool
        net.fuse_stem_conv = False
        off = net(x)[0]
        assert len(calls) == 3 and _same_bits(off, before)
        del net.fuse_stem_conv
        # on and off agree inside the convolution's bound carried through the affine (the pooling picks one of the bounded values)
        a, b = [t.double() for t in fused_norm._bn_affine(net.bn1)]
        d = float((2 * (147 + 2) * 2.0 ** -24 * (a.abs().view(1, -1, 1, 1) * _conv64(x, net.conv1, magnitudes=True) +
                                                b.abs().view(1, -1, 1, 1))).max())
        assert float((on - off).abs().max()) <= d
        # the query: asked with the image's height, width and batch, not asked under force
        del net.force_stem_conv
        events, answer = [], [0]

        def pays(*args):
            events.append(args)
            return answer[0]
        monkeypatch.setattr(L, 'orp_stem_pays', pays)
        net(x)
        assert events == [(76, 68, 1)] and len(calls) == 3
        answer[0] = 1
        assert _same_bits(net(x)[0], on) and len(calls) == 4
        net.force_stem_conv = True
        n = len(events)
        net(x)
        assert len(events) == n and len(calls) == 5
        # what the route does not take
        mp = net.maxpool
        net.maxpool = torch.nn.MaxPool2d(3, 2, 1, ceil_mode=True)
        net(x)
        net.maxpool = mp
        conv1 = net.conv1
        net.conv1 = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=True).to(dev)
        net(x)
        net.conv1 = conv1
        assert len(calls) == 5
        assert not fused_norm.stem_conv_routed(x, torch.nn.Conv2d(3, 64, 7, stride=2, padding=2, bias=False).to(dev), net.bn1, mp, True)
        assert not fused_norm.stem_conv_routed(x, torch.nn.Conv2d(3, 32, 7, stride=2, padding=3, bias=False).to(dev), net.bn1, mp, True)
        assert not fused_norm.stem_conv_routed(x.double(), conv1, net.bn1, mp, True)
        assert fused_norm.stem_conv_routed(x, conv1, net.bn1, mp, True)
    with torch.enable_grad():
        stock = net(x)[0]                                       # autograd on: the module path
    assert len(calls) == 5 and stock.requires_grad


# what the timing runs gave (docs/notebook/round25.md): one image 1024^2, one image 1536^2, two images 1024^2
ROUTED = [1, 1, 1]


def test_the_routing_table_is_closed():
    """nothing beyond the timed corners is routed: smaller or larger images, more than two images, two images off 1024^2"""
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    routed = [L.orp_stem_pays(1024, 1024, 1), L.orp_stem_pays(1536, 1536, 1), L.orp_stem_pays(1024, 1024, 2)]
    assert routed == ROUTED
    for h, w, b in ((1023, 1024, 1), (1024, 1023, 1), (1537, 1536, 1), (1536, 1537, 1), (1024, 1024, 3), (1536, 1536, 2), (1025, 1024, 2),
                    (1, 1024 * 1024, 1), (256, 4096, 1), (2048, 2048, 1), (512, 512, 1), (76, 68, 1), (0, 1024, 1), (1024, -1, 1),
                    (1024, 1024, 0)):
        assert L.orp_stem_pays(h, w, b) == 0, (h, w, b)
    # between two timed corners that both paid an image is routed, and only there
    assert L.orp_stem_pays(1024, 1536, 1) == (1 if routed[0] and routed[1] else 0)
    assert L.orp_stem_pays(1280, 1152, 1) == (1 if routed[0] and routed[1] else 0)


def test_unsupported_arguments_are_rejected(dev):
    """other channel counts, kernel sizes, strides, paddings, null pointers, non-positive sizes, output == input: ORP_EINVAL and nothing
    is written"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import _packed_stem_weight
    L = _lib.lib()
    x = torch.randn(1, 3, 16, 64, device=dev)
    conv = _conv7(dev, 2)
    packed, ab = _packed_stem_weight(conv.weight), torch.ones(64, device=dev)
    assert packed.numel() == 2 * 74 * 64 * 4 == L.orp_stem_packed_bytes(3, 64)
    y = torch.full((1, 64, 8, 32), 7.0, device=dev)
    st = _lib.stream_of(x)
    args = [_lib.ptr(x), _lib.ptr(packed), _lib.ptr(ab), _lib.ptr(ab), _lib.ptr(y)]
    good = (1, 3, 64, 16, 64, 7, 2, 3, 1)
    for k, v in ((0, 0), (0, -1), (1, 4), (1, 1), (2, 32), (2, 128), (3, 0), (3, -16), (4, 0), (4, -64), (5, 3), (5, 5), (6, 1), (7, 2),
                 (7, 0), (8, 2), (8, -1)):
        bad = list(good)
        bad[k] = v
        assert L.orp_stem_conv_bn_relu_pool(*args, *bad, st) == _lib.ORP_EINVAL, (k, v)
    for cin, cout in ((4, 64), (3, 32), (64, 3), (0, 0), (-3, -64)):
        assert L.orp_stem_ok(cin, cout, 7, 2, 3) == 0 and L.orp_stem_packed_bytes(cin, cout) == 0
        assert L.orp_stem_pack_weight(_lib.ptr(conv.weight.detach()), cin, cout, _lib.ptr(packed), st) == _lib.ORP_EINVAL
    assert L.orp_stem_pack_weight(None, 3, 64, _lib.ptr(packed), st) == _lib.ORP_EINVAL
    assert L.orp_stem_pack_weight(_lib.ptr(conv.weight.detach()), 3, 64, None, st) == _lib.ORP_EINVAL
    for k in range(5):
        bad = list(args)
        bad[k] = None
        assert L.orp_stem_conv_bn_relu_pool(*bad, *good, st) == _lib.ORP_EINVAL, k
    raw = list(good)
    raw[8] = 0
    for k in (0, 1, 4):                                         # raw mode takes null scale / shift, nothing else null
        bad = list(args)
        bad[k] = None
        assert L.orp_stem_conv_bn_relu_pool(*bad, *raw, st) == _lib.ORP_EINVAL, k
    args[4] = _lib.ptr(x)
    assert L.orp_stem_conv_bn_relu_pool(*args, *good, st) == _lib.ORP_EINVAL
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
