"""GPU: the bottleneck 1x1 convolution with BatchNorm (+ residual) + ReLU in its epilogue (orp_conv1x1_bn_act).

Exact cases (integer data: the contraction is exact in any order) bit for bit against a float64 convolution cast to fp32 followed by
the passes the epilogue replaces (orp_affine_act / orp_affine2_act), over every (Cin, Cout) x map size x batch x residual form x
ReLU; random data against float64 inside a derived bound that the library path has to meet as well; reproducibility, graph capture,
the Bottleneck call site and the routing query."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()            # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _bn(c, dev, seed, salted=False):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.3)
        if salted:      # non-finite constants, signed zeros, a shift of exactly zero, a scale under which every product underflows
            bn.bias[0] = float('inf'); bn.bias[1] = float('-inf'); bn.weight[2] = float('nan')
            bn.weight[3] = 0.0; bn.weight[4] = -0.0
            bn.running_mean[5] = 0.0; bn.bias[5] = 0.0
            bn.weight[6] = 1e-44; bn.running_mean[6] = 0.0; bn.bias[6] = -0.0
            bn.weight[c - 1] = -3e38
    return bn.to(dev).eval()


def _salt(x, seed):
    """+-inf, NaN, zeros of both signs and magnitudes that underflow to a signed zero behind a scale, at scattered positions"""
    g = torch.Generator().manual_seed(seed)
    flat = x.view(-1)
    vals = [float('inf'), float('-inf'), float('nan'), 0.0, -0.0, 1e-45, -1e-45, -1e-38, 3e38, -3e38]
    n = min(50 * len(vals), flat.numel())
    idx = torch.randperm(flat.numel(), generator=g)[:n].to(x.device)
    for k, v in enumerate(vals):
        flat[idx[k::len(vals)]] = v
    return x


def _conv(cin, cout, dev, seed, integer=False):
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 1, bias=False)
    with torch.no_grad():
        if integer:
            conv.weight.copy_(torch.randint(-7, 8, (cout, cin, 1, 1), generator=g).float())
        else:
            conv.weight.copy_(torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5)      # He scale
    return conv.to(dev).eval()


def _conv64(x, conv, magnitudes=False):
    """the convolution in float64, [B, Cout, Ho, Wo] (magnitudes: of |x| and |w|); columns + matrix product, any kernel size"""
    import torch.nn.functional as F
    w = conv.weight.detach().double().flatten(1)
    xd = x.double()
    if magnitudes:
        w, xd = w.abs(), xd.abs()
    B, _, H, W = x.shape
    if tuple(conv.kernel_size) == (1, 1) and tuple(conv.stride) == (1, 1):
        return torch.einsum('oc,bchw->bohw', w, xd)
    cols = F.unfold(xd, conv.kernel_size, conv.dilation, conv.padding, conv.stride)
    ho = (H + 2 * conv.padding[0] - conv.dilation[0] * (conv.kernel_size[0] - 1) - 1) // conv.stride[0] + 1
    return torch.einsum('ok,bkl->bol', w, cols).reshape(B, w.size(0), ho, -1)


# positions of a workgroup tile: 64 or 128 (the launch chooses; `_tile` asks).  16 x 16 is a multiple of both, 1 x 257 one past it.
# These small maps run the 64 x 64 and 64 x 128 (channels x positions) tiles; the 128 x 128 tile has its own cases below.
MAPS = [(1, 1), (7, 9), (30, 22), (33, 31), (16, 16), (1, 257)]
CINS = [64, 128, 256, 512, 2048]
COUTS = [64, 96, 256, 2048]


@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("cin", CINS)
def test_exact_cases_bit_for_bit(dev, cin, cout):
    """integer data, |x| <= 15 and |w| <= 7 (Cin * 105 < 2^24): float64 conv2d cast to fp32, then the bn_act launches, against the
    fused launch -- every map size x batch (3: the image seam) x residual form x ReLU, salted residual and BatchNorm constants"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, conv1x1_bn_act
    assert _lib.lib().orp_conv1x1_bn_act_ok(cin, cout) == 1
    conv = _conv(cin, cout, dev, 100 + cin + cout, integer=True)
    bn, bnd = _bn(cout, dev, 7, salted=True), _bn(cout, dev, 8, salted=True)
    g = torch.Generator(device=dev).manual_seed(cin * 7 + cout)
    runs = 0
    with torch.no_grad():
        for (h, w) in MAPS:
            for B in (1, 3):
                x = torch.randint(-15, 16, (B, cin, h, w), device=dev, generator=g).float()
                raw = _conv64(x, conv).float().contiguous()
                r = _salt(torch.randn((B, cout, h, w), device=dev, generator=g) * 2 + 0.5, h * 10 + B)
                for residual, residual_bn in ((None, None), (r, None), (r, bnd)):
                    for relu in (False, True):
                        want = bn_act(raw.clone(), bn, residual=residual, residual_bn=residual_bn, relu=relu)
                        got = conv1x1_bn_act(x, conv, bn, residual=residual, residual_bn=residual_bn, relu=relu, force=True)
                        assert got.data_ptr() != x.data_ptr() and got.is_contiguous()
                        assert _same_bits(got, want), (cin, cout, h, w, B, residual is not None, residual_bn is not None, relu)
                        runs += 1
    assert runs == len(MAPS) * 2 * 3 * 2


def _tile(cin, cout, hw, batch):
    import ctypes
    from orientedreppoints_amd import _lib
    bm, bn = ctypes.c_int(0), ctypes.c_int(0)
    assert _lib.lib().orp_conv1x1_bn_act_tile(cin, cout, hw, batch, ctypes.byref(bm), ctypes.byref(bn)) == 1
    return bm.value, bn.value


def test_exact_cases_cover_the_two_narrow_tiles():
    """the launches of test_exact_cases_bit_for_bit run both narrow tiles (host-side query, no launch)"""
    seen = {_tile(cin, cout, h * w, B) for cin in CINS for cout in COUTS for (h, w) in MAPS for B in (1, 3)}
    assert seen == {(64, 64), (64, 128)}


# (Cin, Cout, H, W) at B = 3 that the launch runs with the 128 x 128 tile (it takes the tile only where that leaves 512 workgroups):
# 37 x 35 = 1295 positions, odd -> 4-byte input loads, last tile ragged; 36 x 36 = 1296 -> 16-byte loads, last tile 16 positions, and
# 1984 channels end in the middle of a channel tile; 32 x 44 = 1408 = 11 whole tiles; 105 x 105 = 11025 with 256 channels: the stage 1 /
# stage 2 form (two channel tiles, many position tiles).  Three images: two seams inside the grid.
WIDE = [(64, 2048, 37, 35), (128, 1984, 36, 36), (64, 2048, 32, 44), (64, 256, 105, 105)]


@pytest.mark.parametrize("cin,cout,h,w", WIDE)
def test_exact_cases_on_the_128_x_128_tile(dev, cin, cout, h, w):
    """as test_exact_cases_bit_for_bit, at shapes the launch provably runs with the 128 x 128 tile"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, conv1x1_bn_act
    B = 3
    assert _tile(cin, cout, h * w, B) == (128, 128)
    conv = _conv(cin, cout, dev, 300 + cin + cout, integer=True)
    bn, bnd = _bn(cout, dev, 17, salted=True), _bn(cout, dev, 18, salted=True)
    g = torch.Generator(device=dev).manual_seed(cin + cout + h)
    with torch.no_grad():
        x = torch.randint(-15, 16, (B, cin, h, w), device=dev, generator=g).float()
        raw = _conv64(x, conv).float().contiguous()
        r = _salt(torch.randn((B, cout, h, w), device=dev, generator=g) * 2 + 0.5, h)
        for residual, residual_bn in ((None, None), (r, None), (r, bnd)):
            for relu in (False, True):
                want = bn_act(raw.clone(), bn, residual=residual, residual_bn=residual_bn, relu=relu)
                got = conv1x1_bn_act(x, conv, bn, residual=residual, residual_bn=residual_bn, relu=relu, force=True)
                assert _same_bits(got, want), (residual is not None, residual_bn is not None, relu)


def test_random_data_on_the_128_x_128_tile(dev):
    """N(0, 1) data, 64 -> 256 (stage 1's conv3) at 105 x 105 x 3 images, against float64 inside the derived bound"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine, conv1x1_bn_act
    cin, cout, h, w, B = 64, 256, 105, 105, 3
    assert _tile(cin, cout, h * w, B) == (128, 128)
    conv, bn = _conv(cin, cout, dev, 51), _bn(cout, dev, 52)
    g = torch.Generator(device=dev).manual_seed(53)
    x = torch.randn((B, cin, h, w), device=dev, generator=g)
    r = torch.randn((B, cout, h, w), device=dev, generator=g)
    with torch.no_grad():
        a, b = [t.double() for t in _bn_affine(bn)]
        ref = torch.relu(_conv64(x, conv) * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1) + r.double())
        got = conv1x1_bn_act(x, conv, bn, residual=r, relu=True, force=True)
        assert float(((got.double() - ref).abs() / _bound(x, conv, a, b, r)).max()) <= 1.0


def test_non_finite_inputs(dev):
    """+-inf / NaN in x: finite outputs bit-equal, non-finite ones of the same class as the float64 reference"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, conv1x1_bn_act
    cin, cout = 128, 96
    conv = _conv(cin, cout, dev, 3, integer=True)
    bn = _bn(cout, dev, 9)
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randint(-15, 16, (2, cin, 33, 31), device=dev, generator=g).float()
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(6))[:90].to(dev)
    for k, v in enumerate((float('inf'), float('-inf'), float('nan'))):
        flat[idx[k::3]] = v
    with torch.no_grad():
        want = bn_act(_conv64(x, conv).float().contiguous(), bn, relu=False)
        got = conv1x1_bn_act(x, conv, bn, relu=False, force=True)
    fin = torch.isfinite(want)
    assert int((~fin).sum()) > 0 and torch.equal(fin, torch.isfinite(got))
    assert np.array_equal(_bits(got[fin]), _bits(want[fin]))
    assert torch.equal(torch.isnan(want), torch.isnan(got))
    inf = torch.isinf(want)
    assert torch.equal(torch.sign(want[inf]), torch.sign(got[inf]))


R50_CONV3 = [(64, 256), (128, 512), (256, 1024), (512, 2048)]


def _bound(x, conv, a, b, r):
    """(K + 2) 2^-24 (|a| sum_k |x_k w_k| + |b| + |r|) per output, in float64 (K = Cin for the 1x1 convolutions): K products and sums
    of the fp32 chain, the affine's fma and the residual add, each one rounding of at most 2^-24 relative to a partial result that
    the bracket bounds"""
    t = a.abs().view(1, -1, 1, 1) * _conv64(x, conv, magnitudes=True) + b.abs().view(1, -1, 1, 1)
    if r is not None:
        t = t + r.double().abs()
    return (conv.weight[0].numel() + 2) * 2.0 ** -24 * t


@pytest.mark.parametrize("cin,cout", R50_CONV3)
def test_random_data_inside_the_derived_bound(dev, cin, cout):
    """N(0, 1) activations, He-scale weights, the R-50 conv3 pairs at a 24 x 40 map, against float64 conv + affine; the library path
    (conv + bn_act) has to stay inside the same bound on the same inputs"""
    import conftest
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine, bn_act, conv1x1_bn_act
    conv = _conv(cin, cout, dev, 40 + cin)
    bn = _bn(cout, dev, 41)
    g = torch.Generator(device=dev).manual_seed(cin)
    x = torch.randn((2, cin, 24, 40), device=dev, generator=g)
    r = torch.randn((2, cout, 24, 40), device=dev, generator=g)
    with torch.no_grad():
        a, b = [t.double() for t in _bn_affine(bn)]
        ref = torch.relu(_conv64(x, conv) * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1) + r.double())
        bound = _bound(x, conv, a, b, r)
        got = conv1x1_bn_act(x, conv, bn, residual=r, relu=True, force=True)
        lib = bn_act(conv(x).contiguous(), bn, residual=r, relu=True)
    ours = float(((got.double() - ref).abs() / bound).max())
    theirs = float(((lib.double() - ref).abs() / bound).max())
    conftest.REPORT.append("1x1 convolution + BatchNorm + residual + ReLU %d -> %d at 24 x 40, worst |err| / bound vs float64: fused %.3f, "
                           "library + pass %.3f" % (cin, cout, ours, theirs))
    assert ours <= 1.0
    assert theirs <= 1.0


def test_same_launch_twice_gives_the_same_bits(dev):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act
    conv, bn, bnd = _conv(256, 1024, dev, 1), _bn(1024, dev, 2), _bn(1024, dev, 3)
    g = torch.Generator(device=dev).manual_seed(4)
    x = torch.randn((2, 256, 33, 31), device=dev, generator=g)
    r = torch.randn((2, 1024, 33, 31), device=dev, generator=g)
    with torch.no_grad():
        y0 = conv1x1_bn_act(x, conv, bn, residual=r, residual_bn=bnd, force=True)
        y1 = conv1x1_bn_act(x, conv, bn, residual=r, residual_bn=bnd, force=True)
    assert _same_bits(y0, y1)


def _force_fused(monkeypatch):
    """the Bottleneck's calls of conv1x1_bn_act take the fused kernel at every supported shape, whatever the routing rule says"""
    from orientedreppoints_amd.mmdet_ops import fused_norm
    monkeypatch.setattr(fused_norm, 'conv1x1_bn_act', functools.partial(fused_norm.conv1x1_bn_act, force=True))


def _launch_counter(monkeypatch):
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    orig = L.orp_conv1x1_bn_act
    calls = []

    def spy(*args):
        calls.append(1)
        return orig(*args)
    monkeypatch.setattr(L, 'orp_conv1x1_bn_act', spy)
    return calls


def _bottleneck(dev, inplanes, planes, stride=1, downsample=None):
    from orientedreppoints_amd.mmdet_models.resnet import Bottleneck
    torch.manual_seed(5)
    blk = Bottleneck(inplanes, planes, stride=stride, downsample=downsample).to(dev).eval()
    for i, m in enumerate(m for m in blk.modules() if isinstance(m, torch.nn.BatchNorm2d)):
        m.load_state_dict(_bn(m.num_features, dev, 20 + i).state_dict())
    return blk


def test_captured_bottleneck_replays_the_eager_bits(dev, monkeypatch):
    _force_fused(monkeypatch)
    calls = _launch_counter(monkeypatch)
    blk = _bottleneck(dev, 256, 64)
    x = torch.randn(2, 256, 30, 22, device=dev)
    with torch.no_grad():
        eager = blk(x).clone()
        assert len(calls) == 2                      # conv1 and conv3
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            blk(x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = blk(x)
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert _same_bits(out, eager)


def _stage_bound(x, conv, bn, r=None):
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine
    a, b = [t.double() for t in _bn_affine(bn)]
    return float(_bound(x, conv, a, b, r).max())


def _gain(conv, bn):
    """max over outputs of |a| sum |w|: how far a difference of the inputs can grow through conv + BatchNorm"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine
    a = _bn_affine(bn)[0].double()
    return float((conv.weight.detach().double().flatten(1).abs().sum(1) * a.abs()).max())


def test_bottleneck_switch_at_a_supported_shape(dev, monkeypatch):
    """switch off / on: the outputs agree within the bound of the random-data test carried through the block -- both paths are within
    the bound of float64 at conv1 (so within twice the bound of each other), a difference d of a stage's inputs grows by at most
    max_c |a_c| sum |w_c| through the next convolution + BatchNorm (ReLU and the residual add do not enlarge it), and each later
    stage adds twice its own bound; with grad enabled the module path runs"""
    _force_fused(monkeypatch)
    calls = _launch_counter(monkeypatch)
    blk = _bottleneck(dev, 256, 64)
    x = torch.randn(2, 256, 30, 22, device=dev)
    outs = {}
    with torch.no_grad():
        for flag in (False, True):
            blk.fuse_conv1x1 = flag
            assert blk._conv1x1_fusable() == flag
            n0 = len(calls)
            outs[flag] = blk(x.clone())
            assert len(calls) - n0 == (2 if flag else 0)
        del blk.fuse_conv1x1
        assert blk._conv1x1_fusable()               # default: on
        t1 = torch.relu(blk.bn1(blk.conv1(x)))
        t2 = torch.relu(blk.bn2(blk.conv2(t1)))
        d = 2 * _stage_bound(x, blk.conv1, blk.bn1)
        d = d * _gain(blk.conv2, blk.bn2) + 2 * _stage_bound(t1, blk.conv2, blk.bn2)
        d = d * _gain(blk.conv3, blk.bn3) + 2 * _stage_bound(t2, blk.conv3, blk.bn3, x)
    assert float((outs[True] - outs[False]).abs().max()) <= d
    n0 = len(calls)
    with torch.enable_grad():
        stock = blk(x.clone())                      # autograd on: the unfused module path
    assert len(calls) == n0 and stock.requires_grad
    assert float((outs[True] - stock.detach()).abs().max()) <= 2 * d


def test_bottleneck_at_an_unsupported_shape_and_downsample_switch(dev, monkeypatch):
    """inplanes 64 / planes 32 (conv1 has 32 outputs, conv3 32 inputs: not in the supported set), the stride-2 block of the
    fall-back test: switch off / on give the same bits.  At a supported shape, fuse_downsample_norm False / True with the new switch
    on give the same bits (plain residual of the normalised identity = residual with its affine in the epilogue)."""
    nn = torch.nn
    _force_fused(monkeypatch)
    calls = _launch_counter(monkeypatch)
    ds = nn.Sequential(nn.Conv2d(64, 128, 1, stride=2, bias=False), nn.BatchNorm2d(128))
    blk = _bottleneck(dev, 64, 32, stride=2, downsample=ds)
    x = torch.randn(2, 64, 30, 22, device=dev)
    with torch.no_grad():
        blk.fuse_conv1x1 = False
        off = blk(x.clone())
        blk.fuse_conv1x1 = True
        on = blk(x.clone())
    assert _same_bits(on, off) and len(calls) == 0
    # (stage 1's first block: stride 1, a 64 -> 256 downsample branch -- a shape at which the library's convolutions return the same
    # bits on every call, as the comparison needs; docs/notebook/round12.md has one at which they do not)
    ds = nn.Sequential(nn.Conv2d(64, 256, 1, bias=False), nn.BatchNorm2d(256))
    blk = _bottleneck(dev, 64, 64, stride=1, downsample=ds)
    x = torch.randn(2, 64, 30, 22, device=dev)
    outs = {}
    with torch.no_grad():
        for flag in (False, True):
            blk.fuse_downsample_norm = flag
            n0 = len(calls)
            outs[flag] = blk(x.clone())
            assert len(calls) - n0 == 2
    assert _same_bits(outs[True], outs[False])


def test_routing_query_is_consulted_and_force_bypasses_it(dev, monkeypatch):
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, conv1x1_bn_act
    L = _lib.lib()
    calls = _launch_counter(monkeypatch)
    asked, answer = [], [0]

    def pays(*args):
        asked.append(args)
        return answer[0]
    monkeypatch.setattr(L, 'orp_conv1x1_bn_act_pays', pays)
    conv, bn = _conv(64, 256, dev, 1), _bn(256, dev, 2)
    x = torch.randn(1, 64, 16, 16, device=dev)
    with torch.no_grad():
        want = bn_act(conv(x).contiguous(), bn, relu=True)
        y = conv1x1_bn_act(x, conv, bn)                          # does not pay: library + pass
        assert asked == [(64, 256, 256, 1, 0)] and len(calls) == 0 and _same_bits(y, want)
        answer[0] = 1
        conv1x1_bn_act(x, conv, bn, residual=want)               # pays: the fused launch
        assert asked[1:] == [(64, 256, 256, 1, 1)] and len(calls) == 1
        answer[0] = 0
        conv1x1_bn_act(x, conv, bn, force=True)                  # forced: not asked
        assert len(asked) == 2 and len(calls) == 2
        small = _conv(32, 64, dev, 3)                            # unsupported (Cin < 64): library + pass even when forced
        xs = torch.randn(1, 32, 8, 8, device=dev)
        bns = _bn(64, dev, 4)
        assert _same_bits(conv1x1_bn_act(xs, small, bns, force=True), bn_act(small(xs).contiguous(), bns, relu=True))
        assert len(calls) == 2
