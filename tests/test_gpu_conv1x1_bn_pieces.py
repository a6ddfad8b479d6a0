"""GPU: the bottleneck 1x1 convolution on the bf16-pieces matrix path with BatchNorm (+ residual) + ReLU in its epilogue
(orp_conv1x1_bn_act_pieces; conv1x1_bn_act(pieces=True)).

Exact cases bit for bit against a float64 convolution cast to fp32 followed by the passes the epilogue replaces -- small integers
(x0 w0 alone) over every pair x map x batch x residual form x ReLU and every tile shape, and three constructions that need each of
the six products; random data, the range edges 2^100 and 2^-100 and the fp32 kernel on the same inputs against float64 inside the
fp32 file's bound; non-finite inputs, the range word, reproducibility, graph capture, the Bottleneck call site and the routing."""
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
    """the 1x1 convolution in float64, [B, Cout, H, W] (magnitudes: of |x| and |w|)"""
    w = conv.weight.detach().double().flatten(1)
    xd = x.double()
    if magnitudes:
        w, xd = w.abs(), xd.abs()
    return torch.einsum('oc,bchw->bohw', w, xd)


def _bound(x, conv, a, b, r):
    """the fp32 file's bound: (K + 2) 2^-24 (|a| sum_k |x_k w_k| + |b| + |r|) per output, in float64 (K = Cin)"""
    t = a.abs().view(1, -1, 1, 1) * _conv64(x, conv, magnitudes=True) + b.abs().view(1, -1, 1, 1)
    if r is not None:
        t = t + r.double().abs()
    return (conv.weight[0].numel() + 2) * 2.0 ** -24 * t


def _tile(cin, cout, hw, batch):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act_pieces_tile
    t = conv1x1_bn_act_pieces_tile(cin, cout, hw, batch)
    assert t is not None
    return t


def _spy(monkeypatch, name='orp_conv1x1_bn_act_pieces'):
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    orig = getattr(L, name)
    calls = []

    def spy(*args):
        calls.append(args)
        return orig(*args)
    monkeypatch.setattr(L, name, spy)
    return calls


PAIRS = [(64, 64), (256, 64), (128, 512), (1024, 256), (2048, 512), (512, 2048), (64, 96)]
SMALL_MAPS = [(1, 1), (7, 9), (33, 31), (1, 257)]


def _narrow_positions(cout):
    """positions of the workgroup tile these small maps run with: the 2 x 2 layout's 128 at 64 channels, else the narrowest"""
    return 128 if cout <= 64 else 32


def _maps(cout):
    bn = _narrow_positions(cout)
    return SMALL_MAPS + [(1, bn), (1, bn + 1)]           # one whole position tile, one position more


def _check_forms(dev, conv, bn, bnd, x, r, tag):
    """every residual form x ReLU: the pieces launch against float64 conv cast to fp32 + the bn_act launches, bit for bit"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, conv1x1_bn_act
    raw = _conv64(x, conv).float().contiguous()
    runs = 0
    for residual, residual_bn in ((None, None), (r, None), (r, bnd)):
        for relu in (False, True):
            want = bn_act(raw.clone(), bn, residual=residual, residual_bn=residual_bn, relu=relu)
            got = conv1x1_bn_act(x, conv, bn, residual=residual, residual_bn=residual_bn, relu=relu, pieces=True)
            assert got.data_ptr() != x.data_ptr() and got.is_contiguous()
            assert _same_bits(got, want), tag + (residual is not None, residual_bn is not None, relu)
            runs += 1
    return runs


@pytest.mark.parametrize("cin,cout", PAIRS)
def test_exact_cases_bit_for_bit(dev, monkeypatch, cin, cout):
    """integer data, |x| <= 15 and |w| <= 7 (Cin * 105 < 2^24; one bf16 piece each: x0 w0 alone): every map size x batch (3: the
    image seam) x residual form x ReLU, salted residual and BatchNorm constants"""
    from orientedreppoints_amd import _lib
    assert _lib.lib().orp_conv1x1_bn_act_pieces_ok(cin, cout) == 1
    calls = _spy(monkeypatch)
    conv = _conv(cin, cout, dev, 100 + cin + cout, integer=True)
    bn, bnd = _bn(cout, dev, 7, salted=True), _bn(cout, dev, 8, salted=True)
    g = torch.Generator(device=dev).manual_seed(cin * 7 + cout)
    runs = 0
    with torch.no_grad():
        for (h, w) in _maps(cout):
            for B in (1, 3):
                if h * w in (_narrow_positions(cout), _narrow_positions(cout) + 1):      # the whole tile / one position more
                    assert _tile(cin, cout, h * w, B)[1] == _narrow_positions(cout)
                x = torch.randint(-15, 16, (B, cin, h, w), device=dev, generator=g).float()
                r = _salt(torch.randn((B, cout, h, w), device=dev, generator=g) * 2 + 0.5, h * 10 + B)
                runs += _check_forms(dev, conv, bn, bnd, x, r, (cin, cout, h, w, B))
    assert runs == 6 * 2 * 3 * 2 and len(calls) == runs


# (Cin, Cout, H, W) at B = 3 on the two wide tiles (the launch takes a tile only where that leaves 512 workgroups).  128 x 128:
# 37 x 35 = 1295 positions, odd -> 4-byte input loads, last tile ragged; 36 x 36 = 1296 -> 16-byte loads, last tile 16 positions, and
# 1984 channels end in the middle of a channel tile.  128 x 64: 28 x 24 = 672 -> 16-byte loads, last tile 32 positions; 27 x 25 = 675.
WIDE = [(64, 2048, 37, 35, (128, 128)), (128, 1984, 36, 36, (128, 128)), (64, 2048, 28, 24, (128, 64)), (128, 1984, 27, 25, (128, 64))]


@pytest.mark.parametrize("cin,cout,h,w,tile", WIDE)
def test_exact_cases_on_the_wide_tiles(dev, cin, cout, h, w, tile):
    B = 3
    assert _tile(cin, cout, h * w, B) == tile
    conv = _conv(cin, cout, dev, 300 + cin + cout, integer=True)
    bn, bnd = _bn(cout, dev, 17, salted=True), _bn(cout, dev, 18, salted=True)
    g = torch.Generator(device=dev).manual_seed(cin + cout + h)
    with torch.no_grad():
        x = torch.randint(-15, 16, (B, cin, h, w), device=dev, generator=g).float()
        r = _salt(torch.randn((B, cout, h, w), device=dev, generator=g) * 2 + 0.5, h)
        assert _check_forms(dev, conv, bn, bnd, x, r, (cin, cout, h, w, B)) == 6


def test_exact_cases_cover_every_tile():
    """the launches of the two tests above run every tile shape the kernel has (host-side query, no launch)"""
    seen = {_tile(cin, cout, h * w, B) for (cin, cout) in PAIRS for (h, w) in _maps(cout) for B in (1, 3)}
    assert seen >= {(64, 128), (128, 32)}
    seen |= {_tile(cin, cout, h * w, 3) for (cin, cout, h, w, _t) in WIDE}
    assert seen == {(64, 128), (128, 32), (128, 64), (128, 128)}


def _wide_ints(shape, bits, g, dev):
    """odd integers of exactly `bits` significant bits (a tensor of per-element bit counts, broadcast to shape), random sign"""
    bits = bits.expand(shape).to(torch.int64)
    hi = torch.ones(shape, dtype=torch.int64, device=dev) << (bits - 1)
    u = (torch.rand(shape, device=dev, generator=g, dtype=torch.float64) * hi.double()).to(torch.int64).clamp_(max=(1 << 23) - 1)
    v = ((hi + u % hi) | 1).double()
    return torch.where(torch.rand(shape, device=dev, generator=g) < 0.5, -v, v)


def _keep_some(shape, dim, count, g, dev):
    """0 / 1 mask with exactly count[...] ones along `dim` (count broadcast over the other dimensions), at random places"""
    rank = torch.rand(shape, device=dev, generator=g).argsort(dim=dim).argsort(dim=dim)
    return (rank < count).double()


@pytest.mark.parametrize("kind", ["wide x", "wide w", "both two pieces"])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_exact_cases_that_need_each_product(dev, cin, cout, kind):
    """integers below 2^8 exercise x0 w0 alone.  Three constructions of integer data whose every partial sum stays an integer below
    2^24, so that a dropped, doubled or mis-paired product is a wrong bit:
      wide x: x odd with 24, 23, 22 or 20 significant bits (all three pieces non-zero) in 1, 2, 4 or 16 channels of a position and
              zero in the others, w in {-1, 0, 1} -- x0 w0, x1 w0, x2 w0;
      wide w: the mirror -- w odd with 24 .. 20 bits in 1 .. 16 input channels of an output channel, x in {-1, 0, 1}: x0 w0, x0 w1, x0 w2;
      both two pieces: ONE non-zero channel c per position, w[:, c] odd with 9 + c % 7 bits and x there odd with 24 minus that
              (15 .. 9) bits: the 24-bit product is x0 w0 + x0 w1 + x1 w0 + x1 w1."""
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, conv1x1_bn_act
    B, h, w = 1, 33, 31
    g = torch.Generator(device=dev).manual_seed(cin + 3 * cout + len(kind))
    nz = torch.tensor([1, 2, 4, 16], device=dev)
    nbits = torch.tensor([24, 23, 22, 20], device=dev)
    if kind == "wide x":
        sel = torch.randint(0, 4, (B, 1, h, w), device=dev, generator=g)
        x = _wide_ints((B, cin, h, w), nbits[sel], g, dev) * _keep_some((B, cin, h, w), 1, nz[sel], g, dev)
        wt = torch.randint(-1, 2, (cout, cin), device=dev, generator=g).double()
    elif kind == "wide w":
        sel = torch.randint(0, 4, (cout, 1), device=dev, generator=g)
        wt = _wide_ints((cout, cin), nbits[sel], g, dev) * _keep_some((cout, cin), 1, nz[sel], g, dev)
        x = torch.randint(-1, 2, (B, cin, h, w), device=dev, generator=g).double()
    else:
        wbits = (9 + torch.arange(cin, device=dev) % 7)
        wt = _wide_ints((cout, cin), wbits.view(1, cin), g, dev)
        x = _wide_ints((B, cin, h, w), (24 - wbits).view(1, cin, 1, 1), g, dev) * _keep_some((B, cin, h, w), 1, 1, g, dev)
    assert float(torch.einsum('oc,bchw->bohw', wt.abs(), x.abs()).max()) < 2.0 ** 24        # every partial sum below 2^24
    conv = _conv(cin, cout, dev, 1, integer=True)
    bn = _bn(cout, dev, 27)
    with torch.no_grad():
        conv.weight.copy_(wt.float().view(cout, cin, 1, 1))
        x = x.float()
        assert torch.equal(conv.weight.double().flatten(1), wt)
        raw = _conv64(x, conv).float().contiguous()
        assert torch.equal(raw.double(), _conv64(x, conv))                    # the reference itself is exact in fp32
        for relu in (False, True):
            want = bn_act(raw.clone(), bn, relu=relu)
            got = conv1x1_bn_act(x, conv, bn, relu=relu, pieces=True)
            assert _same_bits(got, want), (kind, cin, cout, relu)


R50_CONV3 = [(64, 256), (128, 512), (256, 1024), (512, 2048)]
RANDOM_PAIRS = R50_CONV3 + [(1024, 256), (2048, 512)]
_random_cache = {}


def _random_case(dev, cin, cout):
    """N(0, 1) activations, He-scale weights, 24 x 40 x 2 images, a residual; computed once per pair and left unchanged"""
    key = (cin, cout)
    if key not in _random_cache:
        conv, bn = _conv(cin, cout, dev, 40 + cin), _bn(cout, dev, 41)
        g = torch.Generator(device=dev).manual_seed(cin)
        x = torch.randn((2, cin, 24, 40), device=dev, generator=g)
        r = torch.randn((2, cout, 24, 40), device=dev, generator=g)
        _random_cache[key] = (conv, bn, x, r)
    return _random_cache[key]


def _worst_ratio(x, conv, bn, r, got):
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine
    a, b = [t.double() for t in _bn_affine(bn)]
    ref = torch.relu(_conv64(x, conv) * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1) + r.double())
    return float(((got.double() - ref).abs() / _bound(x, conv, a, b, r)).max())


@pytest.mark.parametrize("cin,cout", RANDOM_PAIRS)
def test_random_data_inside_the_derived_bound(dev, cin, cout):
    """against float64 conv + affine + residual + ReLU inside the fp32 file's bound; the fp32 kernel on the same inputs is reported"""
    import conftest
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act
    conv, bn, x, r = _random_case(dev, cin, cout)
    with torch.no_grad():
        ours = _worst_ratio(x, conv, bn, r, conv1x1_bn_act(x, conv, bn, residual=r, relu=True, pieces=True))
        fp32 = _worst_ratio(x, conv, bn, r, conv1x1_bn_act(x, conv, bn, residual=r, relu=True, force=True))
    conftest.REPORT.append("1x1 convolution + BatchNorm + residual + ReLU %d -> %d at 24 x 40, worst |err| / bound vs float64: bf16 pieces "
                           "%.3f, fp32 fused %.3f" % (cin, cout, ours, fp32))
    assert ours <= 1.0


@pytest.mark.parametrize("exponent", [100, -100])
@pytest.mark.parametrize("cin,cout", RANDOM_PAIRS)
def test_range_edges_inside_the_bound(dev, cin, cout, exponent):
    """the same data with x scaled by 2^100 / 2^-100 stays inside the same bound: bf16 pieces carry fp32's exponent, which is what
    makes a range word unnecessary"""
    import conftest
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act
    conv, bn, x, r = _random_case(dev, cin, cout)
    xs = x * 2.0 ** exponent
    with torch.no_grad():
        ours = _worst_ratio(xs, conv, bn, r, conv1x1_bn_act(xs, conv, bn, residual=r, relu=True, pieces=True))
    conftest.REPORT.append("1x1 bf16 pieces %d -> %d, x scaled by 2^%d: worst |err| / bound %.3f" % (cin, cout, exponent, ours))
    assert ours <= 1.0


def test_non_finite_inputs(dev):
    """+-inf / NaN in x: the outputs are non-finite exactly where the float64 reference's are (every channel of those positions, of
    possibly another class: NaN where the reference has inf), and bit-equal everywhere else"""
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
        got = conv1x1_bn_act(x, conv, bn, relu=False, pieces=True)
    fin = torch.isfinite(want)
    bad_positions = (~torch.isfinite(x)).any(dim=1, keepdim=True).expand_as(want)
    assert int((~fin).sum()) > 0 and torch.equal(~fin, bad_positions)
    assert torch.equal(fin, torch.isfinite(got))
    assert np.array_equal(_bits(got[fin]), _bits(want[fin]))


def _range_bits(x):
    """max over the finite elements of |x| as float bits (orp_range.hpp: range_bits), a one-element int32 tensor"""
    a = x.detach().abs()
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    return a.max().reshape(1).contiguous().view(torch.int32)


@pytest.mark.parametrize("cin,cout,h,w", [(256, 64, 33, 31), (512, 128, 7, 9), (1024, 256, 1, 257), (256, 128, 16, 16)])
def test_the_range_word(dev, cin, cout, h, w):
    """want_range: the word equals torch's maximum of range_bits(y) -- ragged tiles, three images, Inf / NaN in y (salted BatchNorm)
    -- and y has the bits of the launch without it"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act
    conv = _conv(cin, cout, dev, 60 + cin)
    g = torch.Generator(device=dev).manual_seed(h)
    x = torch.randn((3, cin, h, w), device=dev, generator=g)
    with torch.no_grad():
        for salted in (False, True):
            bn = _bn(cout, dev, 61, salted=salted)
            y, bits = conv1x1_bn_act(x, conv, bn, relu=True, pieces=True, want_range=True)
            assert int(bits.item()) == int(_range_bits(y).item()) and int(bits.item()) > 0
            assert _same_bits(y, conv1x1_bn_act(x, conv, bn, relu=True, pieces=True))


def test_same_launch_twice_gives_the_same_bits(dev):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act
    conv, bn, bnd = _conv(256, 1024, dev, 1), _bn(1024, dev, 2), _bn(1024, dev, 3)
    g = torch.Generator(device=dev).manual_seed(4)
    x = torch.randn((2, 256, 33, 31), device=dev, generator=g)
    r = torch.randn((2, 1024, 33, 31), device=dev, generator=g)
    with torch.no_grad():
        y0 = conv1x1_bn_act(x, conv, bn, residual=r, residual_bn=bnd, pieces=True)
        y1 = conv1x1_bn_act(x, conv, bn, residual=r, residual_bn=bnd, pieces=True)
    assert _same_bits(y0, y1)


def _bottleneck(dev, inplanes, planes, stride=1, downsample=None):
    from orientedreppoints_amd.mmdet_models.resnet import Bottleneck
    torch.manual_seed(5)
    blk = Bottleneck(inplanes, planes, stride=stride, downsample=downsample).to(dev).eval()
    for i, m in enumerate(m for m in blk.modules() if isinstance(m, torch.nn.BatchNorm2d)):
        m.load_state_dict(_bn(m.num_features, dev, 20 + i).state_dict())
    return blk


def _table_says(monkeypatch, answer):
    """the pieces table answers `answer[0]` at every shape; returns the list of what it was asked"""
    from orientedreppoints_amd import _lib
    asked = []

    def pays(*args):
        asked.append(args)
        return answer[0]
    monkeypatch.setattr(_lib.lib(), 'orp_conv1x1_bn_act_pieces_pays', pays)
    return asked


def test_captured_bottleneck_replays_the_eager_bits(dev, monkeypatch):
    _table_says(monkeypatch, [1])
    calls = _spy(monkeypatch)
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
    if tuple(conv.kernel_size) == (1, 1):
        return float(_bound(x, conv, a, b, r).max())
    import torch.nn.functional as F           # conv2: K = 9 Cin products per output
    mag = F.conv2d(x.double().abs(), conv.weight.detach().double().abs(), padding=conv.padding)
    t = a.abs().view(1, -1, 1, 1) * mag + b.abs().view(1, -1, 1, 1)
    return float(((conv.weight[0].numel() + 2) * 2.0 ** -24 * t).max())


def _gain(conv, bn):
    """max over outputs of |a| sum |w|: how far a difference of the inputs can grow through conv + BatchNorm"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine
    a = _bn_affine(bn)[0].double()
    return float((conv.weight.detach().double().flatten(1).abs().sum(1) * a.abs()).max())


def test_bottleneck_pieces_switch_at_a_supported_shape(dev, monkeypatch):
    """fuse_conv1x1_pieces off / on with the table saying yes: the outputs agree within the bound of the random-data test carried
    through the block, as test_gpu_conv1x1_bn.py::test_bottleneck_switch_at_a_supported_shape -- both paths are within the bound of
    float64 at conv1 (so within twice the bound of each other), a difference d of a stage's inputs grows by at most
    max_c |a_c| sum |w_c| through the next convolution + BatchNorm, and each later stage adds twice its own bound"""
    _table_says(monkeypatch, [1])
    calls = _spy(monkeypatch)
    blk = _bottleneck(dev, 256, 64)
    x = torch.randn(2, 256, 30, 22, device=dev)
    outs = {}
    with torch.no_grad():
        for flag in (False, True):
            blk.fuse_conv1x1_pieces = flag
            assert blk._conv1x1_pieces_on() == flag
            n0 = len(calls)
            outs[flag] = blk(x.clone())
            assert len(calls) - n0 == (2 if flag else 0)
        del blk.fuse_conv1x1_pieces
        assert blk._conv1x1_pieces_on()               # default: on
        t1 = torch.relu(blk.bn1(blk.conv1(x)))
        t2 = torch.relu(blk.bn2(blk.conv2(t1)))
        d = 2 * _stage_bound(x, blk.conv1, blk.bn1)
        d = d * _gain(blk.conv2, blk.bn2) + 2 * _stage_bound(t1, blk.conv2, blk.bn2)
        d = d * _gain(blk.conv3, blk.bn3) + 2 * _stage_bound(t2, blk.conv3, blk.bn3, x)
    assert float((outs[True] - outs[False]).abs().max()) <= d
    n0 = len(calls)
    with torch.enable_grad():
        blk(x.clone())                                # autograd on: the unfused module path
    assert len(calls) == n0


def test_switch_off_gives_the_launches_and_bits_of_before(dev, monkeypatch):
    """the attribute off with the table saying yes = the attribute on with the table saying no: no pieces launch, the same bits
    (stage 1's first block at a shape where the library's convolutions return the same bits on every call; the fp32 kernel's table
    answers yes throughout, so conv1 and conv3 are its deterministic launches)"""
    from orientedreppoints_amd import _lib
    nn = torch.nn
    answer = [1]
    _table_says(monkeypatch, answer)
    monkeypatch.setattr(_lib.lib(), 'orp_conv1x1_bn_act_pays', lambda *a: 1)
    calls = _spy(monkeypatch)
    fp32_calls = _spy(monkeypatch, 'orp_conv1x1_bn_act')
    ds = nn.Sequential(nn.Conv2d(64, 256, 1, bias=False), nn.BatchNorm2d(256))
    blk = _bottleneck(dev, 64, 64, stride=1, downsample=ds)
    blk.fuse_conv3x3 = False
    x = torch.randn(2, 64, 30, 22, device=dev)
    with torch.no_grad():
        blk.fuse_conv1x1_pieces = False
        off = blk(x.clone())
        assert len(calls) == 0 and len(fp32_calls) == 2
        blk.fuse_conv1x1_pieces = True
        answer[0] = 0
        before = blk(x.clone())
        assert len(calls) == 0 and len(fp32_calls) == 4
        answer[0] = 1
        blk(x.clone())
        assert len(calls) == 2 and len(fp32_calls) == 4
    assert _same_bits(off, before)


def test_routing_table_is_consulted_first_and_pieces_bypasses_it(dev, monkeypatch):
    from orientedreppoints_amd import _lib, switches
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, conv1x1_bn_act
    L = _lib.lib()
    calls = _spy(monkeypatch)
    fp32_calls = _spy(monkeypatch, 'orp_conv1x1_bn_act')
    answer = [0]
    asked = _table_says(monkeypatch, answer)
    asked32 = []
    monkeypatch.setattr(L, 'orp_conv1x1_bn_act_pays', lambda *a: asked32.append(a) or 0)
    conv, bn = _conv(64, 256, dev, 1), _bn(256, dev, 2)
    x = torch.randn(1, 64, 16, 16, device=dev)
    with torch.no_grad():
        want = bn_act(conv(x).contiguous(), bn, relu=True)
        y = conv1x1_bn_act(x, conv, bn)                          # neither table pays: library + pass, both asked, pieces first
        assert asked == [(64, 256, 256, 1, 0)] and asked32 == [(64, 256, 256, 1, 0)] and len(calls) == 0 and _same_bits(y, want)
        answer[0] = 1
        conv1x1_bn_act(x, conv, bn, residual=want)               # pays: the pieces launch, the fp32 table is not asked
        assert asked[1:] == [(64, 256, 256, 1, 1)] and len(asked32) == 1 and len(calls) == 1 and len(fp32_calls) == 0
        conv1x1_bn_act(x, conv, bn, pieces=False)                # switched off per call: not asked
        assert len(asked) == 2 and len(calls) == 1 and len(asked32) == 2
        monkeypatch.setattr(switches, 'BN_CONV1X1_PIECES', False)
        conv1x1_bn_act(x, conv, bn)                              # ORP_BN_CONV1X1_PIECES=0: not asked
        assert len(asked) == 2 and len(calls) == 1 and len(asked32) == 3
        answer[0] = 0
        conv1x1_bn_act(x, conv, bn, pieces=True)                 # forced: not asked, whatever the switch says
        assert len(asked) == 2 and len(calls) == 2
        monkeypatch.setattr(switches, 'BN_CONV1X1_PIECES', True)
        answer[0] = 1
        conv1x1_bn_act(x, conv, bn, force=True)                  # force keeps meaning the fp32 kernel
        assert len(asked) == 2 and len(calls) == 2 and len(fp32_calls) == 1
        small = _conv(32, 64, dev, 3)                            # unsupported (Cin < 64): library + pass even when forced
        xs = torch.randn(1, 32, 8, 8, device=dev)
        bns = _bn(64, dev, 4)
        assert _same_bits(conv1x1_bn_act(xs, small, bns, pieces=True), bn_act(small(xs).contiguous(), bns, relu=True))
        assert len(calls) == 2


def test_the_routing_table_is_closed():
    """nothing beyond a timed corner is routed: whatever row the table has lies between the R-50 map of a 1024^2 image and that of a
    1536^2 image for one image, at the 1024^2 map for two; no other map, no third image, no pair outside R-50's sixteen"""
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    pairs = {(64, 64): 65536, (256, 64): 65536, (64, 256): 65536, (256, 128): 65536, (512, 128): 16384, (128, 512): 16384,
             (512, 256): 16384, (1024, 256): 4096, (256, 1024): 4096, (1024, 512): 4096, (2048, 512): 1024, (512, 2048): 1024}
    for (cin, cout), hw in pairs.items():
        big = hw * 9 // 4
        for B in (1, 2, 3):
            for q in (hw - 1, hw // 4, big + 1, 4 * hw):
                assert L.orp_conv1x1_bn_act_pieces_pays(cin, cout, q, B, 0) == 0
        assert L.orp_conv1x1_bn_act_pieces_pays(cin, cout, hw, 3, 0) == 0
        assert L.orp_conv1x1_bn_act_pieces_pays(cin, cout, big, 2, 0) == 0
        for r in (0, 1):                                         # a row holds for both residual forms
            assert L.orp_conv1x1_bn_act_pieces_pays(cin, cout, hw, 1, r) == L.orp_conv1x1_bn_act_pieces_pays(cin, cout, hw, 1, 1 - r)
    assert L.orp_conv1x1_bn_act_pieces_pays(96, 96, 65536, 1, 0) == 0 and L.orp_conv1x1_bn_act_pieces_pays(64, 96, 65536, 1, 0) == 0
