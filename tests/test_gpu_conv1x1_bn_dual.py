"""GPU: a bottleneck's conv3 with the block's downsample convolution contracted in the same bf16-pieces launch
(orp_conv1x1_bn_act_pieces_dual; conv1x1_bn_act_dual).

Exact cases bit for bit against float64 convolutions of x and of the sampled x2, each cast to fp32, followed by the pass the epilogue
replaces -- every triple x map (odd and even stride-2 inputs) x batch x ReLU and both tiles, the vector and the scalar fetch; the
elements the stride skips poisoned; two constructions that need each product of the branch; random data bit-equal to the two
pieces launches the dual launch stands for and inside the derived bound of float64, also at 2^100 and 2^-100; non-finite inputs;
reproducibility, graph capture, the Bottleneck call site, the routing table and the argument checks."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_conv1x1_bn_pieces import (_bits, _bn, _bottleneck, _conv, _conv64, _keep_some, _same_bits, _spy, _table_says,  # noqa: E402
                                        _wide_ints, dev)  # noqa: F401

# (Cin, Cin2, Cout, stride): the four R-50 stages and a ragged channel tile
TRIPLES = [(64, 64, 256, 1), (128, 256, 512, 2), (256, 512, 1024, 2), (512, 1024, 2048, 2), (64, 128, 160, 2)]


def _dual_tile(cin, cin2, cout, hw, batch):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act_dual_tile
    t = conv1x1_bn_act_dual_tile(cin, cin2, cout, hw, batch)
    assert t is not None
    return t


def _ds_conv(cin2, cout, stride, dev, seed, integer=False):
    conv = _conv(cin2, cout, dev, seed, integer=integer)
    conv.stride = (stride, stride)
    return conv


def _sampled(x2, s):
    return x2[:, :, ::s, ::s].contiguous()


def _want(x, conv, bn, x2, conv2, bn2, relu):
    """float64 convolutions of x and of the sampled x2, each cast to fp32, then the pass the epilogue replaces"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act
    raw = _conv64(x, conv).float().contiguous()
    raw2 = _conv64(_sampled(x2, conv2.stride[0]), conv2).float().contiguous()
    return bn_act(raw, bn, residual=raw2, residual_bn=bn2, relu=relu)


def _maps(stride, tile_positions):
    """(input h, input w, output h, output w): 1 x 1, 7 x 9, 33 x 31, 1 x 257, one whole position tile and one position more;
    stride 2 with odd input sides (the last row / column is never read) and the even 14 x 18"""
    n = tile_positions
    if stride == 1:
        return [(h, w, h, w) for (h, w) in [(1, 1), (7, 9), (33, 31), (1, 257), (1, n), (1, n + 1)]]
    return [(1, 1, 1, 1), (13, 17, 7, 9), (14, 18, 7, 9), (65, 61, 33, 31), (1, 513, 1, 257), (1, 2 * n - 1, 1, n), (1, 2 * n + 1, 1, n + 1)]


def _ints(shape, lim, g, dev):
    return torch.randint(-lim, lim + 1, shape, device=dev, generator=g).float()


@pytest.mark.parametrize("cin,cin2,cout,stride", TRIPLES)
def test_exact_cases_bit_for_bit(dev, monkeypatch, cin, cin2, cout, stride):
    """integer data, |x| <= 15 and |w| <= 7 (both sums below 2^24): every map x batch (3: the image seam) x ReLU, salted BatchNorm
    constants on both branches"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act_dual
    assert _lib.lib().orp_conv1x1_bn_act_pieces_dual_ok(cin, cin2, cout) == 1
    calls = _spy(monkeypatch, 'orp_conv1x1_bn_act_pieces_dual')
    conv, conv2 = _conv(cin, cout, dev, 100 + cin + cout, integer=True), _ds_conv(cin2, cout, stride, dev, 200 + cin2, integer=True)
    bn, bn2 = _bn(cout, dev, 7, salted=True), _bn(cout, dev, 8, salted=True)
    g = torch.Generator(device=dev).manual_seed(cin * 7 + cout)
    runs = 0
    with torch.no_grad():
        for (h2, w2, h, w) in _maps(stride, 32):
            for B in (1, 3):
                if h * w in (32, 33):                                                     # the whole tile / one position more
                    assert _dual_tile(cin, cin2, cout, h * w, B) == (128, 32)
                x, x2 = _ints((B, cin, h, w), 15, g, dev), _ints((B, cin2, h2, w2), 15, g, dev)
                for relu in (False, True):
                    got = conv1x1_bn_act_dual(x, conv, bn, x2, conv2, bn2, relu=relu)
                    assert got.is_contiguous() and got.data_ptr() not in (x.data_ptr(), x2.data_ptr())
                    assert _same_bits(got, _want(x, conv, bn, x2, conv2, bn2, relu)), (cin, cin2, cout, h2, w2, B, relu)
                    runs += 1
    assert runs == len(_maps(stride, 32)) * 4 and len(calls) == runs


# (Cin, Cin2, Cout, stride, input h, input w) at B = 3 on the 128 x 64 tile (taken only where it leaves 512 workgroups): 52 x 56
# outputs of an even input -> the vector fetch, four 4-byte loads per row; 53 x 55 outputs of the odd 105 x 109 -> one offset per
# position; 76 x 72 at stride 1 -> x2 fetched as x is.  Every last tile is ragged.
WIDE = [(128, 256, 512, 2, 104, 112), (128, 256, 512, 2, 105, 109), (64, 64, 256, 1, 76, 72)]


@pytest.mark.parametrize("cin,cin2,cout,stride,h2,w2", WIDE)
def test_exact_cases_on_the_wide_tile(dev, cin, cin2, cout, stride, h2, w2):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act_dual
    B, h, w = 3, (h2 - 1) // stride + 1, (w2 - 1) // stride + 1
    assert _dual_tile(cin, cin2, cout, h * w, B) == (128, 64) and (h * w) % 64 != 0
    conv, conv2 = _conv(cin, cout, dev, 300 + cin, integer=True), _ds_conv(cin2, cout, stride, dev, 301 + cin2, integer=True)
    bn, bn2 = _bn(cout, dev, 17, salted=True), _bn(cout, dev, 18, salted=True)
    g = torch.Generator(device=dev).manual_seed(h2)
    with torch.no_grad():
        x, x2 = _ints((B, cin, h, w), 15, g, dev), _ints((B, cin2, h2, w2), 15, g, dev)
        for relu in (False, True):
            assert _same_bits(conv1x1_bn_act_dual(x, conv, bn, x2, conv2, bn2, relu=relu), _want(x, conv, bn, x2, conv2, bn2, relu))


def test_exact_cases_cover_both_tiles():
    """the launches of the two tests above run both tiles the dual launch has (host-side query, no launch)"""
    seen = {_dual_tile(cin, cin2, cout, h * w, B) for (cin, cin2, cout, s) in TRIPLES for (_a, _b, h, w) in _maps(s, 32) for B in (1, 3)}
    assert (128, 32) in seen
    seen |= {_dual_tile(cin, cin2, cout, ((h2 - 1) // s + 1) * ((w2 - 1) // s + 1), 3) for (cin, cin2, cout, s, h2, w2) in WIDE}
    assert seen == {(128, 32), (128, 64)}


@pytest.mark.parametrize("cin,cin2,cout,stride", [t for t in TRIPLES if t[3] == 2])
def test_skipped_inputs_are_never_read_into_the_result(dev, cin, cin2, cout, stride):
    """every element of x2 the stride skips -- odd rows, odd columns, the unread last row / column of odd sides -- set to NaN, +inf
    or -inf: the output keeps the bits of the clean input"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act_dual
    conv, conv2 = _conv(cin, cout, dev, 1, integer=True), _ds_conv(cin2, cout, stride, dev, 2, integer=True)
    bn, bn2 = _bn(cout, dev, 7), _bn(cout, dev, 8)
    g = torch.Generator(device=dev).manual_seed(cin)
    with torch.no_grad():
        for (h2, w2) in [(13, 17), (14, 18), (65, 61), (1, 513), (16, 64)]:            # (16 x 64 -> 8 x 32: the vector fetch)
            h, w = (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1
            x, x2 = _ints((3, cin, h, w), 15, g, dev), _ints((3, cin2, h2, w2), 15, g, dev)
            clean = conv1x1_bn_act_dual(x, conv, bn, x2, conv2, bn2)
            skipped = torch.ones((h2, w2), dtype=torch.bool, device=dev)
            skipped[::2, ::2] = False
            poison = torch.tensor([float('nan'), float('inf'), float('-inf')], device=dev)[torch.arange(x2.numel(), device=dev) % 3]
            bad = torch.where(skipped.expand_as(x2), poison.view_as(x2), x2)
            assert int(skipped.sum()) > 0 or (h2, w2) == (1, 1)
            assert torch.equal(_sampled(bad, 2), _sampled(x2, 2))
            assert _same_bits(conv1x1_bn_act_dual(x, conv, bn, bad, conv2, bn2), clean), (h2, w2)
            assert _same_bits(clean, _want(x, conv, bn, x2, conv2, bn2, True))


@pytest.mark.parametrize("kind", ["wide x", "wide w"])
@pytest.mark.parametrize("cin,cin2,cout,stride", TRIPLES)
def test_exact_cases_that_need_each_product_of_the_branch(dev, cin, cin2, cout, stride, kind):
    """the first two constructions of test_gpu_conv1x1_bn_pieces.py::test_exact_cases_that_need_each_product on x2 / w2 (x2 odd with
    24 / 23 / 22 / 20 significant bits in 1 / 2 / 4 / 16 channels against w2 in {-1, 0, 1}, and the mirror), the main branch small
    integers: every partial sum an integer below 2^24, so a dropped, doubled or mis-paired product of the branch is a wrong bit"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act_dual
    B, h, w = 1, 33, 31
    h2, w2 = (h, w) if stride == 1 else (65, 61)
    g = torch.Generator(device=dev).manual_seed(cin2 + 3 * cout + len(kind))
    nz = torch.tensor([1, 2, 4, 16], device=dev)
    nbits = torch.tensor([24, 23, 22, 20], device=dev)
    if kind == "wide x":
        sel = torch.randint(0, 4, (B, 1, h2, w2), device=dev, generator=g)
        x2 = _wide_ints((B, cin2, h2, w2), nbits[sel], g, dev) * _keep_some((B, cin2, h2, w2), 1, nz[sel], g, dev)
        wt = torch.randint(-1, 2, (cout, cin2), device=dev, generator=g).double()
    else:
        sel = torch.randint(0, 4, (cout, 1), device=dev, generator=g)
        wt = _wide_ints((cout, cin2), nbits[sel], g, dev) * _keep_some((cout, cin2), 1, nz[sel], g, dev)
        x2 = torch.randint(-1, 2, (B, cin2, h2, w2), device=dev, generator=g).double()
    assert float(torch.einsum('oc,bchw->bohw', wt.abs(), x2.abs()).max()) < 2.0 ** 24
    conv, conv2 = _conv(cin, cout, dev, 1, integer=True), _ds_conv(cin2, cout, stride, dev, 2, integer=True)
    bn, bn2 = _bn(cout, dev, 27), _bn(cout, dev, 28)
    with torch.no_grad():
        conv2.weight.copy_(wt.float().view(cout, cin2, 1, 1))
        x2 = x2.float()
        assert torch.equal(conv2.weight.double().flatten(1), wt)
        raw2 = _conv64(_sampled(x2, stride), conv2)
        assert torch.equal(raw2.float().double(), raw2) and float(raw2.abs().max()) > 2.0 ** 16   # the reference is exact in fp32
        x = _ints((B, cin, h, w), 15, g, dev)
        for relu in (False, True):
            assert _same_bits(conv1x1_bn_act_dual(x, conv, bn, x2, conv2, bn2, relu=relu), _want(x, conv, bn, x2, conv2, bn2, relu))


_random_cache = {}


def _random_case(dev, cin, cin2, cout, stride):
    """N(0, 1) activations, He-scale weights, 24 x 40 outputs x 2 images (stride 2: of the odd 47 x 79); once per triple, left unchanged"""
    key = (cin, cin2, cout, stride)
    if key not in _random_cache:
        conv, conv2 = _conv(cin, cout, dev, 40 + cin), _ds_conv(cin2, cout, stride, dev, 50 + cin2)
        bn, bn2 = _bn(cout, dev, 41), _bn(cout, dev, 42)
        g = torch.Generator(device=dev).manual_seed(cin + cin2)
        x = torch.randn((2, cin, 24, 40), device=dev, generator=g)
        x2 = torch.randn((2, cin2) + ((24, 40) if stride == 1 else (47, 79)), device=dev, generator=g)
        _random_cache[key] = (conv, bn, conv2, bn2, x, x2)
    return _random_cache[key]


def _worst_ratio(x, conv, bn, x2, conv2, bn2, got):
    """worst |got - float64| over (Cin + 2) 2^-24 (|a| sum |x w| + |b| + |r|) + (Cin2 + 2) 2^-24 (|a2| sum |x2 w2| + |b2|), r from
    float64: the pieces file's bound applied to both branches"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine
    a, b = [t.double().view(1, -1, 1, 1) for t in _bn_affine(bn)]
    a2, b2 = [t.double().view(1, -1, 1, 1) for t in _bn_affine(bn2)]
    xs = _sampled(x2, conv2.stride[0])
    r = _conv64(xs, conv2) * a2 + b2
    ref = torch.relu(_conv64(x, conv) * a + b + r)
    bound = (conv.weight.size(1) + 2) * 2.0 ** -24 * (a.abs() * _conv64(x, conv, magnitudes=True) + b.abs() + r.abs()) + \
        (conv2.weight.size(1) + 2) * 2.0 ** -24 * (a2.abs() * _conv64(xs, conv2, magnitudes=True) + b2.abs())
    return float(((got.double() - ref).abs() / bound).max())


@pytest.mark.parametrize("exponent", [0, 100, -100])
@pytest.mark.parametrize("cin,cin2,cout,stride", TRIPLES)
def test_random_data_equals_the_two_launches_and_stays_inside_the_bound(dev, cin, cin2, cout, stride, exponent):
    """bit-equal to conv1x1_bn_act(sampled x2, downsample conv, its BatchNorm, relu=False, pieces=True) followed by
    conv1x1_bn_act(x, conv3, bn3, residual=that, relu=True, pieces=True), and inside the bound of float64; x and x2 as they are and
    scaled by 2^100 / 2^-100"""
    import conftest
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act, conv1x1_bn_act_dual
    conv, bn, conv2, bn2, x, x2 = _random_case(dev, cin, cin2, cout, stride)
    x, x2 = x * 2.0 ** exponent, x2 * 2.0 ** exponent
    plain = torch.nn.Conv2d(cin2, cout, 1, bias=False).to(dev).eval()          # the stride-1 convolution of the sampled input
    plain.weight = conv2.weight
    with torch.no_grad():
        got = conv1x1_bn_act_dual(x, conv, bn, x2, conv2, bn2, relu=True)
        r = conv1x1_bn_act(_sampled(x2, stride), plain, bn2, relu=False, pieces=True)
        two = conv1x1_bn_act(x, conv, bn, residual=r, relu=True, pieces=True)
        ratio = _worst_ratio(x, conv, bn, x2, conv2, bn2, got)
    conftest.REPORT.append("dual 1x1 launch %d + %d -> %d stride %d at 24 x 40, inputs scaled by 2^%d: worst |err| / bound vs float64 %.3f"
                           % (cin, cin2, cout, stride, exponent, ratio))
    assert _same_bits(got, two)
    assert ratio <= 1.0


@pytest.mark.parametrize("where", ["x2", "x"])
def test_non_finite_inputs(dev, where):
    """+-inf / NaN in the sampled x2 or in x: non-finite outputs exactly where the float64 reference's are, bit-equal elsewhere"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act_dual
    cin, cin2, cout = 128, 256, 96
    conv, conv2 = _conv(cin, cout, dev, 3, integer=True), _ds_conv(cin2, cout, 2, dev, 4, integer=True)
    bn, bn2 = _bn(cout, dev, 9), _bn(cout, dev, 10)
    g = torch.Generator(device=dev).manual_seed(5)
    x, x2 = _ints((2, cin, 33, 31), 15, g, dev), _ints((2, cin2, 65, 61), 15, g, dev)
    idx = torch.randperm(x.numel() if where == "x" else _sampled(x2, 2).numel(), generator=torch.Generator().manual_seed(6))[:90].to(dev)
    salt = torch.tensor([float('inf'), float('-inf'), float('nan')], device=dev)[torch.arange(90, device=dev) % 3]
    if where == "x":
        x.view(-1)[idx] = salt
    else:
        s = _sampled(x2, 2)
        s.view(-1)[idx] = salt
        x2[:, :, ::2, ::2] = s
    with torch.no_grad():
        want = _want(x, conv, bn, x2, conv2, bn2, False)
        got = conv1x1_bn_act_dual(x, conv, bn, x2, conv2, bn2, relu=False)
    src = x if where == "x" else _sampled(x2, 2)
    fin = torch.isfinite(want)
    bad_positions = (~torch.isfinite(src)).any(dim=1, keepdim=True).expand_as(want)
    assert int((~fin).sum()) > 0 and torch.equal(~fin, bad_positions)
    assert torch.equal(fin, torch.isfinite(got))
    assert np.array_equal(_bits(got[fin]), _bits(want[fin]))


def test_same_launch_twice_gives_the_same_bits(dev):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act_dual
    conv, bn, conv2, bn2, x, x2 = _random_case(dev, 256, 512, 1024, 2)
    with torch.no_grad():
        assert _same_bits(conv1x1_bn_act_dual(x, conv, bn, x2, conv2, bn2), conv1x1_bn_act_dual(x, conv, bn, x2, conv2, bn2))


def _dual_table_says(monkeypatch, answer):
    from orientedreppoints_amd import _lib
    asked = []

    def pays(*args):
        asked.append(args)
        return answer[0]
    monkeypatch.setattr(_lib.lib(), 'orp_conv1x1_bn_act_pieces_dual_pays', pays)
    return asked


def _strided_block(dev, inplanes=256, planes=128, stride=2, style='pytorch'):
    from orientedreppoints_amd.mmdet_models.resnet import Bottleneck
    nn = torch.nn
    ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
    torch.manual_seed(5)
    blk = Bottleneck(inplanes, planes, stride=stride, downsample=ds, style=style).to(dev).eval()
    for i, m in enumerate(m for m in blk.modules() if isinstance(m, torch.nn.BatchNorm2d)):
        m.load_state_dict(_bn(m.num_features, dev, 20 + i).state_dict())
    ds_calls = []
    blk.downsample[0].register_forward_hook(lambda *a: ds_calls.append(1))
    return blk, ds_calls


def test_captured_bottleneck_replays_the_eager_bits(dev, monkeypatch):
    """a block with a strided downsample, captured: every replay has the bits of the eager call, and the dual launch inside the graph
    has the bits of the two eager pieces launches on the conv3 input the graph itself produced.  Under
    torch.backends.cudnn.deterministic, as test_gpu_fused_glue.py runs its detector: without it the library's strided conv2 at this
    small map is not held to the same bits from call to call, which no launch behind it can mend; with it, the
    block's first eager call, its later ones and the conv3 input inside the graph are all asserted equal."""
    from orientedreppoints_amd.mmdet_ops import fused_norm
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act
    _table_says(monkeypatch, [1])
    _dual_table_says(monkeypatch, [1])
    calls = _spy(monkeypatch, 'orp_conv1x1_bn_act_pieces_dual')
    seen = []
    wrapped = fused_norm.conv1x1_bn_act_dual

    def recording(t, *args, **kw):
        seen.append(t.clone())
        return wrapped(t, *args, **kw)
    monkeypatch.setattr(fused_norm, 'conv1x1_bn_act_dual', recording)
    blk, ds_calls = _strided_block(dev)
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    x = torch.randn(2, 256, 29, 23, device=dev)
    plain = torch.nn.Conv2d(256, 512, 1, bias=False).to(dev).eval()
    plain.weight = blk.downsample[0].weight
    with torch.no_grad():
        first = blk(x).clone()
        assert len(calls) == 1 and not ds_calls and tuple(first.shape) == (2, 512, 15, 12)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            blk(x)
        torch.cuda.current_stream().wait_stream(s)
        eager = blk(x).clone()
        assert _same_bits(first, eager)                              # (the block itself is reproducible from call to call)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = blk(x)
        r = conv1x1_bn_act(x[:, :, ::2, ::2].contiguous(), plain, blk.downsample[1], relu=False, pieces=True)
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert _same_bits(out, conv1x1_bn_act(seen[-1], blk.conv3, blk.bn3, residual=r, relu=True, pieces=True))
            assert _same_bits(seen[-1], seen[-2])                    # conv3's input inside the graph is the eager one ...
            assert _same_bits(out, eager)                            # ... and so is the block's output


def test_bottleneck_routing(dev, monkeypatch):
    """the dual table is asked after the pieces switch; yes = one dual call and no library downsample convolution, with the bits of the
    two pieces launches; the attribute or the switch off = the launches of before; autograd on = the module path"""
    from orientedreppoints_amd import switches
    from orientedreppoints_amd.mmdet_ops import fused_norm
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act
    seen = []
    wrapped = fused_norm.conv1x1_bn_act_dual

    def recording(t, *args, **kw):
        seen.append(t.clone())
        return wrapped(t, *args, **kw)
    monkeypatch.setattr(fused_norm, 'conv1x1_bn_act_dual', recording)
    _table_says(monkeypatch, [1])
    answer = [1]
    asked = _dual_table_says(monkeypatch, answer)
    dual = _spy(monkeypatch, 'orp_conv1x1_bn_act_pieces_dual')
    pieces = _spy(monkeypatch)
    blk, ds_calls = _strided_block(dev)
    x = torch.randn(2, 256, 29, 23, device=dev)
    with torch.no_grad():
        on = blk(x.clone())
        assert asked == [(128, 256, 512, 15 * 12, 2, 2)] and len(dual) == 1 and not ds_calls
        assert len(pieces) == 1                                    # conv1 (conv2 is strided: the library's)
        # what the launch stands for, on the conv3 input it was given: the pieces launch of the sampled block input, then conv3's
        # with that as its residual
        plain = torch.nn.Conv2d(256, 512, 1, bias=False).to(dev).eval()
        plain.weight = blk.downsample[0].weight
        r = conv1x1_bn_act(x[:, :, ::2, ::2].contiguous(), plain, blk.downsample[1], relu=False, pieces=True)
        assert len(seen) == 1
        assert _same_bits(on, conv1x1_bn_act(seen[0], blk.conv3, blk.bn3, residual=r, relu=True, pieces=True))
        n_pieces = len(pieces)
        # the pieces switch off: the dual table is not asked
        blk.fuse_conv1x1_pieces = False
        blk(x.clone())
        assert len(asked) == 1 and len(dual) == 1 and len(ds_calls) == 1 and len(pieces) == n_pieces
        del blk.fuse_conv1x1_pieces
        # the attribute off with the table saying yes = the attribute on with the table saying no: the launches of before
        blk.fuse_downsample_conv = False
        assert not blk._downsample_conv_fusable()
        blk(x.clone())
        assert len(asked) == 1 and len(dual) == 1 and len(ds_calls) == 2 and len(pieces) == n_pieces + 2     # conv1 and conv3
        del blk.fuse_downsample_conv
        assert blk._downsample_conv_fusable()                       # default: on
        monkeypatch.setattr(switches, 'BN_DOWNSAMPLE_CONV_FUSE', False)
        blk(x.clone())
        assert len(asked) == 1 and len(dual) == 1 and len(ds_calls) == 3 and len(pieces) == n_pieces + 4
        monkeypatch.setattr(switches, 'BN_DOWNSAMPLE_CONV_FUSE', True)
        answer[0] = 0
        blk(x.clone())
        assert len(asked) == 2 and len(dual) == 1 and len(ds_calls) == 4 and len(pieces) == n_pieces + 6
    with torch.enable_grad():
        blk(x.clone())                                              # autograd on: the unfused module path
    assert len(asked) == 2 and len(dual) == 1 and len(pieces) == n_pieces + 6


def test_strided_block_with_the_switch_off_has_the_bits_of_before(dev, monkeypatch):
    """the strided block (under torch.backends.cudnn.deterministic: its library convolutions reproducible): the attribute off with
    the dual table saying yes, the environment switch off, and the attribute on with the table saying no -- the route of before --
    give the same bits, the library downsample convolution runs each time and no dual launch is made"""
    from orientedreppoints_amd import switches
    _table_says(monkeypatch, [1])
    answer = [1]
    _dual_table_says(monkeypatch, answer)
    dual = _spy(monkeypatch, 'orp_conv1x1_bn_act_pieces_dual')
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    blk, ds_calls = _strided_block(dev)
    x = torch.randn(2, 256, 29, 23, device=dev)
    with torch.no_grad():
        blk(x.clone())                                              # (the dual route once: the library has seen every shape)
        assert len(dual) == 1
        answer[0] = 0
        before = blk(x.clone())
        assert _same_bits(before, blk(x.clone()))
        answer[0] = 1
        blk.fuse_downsample_conv = False
        off = blk(x.clone())
        del blk.fuse_downsample_conv
        monkeypatch.setattr(switches, 'BN_DOWNSAMPLE_CONV_FUSE', False)
        env_off = blk(x.clone())
    assert len(dual) == 1 and len(ds_calls) == 4
    assert _same_bits(off, before) and _same_bits(env_off, before)


def test_switch_off_gives_the_launches_and_bits_of_before(dev, monkeypatch):
    """stage 1's first block at the shape where the library's convolutions return the same bits on every call
    (test_gpu_conv1x1_bn_pieces.py): the attribute off with the dual table saying yes has the bits of the attribute on with the
    table saying no, and neither makes a dual call"""
    nn = torch.nn
    _table_says(monkeypatch, [1])
    answer = [1]
    _dual_table_says(monkeypatch, answer)
    dual = _spy(monkeypatch, 'orp_conv1x1_bn_act_pieces_dual')
    ds = nn.Sequential(nn.Conv2d(64, 256, 1, bias=False), nn.BatchNorm2d(256))
    blk = _bottleneck(dev, 64, 64, stride=1, downsample=ds)
    blk.fuse_conv3x3 = False
    x = torch.randn(2, 64, 30, 22, device=dev)
    with torch.no_grad():
        blk.fuse_downsample_conv = False
        off = blk(x.clone())
        blk.fuse_downsample_conv = True
        answer[0] = 0
        before = blk(x.clone())
        assert len(dual) == 0
        answer[0] = 1
        blk(x.clone())
        assert len(dual) == 1
    assert _same_bits(off, before)


def test_the_dual_routing_table_is_closed():
    """as test_gpu_conv1x1_bn_pieces.py::test_the_routing_table_is_closed: whatever row the table has lies between the R-50 map of a
    1024^2 image and that of a 1536^2 image for one image, at the 1024^2 map for two; no other map, no third image, no other stride,
    no triple outside R-50's four"""
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    triples = {(64, 64, 256, 1): 65536, (128, 256, 512, 2): 16384, (256, 512, 1024, 2): 4096, (512, 1024, 2048, 2): 1024}
    for (cin, cin2, cout, s), hw in triples.items():
        big = hw * 9 // 4
        for B in (1, 2, 3):
            for q in (hw - 1, hw // 4, big + 1, 4 * hw):
                assert L.orp_conv1x1_bn_act_pieces_dual_pays(cin, cin2, cout, q, s, B) == 0
        assert L.orp_conv1x1_bn_act_pieces_dual_pays(cin, cin2, cout, hw, s, 3) == 0
        assert L.orp_conv1x1_bn_act_pieces_dual_pays(cin, cin2, cout, big, s, 2) == 0
        assert L.orp_conv1x1_bn_act_pieces_dual_pays(cin, cin2, cout, hw, 3 - s, 1) == 0
        assert L.orp_conv1x1_bn_act_pieces_dual_pays(cin, cin, cout, hw, s, 1) == (1 if cin == cin2 else 0) * \
            L.orp_conv1x1_bn_act_pieces_dual_pays(cin, cin2, cout, hw, s, 1)
    assert L.orp_conv1x1_bn_act_pieces_dual_pays(64, 128, 160, 16384, 2, 1) == 0
    assert L.orp_conv1x1_bn_act_pieces_dual_pays(96, 96, 96, 65536, 1, 1) == 0


def test_argument_errors(dev):
    """ORP_EINVAL for inconsistent ho / wo, stride 3, y aliasing an input, misaligned packs and unsupported channels"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine, _packed_1x1_planes
    L = _lib.lib()
    EINVAL = _lib.ORP_EINVAL
    conv, conv2 = _conv(64, 128, dev, 1), _ds_conv(128, 128, 2, dev, 2)
    bn, bn2 = _bn(128, dev, 3), _bn(128, dev, 4)
    x, x2 = torch.randn(1, 64, 4, 4, device=dev), torch.randn(1, 128, 8, 8, device=dev)
    y = torch.full((1, 128, 4, 4), 7.0, device=dev)
    pk, pk2 = _packed_1x1_planes(conv.weight), _packed_1x1_planes(conv2.weight)
    (a, b), (a2, b2) = _bn_affine(bn), _bn_affine(bn2)
    p = lambda t: t.data_ptr()                                                  # noqa: E731

    def call(x=x, pk=p(pk), x2=x2, pk2=p(pk2), cin2=128, h2=8, w2=8, s=2, y=y, cin=64, cout=128, ho=4, wo=4):
        return L.orp_conv1x1_bn_act_pieces_dual(p(x), pk, p(a), p(b), p(x2), pk2, p(a2), p(b2), cin2, h2, w2, s, p(y), 1, cin, cout, ho, wo,
                                                1, _lib.stream_of(x))
    for kw in (dict(ho=5), dict(wo=3), dict(h2=9, w2=9), dict(s=3), dict(s=0), dict(s=1), dict(y=x), dict(y=x2),
               dict(pk=p(pk) + 8), dict(pk2=p(pk2) + 4), dict(cin=32), dict(cin2=96), dict(cout=100)):
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                      # nothing was launched
    assert call() == 0
    assert call(h2=7, w2=7) == 0                       # (the 7 x 7 corner of the 8 x 8 buffer: an odd side of the same map)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and not bool((y == 7.0).all())
