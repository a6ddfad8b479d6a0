"""GPU: the halo kernel of the split convolution (csrc/orp_dcn_split.hip conv_halo_kernel: 3x3, stride 1, dilation 1, padding 1,
fp16-pieces mode, Cin <= 256 -- spatial tiles of 6 x 16 or 12 x 8 positions whose input halo is staged in LDS once) against the
linear-tile kernel it replaces.  Every case runs the same call with the switch on and off (orp_conv_split_set_halo) and asserts

  * torch.equal on every output tensor: the A values, the weight fragments, the MFMA order per accumulator and the epilogue are the
    linear kernel's, and an MFMA output row depends on its own A row only;
  * equal range words: what each launch read as its range word and weight scale (orp_debug_amax_log, four words per launch);
  * with orp_conv_split_halo_tile, that the "on" run took the halo kernel with the expected tile per level and the "off" run did not.

The level shapes cover exactly one tile, one row / column over, ragged tiles both ways, the narrow tile, and a map smaller than the
halo.  GroupNorm on the way in uses coefficients with b[c] far from 0, so that a padding row normalised instead of zeroed shows.  The
tile partials, merged by orp_conv_split_gn_finish, are held to float64 statistics of the linear kernel's output tensor at the
forward bound of tests/test_gpu_norm.py (4 * 2^-23 * (max |x| max rstd max |gamma| + max |beta|)), taken at gamma = 1, beta = 0 on the
coefficients (a, b) = (rstd, -mean rstd):   max |x| |a - rstd64| + |b + mean64 rstd64|  <=  4 * 2^-23 max |x| rstd64   per group."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES = [(6, 16), (7, 17), (16, 16), (13, 34), (8, 8), (12, 8), (5, 9), (2, 3)]
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _tile(h, w):
    return (6, 16) if w >= 16 else (12, 8)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rand(shape, seed, dev, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).to(dev)


def _inputs(sizes, B, cin, seed, dev):
    return [_cl(_rand((B, cin, h, w), seed + 17 * i, dev)) for i, (h, w) in enumerate(sizes)]


def _logged(fn):
    """fn() with the range words its launches read logged: (tensors, log words)"""
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    log = torch.zeros(4 * 8, dtype=torch.int32, device="cuda:0")
    L.orp_debug_amax_log(ctypes.c_void_p(log.data_ptr()), 8)
    try:
        with torch.no_grad():
            outs = fn()
        torch.cuda.synchronize()
    finally:
        used = L.orp_debug_amax_log(None, 0)
    return list(outs), log[:4 * used].cpu()


def _on_off(fn, sizes, B, cin, cout, halo=True, **geometry):
    """fn() with the halo switch on and off: which kernel each run took, equal outputs and range words; returns (on, off) outputs"""
    from orientedreppoints_amd.mmdet_ops import fused_norm as fn_
    try:
        fn_.conv_split_set_halo(1)
        tiles = fn_.conv_split_halo_tile(sizes, B, cin, cout, **geometry)
        assert tiles == ([_tile(h, w) for h, w in sizes] if halo else None), (tiles, sizes, geometry)
        on, log_on = _logged(fn)
        fn_.conv_split_set_halo(0)
        assert fn_.conv_split_halo_tile(sizes, B, cin, cout, **geometry) is None
        off, log_off = _logged(fn)
    finally:
        fn_.conv_split_set_halo(-1)
    assert len(on) == len(off) and len(on) > 0
    for i, (u, v) in enumerate(zip(on, off)):
        assert u.shape == v.shape and torch.equal(u, v), "output %d of %s B=%d differs from the linear kernel's" % (i, sizes, B)
    assert torch.equal(log_on, log_off), "range words"
    if geometry.get("nprod", 3) == 3:
        assert log_on.numel() >= 4
    return on, off


@pytest.mark.parametrize("B", (1, 3))
def test_every_level_shape_alone_and_together(dev, B):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv_split_weights
    w = _rand((256, 256, 3, 3), 1, dev, 0.05)
    for sizes in [[s] for s in SIZES] + [SIZES]:
        xs = _inputs(sizes, B, 256, 100 + B, dev)
        on, _ = _on_off(lambda: conv_split_weights(xs, w, nprod=3), sizes, B, 256, 256)
        for y, (h, wd) in zip(on, sizes):
            assert y.shape == (B, 256, h, wd) and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("channels_last", (True, False))
@pytest.mark.parametrize("bias_relu", (False, True))
def test_one_layer_two_layers_and_a_layer_per_level(dev, channels_last, bias_relu):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv_split_weights
    B = 3
    xa, xb = _inputs(SIZES, B, 256, 200, dev), _inputs(SIZES, B, 256, 300, dev)
    wa, wb = _rand((256, 256, 3, 3), 2, dev, 0.05), _rand((256, 256, 3, 3), 3, dev, 0.05)
    ba, bb = (_rand((256,), 4, dev), _rand((256,), 5, dev)) if bias_relu else (None, None)
    kw = dict(relu=bias_relu, out_channels_last=channels_last, nprod=3)
    one, _ = _on_off(lambda: conv_split_weights(xa, wa, biases_a=ba, **kw), SIZES, B, 256, 256)

    def pair():
        pa, pb = conv_split_weights(xa, wa, xb, wb, biases_a=ba, bias_b=bb, **kw)
        return pa + pb
    two, _ = _on_off(pair, SIZES, B, 256, 256)
    for u, v in zip(two[:len(SIZES)], one):
        assert torch.equal(u, v), "a grid half of the pair launch: the single launch's bits"
    # the FPN form: one layer per level (orp_conv_split_multi_ex)
    ws = [_rand((256, 256, 3, 3), 10 + i, dev, 0.05) for i in range(len(SIZES))]
    bs = [_rand((256,), 30 + i, dev) for i in range(len(SIZES))] if bias_relu else None
    _on_off(lambda: conv_split_weights(xa, ws, biases_a=bs, **kw), SIZES, B, 256, 256)


@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 512), (128, 64), (128, 512)])
def test_other_channel_counts(dev, cin, cout):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv_split_weights
    w = _rand((cout, cin, 3, 3), cin + cout, dev, 0.05)
    for B in (1, 3):
        xs = _inputs(SIZES, B, cin, 400 + cin, dev)
        for cl in (True, False):
            _on_off(lambda: conv_split_weights(xs, w, out_channels_last=cl, nprod=3), SIZES, B, cin, cout)


def _gn_launch(xs_a, xs_b, wa, wb, coef_in, relu_in, amax, G):
    """orp_conv_split_multi_gn + orp_conv_split_gn_finish (gamma 1, beta 0) -> (outputs a + b, coefficients [2 n, B, C, 2])"""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import _ConvLevel
    from orientedreppoints_amd.mmdet_ops.deform_conv import _packed_weight
    L = _lib.lib()
    n, B, cin, cout = len(xs_a), xs_a[0].size(0), xs_a[0].size(1), wa.size(0)
    dev = xs_a[0].device
    levels = (_ConvLevel * n)()
    outs_a, outs_b = [], []
    for i in range(n):
        H, W = xs_a[i].size(2), xs_a[i].size(3)
        oa = torch.empty((B, cout, H, W), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        ob = torch.empty((B, cout, H, W), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        outs_a.append(oa); outs_b.append(ob)
        levels[i] = _ConvLevel(xs_a[i].data_ptr(), xs_b[i].data_ptr(), oa.data_ptr(), ob.data_ptr(), H, W)
    pf = int(L.orp_conv_split_gn_partial_floats(levels, n, B, G, 2))
    partials = torch.zeros((pf,), dtype=torch.float32, device=dev)
    ws = _lib.workspace(dev, 256)
    pa, pb = _packed_weight(wa), _packed_weight(wb)
    st = _lib.stream_of(xs_a[0])
    rc = L.orp_conv_split_multi_gn(levels, n, B, cin, cout, _lib.ptr(pa), _lib.ptr(pb), 3, 3, 1, 1, 1, 1, 3, _lib.ptr(coef_in), relu_in,
                                   _lib.ptr(partials), pf, G, _lib.ptr(ws), ws.numel(), amax.data_ptr(), 1, 1, st)
    _lib.check(rc, "orp_conv_split_multi_gn")
    coef = torch.empty((2 * n, B, cout, 2), dtype=torch.float32, device=dev)
    ones, zeros = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
    gam = (ctypes.c_void_p * (2 * n))(*[ones.data_ptr()] * (2 * n))
    bet = (ctypes.c_void_p * (2 * n))(*[zeros.data_ptr()] * (2 * n))
    rc = L.orp_conv_split_gn_finish(levels, n, B, cout, G, 2, EPS, gam, bet, _lib.ptr(partials), _lib.ptr(coef), None, st)
    _lib.check(rc, "orp_conv_split_gn_finish")
    return outs_a + outs_b + [coef]


def _stat_errors(outs, coef, G):
    """per (tensor, image, group): (max |x| |a - rstd64| + |b + mean64 rstd64|) / (4 * 2^-23 max |x| rstd64), the maximum"""
    worst = 0.0
    for t, o in enumerate(outs):
        B, C = o.size(0), o.size(1)
        x = o.double().cpu().reshape(B, G, -1)
        mean, var = x.mean(dim=2), x.var(dim=2, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + EPS)
        amax = x.abs().amax(dim=2)
        a = coef[t, :, :, 0].double().cpu().reshape(B, G, C // G)
        b = coef[t, :, :, 1].double().cpu().reshape(B, G, C // G)
        err = amax[:, :, None] * (a - rstd[:, :, None]).abs() + (b + (mean * rstd)[:, :, None]).abs()
        bound = 4.0 * 2.0 ** -23 * amax * rstd
        worst = max(worst, float((err / bound[:, :, None]).max()))
    return worst


@pytest.mark.parametrize("relu_in", (0, 1))
@pytest.mark.parametrize("B", (1, 3))
def test_groupnorm_on_the_way_in_and_tile_partials(dev, B, relu_in):
    G = 32
    sizes = SIZES
    n = len(sizes)
    xa, xb = _inputs(sizes, B, 256, 500, dev), _inputs(sizes, B, 256, 600, dev)
    wa, wb = _rand((256, 256, 3, 3), 6, dev, 0.05), _rand((256, 256, 3, 3), 7, dev, 0.05)
    g = torch.Generator().manual_seed(8)
    coef_in = torch.stack([0.5 + torch.rand((2, n, B, 256), generator=g), 3.0 + torch.randn((2, n, B, 256), generator=g)], dim=-1).to(dev).contiguous()
    # the range words the producer of the coefficients would leave: an upper bound of max |relu?(x a + b)| per layer
    bounds = []
    for cv, xs in enumerate((xa, xb)):
        m = 0.0
        for i, x in enumerate(xs):
            y = x * coef_in[cv, i, :, :, 0][:, :, None, None] + coef_in[cv, i, :, :, 1][:, :, None, None]
            m = max(m, float((y.clamp(min=0) if relu_in else y).abs().max()))
        bounds.append(m * 1.001)
    amax = torch.tensor(bounds, dtype=torch.float32).view(torch.int32).to(dev)
    on, off = _on_off(lambda: _gn_launch(xa, xb, wa, wb, coef_in, relu_in, amax, G)[:2 * n], sizes, B, 256, 256)
    # the statistics: the same launches again for their coefficients (deterministic: the outputs are the bits above)
    from orientedreppoints_amd.mmdet_ops import fused_norm as fn_
    figs = {}
    try:
        for name, sw in (("halo", 1), ("linear", 0)):
            fn_.conv_split_set_halo(sw)
            res = _gn_launch(xa, xb, wa, wb, coef_in, relu_in, amax, G)
            torch.cuda.synchronize()
            for u, v in zip(res[:2 * n], off):
                assert torch.equal(u, v)
            figs[name] = _stat_errors(off, res[2 * n], G)
    finally:
        fn_.conv_split_set_halo(-1)
    print("merged tile statistics against float64, worst error / bound: halo %.3f, linear %.3f" % (figs["halo"], figs["linear"]))
    assert figs["halo"] <= 1.0, figs
    # a padding row that was normalised (b far from 0) instead of zeroed would move the border outputs: the float64 convolution of the
    # normalised, zero-padded tensor
    x0 = xa[0].double().cpu()
    y0 = x0 * coef_in[0, 0, :, :, 0].double().cpu()[:, :, None, None] + coef_in[0, 0, :, :, 1].double().cpu()[:, :, None, None]
    want = torch.nn.functional.conv2d(y0.clamp(min=0) if relu_in else y0, wa.double().cpu(), padding=1)
    assert float((on[0].double().cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_other_geometries_and_modes_keep_the_linear_kernel(dev):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv_split_weights
    B, sizes = 2, [(13, 34), (5, 9)]
    for cin, k, stride, pad, dil, nprod in ((128, 3, 2, 1, 1, 3), (128, 3, 1, 2, 2, 3), (128, 1, 1, 0, 1, 3), (512, 3, 1, 1, 1, 3),
                                            (256, 3, 1, 1, 1, 6), (256, 3, 1, 1, 1, 9)):
        w = _rand((64, cin, k, k), 700 + cin + k, dev, 0.05)
        xs = _inputs(sizes, B, cin, 800 + cin, dev)
        _on_off(lambda: conv_split_weights(xs, w, stride=(stride, stride), padding=(pad, pad), dilation=(dil, dil), nprod=nprod),
                sizes, B, cin, 64, halo=False, kh=k, kw=k, stride=stride, pad=pad, dil=dil, nprod=nprod)


def test_a_captured_graph_keeps_its_kernel(dev):
    from orientedreppoints_amd.mmdet_ops import fused_norm as fn_
    B, sizes = 2, [(13, 34), (5, 9)]
    w = _rand((256, 256, 3, 3), 9, dev, 0.05)
    xs = _inputs(sizes, B, 256, 900, dev)
    try:
        fn_.conv_split_set_halo(1)
        assert fn_.conv_split_halo_tile(sizes, B, 256, 256) == [_tile(h, wd) for h, wd in sizes]
        with torch.no_grad():
            eager = fn_.conv_split_weights(xs, w, nprod=3)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                outs = fn_.conv_split_weights(xs, w, nprod=3)
        fn_.conv_split_set_halo(0)
        assert fn_.conv_split_halo_tile(sizes, B, 256, 256) is None
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(outs, eager):
            assert torch.equal(u, v), "the replay of a graph captured with the halo kernel"
    finally:
        fn_.conv_split_set_halo(-1)
