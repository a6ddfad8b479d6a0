"""GPU: orp_token_layernorm (csrc/orp_token_layernorm.hip) -- nn.LayerNorm over fp32 tokens with the layout glue beside it, in its
four layouts -- against float64 on the same fp32 inputs, bit for bit against itself across launches and layouts, and the Swin modules
that route their LayerNorms through it.  Every launch here is forced: the routing table is not asked.

The shape grid: every lanes-per-row shape of the kernel (C = 32 and 96: 8 lanes, 192: 16, 384: 32, 768: 64, 1536: 64 lanes x 8 float4,
4096: x 16) at T = 1, one less than / exactly / one more than the rows of a workgroup, and 257 (more than one workgroup, a ragged last
one; 32 LDS tiles of 8 tokens and one of 1 for the NCHW variants).  The 16- and 32-token tiles need 4096 and 8192 tokens to be chosen:
`test_from_and_to_nchw_on_the_wide_tiles`."""
import copy
import ctypes

import pytest
import torch

from orientedreppoints_amd import _lib, switches
from orientedreppoints_amd.mmdet_models.swin import PatchEmbed, PatchMerging, SwinStage, SwinTransformer
from orientedreppoints_amd.mmdet_ops.token_norm import LAYOUTS, token_layernorm, token_layernorm_ok, token_layernorm_reference, token_layernorm_routed

pytestmark = pytest.mark.gpu
F = torch.nn.functional

CS = (32, 96, 192, 384, 768, 1536, 4096)
U = 2.0 ** -24
EPS = 1e-5
# (mean, std) of the rows: N(0, 1); a mean eight deviations off; a mean that costs 13 of the 24 bits; a variance (1e-6) below eps
DISTRIBUTIONS = ((0.0, 1.0), (8.0, 1.0), (1e4, 1.0), (0.0, 1e-3))


def _ln(C, seed=1, gamma=None, beta=None):
    g = torch.Generator().manual_seed(seed)
    ln = torch.nn.LayerNorm(C, eps=EPS)
    with torch.no_grad():
        ln.weight.copy_(1.0 + torch.randn((C,), generator=g) if gamma is None else gamma)
        ln.bias.copy_(torch.randn((C,), generator=g) if beta is None else beta)
    return ln.cuda()


def _rows(T, C, seed, mean=0.0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (mean + std * torch.randn((T, C), generator=g)).cuda()


def _source(rows, layout):
    """(x, hw): a source in `layout` whose normalised rows are `rows` [T, C], in this order"""
    T, C = rows.shape
    if layout == 'tokens':
        return rows.view(1, T, C), None
    if layout == 'merge':       # a 2 x 2T map: quarter q = dr + 2 dc of row t is the source position (dr, 2 t + dc)
        return rows.view(T, 2, 2, C // 4).permute(2, 0, 1, 3).reshape(1, 2 * 2 * T, C // 4).contiguous(), (2, 2 * T)
    if layout == 'from_nchw':
        return rows.t().contiguous().view(1, C, T), None
    return rows.view(1, T, C), (T, 1)


def _as_rows(y, layout, T, C):
    return y.view(C, T).t() if layout == 'to_nchw' else y.view(T, C)


def _run(rows, ln, layout):
    x, hw = _source(rows, layout)
    with torch.no_grad():
        assert token_layernorm_ok(ln, x, layout, hw)
        return _as_rows(token_layernorm(x, ln, layout, hw, force=True), layout, *rows.shape)


def _rows_per_workgroup(C):
    return _lib.tile_query("orp_token_layernorm_plan", 3, 1, 1, 1, C, LAYOUTS['tokens'])[1]


def _bound(rows, ln):
    """(y64, the first-order bound 2^-24 [(C/2 + 8) |d r gamma| + C mean_k|x_k| r |gamma| + |y64| + |beta|]), d = x - mean and
    r = rsqrt(var + eps) in float64: C/2 of the first term for the sum of squares in any order (relative error of r is half that of
    the variance), 8 for the subtraction, r, the product and the fma; the second term is the mean's rounding, (C - 1) u mean|x| in any
    order plus the division, carried to the output through r gamma"""
    C = rows.size(1)
    x, g, b = rows.double(), ln.weight.detach().double(), ln.bias.detach().double()
    d = x - x.mean(1, keepdim=True)
    r = torch.rsqrt(d.pow(2).mean(1, keepdim=True) + EPS)
    y64 = d * r * g + b
    return y64, U * ((C / 2 + 8) * (d * r * g).abs() + C * x.abs().mean(1, keepdim=True) * r * g.abs() + y64.abs() + b.abs())


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_against_float64_inside_the_first_order_bound(layout):
    from conftest import REPORT
    worst = stock = 0.0
    n = 0
    for C in CS:
        ln = _ln(C, seed=C)
        R = _rows_per_workgroup(C)
        for T in sorted({1, R - 1, R, R + 1, 257} - {0}):
            for k, (mean, std) in enumerate(DISTRIBUTIONS):
                rows = _rows(T, C, 1000 * k + T, mean, std)
                y64, bound = _bound(rows, ln)
                if T == 257 and k == 0:
                    want = token_layernorm_reference(_source(rows.double(), layout)[0], ln.weight.detach().double(), ln.bias.detach().double(),
                                                     EPS, layout, _source(rows, layout)[1])
                    assert float((_as_rows(want, layout, T, C) - y64).abs().max()) < 1e-12          # the bound's y64 is the reference's
                got = _run(rows, ln, layout)
                with torch.no_grad():
                    theirs = ln(rows)
                worst = max(worst, float(((got.double() - y64).abs() / bound).max()))
                stock = max(stock, float(((theirs.double() - y64).abs() / bound).max()))
                n += 1
    line = "token_layernorm %-9s worst error / bound: kernel %.4f, framework %.4f (%d launches)" % (layout, worst, stock, n)
    print(line)
    REPORT.append(line)
    assert worst <= 1.0, line


@pytest.mark.parametrize("C", [96, 160, 768, 1536])
def test_a_row_does_not_depend_on_the_launch(C):
    """a row launched alone has the bits of the same row inside T = 257 and inside T = 10 900; the same launch twice gives the same bits"""
    ln = _ln(C)
    rows = _rows(10900, C, 7, 0.5, 2.0)
    full = _run(rows, ln, 'tokens')
    assert torch.equal(full, _run(rows, ln, 'tokens'))
    assert torch.equal(_run(rows[:257].contiguous(), ln, 'tokens'), full[:257])
    for t in (0, 3, 31, 32, 100, 256, 257, 10899):
        assert torch.equal(_run(rows[t:t + 1].contiguous(), ln, 'tokens')[0], full[t]), t


@pytest.mark.parametrize("shape", [(2, 15, 21, 24), (1, 16, 20, 96), (3, 1, 1, 8), (1, 7, 1, 48)])
def test_merge_is_tokens_on_the_materialised_cat(shape):
    """odd H and W: the zeros of the padding enter the statistics, as F.pad in front of the LayerNorm makes them"""
    B, H, W, Cs = shape
    ln = _ln(4 * Cs)
    g = torch.Generator().manual_seed(2)
    x = (0.3 + torch.randn(shape, generator=g)).cuda()
    v = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    cat = torch.cat([v[:, 0::2, 0::2], v[:, 1::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 1::2]], -1).view(B, -1, 4 * Cs).contiguous()
    with torch.no_grad():
        want = token_layernorm(cat, ln, 'tokens', force=True)
        got = token_layernorm(x, ln, 'merge', force=True)
        assert got.shape == want.shape and got.is_contiguous() and torch.equal(got, want)
        assert torch.equal(token_layernorm(x.view(B, H * W, Cs), ln, 'merge', (H, W), force=True), want)
        y64 = token_layernorm_reference(x.double(), ln.weight.double(), ln.bias.double(), EPS, 'merge')
        assert float((got.double() - y64).abs().max()) <= 2e-5 * max(1.0, float(y64.abs().max()))


NCHW_SHAPES = [(2, 96, 7 * 9), (1, 32, 300), (2, 192, 33), (1, 768, 40), (3, 384, 1)]


@pytest.mark.parametrize("shape", NCHW_SHAPES)
def test_from_nchw_is_tokens_on_the_transposed_copy(shape):
    B, C, L = shape
    ln = _ln(C)
    g = torch.Generator().manual_seed(4)
    x = (0.3 + torch.randn(shape, generator=g)).cuda()
    with torch.no_grad():
        want = token_layernorm(x.transpose(1, 2).contiguous(), ln, 'tokens', force=True)
        got = token_layernorm(x, ln, 'from_nchw', force=True)
        assert tuple(got.shape) == (B, L, C) and got.is_contiguous() and torch.equal(got, want)
        y64 = token_layernorm_reference(x.double(), ln.weight.double(), ln.bias.double(), EPS, 'from_nchw')
        assert float((got.double() - y64).abs().max()) <= 2e-5 * max(1.0, float(y64.abs().max()))


@pytest.mark.parametrize("shape", NCHW_SHAPES)
def test_to_nchw_is_tokens_permuted_and_contiguous(shape):
    B, C, L = shape
    H, W = (7, 9) if L == 63 else (L, 1) if L < 40 else (L // 4, 4)
    ln = _ln(C)
    g = torch.Generator().manual_seed(5)
    x = (0.3 + torch.randn((B, L, C), generator=g)).cuda()
    with torch.no_grad():
        want = token_layernorm(x, ln, 'tokens', force=True).view(-1, H, W, C).permute(0, 3, 1, 2).contiguous()
        got = token_layernorm(x, ln, 'to_nchw', (H, W), force=True)
        assert got.shape == want.shape and got.is_contiguous() and torch.equal(got, want)
        stock = ln(x).view(-1, H, W, C).permute(0, 3, 1, 2).contiguous()
        assert got.shape == stock.shape
        if L > 1:       # (one token per image: the permuted view is contiguous as it stands and keeps its own strides)
            assert got.stride() == want.stride() == stock.stride()


@pytest.mark.parametrize("L", [4100, 8200])
def test_from_and_to_nchw_on_the_wide_tiles(L):
    """257 tiles of 16 or of 32 tokens (the last one ragged): the widest tile that still gives every CU a workgroup"""
    C = 96
    assert _lib.tile_query("orp_token_layernorm_plan", 3, 1, L, 1, C, LAYOUTS['to_nchw'])[1] == (16 if L == 4100 else 32)
    ln = _ln(C)
    x = _rows(L, C, 6).view(1, L, C)
    with torch.no_grad():
        want = token_layernorm(x, ln, 'tokens', force=True)
        got = token_layernorm(x, ln, 'to_nchw', (L // 4, 4), force=True)
        assert torch.equal(got.view(C, L).t(), want[0])
        back = token_layernorm(x.transpose(1, 2).contiguous(), ln, 'from_nchw', force=True)
        assert torch.equal(back, want)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_exact_rows(layout):
    """a constant row (values whose C-fold sum is exact in fp32, so the mean is the value and every difference a zero) returns beta
    bit for bit; gamma = 0 returns beta bit for bit whatever the row holds"""
    for C in (96, 768, 4096):
        ln = _ln(C)
        T = 37
        rows = torch.tensor([3.0, -0.5, 1024.0, 0.0, 0.375, -7.0, 2.0 ** -20], device='cuda').repeat(6)[:T].view(T, 1).expand(T, C).contiguous()
        got = _run(rows, ln, layout)
        assert torch.equal(got, ln.bias.detach().expand(T, C))
        ln0 = _ln(C, gamma=torch.zeros(C))
        got = _run(_rows(T, C, 3, 2.0, 5.0), ln0, layout)
        assert torch.equal(got, ln0.bias.detach().expand(T, C))


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_non_finite_rows_stay_in_their_row(layout):
    for C in (96, 384):
        ln = _ln(C)
        rows = _rows(129, C, 9)
        clean = _run(rows, ln, layout)
        bad = rows.clone()
        bad[37, 5] = float('inf')
        bad[64, C - 1] = float('nan')
        bad[100, 0] = float('-inf')
        bad[100, 17] = float('inf')
        got = _run(bad, ln, layout)
        keep = torch.ones(129, dtype=torch.bool, device='cuda')
        keep[[37, 64, 100]] = False
        assert torch.equal(got[keep], clean[keep])
        assert torch.isnan(got[~keep]).all()


def _raw(x, ln, y, batch, h, w, C, layout):
    return _lib.lib().orp_token_layernorm(_lib.ptr(x), _lib.ptr(ln.weight.detach()), _lib.ptr(ln.bias.detach()), _lib.ptr(y), batch, h, w, C,
                                          ctypes.c_float(EPS), LAYOUTS[layout], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_stores_cover_y_and_nothing_else(layout):
    for C, (B, H, W) in ((96, (2, 5, 7)), (768, (1, 3, 3)), (192, (1, 1, 1)), (1536, (2, 9, 1))):
        ln = _ln(C)
        src = (B, H, W, C // 4) if layout == 'merge' else (B, C, H * W) if layout == 'from_nchw' else (B, H * W, C)
        x = torch.randn(src, device='cuda')
        want = token_layernorm_reference(x, ln.weight.detach(), ln.bias.detach(), EPS, layout, (H, W) if layout != 'from_nchw' else None)
        n = want.numel()
        buf = torch.full((1024 + n + 1024,), float('nan'), device='cuda')
        y = buf[1024:1024 + n]
        assert _raw(x, ln, y, B, H if layout != 'from_nchw' else H * W, W if layout != 'from_nchw' else 1, C, layout) == _lib.ORP_OK
        torch.cuda.synchronize()
        assert torch.isnan(buf[:1024]).all() and torch.isnan(buf[1024 + n:]).all()
        assert float((y - want.reshape(-1)).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))


def test_argument_rules_on_the_device():
    T, C = 33, 96
    ln = _ln(C)
    x = _rows(T, C, 6)
    y = torch.full((T, C), 7.0, device='cuda')
    E = _lib.ORP_EINVAL
    big = torch.zeros(T * C + 4, device='cuda')
    assert _raw(big[1:1 + T * C], ln, y, T, 1, 1, C, 'tokens') == E                # 4 bytes off
    assert _raw(x, ln, big[1:1 + T * C], T, 1, 1, C, 'tokens') == E
    assert _raw(x, ln, x, T, 1, 1, C, 'tokens') == E
    assert _raw(x, ln, y, -1, 1, 1, C, 'tokens') == E and _raw(x, ln, y, T, 1, 1, 100, 'tokens') == E
    assert _raw(x, ln, y, 0, 1, 1, C, 'tokens') == _lib.ORP_OK
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                                   # nothing was launched
    with torch.no_grad():
        assert tuple(token_layernorm(x.view(3, 11, C), ln, force=True).shape) == (3, 11, C)      # any leading dimensions
        assert tuple(token_layernorm(x[:0], ln, force=True).shape) == (0, C)
        assert tuple(token_layernorm(x.view(1, T, C)[:, :0], ln, 'to_nchw', (0, 5), force=True).shape) == (1, C, 0, 5)
        with pytest.raises(ValueError):
            token_layernorm(x, ln)                                                  # not in the table, not forced
        with pytest.raises(ValueError):
            token_layernorm(x, ln, 'nhwc', force=True)
        with pytest.raises(ValueError):
            token_layernorm(x.t().contiguous().t(), ln, force=True)                 # non-contiguous tokens
        with pytest.raises(ValueError):
            token_layernorm(x.double(), ln, force=True)
        with torch.autocast('cuda', dtype=torch.float16):
            assert not token_layernorm_ok(ln, x)
        assert not token_layernorm_routed(ln, x)
    with pytest.raises(ValueError):
        token_layernorm(x, ln, force=True)                                          # gradients enabled


class _Spy:
    """`_lib.lib()` with the launches of orp_token_layernorm counted"""

    def __init__(self, real):
        self._real, self.launches = real, 0

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name != "orp_token_layernorm":
            return fn

        def counted(*a):
            self.launches += 1
            return fn(*a)
        return counted


@pytest.fixture
def spy(monkeypatch):
    s = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: s)
    return s


def gate(got, want64, what):
    """test_gpu_token_linear.py's gate"""
    err, top = float((got.double() - want64).abs().max()), float(want64.abs().max())
    assert err <= 2e-5 * max(1.0, top), (what, err, top)
    return err / max(1.0, top)


def _randomise(model):
    with torch.no_grad():
        for p in model.parameters():                               # (biases and the position tables are zeros as constructed)
            if p.dim() == 1 or p.size(-1) <= 24:
                p.normal_(0.0, 0.3)
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.add_(1.0)
    return model


def _force(model, on=True):
    for m in model.modules():
        if hasattr(m, 'force_token_norm'):
            m.force_token_norm = on
    return model


def _stage(downsample=False):
    torch.manual_seed(0)
    return _force(_randomise(SwinStage(96, 2, 3, 7, 4., True, None, 0., 0., [0., 0.1], downsample, False)).cuda().eval())


def _report(what, got, stock, want):
    from conftest import REPORT
    theirs = float((stock.double() - want).abs().max()) / max(1.0, float(want.abs().max()))
    line = "%s: error / max(1, |y64|) forced norms %.3e, stock %.3e" % (what, gate(got, want, what), theirs)
    print(line)
    REPORT.append(line)


def test_swin_blocks_forced_against_float64(spy, monkeypatch):
    """(C, heads) = (96, 3) on a 15 x 20 map, shift 0 and 3: two launches per block on each of its routes, none with the switch off,
    under autocast, with gradients or in a .half() block; unforced, these 300 tokens keep the modules' bits"""
    monkeypatch.setattr(switches, "SWIN_NORM_FUSE", True)
    linear_fuse, attn_fuse = switches.SWIN_LINEAR_FUSE, switches.SWIN_ATTN_FUSE
    H, W = 15, 20
    st = _stage()
    st64 = copy.deepcopy(st).double()
    x = torch.randn(1, H * W, 96, device='cuda')
    with torch.no_grad():
        mask = st.shift_mask(H, W, x.device)
        for blk, blk64 in zip(st.blocks, st64.blocks):
            want = blk64(x.double(), H, W, mask.double())
            assert spy.launches == 0
            got = blk(x, H, W, mask)
            assert spy.launches == 2
            blk.fuse_token_norm = False
            stock = blk(x, H, W, mask)
            assert spy.launches == 2
            blk.fuse_token_norm = None
            _report("SwinBlock (96, 3) 15 x 20 shift %d" % blk.shift, got, stock, want)
            # the other two branches of forward: the fused attention between stock linears, then the stock attention
            monkeypatch.setattr(switches, "SWIN_LINEAR_FUSE", False)
            gate(blk(x, H, W, mask), want, "no fused linears")
            assert spy.launches == 4
            monkeypatch.setattr(switches, "SWIN_ATTN_FUSE", False)
            gate(blk(x, H, W, mask), want, "stock attention")
            assert spy.launches == 6
            monkeypatch.setattr(switches, "SWIN_LINEAR_FUSE", linear_fuse)
            monkeypatch.setattr(switches, "SWIN_ATTN_FUSE", attn_fuse)
            # outside the table the unforced block runs the framework's LayerNorm with its bits
            blk.force_token_norm = False
            assert torch.equal(blk(x, H, W, mask), stock) and spy.launches == 6
            blk.force_token_norm = True
            spy.launches = 0
        monkeypatch.setattr(switches, "SWIN_NORM_FUSE", False)
        st(x, H, W)
        assert spy.launches == 0
        monkeypatch.setattr(switches, "SWIN_NORM_FUSE", True)
        st(x, H, W)
        assert spy.launches == 4
        spy.launches = 0
        with torch.autocast('cuda', dtype=torch.float16):
            st(x, H, W)
        assert spy.launches == 0
        copy.deepcopy(st).half()(x.half(), H, W)
        assert spy.launches == 0
    with torch.enable_grad():
        st(x, H, W)
    assert spy.launches == 0


def test_patch_merging_forced_against_float64(spy, monkeypatch):
    """15 x 20 is odd: padded to 16 x 20, 80 rows of 384 channels per image, gathered by the kernel"""
    monkeypatch.setattr(switches, "SWIN_NORM_FUSE", True)
    torch.manual_seed(1)
    pm = _randomise(PatchMerging(96)).cuda().eval()
    pm64 = copy.deepcopy(pm).double()
    x = torch.randn(2, 15 * 20, 96, device='cuda')
    with torch.no_grad():
        want = pm64(x.double(), 15, 20)
        stock = pm(x, 15, 20)
        assert spy.launches == 0                                   # unforced: not in the table
        monkeypatch.setattr(switches, "SWIN_NORM_FUSE", False)
        assert torch.equal(pm(x, 15, 20), stock)
        monkeypatch.setattr(switches, "SWIN_NORM_FUSE", True)
        pm.force_token_norm = True
        got = pm(x, 15, 20)
        assert spy.launches == 1 and tuple(got.shape) == (2, 80, 192)
        _report("PatchMerging 96 -> 192 at 15 x 20", got, stock, want)
        pm.fuse_token_norm = False
        assert torch.equal(pm(x, 15, 20), stock) and spy.launches == 1
        pm.fuse_token_norm = None
        with torch.autocast('cuda', dtype=torch.float16):
            pm(x, 15, 20)
        copy.deepcopy(pm).half()(x.half(), 15, 20)
        assert spy.launches == 1
    with torch.enable_grad():
        assert torch.equal(pm(x, 15, 20), stock) and spy.launches == 1


def test_patch_embed_forced_against_float64(spy, monkeypatch):
    """a 61 x 83 image: padded to 64 x 84, 16 x 21 patches of 96 channels read from the convolution's NCHW output"""
    monkeypatch.setattr(switches, "SWIN_NORM_FUSE", True)
    torch.manual_seed(2)
    pe = _randomise(PatchEmbed()).cuda().eval()
    pe64 = copy.deepcopy(pe).double()
    img = torch.randn(2, 3, 61, 83, device='cuda')
    with torch.no_grad():
        want = pe64(img.double())
        stock = pe(img)
        assert spy.launches == 0
        monkeypatch.setattr(switches, "SWIN_NORM_FUSE", False)
        assert torch.equal(pe(img), stock)
        monkeypatch.setattr(switches, "SWIN_NORM_FUSE", True)
        pe.force_token_norm = True
        got = pe(img)
        assert spy.launches == 1 and got.shape == stock.shape == (2, 96, 16, 21) and got.stride() == stock.stride()
        _report("PatchEmbed at 61 x 83", got, stock, want)
        with torch.autocast('cuda', dtype=torch.float16):
            pe(img)
        copy.deepcopy(pe).half()(img.half())
        assert spy.launches == 1
    with torch.enable_grad():
        assert torch.equal(pe(img), stock) and spy.launches == 1


def test_backbone_forced_against_float64(spy, monkeypatch):
    """two stages on a 61 x 83 image: one launch for the embedding, two per block, one per merge and one per output stage"""
    monkeypatch.setattr(switches, "SWIN_NORM_FUSE", True)
    torch.manual_seed(3)
    net = _randomise(SwinTransformer(embed_dim=96, depths=(2, 2), num_heads=(3, 6), out_indices=(0, 1), drop_path_rate=0.)).cuda().eval()
    net64 = copy.deepcopy(net).double()
    img = torch.randn(1, 3, 61, 83, device='cuda')
    with torch.no_grad():
        want = net64(img.double())
        stock = net(img)
        assert spy.launches == 0
        monkeypatch.setattr(switches, "SWIN_NORM_FUSE", False)
        off = net(img)
        assert all(torch.equal(a, b) for a, b in zip(off, stock))
        monkeypatch.setattr(switches, "SWIN_NORM_FUSE", True)
        net.force_token_norm = True                                 # the output norms alone
        got = net(img)
        assert spy.launches == 2
        _force(net)
        spy.launches = 0
        got = net(img)
        assert spy.launches == 1 + 2 * 4 + 1 + 2
        for i, (a, b, c) in enumerate(zip(got, stock, want)):
            assert a.shape == b.shape and a.stride() == b.stride() and a.is_contiguous()
            _report("SwinTransformer (96, 2 + 2) at 61 x 83, output %d" % i, a, b, c)
        spy.launches = 0
        with torch.autocast('cuda', dtype=torch.float16):
            net(img)
        assert spy.launches == 0
    with torch.enable_grad():
        net(img)
    assert spy.launches == 0


def test_forced_stage_captured_and_replayed_is_bitwise_eager(spy, monkeypatch):
    monkeypatch.setattr(switches, "SWIN_NORM_FUSE", True)
    H, W = 15, 20
    st = _stage(downsample=True)
    g = torch.Generator().manual_seed(3)
    data = [torch.randn((1, H * W, 96), generator=g).cuda() for _ in range(3)]
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager = [[t.clone() for t in st(d, H, W)[:2]] for d in data]
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        static = data[0].clone()
        spy.launches = 0
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = st(static, H, W)[:2]
        assert spy.launches == 5                                   # two blocks of two and the merge
        for d, want in zip(data[1:], eager[1:]):
            static.copy_(d)
            for y in outs:
                y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(outs, want))
