"""GPU: orp_token_linear (csrc/orp_token_linear.hip) -- a per-token linear with bias, exact GELU and residual in its epilogue on the
bf16-pieces matrix path -- against float64 at the smallest shapes at which each of its mechanisms can go wrong, and the Swin modules
that route their linears through it.  Every launch here is forced: the routing table is not asked.

The shape grid: T around the 32-token MFMA block and the 32 / 64 / 128-token tiles (1, 31, 32, 33, 127, 129, 257), K a whole and a
ragged number of 64-wide steps (32, 64, 96, 160), N below, at and across the 128-channel tile (32, 96, 160, 288); two long token
counts switch the launch to its 64- and 128-token tiles (the tile is chosen from the number of workgroups)."""
import copy
import ctypes
import importlib

import pytest
import torch

from orientedreppoints_amd import _lib, _packcache, switches
from orientedreppoints_amd.mmdet_models.swin import PatchMerging, SwinStage
from orientedreppoints_amd.mmdet_ops.token_linear import token_linear, token_linear_ok, token_linear_reference, token_linear_routed

pytestmark = pytest.mark.gpu
TL = importlib.import_module("orientedreppoints_amd.mmdet_ops.token_linear")      # (the package exports the function under the same name)

TS = (1, 31, 32, 33, 127, 129, 257)
KS = (32, 64, 96, 160)
NS = (32, 96, 160, 288)
EXACT_KN = ((32, 32), (96, 96), (96, 288), (160, 160))
LONG = ((10900, 96, 288), (21900, 96, 288))          # 3 x 171 and 3 x 172 workgroups: the 64- and the 128-token tile
# (bias, act, residual): PatchMerging.reduction, attn.qkv, mlp.fc1, attn.proj / mlp.fc2 -- and a bias-free residual for the epilogue's sake
EPILOGUES = {"none": (False, None, False), "bias": (True, None, False), "bias_gelu": (True, 'gelu', False),
             "bias_res": (True, None, True), "res": (False, None, True)}
U = 2.0 ** -24


def gate(got, want64, what):
    err, top = float((got.double() - want64).abs().max()), float(want64.abs().max())
    assert err <= 2e-5 * max(1.0, top), (what, err, top)
    return err / max(1.0, top)


def _linear(K, N, bias, w, b=None):
    lin = torch.nn.Linear(K, N, bias=bias).cuda()
    with torch.no_grad():
        lin.weight.copy_(w)
        if bias:
            lin.bias.copy_(b)
    return lin


def _random(T, K, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((T, K), generator=g)
    w = torch.randn((N, K), generator=g)
    b = torch.randn((N,), generator=g)
    r = torch.randn((T, N), generator=g)
    return x.cuda(), w.cuda(), b.cuda(), r.cuda()


def _integers(T, K, N, seed):
    """|x|, |w| <= 8 and |bias|, |res| <= 64: every product, every partial sum in any order (<= 160 * 64) and the epilogue are exact"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (T, K), generator=g).float()
    w = torch.randint(-8, 9, (N, K), generator=g).float()
    b = torch.randint(-64, 65, (N,), generator=g).float()
    r = torch.randint(-64, 65, (T, N), generator=g).float()
    return x.cuda(), w.cuda(), b.cuda(), r.cuda()


def _run(x, w, b, r, epi):
    bias, act, res = EPILOGUES[epi]
    lin = _linear(w.size(1), w.size(0), bias, w, b)
    with torch.no_grad():
        assert token_linear_ok(lin, x)
        return token_linear(x, lin, act, r if res else None, force=True)


def _want64(x, w, b, r, epi):
    bias, act, res = EPILOGUES[epi]
    return token_linear_reference(x.double(), w.double(), b.double() if bias else None, act, r.double() if res else None)


@pytest.mark.parametrize("K,N", EXACT_KN)
def test_exact_integer_data_is_bit_exact(K, N):
    """bit for bit the float64 result cast to fp32, over the whole T list (the epilogues without the GELU, which is not exact)"""
    for T in TS:
        x, w, b, r = _integers(T, K, N, 11 + T)
        for epi in ("none", "bias", "bias_res", "res"):
            got = _run(x, w, b, r, epi)
            want = _want64(x, w, b, r, epi).float()
            assert got.shape == want.shape and torch.equal(got, want), (T, K, N, epi)


@pytest.mark.parametrize("T,K,N", LONG)
def test_exact_integer_data_on_the_wide_tiles(T, K, N):
    x, w, b, r = _integers(T, K, N, 5)
    for epi in ("none", "bias_res"):
        assert torch.equal(_run(x, w, b, r, epi), _want64(x, w, b, r, epi).float()), (T, epi)


@pytest.mark.parametrize("K,N", [(160, 288), (96, 96), (32, 160)])
def test_one_hot_probes(K, N):
    """each k alone: token t = e_k returns column k of the weight, bit for bit (w0 + w1 + w2 is w).  Each n alone at the channel-tile
    and wave seams: a weight with one row of ones returns the tokens' sums in that channel and exact zeros elsewhere."""
    g = torch.Generator().manual_seed(2)
    w = torch.randn((N, K), generator=g).cuda()
    x = torch.eye(K, device='cuda')
    y = _run(x, w, None, None, "none")
    assert torch.equal(y, w.t().contiguous())
    xi = torch.randint(-8, 9, (33, K), generator=g).float().cuda()
    for n in sorted({0, 31, 32, 95, 96, 127, 128, 159, 255, 256, N - 1} & set(range(N))):
        w1 = torch.zeros((N, K), device='cuda')
        w1[n] = 1.0
        y = _run(xi, w1, None, None, "none")
        want = torch.zeros((33, N), device='cuda')
        want[:, n] = xi.sum(1)
        assert torch.equal(y, want), n


def _fractions(x, w, b, r, epi):
    """(worst error of the kernel, of the stock route) as fractions of the first-order bound
    2^-24 [(K + 5) sum_k |x w| + 2 (|bias| + |res|) + |y64|] -- 2 of the 5 for the fp32 sum, 3 for the three dropped piece products; with
    the GELU 1.13 x that bound on the pre-activation (|gelu'| <= 1.13) plus 4 * 2^-24 (|u| + |gelu(u)|) for erff and the products"""
    bias, act, res = EPILOGUES[epi]
    K = x.size(1)
    x64, w64 = x.double(), w.double()
    absum = x64.abs() @ w64.abs().t()
    b64 = b.double() if bias else torch.zeros_like(b, dtype=torch.float64)
    r64 = r.double() if res else torch.zeros_like(r, dtype=torch.float64)
    y64 = _want64(x, w, b, r, epi)
    if act == 'gelu':
        u64 = x64 @ w64.t() + b64
        bound = 1.13 * U * ((K + 5) * absum + 2 * b64.abs() + u64.abs()) + 4 * U * (u64.abs() + y64.abs())
    else:
        bound = U * ((K + 5) * absum + 2 * (b64.abs() + r64.abs()) + y64.abs())
    got = _run(x, w, b, r, epi)
    with torch.no_grad():
        stock = TL.stock_linear(_linear(K, w.size(0), bias, w, b), x, act, r if res else None)
    return float(((got.double() - y64).abs() / bound).max()), float(((stock.double() - y64).abs() / bound).max())


@pytest.mark.parametrize("epi", sorted(EPILOGUES))
def test_random_data_against_float64(epi):
    """N(0, 1) data over the whole grid and the two long token counts: the worst error is inside the first-order bound and at most twice
    the worst error of the library's route (F.linear, F.gelu, addition) on the same inputs, both as fractions of that bound"""
    from conftest import REPORT
    worst = stock = 0.0
    shapes = [(T, K, N) for T in TS for K in KS for N in NS] + list(LONG)
    for i, (T, K, N) in enumerate(shapes):
        ours, theirs = _fractions(*_random(T, K, N, 100 + i), epi)
        worst, stock = max(worst, ours), max(stock, theirs)
    line = "token_linear %-9s worst error / bound: kernel %.4f, stock route %.4f (%d shapes)" % (epi, worst, stock, len(shapes))
    print(line)
    REPORT.append(line)
    assert worst < 1.0, line
    assert worst <= 2.0 * stock, line


@pytest.mark.parametrize("K,N,epi", [(96, 288, "bias"), (160, 288, "bias_gelu"), (64, 288, "bias_res")])
def test_a_row_does_not_depend_on_the_launch(K, N, epi):
    """tiling independence: a row launched alone (T = 1) has the bits of the same row inside T = 257 and inside the launches that take
    the 64- and 128-token tiles; determinism: the same launch twice gives the same bits"""
    x, w, b, r = _random(21900, K, N, 7)
    full = _run(x, w, b, r, epi)
    assert torch.equal(full, _run(x, w, b, r, epi))
    for T in (257, 10900):
        part = _run(x[:T].contiguous(), w, b, r[:T].contiguous(), epi)
        assert torch.equal(part, full[:T]), T
    for t in (0, 31, 32, 100, 256, 10899, 21899):
        alone = _run(x[t:t + 1].contiguous(), w, b, r[t:t + 1].contiguous(), epi)
        assert torch.equal(alone[0], full[t]), t


def test_non_finite_rows_stay_in_their_token():
    x, w, b, r = _random(129, 96, 160, 9)
    clean = _run(x, w, b, r, "bias_res")
    bad = x.clone()
    bad[37, 5] = float('inf')
    bad[37, 70] = float('nan')
    got = _run(bad, w, b, r, "bias_res")
    keep = torch.ones(129, dtype=torch.bool, device='cuda')
    keep[37] = False
    assert torch.equal(got[keep], clean[keep])
    assert not torch.isfinite(got[37]).any()


def _raw(x, planes, b, r, y, T, K, N, act):
    return _lib.lib().orp_token_linear(_lib.ptr(x), _lib.ptr(planes), _lib.ptr(b), _lib.ptr(r), _lib.ptr(y), T, K, N, act,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("T,K,N", [(1, 32, 32), (33, 96, 96), (129, 160, 288), (257, 64, 160)])
def test_stores_cover_y_and_nothing_else(T, K, N):
    x, w, b, r = _random(T, K, N, 4)
    planes = TL._packed_weight(_linear(K, N, False, w).weight)
    buf = torch.full((1024 + T * N + 1024,), float('nan'), device='cuda')
    y = buf[1024:1024 + T * N].view(T, N)
    assert _raw(x, planes, b, r, y, T, K, N, 1) == _lib.ORP_OK
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    assert torch.isnan(buf[:1024]).all() and torch.isnan(buf[1024 + T * N:]).all()
    want = token_linear_reference(x.double(), w.double(), b.double(), 'gelu', r.double())
    gate(y, want, (T, K, N))


def test_argument_rules_on_the_device():
    T, K, N = 33, 96, 96
    x, w, b, r = _random(T, K, N, 6)
    planes = TL._packed_weight(_linear(K, N, False, w).weight)
    y = torch.full((T, N), 7.0, device='cuda')
    E = _lib.ORP_EINVAL
    big = torch.zeros(T * K + 4, device='cuda')
    assert _raw(big[1:1 + T * K], planes, b, r, y, T, K, N, 0) == E             # 4 bytes off
    assert _raw(x, planes, b, r, torch.zeros(T * N + 4, device='cuda')[1:1 + T * N], T, K, N, 0) == E
    assert _raw(x, planes, b, x, x, T, K, N, 0) == E and _raw(x, planes, b, y, y, T, K, N, 0) == E
    assert _raw(x, planes, b, r, y, -1, K, N, 0) == E and _raw(x, planes, b, r, y, T, 24, N, 0) == E
    assert _raw(x, planes, b, r, y, T, K, 20, 0) == E and _raw(x, planes, b, r, y, T, K, N, 3) == E
    assert _raw(None, planes, b, r, y, T, K, N, 0) == E and _raw(x, None, b, r, y, T, K, N, 0) == E
    assert _raw(x, planes, b, r, y, 0, K, N, 0) == _lib.ORP_OK
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                              # nothing was launched
    lin = _linear(K, N, True, w, b)
    with torch.no_grad():
        assert tuple(token_linear(x.view(3, 11, K), lin, force=True).shape) == (3, 11, N)      # any leading dimensions
        assert tuple(token_linear(x[:0], lin, force=True).shape) == (0, N)
        with pytest.raises(ValueError):
            token_linear(x, lin)                                               # not in the table, not forced
        with pytest.raises(ValueError):
            token_linear(x, lin, act='relu', force=True)
        with pytest.raises(ValueError):
            token_linear(x, lin, residual=r[:, :32], force=True)
        with pytest.raises(ValueError):
            token_linear(x.t().contiguous().t(), lin, force=True)              # non-contiguous tokens
        with torch.autocast('cuda', dtype=torch.float16):
            assert not token_linear_ok(lin, x)
        assert not token_linear_routed(lin, x)
    with pytest.raises(ValueError):
        token_linear(x, lin, force=True)                                       # gradients enabled


def test_pack_cache():
    x, w, b, r = _random(33, 96, 96, 8)
    lin = _linear(96, 96, True, w, b)
    cache = TL._packed
    assert cache in _packcache._all and cache.name == "token_linear_weight"
    with torch.no_grad():
        h, m = cache.hits, cache.misses
        y1 = token_linear(x, lin, force=True)
        assert (cache.hits, cache.misses) == (h, m + 1)
        y2 = token_linear(x, lin, force=True)
        assert (cache.hits, cache.misses) == (h + 1, m + 1) and torch.equal(y1, y2)
        lin.weight.mul_(2.0)                                                   # in place: the version counter moves
        lin.bias.mul_(2.0)
        y3 = token_linear(x, lin, force=True)
        assert (cache.hits, cache.misses) == (h + 1, m + 2) and torch.equal(y3, 2.0 * y1)
        _packcache.invalidate_all()
        token_linear(x, lin, force=True)
        assert cache.misses == m + 3


class _Spy:
    """`_lib.lib()` with the launches of orp_token_linear counted"""

    def __init__(self, real):
        self._real, self.launches = real, 0

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name != "orp_token_linear":
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


def _stage(force=True, downsample=False):
    torch.manual_seed(0)
    st = SwinStage(96, 2, 3, 7, 4., True, None, 0., 0., [0., 0.1], downsample, False)
    with torch.no_grad():
        for p in st.parameters():                                  # (biases and the position table are zeros as constructed)
            if p.dim() == 1 or p.size(-1) == 3:
                p.normal_(0.0, 0.3)
        for m in st.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.add_(1.0)
    st = st.cuda().eval()
    for m in list(st.blocks) + ([st.downsample] if downsample else []):
        m.force_token_linear = force
    return st


def test_swin_blocks_forced_against_float64(spy, monkeypatch):
    """(C, heads) = (96, 3) on a 15 x 20 map, shift 0 and 3: the forced route against a float64 copy of the block under the gate of the
    attention tests, the stock route's error beside it; four launches per block, none with the switch off, with gradients or autocast"""
    from conftest import REPORT
    monkeypatch.setattr(switches, "SWIN_LINEAR_FUSE", True)
    monkeypatch.setattr(switches, "SWIN_ATTN_FUSE", True)
    H, W = 15, 20
    st = _stage()
    st64 = copy.deepcopy(st).double()
    x = torch.randn(1, H * W, 96, device='cuda')
    with torch.no_grad():
        mask = st.shift_mask(H, W, x.device)
        for blk, blk64 in zip(st.blocks, st64.blocks):
            want = blk64(x.double(), H, W, mask.double())
            spy.launches = 0
            got = blk(x, H, W, None)
            assert spy.launches == 4
            err = gate(got, want, ("forced", blk.shift))
            blk.fuse_token_linear = False
            stock = blk(x, H, W, None)
            assert spy.launches == 4
            blk.fuse_token_linear = None
            line = "SwinBlock (96, 3) 15 x 20 shift %d: error / max(1, |y64|) forced %.3e, stock %.3e" % (blk.shift, err, gate(stock, want, "stock"))
            print(line)
            REPORT.append(line)
            # outside the table the unforced block runs the library's launches with their bits
            blk.force_token_linear = False
            assert torch.equal(blk(x, H, W, None), stock) and spy.launches == 4
            blk.force_token_linear = True
            # a non-contiguous x keeps the modules
            xt = x.transpose(1, 2).contiguous().transpose(1, 2)
            assert not xt.is_contiguous() and not blk.fuses_linears(xt)
            blk(xt, H, W, None)
            assert spy.launches == 4
        spy.launches = 0
        monkeypatch.setattr(switches, "SWIN_LINEAR_FUSE", False)
        st(x, H, W)
        assert spy.launches == 0
        monkeypatch.setattr(switches, "SWIN_LINEAR_FUSE", True)
        st(x, H, W)
        assert spy.launches == 8
        spy.launches = 0
        with torch.autocast('cuda', dtype=torch.float16):
            st(x, H, W)
        assert spy.launches == 0
        st.train()
        st(x, H, W)
        assert spy.launches == 0
        st.eval()
        monkeypatch.setattr(switches, "SWIN_ATTN_FUSE", False)                    # the stock attention branch
        st(x, H, W)
        assert spy.launches == 0
    with torch.enable_grad():
        st(x, H, W)
    assert spy.launches == 0


def test_patch_merging_forced_against_float64(spy, monkeypatch):
    """15 x 20 is odd: padded to 16 x 20, 80 tokens of 384 channels -> 192"""
    from conftest import REPORT
    monkeypatch.setattr(switches, "SWIN_LINEAR_FUSE", True)
    torch.manual_seed(1)
    pm = PatchMerging(96).cuda().eval()
    pm64 = copy.deepcopy(pm).double()
    x = torch.randn(2, 15 * 20, 96, device='cuda')
    with torch.no_grad():
        want = pm64(x.double(), 15, 20)
        stock = pm(x, 15, 20)
        assert spy.launches == 0
        pm.force_token_linear = True
        got = pm(x, 15, 20)
        assert spy.launches == 1 and tuple(got.shape) == (2, 80, 192)
        line = "PatchMerging 96 -> 192 at 15 x 20: error / max(1, |y64|) forced %.3e, stock %.3e" % (gate(got, want, "forced"), gate(stock, want, "stock"))
        print(line)
        REPORT.append(line)
        pm.fuse_token_linear = False
        assert torch.equal(pm(x, 15, 20), stock) and spy.launches == 1
    with torch.enable_grad():
        pm.fuse_token_linear = None
        assert torch.equal(pm(x, 15, 20), stock) and spy.launches == 1


def test_forced_stage_captured_and_replayed_is_bitwise_eager(spy, monkeypatch):
    monkeypatch.setattr(switches, "SWIN_LINEAR_FUSE", True)
    monkeypatch.setattr(switches, "SWIN_ATTN_FUSE", True)
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
        assert spy.launches == 9                                   # two blocks of four and the merge
        for d, want in zip(data[1:], eager[1:]):
            static.copy_(d)
            for y in outs:
                y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(outs, want))
