"""GPU: `orp_window_attention` (csrc/orp_window_attn.hip) -- Swin's (shifted-)window attention at inference as one fp32 kernel -- and the
route SwinBlock.forward takes through it.

One accuracy gate for everything here: max |y - y64| <= 2e-5 * max(1, max |y64|), this project's Swin tolerance
(tests/test_swin_backbone.py).  The stock fp32 block sits at 1.5e-7 ... 5.4e-7 of the output's maximum against its float64 twin on
these shapes, so the gate leaves about 40 x to a correct fp32 evaluation, while any indexing error (a transposed bias lookup, a band
off by one, padded keys taken as zero, a wrong batch stride) moves the result by orders of magnitude more.  The float64 reference is
`window_attention_reference`, which tests/test_window_attention_cpu.py holds to the stock block at 1e-12."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from orientedreppoints_amd import _lib, switches
from orientedreppoints_amd.mmdet_models.swin import SwinStage, SwinTransformer, from_windows, to_windows
from orientedreppoints_amd.mmdet_ops import window_attention, window_attention_ok, window_attention_reference

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HEADS = [(2, 12), (4, 24), (3, 32), (24, 32)]                       # (heads, head_dim): the golden config's, Swin-T's first and last stage
MAPS = [(2, 14, 14), (1, 15, 20), (1, 5, 9), (1, 38, 51)]            # whole windows + batch 2; padded on both axes; smaller than a window; many
CASES = [(h, m, s) for h in HEADS for m in MAPS for s in (0, 3)] + [((3, 32), (1, 15, 20), 1), ((3, 32), (1, 15, 20), 6)]


def gate(got, want64, what):
    err, top = float((got.double() - want64).abs().max()), float(want64.abs().max())
    assert err <= 2e-5 * max(1.0, top), (what, err, top)
    return err / max(1.0, top)


def _gen():
    spec = importlib.util.spec_from_file_location("make_golden_swin", os.path.join(HERE, "golden", "make_golden_swin.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def operands(heads, hd, shape, seed, bias=True):
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((B, H * W, 3 * heads * hd), generator=g, dtype=torch.float64)
    qb = torch.randn((3 * heads * hd,), generator=g, dtype=torch.float64) if bias else None
    table = 0.5 * torch.randn((169, heads), generator=g, dtype=torch.float64)
    return [None if t is None else t.cuda() for t in (qkv, qb, table)]


def stock_path(qkv, qb, table, H, W, heads, shift, scale):
    """what the stock SwinBlock + WindowAttention do to the same q / k / v, in their order and with their calls: pad (a padded token's
    q / k / v are the bias), roll, windows, (bias + shift mask) materialised and repeated, scaled_dot_product_attention, back"""
    B, ws, C = qkv.size(0), 7, qkv.size(2) // 3
    y = qkv.view(B, H, W, 3 * C)
    pr, pb = (ws - W % ws) % ws, (ws - H % ws) % ws
    Hp, Wp = H + pb, W + pr
    if pr or pb:
        y = F.pad(y, (0, 0, 0, pr, 0, pb))
        if qb is not None:
            y[:, H:], y[:, :H, W:] = qb, qb
    if shift:
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2))
    w = to_windows(y, ws)
    BW, N = w.shape[:2]
    q, k, v = w.view(BW, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    pos = torch.arange(N, device=qkv.device)
    rel = (pos[:, None] // ws - pos[None, :] // ws + ws - 1) * (2 * ws - 1) + (pos[:, None] % ws - pos[None, :] % ws + ws - 1)
    bias = table[rel.view(-1)].view(N, N, -1).permute(2, 0, 1).unsqueeze(0)
    if shift:
        st = SwinStage.__new__(SwinStage)
        st.ws, st.shift, st._masks = ws, shift, {}
        m = SwinStage.shift_mask(st, H, W, qkv.device).to(q.dtype)
        bias = (bias + m.unsqueeze(1)).repeat(BW // m.size(0), 1, 1, 1)
    out = F.scaled_dot_product_attention(q, k, v, attn_mask=bias, scale=scale)
    y = from_windows(out.transpose(1, 2).reshape(BW, N, C), ws, Hp, Wp)
    if shift:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    return y[:, :H, :W, :].reshape(B, H * W, C)


@pytest.mark.parametrize("heads_hd,shape,shift", CASES)
def test_operator_against_float64(heads_hd, shape, shift):
    (heads, hd), (B, H, W) = heads_hd, shape
    qkv, qb, table = operands(heads, hd, shape, seed=1000 * heads + 10 * H + shift)
    scale = hd ** -0.5
    want = window_attention_reference(qkv, qb, table, H, W, heads, 7, shift, scale)
    got = window_attention(qkv.float(), qb.float(), table.float(), H, W, heads, 7, shift, scale)
    assert got.shape == want.shape and got.dtype == torch.float32
    stock = stock_path(qkv.float(), qb.float(), table.float(), H, W, heads, shift, scale)
    top = max(1.0, float(want.abs().max()))
    print("window_attention heads %d head_dim %d map %s shift %d: fused %.3g stock %.3g (of max(1, max |y64|))"
          % (heads, hd, shape, shift, float((got.double() - want).abs().max()) / top, float((stock.double() - want).abs().max()) / top))
    gate(got, want, (heads_hd, shape, shift))


def test_operator_without_a_bias_and_five_dimensional_qkv():
    heads, hd, (B, H, W) = 3, 32, (1, 15, 20)
    qkv, _, table = operands(heads, hd, (B, H, W), seed=5, bias=False)
    want = window_attention_reference(qkv, None, table, H, W, heads, 7, 3, hd ** -0.5)
    got = window_attention(qkv.float().view(B, H * W, 3, heads, hd), None, table.float(), H, W, heads, 7, 3, hd ** -0.5)
    gate(got, want, "no bias")
    # the padded keys matter: with a bias in their place the result is another one by far more than the gate
    other = window_attention(qkv.float(), torch.ones(3 * heads * hd, device='cuda'), table.float(), H, W, heads, 7, 3, hd ** -0.5)
    assert float((other.double() - want).abs().max()) > 1e-2


@pytest.mark.parametrize("window,heads,hd,shift", [(8, 2, 12, 0), (7, 2, 36, 0), (7, 2, 10, 0), (7, 2, 12, 7)])
def test_argument_rules(window, heads, hd, shift):
    B, H, W = 1, 9, 10
    qkv = torch.randn(B, H * W, 3 * heads * hd, device='cuda')
    qb = torch.randn(3 * heads * hd, device='cuda')
    table = torch.randn((2 * window - 1) ** 2, heads, device='cuda')
    out = torch.full((B, H * W, heads * hd), 7.25, device='cuda')
    with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
        window_attention(qkv, qb, table, H, W, heads, window, shift, hd ** -0.5, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.25).all())


def test_operator_refuses_what_is_not_its_input():
    qkv, qb, table = [t.float() for t in operands(2, 12, (1, 9, 10), seed=3)]
    args = (9, 10, 2, 7, 3, 12 ** -0.5)
    with pytest.raises(TypeError):
        window_attention(qkv.cpu(), qb, table, *args)
    with pytest.raises(TypeError):
        window_attention(qkv.double(), qb, table, *args)
    with pytest.raises(ValueError):
        window_attention(qkv.transpose(1, 2).contiguous().transpose(1, 2), qb, table, *args)      # the right shape, not contiguous
    with pytest.raises(ValueError):
        window_attention(qkv, qb[:-1], table, *args)
    with pytest.raises(ValueError):
        window_attention(qkv, qb, table[:-1], *args)
    with pytest.raises(ValueError):
        window_attention(qkv, qb, table, 9, 11, 2, 7, 3, 12 ** -0.5)


def test_routing_rule_on_the_device():
    def stage(**kw):
        a = dict(dim=24, depth=2, num_heads=2, window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=[0., 0.], downsample=False, use_checkpoint=False)
        a.update(kw)
        return SwinStage(**a).cuda().eval()
    x = torch.randn(1, 49, 24, device='cuda')
    st = stage()
    with torch.no_grad():
        assert window_attention_ok(st.blocks[0].attn, x) and st.blocks[1].fuses_attention(x)
        assert not window_attention_ok(st.blocks[0].attn, x.cpu())
        assert not window_attention_ok(st.blocks[0].attn, x.half()) and not window_attention_ok(st.blocks[0].attn, x.double())
        assert not window_attention_ok(copy.deepcopy(st).half().blocks[0].attn, x)
        assert not window_attention_ok(stage(window_size=4).blocks[0].attn, x)
        assert not window_attention_ok(stage(num_heads=4).blocks[0].attn, x)            # head dim 6
        assert not window_attention_ok(stage(attn_drop=0.1).train().blocks[0].attn, x)
        assert window_attention_ok(stage(attn_drop=0.1).blocks[0].attn, x)               # dropout inactive in eval mode
        with torch.autocast('cuda', dtype=torch.float16):
            assert not window_attention_ok(st.blocks[0].attn, x)
    with torch.enable_grad():
        assert not window_attention_ok(st.blocks[0].attn, x)


class _Spy:
    """`_lib.lib()` with the launches of orp_window_attention counted"""

    def __init__(self, real):
        self._real, self.launches = real, 0

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name != "orp_window_attention":
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


def test_backbone_against_the_golden_outputs_and_launch_counts(spy, monkeypatch):
    gen = _gen()
    G = np.load(os.path.join(HERE, "golden", "swin_py.npz"))
    model = SwinTransformer(**gen.CFG).eval()
    gen.fill_parameters(model)
    model.cuda()
    monkeypatch.setattr(switches, "SWIN_ATTN_FUSE", True)
    with torch.no_grad():
        for ci, case in enumerate(gen.CASES):
            for st in model.layers:
                st._masks.clear()
            spy.launches = 0
            outs = model(gen.inputs(case).cuda())
            assert spy.launches == 8, (case, spy.launches)                                  # once per block
            assert all(len(st._masks) == 0 for st in model.layers)                           # the shift mask is not evaluated
            for li, y in enumerate(outs):
                want = torch.from_numpy(G["case%d_out%d" % (ci, li)]).double().cuda()
                assert tuple(y.shape) == tuple(want.shape)
                gate(y, want, (case, li))
        x = gen.inputs(gen.CASES[2]).cuda()
        fused = model(x)
        spy.launches = 0
        monkeypatch.setattr(switches, "SWIN_ATTN_FUSE", False)
        stock = model(x)
        assert spy.launches == 0
        monkeypatch.setattr(switches, "SWIN_ATTN_FUSE", True)
        for blk in [b for st in model.layers for b in st.blocks]:
            blk.fuse_window_attention = False
        assert all(torch.equal(a, b) for a, b in zip(model(x), stock)) and spy.launches == 0
        model.layers[0].blocks[1].fuse_window_attention = None                                # per object: back to the module's switch
        model(x)
        assert spy.launches == 1
    with torch.enable_grad():
        model(x)
        assert spy.launches == 1
    for a, b in zip(fused, stock):
        gate(a, b.double(), "fused against stock")


def test_swin_tiny_dota_config_fused_against_stock(reference_configs, monkeypatch):
    from orientedreppoints_amd.mmdet_models import Config, build_detector
    cfg = Config(copy.deepcopy(dict(reference_configs["orientedrepoints_swin_tiny_demo.py"]._cfg_dict)))
    cfg.model.pretrained = None
    torch.manual_seed(0)
    m = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).cuda().eval()
    x = torch.randn(1, 3, 128, 160, device='cuda')
    feats = {}
    with torch.no_grad():
        for on in (True, False):
            monkeypatch.setattr(switches, "SWIN_ATTN_FUSE", on)
            feats[on] = [f.clone() for f in m.neck(m.backbone(x))]
    assert [tuple(f.shape[1:]) for f in feats[True]] == [(256, 16, 20), (256, 8, 10), (256, 4, 5), (256, 2, 3), (256, 1, 2)]
    for li, (a, b) in enumerate(zip(feats[True], feats[False])):
        gate(a, b.double(), ("level", li))


def test_fused_backbone_is_bitwise_reproducible_eager_and_replayed(spy, monkeypatch):
    gen = _gen()
    model = SwinTransformer(**gen.CFG).eval()
    gen.fill_parameters(model)
    model.cuda()
    monkeypatch.setattr(switches, "SWIN_ATTN_FUSE", True)
    x = gen.inputs(gen.CASES[2]).cuda()
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager = [y.clone() for y in model(x)]
            again = [y.clone() for y in model(x)]
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, again))
        spy.launches = 0
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = model(x)
        assert spy.launches == 8
        replays = []
        for _ in range(2):
            for y in outs:
                y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            replays.append([y.clone() for y in outs])
    for a, b, c in zip(eager, replays[0], replays[1]):
        assert torch.equal(b, c) and torch.equal(a, b)
