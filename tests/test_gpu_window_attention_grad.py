"""GPU: Swin's (shifted-)window attention in training -- `orp_window_attention_train` (the forward that keeps the rows' log-sum-exp) and
`orp_window_attention_backward` (csrc/orp_window_attn.hip) -- and the route SwinBlock.forward takes through them.

One accuracy gate for every gradient tensor g: max |g - g64| <= 2e-5 * max(1, max |g64|), this project's Swin tolerance
(tests/test_gpu_window_attention.py).  g64 comes from torch.autograd.grad through `window_attention_reference` in float64, which
tests/test_window_attention_grad_cpu.py holds to the stock block's autograd at 1e-10.  The same reference evaluated in fp32 differs
from its float64 gradients by at most 5.7e-7 (qkv), 1.8e-7 (qkv_bias) and 5.9e-7 (bias_table) of that scale on these shapes, so the
gate leaves about 30 x to a correct fp32 evaluation, while an indexing error moves a gradient by orders of magnitude more.  The
stock GPU path's error (autograd through `stock_path`'s construction) is printed next to the fused one; there is no gate on their
ratio."""
import copy
import functools

import pytest
import torch

from orientedreppoints_amd import _lib, switches
from orientedreppoints_amd.mmdet_models.swin import StochasticDepth
from orientedreppoints_amd.mmdet_ops import (window_attention, window_attention_backward, window_attention_forward_lse,
                                             window_attention_reference, window_attention_train, window_attention_train_ok)
from test_gpu_window_attention import CASES, gate, operands, stock_path
from test_window_attention_cpu import make_stage

pytestmark = pytest.mark.gpu
HEADS = [(2, 12), (4, 24), (3, 32), (24, 32)]                       # (heads, head_dim): the golden config's, Swin-T's first and last stage
MAPS = [(2, 14, 14), (1, 15, 20), (1, 5, 9)]                         # whole windows + batch 2; padded on both axes; smaller than a window
GRAD_CASES = ([(h, m, s) for h in HEADS for m in MAPS for s in (0, 3)]
              + [((3, 32), (1, 15, 20), 1), ((3, 32), (1, 15, 20), 6)]
              # 96 windows per head: the reduction across windows (sixteen interleaved slices of six)
              + [((2, 12), (2, 38, 51), 0), ((2, 12), (2, 38, 51), 3), ((3, 32), (2, 38, 51), 0), ((3, 32), (2, 38, 51), 3)]
              # 30 windows per head: more than the reduction's sixteen slices and no multiple of them
              + [((2, 12), (1, 30, 40), 3)]
              # every head dim once
              + [((2, hd), (1, 15, 20), 3) for hd in range(4, 33, 4) if hd != 12])


@functools.lru_cache(maxsize=None)
def case(heads_hd, shape, shift, bias=True):
    """operands (float64, the existing test's generator), grad_out ~ N(0, 1) and the float64 reference: out, lse, the three gradients.
    Computed once per case and shared; nothing changes it."""
    (heads, hd), (B, H, W) = heads_hd, shape
    qkv, qb, table = operands(heads, hd, shape, seed=1000 * heads + 10 * H + shift, bias=bias)
    go = torch.randn((B, H * W, heads * hd), generator=torch.Generator().manual_seed(77 + H + shift), dtype=torch.float64).cuda()
    leaves = [t.requires_grad_() for t in (qkv, qb, table) if t is not None]
    out, lse = window_attention_reference(qkv, qb, table, H, W, heads, 7, shift, hd ** -0.5, with_lse=True)
    grads = list(torch.autograd.grad((out * go).sum(), leaves))
    if qb is None:
        grads.insert(1, None)
    return dict(ops=[None if t is None else t.detach() for t in (qkv, qb, table)], go=go, out=out.detach(), lse=lse.detach(), grads=grads,
                geometry=(H, W, heads, 7, shift, hd ** -0.5))


def f32(ts):
    return [None if t is None else t.float() for t in ts]


def fused_gradients(c, **kw):
    qkv, qb, table = f32(c["ops"])
    out, lse = window_attention_forward_lse(qkv, qb, table, *c["geometry"])
    return window_attention_backward(qkv, qb, table, out, lse, c["go"].float(), *c["geometry"], **kw)


def stock_gradients(c):
    leaves = [t.requires_grad_() for t in f32(c["ops"])]
    H, W, heads, _, shift, scale = c["geometry"]
    grads = torch.autograd.grad((stock_path(*leaves, H, W, heads, shift, scale) * c["go"].float()).sum(), leaves, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]          # (no padded token: the bias is not read)


def rel(got, want64):
    return float((got.double() - want64).abs().max()) / max(1.0, float(want64.abs().max()))


@pytest.mark.parametrize("heads_hd,shape,shift", CASES)
def test_training_forward_is_the_inference_kernel_bit_for_bit_and_lse_against_float64(heads_hd, shape, shift):
    c = case(heads_hd, shape, shift)
    qkv, qb, table = f32(c["ops"])
    out, lse = window_attention_forward_lse(qkv, qb, table, *c["geometry"])
    assert torch.equal(out, window_attention(qkv, qb, table, *c["geometry"]))
    assert lse.shape == c["lse"].shape and lse.dtype == torch.float32
    gate(lse, c["lse"], ("lse", heads_hd, shape, shift))
    gate(out, c["out"], ("out", heads_hd, shape, shift))


@pytest.mark.parametrize("heads_hd,shape,shift", GRAD_CASES)
def test_gradients_against_float64(heads_hd, shape, shift):
    c = case(heads_hd, shape, shift)
    got, stock = fused_gradients(c), stock_gradients(c)
    print("window_attention_backward heads %d head_dim %d map %s shift %d (fused / stock, of max(1, max |g64|)): %s"
          % (heads_hd + (shape, shift, "  ".join("%s %.3g / %.3g" % (n, rel(g, w), rel(s, w))
                                                 for n, g, s, w in zip(("qkv", "qkv_bias", "bias_table"), got, stock, c["grads"])))))
    for name, g, w in zip(("grad_qkv", "grad_qkv_bias", "grad_bias_table"), got, c["grads"]):
        assert g.shape == w.shape and g.dtype == torch.float32
        gate(g, w, (name, heads_hd, shape, shift))
    # structure of the bias gradient: a padded query has no output, so the q third is exactly zero; without padded tokens so are k and v
    C = heads_hd[0] * heads_hd[1]
    assert bool((got[1][:C] == 0).all())
    if shape[1] % 7 == 0 and shape[2] % 7 == 0:
        assert bool((got[1] == 0).all())
    else:
        assert float(got[1][C:2 * C].abs().max()) > 0 and float(got[1][2 * C:].abs().max()) > 0


def test_gradients_without_a_bias_and_five_dimensional_qkv():
    heads, hd, (B, H, W) = 3, 32, (1, 15, 20)
    c = case((heads, hd), (B, H, W), 3, bias=False)
    qkv, _, table = f32(c["ops"])
    qkv5 = qkv.view(B, H * W, 3, heads, hd)
    out, lse = window_attention_forward_lse(qkv5, None, table, *c["geometry"])
    gq, gb, gt = window_attention_backward(qkv5, None, table, out, lse, c["go"].float(), *c["geometry"])
    assert gb is None and gq.shape == qkv5.shape
    gate(gq.view(B, H * W, -1), c["grads"][0], "grad_qkv, no bias")
    gate(gt, c["grads"][2], "grad_bias_table, no bias")
    with pytest.raises(ValueError):
        window_attention_backward(qkv5, None, table, out, lse, c["go"].float(), *c["geometry"],
                                  grads=(None, torch.zeros(3 * heads * hd, device='cuda'), None))


@pytest.mark.parametrize("heads_hd,shape,shift", [((3, 32), (1, 15, 20), 3), ((2, 12), (2, 14, 14), 0), ((2, 12), (2, 38, 51), 3)])
def test_every_element_is_written(heads_hd, shape, shift):
    c = case(heads_hd, shape, shift)
    qkv, qb, table = f32(c["ops"])
    nan = float('nan')
    out, lse = window_attention_forward_lse(qkv, qb, table, *c["geometry"], out=torch.full_like(c["out"], nan, dtype=torch.float32),
                                            lse=torch.full_like(c["lse"], nan, dtype=torch.float32))
    grads = tuple(torch.full_like(t, nan) for t in (qkv, qb, table))
    got = window_attention_backward(qkv, qb, table, out, lse, c["go"].float(), *c["geometry"], grads=grads)
    assert all(a is b for a, b in zip(got, grads))
    for name, g, w in zip(("out", "lse", "grad_qkv", "grad_qkv_bias", "grad_bias_table"), (out, lse) + got, [c["out"], c["lse"]] + c["grads"]):
        assert bool(torch.isfinite(g).all()), name
        gate(g, w, (name, "pre-filled with NaN"))


@pytest.mark.parametrize("window,heads,hd,shift", [(8, 2, 12, 0), (7, 2, 36, 0), (7, 2, 10, 0), (7, 2, 12, 7)])
def test_argument_rules(window, heads, hd, shift):
    B, H, W = 1, 9, 10
    C = heads * hd
    qkv = torch.randn(B, H * W, 3 * C, device='cuda')
    qb = torch.randn(3 * C, device='cuda')
    table = torch.randn((2 * window - 1) ** 2, heads, device='cuda')
    out, lse = torch.full((B, H * W, C), 7.25, device='cuda'), torch.full((B, H * W, heads), 7.25, device='cuda')
    with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
        window_attention_forward_lse(qkv, qb, table, H, W, heads, window, shift, hd ** -0.5, out=out, lse=lse)
    grads = tuple(torch.full_like(t, 7.25) for t in (qkv, qb, table))
    with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
        window_attention_backward(qkv, qb, table, out, lse, torch.randn(B, H * W, C, device='cuda'), H, W, heads, window, shift, hd ** -0.5,
                                  grads=grads, workspace=torch.empty(1 << 20, dtype=torch.uint8, device='cuda'))
    torch.cuda.synchronize()
    assert all(bool((t == 7.25).all()) for t in (out, lse) + grads)


def test_a_workspace_that_is_too_small_is_refused():
    c = case((2, 12), (1, 15, 20), 3)
    qkv, qb, table = f32(c["ops"])
    H, W, heads, window = c["geometry"][:4]
    need = _lib.lib().orp_window_attention_backward_workspace_bytes(1, H, W, heads, 12, window)
    assert need == 3 * 3 * heads * (169 + 2 * 12) * 4
    assert _lib.lib().orp_window_attention_backward_workspace_bytes(1, H, W, heads, 10, window) == 0
    out, lse = window_attention_forward_lse(qkv, qb, table, *c["geometry"])
    grads = tuple(torch.full_like(t, 7.25) for t in (qkv, qb, table))
    with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
        window_attention_backward(qkv, qb, table, out, lse, c["go"].float(), *c["geometry"], grads=grads,
                                  workspace=torch.empty(need - 4, dtype=torch.uint8, device='cuda'))
    torch.cuda.synchronize()
    assert all(bool((t == 7.25).all()) for t in grads)
    got = window_attention_backward(qkv, qb, table, out, lse, c["go"].float(), *c["geometry"], grads=grads,
                                    workspace=torch.empty(need, dtype=torch.uint8, device='cuda'))     # exactly enough
    for g, w in zip(got, c["grads"]):
        gate(g, w, "a workspace of exactly the size asked for")


def test_operators_refuse_what_is_not_their_input():
    c = case((2, 12), (1, 9, 10), 3)
    qkv, qb, table = f32(c["ops"])
    go, geo = c["go"].float(), c["geometry"]
    out, lse = window_attention_forward_lse(qkv, qb, table, *geo)
    crooked = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)                            # the right shape, not contiguous
    for fwd in (window_attention_forward_lse, window_attention_train):
        with pytest.raises(TypeError):
            fwd(qkv.cpu(), qb, table, *geo)
        with pytest.raises(TypeError):
            fwd(qkv.double(), qb, table, *geo)
        with pytest.raises(ValueError):
            fwd(crooked(qkv), qb, table, *geo)
        with pytest.raises(ValueError):
            fwd(qkv, qb[:-1], table, *geo)
        with pytest.raises(ValueError):
            fwd(qkv, qb, table[:-1], *geo)
    with pytest.raises(TypeError):
        window_attention_backward(qkv, qb, table, out, lse, go.cpu(), *geo)
    with pytest.raises(TypeError):
        window_attention_backward(qkv, qb, table, out.double(), lse, go, *geo)
    with pytest.raises(ValueError):
        window_attention_backward(qkv, qb, table, out, lse, crooked(go), *geo)
    with pytest.raises(ValueError):
        window_attention_backward(qkv, qb, table, out, lse[:, :-1], go, *geo)
    with pytest.raises(ValueError):
        window_attention_backward(qkv, qb, table, out, lse, go, *geo, grads=(torch.empty_like(qkv)[:, :-1], None, None))


def test_autograd_function_gives_the_three_gradients_and_takes_any_grad_out():
    c = case((3, 32), (1, 15, 20), 3)
    leaves = [t.requires_grad_() for t in f32(c["ops"])]
    y = window_attention_train(*leaves, *c["geometry"])
    assert y.requires_grad and torch.equal(y.detach(), window_attention_forward_lse(*f32(c["ops"]), *c["geometry"])[0])
    go = c["go"].float().transpose(1, 2).contiguous().transpose(1, 2)                              # not contiguous: the Function makes it so
    got = torch.autograd.grad(y, leaves, grad_outputs=go)
    for g, w in zip(got, fused_gradients(c)):
        assert torch.equal(g, w)
    assert not window_attention_train(*f32(c["ops"]), *c["geometry"]).requires_grad


def test_backward_is_bitwise_reproducible_also_on_a_side_stream():
    c = case((3, 32), (2, 38, 51), 3)
    first, again = fused_gradients(c), fused_gradients(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = fused_gradients(c)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for a, b, s in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, s)


class _Spy:
    """`_lib.lib()` with the launches of the window-attention symbols counted"""

    def __init__(self, real):
        self._real, self.launches = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("orp_window_attention") or name.endswith("_bytes"):
            return fn

        def counted(*a):
            self.launches[name] = self.launches.get(name, 0) + 1
            return fn(*a)
        return counted


@pytest.fixture
def spy(monkeypatch):
    s = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: s)
    return s


def stage_gradients(st, x, w, H, W):
    x = x.clone().requires_grad_()
    params = dict(st.named_parameters())
    grads = torch.autograd.grad((st(x, H, W)[0] * w).sum(), [x] + list(params.values()))
    return dict(zip(["input"] + list(params), grads))


def test_stage_gradients_against_the_float64_stock_twin_and_launch_counts(spy, monkeypatch):
    B, H, W = 1, 15, 20
    twin = make_stage(24, 2).train()                                                              # float64, CPU: the stock route
    g = torch.Generator().manual_seed(5)
    x = torch.randn((B, H * W, 24), generator=g, dtype=torch.float64)
    w = torch.randn((B, H * W, 24), generator=g, dtype=torch.float64)
    want = stage_gradients(twin, x, w, H, W)
    st = copy.deepcopy(twin).float().cuda().train()
    st._masks.clear()                                                                             # (the copy took the twin's CPU mask along)
    xs, ws = x.float().cuda(), w.float().cuda()
    fwd, bwd, inf = "orp_window_attention_train", "orp_window_attention_backward", "orp_window_attention"
    monkeypatch.setattr(switches, "SWIN_ATTN_TRAIN_FUSE", True)
    assert all(window_attention_train_ok(b.attn, xs) and b.fuses_attention_train(xs) and not b.fuses_attention(xs) for b in st.blocks)
    got = stage_gradients(st, xs, ws, H, W)
    assert spy.launches == {fwd: 2, bwd: 2} and len(st._masks) == 0                                # once per block; no shift mask evaluated
    assert sorted(got) == sorted(want)
    for name in want:
        gate(got[name].cpu(), want[name], ("fused route", name))
    # activation checkpointing recomputes the block's forward: two forwards per block, the same gradients
    spy.launches.clear()
    st.use_checkpoint = True
    again = stage_gradients(st, xs, ws, H, W)
    assert spy.launches == {fwd: 4, bwd: 2}
    for name in want:
        gate(again[name].cpu(), want[name], ("fused route, checkpointed", name))
    st.use_checkpoint = False
    # off by the switch, off per block
    spy.launches.clear()
    monkeypatch.setattr(switches, "SWIN_ATTN_TRAIN_FUSE", False)
    stock = stage_gradients(st, xs, ws, H, W)
    monkeypatch.setattr(switches, "SWIN_ATTN_TRAIN_FUSE", True)
    for b in st.blocks:
        b.fuse_window_attention_train = False
    stage_gradients(st, xs, ws, H, W)
    assert spy.launches == {}
    st.blocks[1].fuse_window_attention_train = None                                                 # per object: back to the module's switch
    stage_gradients(st, xs, ws, H, W)
    assert spy.launches == {fwd: 1, bwd: 1}
    for name in want:
        gate(stock[name].cpu(), want[name], ("stock route", name))
    # an eval model under enable_grad takes the training symbols too, never the inference kernel
    spy.launches.clear()
    monkeypatch.setattr(switches, "SWIN_ATTN_FUSE", True)
    st.eval()
    with torch.enable_grad():
        st(xs, H, W)
    assert inf not in spy.launches and spy.launches[fwd] == 1
    with torch.no_grad():
        st(xs, H, W)
    assert spy.launches[inf] == 2 and spy.launches[fwd] == 1
    assert sorted(k for k in st.state_dict() if 'fuse' in k) == []


def test_swin_tiny_dota_config_gradients_fused_and_stock_against_float64(reference_configs, monkeypatch):
    """Swin-T (DOTA config) through the neck at 128 x 160, loss = sum of the neck outputs . fixed random weights: for every parameter
    gradient err_fused <= max(4 * err_stock, 1e-6 * max(1, max |g64|)), both errors against a float64 copy of backbone + neck on the
    same input.  The unit is the stock fp32 path's own error; 4 covers two correct fp32 evaluations with different summation orders."""
    from orientedreppoints_amd.mmdet_models import Config, build_detector
    cfg = Config(copy.deepcopy(dict(reference_configs["orientedrepoints_swin_tiny_demo.py"]._cfg_dict)))
    cfg.model.pretrained = None
    torch.manual_seed(0)
    m = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).train()
    for mod in m.modules():
        if isinstance(mod, StochasticDepth):
            mod.p = 0.0                                                                            # the three evaluations must be the same function
    g = torch.Generator().manual_seed(1)
    x = torch.randn((1, 3, 128, 160), generator=g)
    shapes = [(256, 16, 20), (256, 8, 10), (256, 4, 5), (256, 2, 3), (256, 1, 2)]
    ws = [torch.randn((1,) + s, generator=g) for s in shapes]

    def gradients(backbone, neck, x, ws):
        params = dict([("backbone." + k, p) for k, p in backbone.named_parameters() if p.requires_grad]
                      + [("neck." + k, p) for k, p in neck.named_parameters() if p.requires_grad])
        feats = neck(backbone(x))
        assert [tuple(f.shape[1:]) for f in feats] == shapes
        grads = torch.autograd.grad(sum((f * w).sum() for f, w in zip(feats, ws)), list(params.values()), allow_unused=True)
        return {k: g for k, g in zip(params, grads) if g is not None}
    want = gradients(copy.deepcopy(m.backbone).double(), copy.deepcopy(m.neck).double(), x.double(), [w.double() for w in ws])
    m.cuda()
    xs, wss = x.cuda(), [w.cuda() for w in ws]
    got = {}
    for on in (True, False):
        monkeypatch.setattr(switches, "SWIN_ATTN_TRAIN_FUSE", on)
        got[on] = gradients(m.backbone, m.neck, xs, wss)
    assert sorted(got[True]) == sorted(want) == sorted(got[False]) and sum('attn.relative_position_bias_table' in k for k in want) == 12
    worst = (0.0, None)
    for name, w64 in want.items():
        top = max(1.0, float(w64.abs().max()))
        ef, es = (float((got[on][name].double().cpu() - w64).abs().max()) for on in (True, False))
        worst = max(worst, (ef / es if es > 0 else 0.0, name))
        assert ef <= max(4 * es, 1e-6 * top), (name, ef, es, top)
    print("Swin-T through the neck, parameter gradients: largest err_fused / err_stock %.3g (%s)" % worst)
