"""GPU: Swin's (shifted-)window attention on fp16 / bf16 operands -- `orp_window_attention_h` and `orp_window_attention_backward_h`
(csrc/orp_window_attn.hip) -- and the route SwinBlock.forward takes through them under autocast.

The accuracy argument has two parts.
  * Bit for bit: the 16-bit kernels are the fp32 kernels' arithmetic between a widening load and one rounded store.  So on fp32 copies
    of the same 16-bit operands, with the bias rounded to the operand type, the fp32 operators (held to float64 at 2e-5 by
    tests/test_gpu_window_attention.py and tests/test_gpu_window_attention_grad.py) give the same lse, grad_qkv_bias and
    grad_bias_table, and `out` / `grad_qkv` that round to what the 16-bit kernels stored.  `torch.equal`, no tolerance.
  * Against float64 through the autograd Function, the unit is the STOCK autocast route's own error on the same operands: for every
    gradient err_fused <= 4 * err_stock, both as fractions of max(1, max |g64|); 4 is what round 20 allowed two correct evaluations
    of different summation orders.  g64: torch.autograd.grad through `window_attention_reference` in float64 on the widened operands
    and the rounded bias (tests/test_window_attention_half_cpu.py).  The one deliberate difference from exact autograd is
    D_i = grad_out_i . out_i formed from the 16-bit `out`, as the stock 16-bit attention does too.  At operator level the stock
    route is the stock block's own sequence of calls on the same 16-bit q / k / v (`stock_path` of tests/test_gpu_window_attention.py
    under autocast: the block itself takes tokens, not q / k / v); the stage and the Swin-T model are compared as they are."""
import copy
import functools

import pytest
import torch

from orientedreppoints_amd import _lib, switches
from orientedreppoints_amd.mmdet_models.swin import StochasticDepth
from orientedreppoints_amd.mmdet_ops import (window_attention_backward, window_attention_backward_half, window_attention_forward_lse,
                                             window_attention_forward_lse_half, window_attention_half, window_attention_half_ok,
                                             window_attention_ok, window_attention_reference, window_attention_train_half,
                                             window_attention_train_half_ok, window_attention_train_ok)
from test_gpu_window_attention import stock_path
from test_window_attention_cpu import make_stage

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
MAPS = [(2, 14, 14), (1, 15, 20), (1, 5, 9)]                         # whole windows + batch 2; padded on both axes; smaller than a window
HEADS_OF = {4: 5, 8: 1, 12: 3, 16: 2, 20: 4, 24: 2, 28: 3, 32: 1}    # every head dim once, with its own number of heads
CASES = ([(h, m, s, True) for h in [(2, 12), (3, 32)] for m in MAPS for s in (0, 3)]
         + [((HEADS_OF[hd], hd), (1, 15, 20), 3, True) for hd in range(4, 33, 4)]
         + [((3, 32), (1, 15, 20), 1, True), ((2, 12), (1, 15, 20), 6, True)]
         # 30 windows per head: more than the reduction's sixteen slices and no multiple of them
         + [((2, 12), (1, 30, 40), 3, True)]
         + [((3, 32), (1, 15, 20), 3, False)])                        # no qkv bias: a padded token's q / k / v are zero
case_params = pytest.mark.parametrize("heads_hd,shape,shift,bias", CASES)
dtype_params = pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])


@functools.lru_cache(maxsize=None)
def case(heads_hd, shape, shift, bias, dt):
    """16-bit qkv and grad_out, fp32 bias and table; q, k ~ 1.4 N(0, 1) so that the scores (scale * q . k ~ 2 N(0, 1) plus the table)
    reach about +-8; the forward and the three gradients of the float64 reference on the widened operands and the rounded bias.
    Computed once per case and shared; nothing changes it."""
    (heads, hd), (B, H, W) = heads_hd, shape
    g = torch.Generator().manual_seed(1000 * heads + 10 * H + shift)
    qkv = (1.4 * torch.randn((B, H * W, 3 * heads * hd), generator=g)).cuda().to(dt)
    qb = torch.randn((3 * heads * hd,), generator=g).cuda() if bias else None
    table = (0.5 * torch.randn((169, heads), generator=g)).cuda()
    go = torch.randn((B, H * W, heads * hd), generator=g).cuda().to(dt)
    geometry = (H, W, heads, 7, shift, hd ** -0.5)
    leaves = [t.requires_grad_() for t in (qkv.double(), None if qb is None else qb.to(dt).double(), table.double()) if t is not None]
    wide = leaves if bias else [leaves[0], None, leaves[1]]
    out, lse = window_attention_reference(*wide, *geometry, with_lse=True)
    grads = list(torch.autograd.grad((out * go.double()).sum(), leaves))
    if not bias:
        grads.insert(1, None)
    return dict(ops=(qkv, qb, table), go=go, out=out.detach(), lse=lse.detach(), grads=grads, geometry=geometry, dt=dt)


def widened(c):
    """the operands as the fp32 operators take them: the 16-bit values as fp32, the bias rounded to the operand type"""
    qkv, qb, table = c["ops"]
    return qkv.float(), None if qb is None else qb.to(c["dt"]).float(), table


def rel(got, want64):
    return float((got.double() - want64).abs().max()) / max(1.0, float(want64.abs().max()))


@dtype_params
@case_params
def test_forward_is_the_fp32_kernel_rounded_once(heads_hd, shape, shift, bias, dt):
    c = case(heads_hd, shape, shift, bias, dt)
    out, lse = window_attention_forward_lse_half(*c["ops"], *c["geometry"])
    out32, lse32 = window_attention_forward_lse(*widened(c), *c["geometry"])
    assert out.dtype == dt and lse.dtype == torch.float32 and out.shape == out32.shape
    assert torch.equal(out, out32.to(dt))
    assert torch.equal(lse, lse32)
    assert torch.equal(window_attention_half(*c["ops"], *c["geometry"]), out)


@dtype_params
@case_params
def test_backward_is_the_fp32_backward_rounded_once(heads_hd, shape, shift, bias, dt):
    c = case(heads_hd, shape, shift, bias, dt)
    out, lse = window_attention_forward_lse_half(*c["ops"], *c["geometry"])
    gq, gb, gt = window_attention_backward_half(*c["ops"], out, lse, c["go"], *c["geometry"])
    wq, wb, wt = window_attention_backward(*widened(c), out.float(), lse, c["go"].float(), *c["geometry"])
    assert gq.dtype == dt and gt.dtype == torch.float32
    assert torch.equal(gq, wq.to(dt))
    assert torch.equal(gt, wt)
    if bias:
        assert gb.dtype == torch.float32 and torch.equal(gb, wb)
        C = heads_hd[0] * heads_hd[1]
        assert bool((gb[:C] == 0).all())                               # a padded query has no output: the q third is exactly zero
    else:
        assert gb is None and wb is None


def stock_gradients(c):
    """autograd through the stock block's calls on the same 16-bit q / k / v under autocast: the bias and the table are fp32 parameters
    cast to the operand type (the 16-bit linear layer's bias; `bias.to(q.dtype)` in WindowAttention.forward), the attention is 16-bit"""
    qkv, qb, table = c["ops"]
    H, W, heads, _, shift, scale = c["geometry"]
    leaves = [t.detach().clone().requires_grad_() for t in (qkv, qb, table) if t is not None]
    with torch.autocast('cuda', dtype=c["dt"]):
        cast = [t.to(c["dt"]) for t in leaves]
        y = stock_path(cast[0], cast[1] if qb is not None else None, cast[-1], H, W, heads, shift, scale)
    grads = list(torch.autograd.grad((y.float() * c["go"].float()).sum(), leaves, allow_unused=True))
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]          # (no padded token: the bias is not read)
    if qb is None:
        grads.insert(1, None)
    return grads


@dtype_params
@case_params
def test_function_gradients_against_float64_in_units_of_the_stock_autocast_route(heads_hd, shape, shift, bias, dt):
    c = case(heads_hd, shape, shift, bias, dt)
    leaves = [t.detach().clone().requires_grad_() for t in c["ops"] if t is not None]
    args = leaves if bias else [leaves[0], None, leaves[1]]
    y = window_attention_train_half(*args, *c["geometry"])
    assert y.requires_grad and y.dtype == dt
    got = list(torch.autograd.grad(y, leaves, grad_outputs=c["go"]))
    if not bias:
        got.insert(1, None)
    stock = stock_gradients(c)
    names = ("grad_qkv", "grad_qkv_bias", "grad_bias_table")
    errs = [(n, rel(g, w), rel(s, w)) for n, g, s, w in zip(names, got, stock, c["grads"]) if w is not None]
    print("window_attention_train_half %s heads %d head_dim %d map %s shift %d (fused / stock, of max(1, max |g64|)): %s"
          % ((str(dt).replace("torch.", ""),) + heads_hd + (shape, shift, "  ".join("%s %.3g / %.3g" % e for e in errs))))
    assert got[0].dtype == dt and got[2].dtype == torch.float32 and (got[1] is None or got[1].dtype == torch.float32)
    for name, ef, es in errs:
        assert ef <= 4 * es, (name, heads_hd, shape, shift, ef, es)


@dtype_params
@pytest.mark.parametrize("heads_hd,shape,shift", [((3, 32), (1, 15, 20), 3), ((2, 12), (2, 14, 14), 0), ((2, 12), (1, 30, 40), 3)])
def test_every_element_is_written(heads_hd, shape, shift, dt):
    c = case(heads_hd, shape, shift, True, dt)
    qkv, qb, table = c["ops"]
    nan = float('nan')
    first = window_attention_forward_lse_half(qkv, qb, table, *c["geometry"])
    out, lse = window_attention_forward_lse_half(qkv, qb, table, *c["geometry"], out=torch.full_like(first[0], nan), lse=torch.full_like(first[1], nan))
    only = window_attention_half(qkv, qb, table, *c["geometry"], out=torch.full_like(first[0], nan))
    grads = tuple(torch.full_like(t, nan) for t in (qkv, qb, table))
    got = window_attention_backward_half(qkv, qb, table, out, lse, c["go"], *c["geometry"], grads=grads)
    assert all(a is b for a, b in zip(got, grads))
    want = first + window_attention_backward_half(qkv, qb, table, first[0], first[1], c["go"], *c["geometry"])
    for name, g, w in zip(("out", "lse", "grad_qkv", "grad_qkv_bias", "grad_bias_table"), (out, lse) + got, want):
        assert bool(torch.isfinite(g).all()) and torch.equal(g, w), name
    assert torch.equal(only, first[0])


def test_refused_arguments_leave_the_outputs_untouched():
    dt, other = torch.float16, torch.bfloat16
    c = case((2, 12), (1, 15, 20), 3, True, dt)
    qkv, qb, table = c["ops"]
    geo, go = c["geometry"], c["go"]
    H, W, heads = geo[:3]
    out, lse = window_attention_forward_lse_half(qkv, qb, table, *geo)
    fill = 7.25
    o, l = torch.full_like(out, fill), torch.full_like(lse, fill)
    grads = tuple(torch.full_like(t, fill) for t in (qkv, qb, table))
    need = _lib.lib().orp_window_attention_backward_workspace_bytes(1, H, W, heads, 12, 7)
    assert need == 3 * 3 * heads * (169 + 2 * 12) * 4
    big = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    # the operator's own rules: a dtype mix, an fp32 qkv, a 16-bit table or bias, an fp32 grad_out
    for bad in (lambda: window_attention_forward_lse_half(qkv, qb, table, *geo, out=o.to(other), lse=l),
                lambda: window_attention_forward_lse_half(qkv.float(), qb, table, *geo, out=o, lse=l),
                lambda: window_attention_forward_lse_half(qkv, qb, table.to(dt), *geo, out=o, lse=l),
                lambda: window_attention_forward_lse_half(qkv, qb.to(dt), table, *geo, out=o, lse=l),
                lambda: window_attention_forward_lse_half(qkv, qb, table, *geo, out=o, lse=l.to(dt)),
                lambda: window_attention_half(qkv.float(), qb, table, *geo, out=o),
                lambda: window_attention_train_half(qkv.float(), qb, table, *geo),
                lambda: window_attention_backward_half(qkv, qb, table, out, lse, go.to(other), *geo, grads=grads),
                lambda: window_attention_backward_half(qkv, qb, table, out, lse, go.float(), *geo, grads=grads),
                lambda: window_attention_backward_half(qkv.float(), qb, table, out, lse, go, *geo, grads=grads),
                lambda: window_attention_backward_half(qkv, qb, table.to(dt), out, lse, go, *geo, grads=grads),
                lambda: window_attention_backward_half(qkv, qb, table, out.to(other), lse, go, *geo, grads=grads),
                lambda: window_attention_backward_half(qkv, qb, table, out, lse, go, *geo, grads=(grads[0].float(), grads[1], grads[2])),
                lambda: window_attention_backward_half(qkv, qb, table, out, lse, go, *geo, grads=(grads[0], grads[1].to(dt), grads[2]))):
        with pytest.raises(TypeError):
            bad()
    # the library's: a workspace one float short, window 8, head dim 6, a shift of 7, a tensor misaligned by 2 bytes
    with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
        window_attention_backward_half(qkv, qb, table, out, lse, go, *geo, grads=grads, workspace=torch.empty(need - 4, dtype=torch.uint8, device='cuda'))
    table8 = torch.randn(225, heads, device='cuda')
    with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
        window_attention_forward_lse_half(qkv, qb, table8, H, W, heads, 8, 0, geo[5], out=o, lse=l)
    with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
        window_attention_backward_half(qkv, qb, table8, out, lse, go, H, W, heads, 8, 0, geo[5], grads=(grads[0], grads[1], torch.full_like(table8, fill)), workspace=big)
    table4, l4 = torch.randn(169, 4, device='cuda'), torch.full((1, H * W, 4), fill, device='cuda')   # 24 channels as 4 heads of 6
    with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
        window_attention_forward_lse_half(qkv, qb, table4, H, W, 4, 7, 3, geo[5], out=o, lse=l4)
    with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
        window_attention_backward_half(qkv, qb, table4, out, torch.zeros(1, H * W, 4, device='cuda'), go, H, W, 4, 7, 3, geo[5],
                                       grads=(grads[0], grads[1], torch.full_like(table4, fill)), workspace=big)
    assert bool((l4 == fill).all())
    with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
        window_attention_forward_lse_half(qkv, qb, table, H, W, heads, 7, 7, geo[5], out=o, lse=l)

    def shifted(t):                                                    # the same values one element (2 bytes) further: contiguous, misaligned
        buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
        view = buf[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 8 == 2
        return view
    for bad in (lambda: window_attention_forward_lse_half(shifted(qkv), qb, table, *geo, out=o, lse=l),
                lambda: window_attention_forward_lse_half(qkv, qb, table, *geo, out=shifted(o), lse=l),
                lambda: window_attention_backward_half(shifted(qkv), qb, table, out, lse, go, *geo, grads=grads),
                lambda: window_attention_backward_half(qkv, qb, table, shifted(out), lse, go, *geo, grads=grads),
                lambda: window_attention_backward_half(qkv, qb, table, out, lse, shifted(go), *geo, grads=grads)):
        with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
            bad()
    gq_off = shifted(grads[0])
    with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
        window_attention_backward_half(qkv, qb, table, out, lse, go, *geo, grads=(gq_off, grads[1], grads[2]))
    torch.cuda.synchronize()
    assert all(bool((t == fill).all()) for t in (o, l, gq_off) + grads)
    # ... and a workspace of exactly the size asked for is enough
    got = window_attention_backward_half(qkv, qb, table, out, lse, go, *geo, grads=grads, workspace=torch.empty(need, dtype=torch.uint8, device='cuda'))
    for g, w in zip(got, window_attention_backward_half(qkv, qb, table, out, lse, go, *geo)):
        assert torch.equal(g, w)


@dtype_params
def test_calls_are_bitwise_reproducible_also_on_a_side_stream(dt):
    c = case((2, 12), (1, 30, 40), 3, True, dt)

    def both():
        out, lse = window_attention_forward_lse_half(*c["ops"], *c["geometry"])
        return (out, lse) + window_attention_backward_half(*c["ops"], out, lse, c["go"], *c["geometry"])
    first, again = both(), both()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = both()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for a, b, s in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, s)


@dtype_params
def test_function_takes_a_grad_out_that_is_not_contiguous(dt):
    c = case((3, 32), (1, 15, 20), 3, True, dt)
    leaves = [t.detach().clone().requires_grad_() for t in c["ops"]]
    y = window_attention_train_half(*leaves, *c["geometry"])
    out, lse = window_attention_forward_lse_half(*c["ops"], *c["geometry"])
    assert torch.equal(y.detach(), out)
    go = c["go"].transpose(1, 2).contiguous().transpose(1, 2)
    assert not go.is_contiguous()
    got = torch.autograd.grad(y, leaves, grad_outputs=go)
    for g, w in zip(got, window_attention_backward_half(*c["ops"], out, lse, c["go"], *c["geometry"])):
        assert torch.equal(g, w)
    assert not window_attention_train_half(*c["ops"], *c["geometry"]).requires_grad


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


def stage_run(st, x, w, H, W, dt):
    """the stage's output and the gradient of (output . w) with respect to the input, under autocast(dt) (dt None: as it is)"""
    x = x.clone().requires_grad_()
    if dt is None:
        y = st(x, H, W)[0]
    else:
        with torch.autocast('cuda', dtype=dt):
            y = st(x, H, W)[0]
    return y.detach(), torch.autograd.grad((y * w).sum(), x)[0]


@dtype_params
def test_stage_route_under_autocast_launch_counts_and_the_stock_stage(spy, monkeypatch, dt):
    B, H, W = 1, 15, 20
    twin = make_stage(24, 2).train()                                                              # float64, CPU: the stock route
    g = torch.Generator().manual_seed(5)
    x = torch.randn((B, H * W, 24), generator=g, dtype=torch.float64)
    w = torch.randn((B, H * W, 24), generator=g, dtype=torch.float64)
    want = stage_run(twin, x, w, H, W, None)
    st = copy.deepcopy(twin).float().cuda().train()
    st._masks.clear()                                                                             # (the copy took the twin's CPU mask along)
    xs, ws = x.float().cuda(), w.float().cuda()
    fwd, bwd = "orp_window_attention_h", "orp_window_attention_backward_h"
    for name in ("SWIN_ATTN_FUSE", "SWIN_ATTN_TRAIN_FUSE", "SWIN_ATTN_HALF_FUSE"):
        monkeypatch.setattr(switches, name, True)
    with torch.autocast('cuda', dtype=dt):
        for b in st.blocks:
            assert window_attention_train_half_ok(b.attn, xs) and not window_attention_half_ok(b.attn, xs)
            assert b.fused_attention(xs) is window_attention_train_half
            assert not window_attention_ok(b.attn, xs) and not window_attention_train_ok(b.attn, xs)
            with torch.no_grad():
                assert window_attention_half_ok(b.attn, xs) and not window_attention_train_half_ok(b.attn, xs)
                assert b.fused_attention(xs) is window_attention_half
                assert window_attention_half_ok(b.attn, xs.to(dt))          # 16-bit tokens of the autocast dtype: every stage after a PatchMerging
                other = torch.bfloat16 if dt == torch.float16 else torch.float16
                assert not window_attention_half_ok(b.attn, xs.to(other)) and not window_attention_half_ok(b.attn, xs.double())
                assert not window_attention_half_ok(b.attn, xs.cpu())
        with torch.autocast('cuda', dtype=dt, enabled=False):
            assert not window_attention_train_half_ok(st.blocks[0].attn, xs)
    assert not window_attention_train_half_ok(st.blocks[0].attn, xs)                                # no autocast: the fp32 route's
    assert not window_attention_train_half_ok(copy.deepcopy(st).to(dt).blocks[0].attn, xs.to(dt))   # model.half(): the stock route
    # gradients enabled: one forward and one backward per block, no shift mask, never an fp32 entry
    fused = stage_run(st, xs, ws, H, W, dt)
    assert spy.launches == {fwd: 2, bwd: 2} and len(st._masks) == 0
    # activation checkpointing recomputes the block's forward under the same autocast state: two forwards per block
    spy.launches.clear()
    st.use_checkpoint = True
    again = stage_run(st, xs, ws, H, W, dt)
    assert spy.launches == {fwd: 4, bwd: 2}
    assert torch.equal(again[0], fused[0])
    st.use_checkpoint = False
    # no gradients: the forward entry once per block (no lse kept)
    spy.launches.clear()
    with torch.no_grad(), torch.autocast('cuda', dtype=dt):
        y = st(xs, H, W)[0]
    assert spy.launches == {fwd: 2} and len(st._masks) == 0
    assert torch.equal(y, fused[0])                                                                # the same forward arithmetic
    # off by the switch, off per block
    spy.launches.clear()
    monkeypatch.setattr(switches, "SWIN_ATTN_HALF_FUSE", False)
    stock = stage_run(st, xs, ws, H, W, dt)
    with torch.no_grad(), torch.autocast('cuda', dtype=dt):
        st(xs, H, W)
    monkeypatch.setattr(switches, "SWIN_ATTN_HALF_FUSE", True)
    for b in st.blocks:
        b.fuse_window_attention_half = False
    stage_run(st, xs, ws, H, W, dt)
    assert spy.launches == {}
    st.blocks[1].fuse_window_attention_half = None                                                  # per object: back to the module's switch
    stage_run(st, xs, ws, H, W, dt)
    assert spy.launches == {fwd: 1, bwd: 1}
    # without autocast the same stage takes the fp32 entries, and only those
    spy.launches.clear()
    stage_run(st, xs, ws, H, W, None)
    assert spy.launches == {"orp_window_attention_train": 2, "orp_window_attention_backward": 2}
    # the fused stage agrees with the stock autocast stage within 4 x the stock stage's own distance to its float64 twin
    for name, f, s, w64 in zip(("output", "input gradient", "input gradient, checkpointed"), fused + again[1:], stock + stock[1:], want + want[1:]):
        d_stock, d_fused = float((s.double().cpu() - w64).abs().max()), float((f.double() - s.double()).abs().max())
        print("stage under %s autocast, %s: |fused - stock| %.3g, |stock - float64| %.3g, |fused - float64| %.3g"
              % (str(dt).replace("torch.", ""), name, d_fused, d_stock, float((f.double().cpu() - w64).abs().max())))
        assert d_stock > 0 and d_fused <= 4 * d_stock, (name, d_fused, d_stock)
    assert sorted(k for k in st.state_dict() if 'fuse' in k) == []


def test_swin_tiny_dota_config_gradients_under_fp16_autocast_fused_and_stock_against_float64(reference_configs, monkeypatch):
    """Swin-T (DOTA config) through the neck at 128 x 160 under fp16 autocast, loss = 1024 * sum of the neck outputs . fixed random
    weights (a GradScaler's constant scale), gradients divided by it: all finite, and for every parameter gradient
    err_fused <= 4 * err_stock, both errors against a float64 copy of backbone + neck on the same input."""
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
    # (weights ~ N(0, 1) / 64: with N(0, 1) the largest gradient, patch_embed.proj.weight's, is about 64, and 1024 times that leaves
    # fp16's range on either route -- a GradScaler would have lowered its scale)
    ws = [torch.randn((1,) + s, generator=g) / 64 for s in shapes]
    scale = 1024.0

    def gradients(backbone, neck, x, ws, dt):
        params = dict([("backbone." + k, p) for k, p in backbone.named_parameters() if p.requires_grad]
                      + [("neck." + k, p) for k, p in neck.named_parameters() if p.requires_grad])
        if dt is None:
            feats = neck(backbone(x))
        else:
            with torch.autocast('cuda', dtype=dt):
                feats = neck(backbone(x))
        assert [tuple(f.shape[1:]) for f in feats] == shapes
        loss = scale * sum((f.float() * w).sum() if dt is not None else (f * w).sum() for f, w in zip(feats, ws))
        grads = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
        return {k: g / scale for k, g in zip(params, grads) if g is not None}
    want = gradients(copy.deepcopy(m.backbone).double(), copy.deepcopy(m.neck).double(), x.double(), [w.double() for w in ws], None)
    m.cuda()
    xs, wss = x.cuda(), [w.cuda() for w in ws]
    launches = {}
    real = _lib.lib()
    got = {}
    for on in (True, False):
        monkeypatch.setattr(switches, "SWIN_ATTN_HALF_FUSE", on)
        s = _Spy(real)
        monkeypatch.setattr(_lib, "lib", lambda s=s: s)
        got[on] = gradients(m.backbone, m.neck, xs, wss, torch.float16)
        launches[on] = dict(s.launches)
    assert launches[True] == {"orp_window_attention_h": 12, "orp_window_attention_backward_h": 12} and launches[False] == {}
    assert sorted(got[True]) == sorted(want) == sorted(got[False]) and sum('attn.relative_position_bias_table' in k for k in want) == 12
    worst, failed = (0.0, None), []
    for name, w64 in want.items():
        assert bool(torch.isfinite(got[True][name]).all()) and bool(torch.isfinite(got[False][name]).all()), name
        assert got[True][name].dtype == torch.float32, name
        top = max(1.0, float(w64.abs().max()))
        ef, es = (float((got[on][name].double().cpu() - w64).abs().max()) / top for on in (True, False))
        worst = max(worst, (ef / es if es > 0 else (0.0 if ef == 0 else float('inf')), name))
        if ef > 4 * es:
            failed.append((name, ef, es))
    print("Swin-T through the neck under fp16 autocast, parameter gradients: largest err_fused / err_stock %.3g (%s)" % worst)
    assert not failed, failed
