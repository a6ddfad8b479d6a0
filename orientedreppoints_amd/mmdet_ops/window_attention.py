"""Swin's (shifted-)window attention as HIP kernels -- at inference one (`orp_window_attention`, include/orp_hip.h), in training a
forward that keeps the rows' log-sum-exp and a backward (`orp_window_attention_train`, `orp_window_attention_backward`): everything between
`attn.qkv` and `attn.proj` of a Swin block (mmdet/models/backbones/swin_transformer.py: SwinTransformerBlock.forward:199-250,
WindowAttention.forward:122-155, the mask of BasicLayer.forward:370-390).

The reformulation it rests on: `qkv` and `proj` are per-token linears, so both run on the un-padded, un-rolled [B, H * W, C] tokens;
the pad comes after norm1, so a padded token is a zero vector in front of `qkv` and its q / k / v are the `qkv` bias (zero without
one); pad, roll, window partition, relative-position bias, shift mask, window reverse, un-roll and crop are index arithmetic.
`window_attention_reference` states exactly that in plain torch (any dtype, any device) and is what the tests hold the kernel to.

Under fp16 / bf16 autocast `attn.qkv` yields 16-bit q / k / v: `window_attention_half`, `window_attention_train_half` and their
low-level calls (`orp_window_attention_h`, `orp_window_attention_backward_h`) take them as they are -- fp32 arithmetic in the fp32
kernels' order, a padded token's q / k / v = the bias rounded to the operand type.  The fp32 functions and predicates do not change.

All of them are one forward, one backward, one autograd function and one routing rule here, as they are one kernel each in
csrc/orp_window_attn.hip: the public functions differ in the operand dtype they insist on and in the C entry point that follows from it.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib

WINDOW = 7                                   # the kernel's window side
HEAD_DIMS = tuple(range(4, 33, 4))           # ... and head dims
HALF_DTYPES = {torch.float16: 1, torch.bfloat16: 2}          # the library's dtype codes (orp_dcn_forward_multi_h's convention)


def _shapes(qkv, qkv_bias, bias_table, H, W, heads, window):
    if qkv.dim() not in (3, 5) or H < 1 or W < 1 or heads < 1 or window < 1 or qkv.size(1) != H * W:
        raise ValueError("qkv must be [B, H * W, 3 * C] or [B, H * W, 3, heads, head_dim], got %s for H, W = %d, %d"
                         % (tuple(qkv.shape), H, W))
    c3 = qkv[0, 0].numel()
    if c3 % (3 * heads) or (qkv.dim() == 5 and tuple(qkv.shape[2:4]) != (3, heads)):
        raise ValueError("qkv %s does not hold q, k, v of %d heads" % (tuple(qkv.shape), heads))
    if qkv_bias is not None and tuple(qkv_bias.shape) != (c3,):
        raise ValueError("qkv_bias must be [%d], got %s" % (c3, tuple(qkv_bias.shape)))
    if tuple(bias_table.shape) != ((2 * window - 1) ** 2, heads):
        raise ValueError("bias_table must be [%d, %d], got %s" % ((2 * window - 1) ** 2, heads, tuple(bias_table.shape)))
    return qkv.size(0), c3 // 3, c3 // (3 * heads)


def _shaped(t, shape, name):
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be %s, got %s" % (name, list(shape), tuple(t.shape)))
    return t


def _check(qkv, half, operands, floats, optional):
    """The argument rule of every call.  `qkv` and the (name, tensor) pairs in `operands` are of the operand dtype -- float32 for the fp32
    calls, qkv's own float16 / bfloat16 for the 16-bit ones (half) --, those in `floats` float32; all contiguous CUDA tensors on qkv's
    device, None only for a name in `optional`.  Returns the operand dtype."""
    _lib.require_cuda(qkv, "qkv")
    if half and qkv.dtype not in HALF_DTYPES:
        raise TypeError("qkv must be a float16 or bfloat16 tensor, got %s" % qkv.dtype)
    dt = qkv.dtype if half else torch.float32
    for want, group in ((dt, (("qkv", qkv),) + tuple(operands)), (torch.float32, floats)):
        for name, t in group:
            if t is None and name in optional:
                continue
            _lib.require_cuda(t, name)
            if t.dtype != want or t.device != qkv.device:
                raise TypeError("%s must be a %s tensor on qkv's device" % (name, str(want).replace("torch.", "")))
            if not t.is_contiguous():
                raise ValueError("%s must be contiguous" % name)
    return dt


def _forward(half, keep_lse, qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale, out, lse):
    """every forward: the fp32 operands go to orp_window_attention (no lse) or orp_window_attention_train, the 16-bit ones to
    orp_window_attention_h"""
    dt = _check(qkv, half, (("out", out),), (("qkv_bias", qkv_bias), ("bias_table", bias_table), ("lse", lse)), ("qkv_bias", "out", "lse"))
    B, C, hd = _shapes(qkv, qkv_bias, bias_table, H, W, heads, window)
    out = torch.empty((B, H * W, C), dtype=dt, device=qkv.device) if out is None else _shaped(out, (B, H * W, C), "out")
    if keep_lse:
        lse = torch.empty((B, H * W, heads), dtype=torch.float32, device=qkv.device) if lse is None else _shaped(lse, (B, H * W, heads), "lse")
    elif lse is not None:
        raise ValueError("lse given with keep_lse=False")
    if half:
        name, last = "orp_window_attention_h", (_lib.ptr(lse), HALF_DTYPES[dt])
    else:
        name, last = ("orp_window_attention_train", (_lib.ptr(lse),)) if keep_lse else ("orp_window_attention", ())
    _lib.call(name, qkv.device, _lib.ptr(qkv.detach()), _lib.ptr(None if qkv_bias is None else qkv_bias.detach()),
              _lib.ptr(bias_table.detach()), B, H, W, heads, hd, window, shift, float(scale), _lib.ptr(out), *last, _lib.stream_of(qkv))
    return out, lse


def _backward(half, qkv, qkv_bias, bias_table, out, lse, grad_out, H, W, heads, window, shift, scale, grads, workspace):
    """both backwards: orp_window_attention_backward for fp32 operands, orp_window_attention_backward_h for 16-bit ones"""
    gq, gb, gt = (None, None, None) if grads is None else grads
    dt = _check(qkv, half, (("out", out), ("grad_out", grad_out), ("grad_qkv", gq)),
                (("qkv_bias", qkv_bias), ("bias_table", bias_table), ("lse", lse), ("grad_qkv_bias", gb), ("grad_bias_table", gt)),
                ("qkv_bias", "grad_qkv", "grad_qkv_bias", "grad_bias_table"))
    B, C, hd = _shapes(qkv, qkv_bias, bias_table, H, W, heads, window)
    _shaped(out, (B, H * W, C), "out"), _shaped(lse, (B, H * W, heads), "lse"), _shaped(grad_out, (B, H * W, C), "grad_out")
    if gb is not None and qkv_bias is None:
        raise ValueError("grad_qkv_bias without a qkv_bias")
    gq = torch.empty_like(qkv) if gq is None else _shaped(gq, qkv.shape, "grad_qkv")
    gt = torch.empty_like(bias_table) if gt is None else _shaped(gt, bias_table.shape, "grad_bias_table")
    if qkv_bias is not None:
        gb = torch.empty_like(qkv_bias) if gb is None else _shaped(gb, qkv_bias.shape, "grad_qkv_bias")
    name, last = ("orp_window_attention_backward_h", (HALF_DTYPES[dt],)) if half else ("orp_window_attention_backward", ())
    L = _lib.lib()
    if workspace is None:
        with torch.cuda.device(qkv.device):                # (workspace asks whether the current device's stream is capturing)
            workspace = _lib.workspace(qkv.device, L.orp_window_attention_backward_workspace_bytes(B, H, W, heads, hd, window))
    elif not (isinstance(workspace, torch.Tensor) and workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise TypeError("workspace must be a contiguous uint8 CUDA tensor")
    _lib.call(name, qkv.device, _lib.ptr(qkv.detach()), _lib.ptr(None if qkv_bias is None else qkv_bias.detach()),
              _lib.ptr(bias_table.detach()), _lib.ptr(out.detach()), _lib.ptr(lse), _lib.ptr(grad_out), B, H, W, heads, hd, window, shift,
              float(scale), _lib.ptr(gq), _lib.ptr(gb), _lib.ptr(gt), _lib.ptr(workspace), workspace.numel(), *last, _lib.stream_of(qkv))
    return gq, gb, gt


def window_attention(qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale, out=None):
    """qkv [B, H * W, 3 * C] (= [B, H * W, 3, heads, head_dim]) fp32 CUDA: `attn.qkv` of the un-padded, un-rolled tokens; qkv_bias [3 * C]
    or None; bias_table [(2 * window - 1)^2, heads].  Returns [B, H * W, C]: every token's attention result in its own place, before
    `proj`.  Shapes the kernel does not take (window != 7, shift outside [0, 7), head_dim not a multiple of 4 up to 32) raise through
    `_lib.check`; nothing is written then."""
    return _forward(False, False, qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale, out, None)[0]


def window_attention_forward_lse(qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale, out=None, lse=None):
    """`window_attention` for training: returns (out, lse) -- `out` bit for bit `window_attention`'s, `lse` [B, H * W, heads] the
    log-sum-exp of every token's row of scores, which is all the backward needs besides the operands.  Not differentiable by itself
    (`window_attention_train` is); the same argument rules, nothing written where they raise."""
    return _forward(False, True, qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale, out, lse)


def window_attention_backward(qkv, qkv_bias, bias_table, out, lse, grad_out, H, W, heads, window, shift, scale, grads=None,
                              workspace=None):
    """The gradients of `window_attention` (include/orp_hip.h: orp_window_attention_backward) from the operands, the forward's `out` and
    `lse` and grad_out [B, H * W, C]: (grad_qkv like qkv, grad_qkv_bias [3 * C] -- the padded tokens' share; None without a qkv_bias --,
    grad_bias_table [169, heads]).  Every element is written, in one fixed summation order.  `grads`: the three as preallocated tensors
    (None in the bias's place without one); `workspace`: a uint8 CUDA tensor in place of the cached one."""
    return _backward(False, qkv, qkv_bias, bias_table, out, lse, grad_out, H, W, heads, window, shift, scale, grads, workspace)


def window_attention_forward_lse_half(qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale, out=None, lse=None, keep_lse=True):
    """`window_attention_forward_lse` on 16-bit operands (include/orp_hip.h: orp_window_attention_h): qkv and `out` fp16 or bf16 and
    of one dtype, qkv_bias / bias_table / `lse` float32.  All arithmetic is fp32 in the fp32 kernel's order; a padded token's q / k / v
    are the bias rounded to qkv's dtype; `out` is rounded once as it is stored, `lse` is the fp32 kernel's for the widened operands.
    Returns (out, lse); keep_lse=False keeps none (lse is None).  A dtype mix raises TypeError, nothing is written where the rules raise."""
    return _forward(True, keep_lse, qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale, out, lse)


def window_attention_half(qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale, out=None):
    """`window_attention` on 16-bit operands, forward only: qkv fp16 or bf16 CUDA, qkv_bias / bias_table float32 (the parameters stay
    fp32 under autocast).  Returns [B, H * W, C] of qkv's dtype."""
    return _forward(True, False, qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale, out, None)[0]


def window_attention_backward_half(qkv, qkv_bias, bias_table, out, lse, grad_out, H, W, heads, window, shift, scale, grads=None,
                                   workspace=None):
    """`window_attention_backward` on 16-bit operands (orp_window_attention_backward_h): qkv, out, grad_out and grad_qkv of one 16-bit
    dtype; qkv_bias, bias_table, lse, grad_qkv_bias and grad_bias_table float32.  D_i is formed from the 16-bit `out`; everything else is
    the fp32 backward's arithmetic on the widened operands, grad_qkv rounded once as it is stored.  The workspace is the fp32 call's."""
    return _backward(True, qkv, qkv_bias, bias_table, out, lse, grad_out, H, W, heads, window, shift, scale, grads, workspace)


class _WindowAttentionTrain(torch.autograd.Function):
    """saves the operands and `out` (fp32, or 16-bit for `half`) and the fp32 `lse` -- nothing of size 49 x 49"""

    @staticmethod
    def forward(ctx, half, qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale):
        out, lse = _forward(half, True, qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale, None, None)
        ctx.save_for_backward(qkv, qkv_bias, bias_table, out, lse)
        ctx.half, ctx.geometry = half, (H, W, heads, window, shift, scale)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        qkv, qkv_bias, bias_table, out, lse = ctx.saved_tensors
        if ctx.half:
            grad_out = grad_out.to(out.dtype)
        gq, gb, gt = _backward(ctx.half, qkv, qkv_bias, bias_table, out, lse, grad_out.contiguous(), *ctx.geometry, None, None)
        return (None, gq, gb, gt) + (None,) * 6


def window_attention_train(qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale):
    """`window_attention` with a backward: gradients for qkv, qkv_bias (the padded tokens' share: their k / v are the bias) and
    bias_table, all three always computed.  Once differentiable."""
    return _WindowAttentionTrain.apply(False, qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale)


def window_attention_train_half(qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale):
    """`window_attention_half` with a backward: a 16-bit gradient for qkv, fp32 gradients for qkv_bias (the padded tokens' share) and
    bias_table, all three always computed.  Once differentiable."""
    return _WindowAttentionTrain.apply(True, qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale)


def _route_ok(attn_module, x, grad, half):
    """the routing rule behind the four predicates: gradients enabled or not (grad); autocast off and fp32 tokens, or (half) CUDA
    autocast on with a 16-bit dtype and tokens that are fp32 or of that dtype"""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or torch.is_grad_enabled() != grad:
        return False
    if half:
        if not torch.is_autocast_enabled() or torch.get_autocast_dtype('cuda') not in HALF_DTYPES:
            return False
        if x.dtype not in (torch.float32, torch.get_autocast_dtype('cuda')):
            return False
    elif x.dtype != torch.float32 or torch.is_autocast_enabled():
        return False
    a = attn_module
    if a.ws != WINDOW or a.dim % a.num_heads or (a.dim // a.num_heads) not in HEAD_DIMS:
        return False
    if a.training and a.attn_drop.p > 0.0:
        return False
    params = [a.qkv.weight, a.proj.weight, a.relative_position_bias_table] + ([] if a.qkv.bias is None else [a.qkv.bias])
    return all(p.dtype == torch.float32 and p.device == x.device for p in params)


def window_attention_ok(attn_module, x):
    """The routing rule of the fused Swin block: fp32 CUDA tokens and parameters, window 7, a head dim the kernel has, attention
    dropout inactive, gradients (and autocast) disabled."""
    return _route_ok(attn_module, x, grad=False, half=False)


def window_attention_train_ok(attn_module, x):
    """The routing rule of the fused Swin block in training: `window_attention_ok`'s with gradients ENABLED -- fp32 CUDA tokens and
    parameters, window 7, a head dim the kernels have, attention dropout inactive, no autocast."""
    return _route_ok(attn_module, x, grad=True, half=False)


def window_attention_half_ok(attn_module, x):
    """The routing rule of the fused Swin block at inference under autocast: CUDA tokens, fp32 parameters on their device, CUDA
    autocast ENABLED with dtype fp16 or bf16 (so `attn.qkv` yields 16-bit q / k / v and `attn.proj` takes a 16-bit operand), window 7, a
    head dim the kernels have, attention dropout inactive, gradients disabled.  The tokens are fp32 or of the autocast dtype: the
    first stage's are fp32, but PatchMerging's linear layer hands every later stage 16-bit tokens (norm1 widens them again).  A
    `model.half()` model (16-bit parameters, no autocast) is not detected and keeps the stock route."""
    return _route_ok(attn_module, x, grad=False, half=True)


def window_attention_train_half_ok(attn_module, x):
    """`window_attention_half_ok` with gradients ENABLED: the routing rule of `window_attention_train_half`."""
    return _route_ok(attn_module, x, grad=True, half=True)


def _bands(n, window, shift, device):
    """band of every rolled coordinate of an axis of padded length n: 0 below n - window, 1 below n - shift, else 2"""
    r = torch.arange(n, device=device)
    return (r >= n - window).long() + (r >= n - shift).long()


def window_attention_reference(qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale, with_lse=False):
    """`window_attention` in plain torch, written from the semantics in include/orp_hip.h: any dtype, any device, any window;
    differentiable, which defines the backward.  with_lse: returns (out, lse [B, H * W, heads]) as `window_attention_forward_lse`."""
    B, C, hd = _shapes(qkv, qkv_bias, bias_table, H, W, heads, window)
    ws, N, dev = window, window * window, qkv.device
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    nwy, nwx = Hp // ws, Wp // ws
    # the padded map: a padded token's q / k / v are the bias
    full = qkv.new_zeros((B, Hp, Wp, 3 * C))
    if qkv_bias is not None:
        full = full + qkv_bias.to(qkv.dtype)
    full[:, :H, :W] = qkv.reshape(B, H, W, 3 * C)
    # rolled coordinate r reads the padded map at (r + shift) mod padded size
    sy, sx = (torch.arange(Hp, device=dev) + shift) % Hp, (torch.arange(Wp, device=dev) + shift) % Wp
    rolled = full[:, sy][:, :, sx]
    q, k, v = rolled.view(B, nwy, ws, nwx, ws, 3, heads, hd).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B, nwy, nwx, heads, N, hd)
    score = scale * (q @ k.transpose(-1, -2))                                 # [B, nwy, nwx, heads, N(query), N(key)]
    pi, pj = torch.arange(N, device=dev) // ws, torch.arange(N, device=dev) % ws
    rel = (pi[:, None] - pi[None, :] + ws - 1) * (2 * ws - 1) + (pj[:, None] - pj[None, :] + ws - 1)
    score = score + bias_table.to(qkv.dtype)[rel].permute(2, 0, 1)             # [heads, N, N]
    if shift > 0:
        band = 3 * _bands(Hp, ws, shift, dev)[:, None] + _bands(Wp, ws, shift, dev)[None, :]          # on rolled coordinates
        band = band.view(nwy, ws, nwx, ws).permute(0, 2, 1, 3).reshape(nwy, nwx, 1, N)
        score = score + (band[..., :, None] != band[..., None, :]).to(qkv.dtype) * -100.0
    top = score.amax(-1, keepdim=True)
    p = torch.exp(score - top)
    o = (p / p.sum(-1, keepdim=True)) @ v                                      # [B, nwy, nwx, heads, N, hd]

    def to_tokens(t):                                                          # [B, nwy, nwx, heads, N, last] -> [B, H * W, heads * last]
        t = t.view(B, nwy, nwx, heads, ws, ws, -1).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, Hp, Wp, -1)
        back = torch.empty_like(t)
        back[:, sy[:, None], sx[None, :]] = t                                  # un-roll
        return back[:, :H, :W].reshape(B, H * W, -1)
    if with_lse:
        return to_tokens(o), to_tokens(top + torch.log(p.sum(-1, keepdim=True)))
    return to_tokens(o)
