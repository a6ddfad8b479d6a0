"""Swin's (shifted-)window attention at inference as one HIP kernel (`orp_window_attention`, include/orp_hip.h): everything between
`attn.qkv` and `attn.proj` of a Swin block (mmdet/models/backbones/swin_transformer.py: SwinTransformerBlock.forward:199-250,
WindowAttention.forward:122-155, the mask of BasicLayer.forward:370-390).

The reformulation it rests on: `qkv` and `proj` are per-token linears, so both run on the un-padded, un-rolled [B, H * W, C] tokens;
the pad comes after norm1, so a padded token is a zero vector in front of `qkv` and its q / k / v are the `qkv` bias (zero without
one); pad, roll, window partition, relative-position bias, shift mask, window reverse, un-roll and crop are index arithmetic.
`window_attention_reference` states exactly that in plain torch (any dtype, any device) and is what the tests hold the kernel to.
"""
import torch

from .. import _lib

WINDOW = 7                                   # the kernel's window side
HEAD_DIMS = tuple(range(4, 33, 4))           # ... and head dims


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


def window_attention(qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale, out=None):
    """qkv [B, H * W, 3 * C] (= [B, H * W, 3, heads, head_dim]) fp32 CUDA: `attn.qkv` of the un-padded, un-rolled tokens; qkv_bias [3 * C]
    or None; bias_table [(2 * window - 1)^2, heads].  Returns [B, H * W, C]: every token's attention result in its own place, before
    `proj`.  Shapes the kernel does not take (window != 7, shift outside [0, 7), head_dim not a multiple of 4 up to 32) raise through
    `_lib.check`; nothing is written then."""
    for name, t in (("qkv", qkv), ("qkv_bias", qkv_bias), ("bias_table", bias_table), ("out", out)):
        if t is None and name in ("qkv_bias", "out"):
            continue
        _lib.require_cuda(t, name)
        if t.dtype != torch.float32 or t.device != qkv.device:
            raise TypeError("%s must be a float32 tensor on qkv's device" % name)
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    B, C, hd = _shapes(qkv, qkv_bias, bias_table, H, W, heads, window)
    if out is None:
        out = torch.empty((B, H * W, C), dtype=torch.float32, device=qkv.device)
    elif tuple(out.shape) != (B, H * W, C):
        raise ValueError("out must be [%d, %d, %d], got %s" % (B, H * W, C, tuple(out.shape)))
    with torch.cuda.device(qkv.device):
        rc = _lib.lib().orp_window_attention(_lib.ptr(qkv.detach()), _lib.ptr(None if qkv_bias is None else qkv_bias.detach()),
                                             _lib.ptr(bias_table.detach()), B, H, W, heads, hd, window, shift, float(scale),
                                             _lib.ptr(out), _lib.stream_of(qkv))
    _lib.check(rc, "orp_window_attention")
    return out


def window_attention_ok(attn_module, x):
    """The routing rule of the fused Swin block: fp32 CUDA tokens and parameters, window 7, a head dim the kernel has, attention
    dropout inactive, gradients (and autocast) disabled."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
        return False
    if torch.is_grad_enabled() or torch.is_autocast_enabled():
        return False
    a = attn_module
    if a.ws != WINDOW or a.dim % a.num_heads or (a.dim // a.num_heads) not in HEAD_DIMS:
        return False
    if a.training and a.attn_drop.p > 0.0:
        return False
    params = [a.qkv.weight, a.proj.weight, a.relative_position_bias_table] + ([] if a.qkv.bias is None else [a.qkv.bias])
    return all(p.dtype == torch.float32 and p.device == x.device for p in params)


def _bands(n, window, shift, device):
    """band of every rolled coordinate of an axis of padded length n: 0 below n - window, 1 below n - shift, else 2"""
    r = torch.arange(n, device=device)
    return (r >= n - window).long() + (r >= n - shift).long()


def window_attention_reference(qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale):
    """`window_attention` in plain torch, written from the semantics in include/orp_hip.h: any dtype, any device, any window."""
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
    p = torch.exp(score - score.amax(-1, keepdim=True))
    o = (p / p.sum(-1, keepdim=True)) @ v                                      # [B, nwy, nwx, heads, N, hd]
    o = o.view(B, nwy, nwx, heads, ws, ws, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, Hp, Wp, C)
    back = qkv.new_empty((B, Hp, Wp, C))
    back[:, sy[:, None], sx[None, :]] = o                                      # un-roll
    return back[:, :H, :W].reshape(B, H * W, C)
