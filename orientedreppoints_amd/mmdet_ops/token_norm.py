"""nn.LayerNorm over the last axis of fp32 tokens with the layout glue beside it as one HIP launch (`orp_token_layernorm`,
include/orp_hip.h; csrc/orp_token_layernorm.hip):

    y = (x - mean) * rsqrt(var + eps) * weight + bias          per row of C floats, biased variance

in four (source, destination) layouts -- what Swin runs at inference as
    'tokens'     x [..., C]                          -> [..., C]            a block's norm1 / norm2
    'merge'      x [B, H W, C/4] (hw) or [B, H, W, C/4] -> [B, ceil(H/2) ceil(W/2), C]   pad + cat of the 2 x 2 neighbourhood + PatchMerging.norm
    'from_nchw'  x [B, C, L] or [B, C, H, W]         -> [B, L, C]           the contiguous copy of flatten(2).transpose(1, 2) + PatchEmbed.norm
    'to_nchw'    x [B, H W, C] (hw)                  -> [B, C, H, W]        norm<i> + view + permute(0, 3, 1, 2).contiguous()
One statistics routine and one affine step behind all four: a row has the same bits in every layout and in every launch.
`token_layernorm_reference` states the four operators in plain torch, the gathered ones as mmdet_models/swin.py writes them, and is what
the tests hold the kernel to.  There is no fall-back inside `token_layernorm`: arguments it does not take raise.
"""
import torch
import torch.nn.functional as F

from .. import _lib

LAYOUTS = {'tokens': _lib._CONSTANTS["ORP_LN_TOKENS"], 'merge': _lib._CONSTANTS["ORP_LN_MERGE"],
           'from_nchw': _lib._CONSTANTS["ORP_LN_FROM_NCHW"], 'to_nchw': _lib._CONSTANTS["ORP_LN_TO_NCHW"]}


def _geometry(shape, C, layout, hw):
    """(batch, h, w) of the launch and the output's shape for a source of this shape, or None where the shape is not the layout's"""
    shape = tuple(int(s) for s in shape)
    if hw is not None:
        hw = (int(hw[0]), int(hw[1]))
        if hw[0] < 0 or hw[1] < 0:
            return None
    if layout == 'tokens':
        if len(shape) < 1 or shape[-1] != C:
            return None
        rows = 1
        for s in shape[:-1]:
            rows *= s
        return (rows, 1, 1), shape
    if layout == 'merge':
        if len(shape) == 4 and hw is None:
            hw = shape[1:3]
        if hw is None or len(shape) not in (3, 4) or 4 * shape[-1] != C:
            return None
        if (len(shape) == 3 and shape[1] != hw[0] * hw[1]) or (len(shape) == 4 and tuple(shape[1:3]) != tuple(hw)):
            return None
        return (shape[0], hw[0], hw[1]), (shape[0], ((hw[0] + 1) // 2) * ((hw[1] + 1) // 2), C)
    if layout == 'from_nchw':
        if len(shape) not in (3, 4) or shape[1] != C:
            return None
        h, w = (shape[2], 1) if len(shape) == 3 else shape[2:]
        return (shape[0], h, w), (shape[0], h * w, C)
    if layout == 'to_nchw':
        if hw is None or len(shape) != 3 or shape[-1] != C or shape[1] != hw[0] * hw[1]:
            return None
        return (shape[0], hw[0], hw[1]), (shape[0], C, hw[0], hw[1])
    return None


def _checked(ln, x, layout, hw):
    """the conditions of `token_layernorm_ok`, evaluated once: ((batch, h, w), output shape) of the launch, or None"""
    if torch.is_grad_enabled() or torch.is_autocast_enabled():
        return None
    if not (isinstance(ln, torch.nn.LayerNorm) and len(ln.normalized_shape) == 1 and ln.weight is not None and ln.bias is not None):
        return None
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        return None
    w, b = ln.weight, ln.bias
    if not (w.dtype == torch.float32 and b.dtype == torch.float32 and w.device == x.device and b.device == x.device):
        return None
    C = int(ln.normalized_shape[0])
    if layout not in LAYOUTS or not _lib.lib().orp_token_layernorm_ok(C):
        return None
    return _geometry(x.shape, C, layout, hw)


def _pays(ln, geo, layout):
    C = int(ln.normalized_shape[0])
    rows = 1
    for s in geo[1]:
        rows *= s
    return bool(_lib.lib().orp_token_layernorm_pays(rows // C, C, LAYOUTS[layout]))


def _launch(x, ln, layout, geo):
    (batch, h, w), out = geo
    x = x.detach()
    y = torch.empty(out, dtype=torch.float32, device=x.device)
    if y.numel() == 0:
        return y
    _lib.call("orp_token_layernorm", x.device, _lib.ptr(x), _lib.ptr(ln.weight.detach()), _lib.ptr(ln.bias.detach()), _lib.ptr(y),
              batch, h, w, int(ln.normalized_shape[0]), float(ln.eps), LAYOUTS[layout], _lib.stream_of(x))
    return y


def token_layernorm_ok(ln, x, layout='tokens', hw=None):
    """`token_layernorm` takes these: an nn.LayerNorm over one axis with fp32 affine parameters on x's device, of a width the kernel has
    (`orp_token_layernorm_ok`); x fp32 CUDA, contiguous, of the layout's source shape; gradients and autocast disabled (inference only)."""
    return _checked(ln, x, layout, hw) is not None


def token_layernorm_routed(ln, x, layout='tokens', hw=None):
    """the routing rule: `token_layernorm_ok` and the launch was measured faster than the stock span it replaces at this row count,
    width and layout (`orp_token_layernorm_pays`, a closed table)"""
    geo = _checked(ln, x, layout, hw)
    return geo is not None and _pays(ln, geo, layout)


def token_layernorm(x, ln, layout='tokens', hw=None, force=False):
    """the LayerNorm `ln` of x in `layout` as ONE launch and a new contiguous tensor (module docstring: shapes per layout; hw = (H, W)
    where x does not carry it).  force=False asks the routing table and raises ValueError where it says no -- the caller decides what
    runs instead; force=True launches at every shape the kernel takes.  ValueError where `token_layernorm_ok` is false."""
    if layout not in LAYOUTS:
        raise ValueError("token_layernorm: layout must be one of %s, got %r" % (sorted(LAYOUTS), layout))
    geo = _checked(ln, x, layout, hw)
    if geo is None:
        raise ValueError("token_layernorm: not an fp32 inference call on a contiguous CUDA source of a supported width in layout %r" % layout)
    if not force and not _pays(ln, geo, layout):
        raise ValueError("token_layernorm: this shape is not routed (force=True launches it anyway)")
    return _launch(x, ln, layout, geo)


def token_layernorm_if_routed(x, ln, layout='tokens', hw=None, force=False):
    """for a caller that has the stock lines of the span itself: `token_layernorm`'s result where `token_layernorm_routed` holds (force:
    where `token_layernorm_ok` holds), else None and nothing launched -- the conditions evaluated once per call, not once per question"""
    geo = _checked(ln, x, layout, hw)
    if geo is None or not (force or _pays(ln, geo, layout)):
        return None
    return _launch(x, ln, layout, geo)


def token_layernorm_reference(x, weight, bias, eps=1e-5, layout='tokens', hw=None):
    """the four operators in plain torch, any dtype and device; 'merge' and the NCHW forms as mmdet_models/swin.py writes them"""
    if layout not in LAYOUTS:
        raise ValueError("token_layernorm_reference: layout must be one of %s, got %r" % (sorted(LAYOUTS), layout))
    C = int(weight.shape[0])
    geo = _geometry(x.shape, C, layout, hw)
    if geo is None:
        raise ValueError("token_layernorm_reference: x %s is not a %r source of width %d" % (tuple(x.shape), layout, C))
    (B, H, W), _ = geo
    if layout == 'tokens':
        return F.layer_norm(x, (C,), weight, bias, eps)
    if layout == 'merge':
        x = x.view(B, H, W, C // 4)
        if H % 2 or W % 2:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
        return F.layer_norm(x.view(B, -1, C), (C,), weight, bias, eps)
    if layout == 'from_nchw':
        return F.layer_norm(x.flatten(2).transpose(1, 2), (C,), weight, bias, eps)
    return F.layer_norm(x, (C,), weight, bias, eps).view(-1, H, W, C).permute(0, 3, 1, 2).contiguous()
