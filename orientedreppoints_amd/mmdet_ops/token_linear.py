"""A per-token linear layer with its epilogue as one HIP launch (`orp_token_linear`, include/orp_hip.h; csrc/orp_token_linear.hip):

    y = act(F.linear(x, weight, bias)) + residual          act = None | 'gelu' (exact, erf), bias and residual optional

on fp32 CUDA tokens at inference: what a Swin block runs as `attn.qkv`, `attn.proj` (+ the block input), `mlp.fc1` (+ GELU) and `mlp.fc2`
(+ residual), and `PatchMerging` as its bias-free `reduction`.  The contraction runs on the bf16 matrix pipe with every fp32 operand
split exactly into three bf16 pieces (six products, fp32 accumulation, one fixed summation order per output): fp32-grade results,
not bit-identical to the library's GEMM.  `token_linear_reference` states the operator in plain torch and is what the tests hold the
kernel to.  There is no fall-back inside `token_linear`: arguments it does not take raise.
"""
import torch
import torch.nn.functional as F

from .. import _lib, _packcache

EPI_BIAS, EPI_GELU, EPI_RES = 1, 2, 4        # the bits of `orp_token_linear_pays`' epilogue argument
ACTS = {None: 0, 'gelu': 1}

_packed = _packcache.new_cache("token_linear_weight")


def _packed_weight(weight):
    """[N, K] -> the three bf16 planes `orp_token_linear` reads (`orp_token_linear_pack_weight`: 6 bytes per weight), cached on the live
    parameter as `_packcache.packed_planes` says (and kept alive for a graph that is being captured)"""
    return _packcache.packed_planes(_packed, weight, "orp_token_linear_packed_bytes", "orp_token_linear_pack_weight",
                                    lambda w: w.float().contiguous())


def epilogue_bits(linear, act, residual):
    return (EPI_BIAS if linear.bias is not None else 0) | (EPI_GELU if act == 'gelu' else 0) | (EPI_RES if residual is not None else 0)


def token_linear_ok(linear, x):
    """`token_linear` takes these: an nn.Linear with fp32 parameters on x's device, of a shape the kernel has (`orp_token_linear_ok`), x contiguous fp32
    CUDA tokens [..., K]; gradients and autocast disabled (inference only)."""
    if torch.is_grad_enabled() or torch.is_autocast_enabled():
        return False
    if not (isinstance(linear, torch.nn.Linear) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        return False
    w, b = linear.weight, linear.bias
    if not (w.dtype == torch.float32 and w.device == x.device and (b is None or (b.dtype == torch.float32 and b.device == x.device))):
        return False
    if x.dim() < 1 or x.shape[-1] != w.shape[1]:
        return False
    return bool(_lib.lib().orp_token_linear_ok(int(w.shape[1]), int(w.shape[0])))


def token_linear_routed(linear, x, act=None, residual=None):
    """the routing rule: `token_linear_ok` and the launch was measured faster than the stock span it replaces at this token count, shape and
    epilogue (`orp_token_linear_pays`, a closed table)"""
    if act not in ACTS or not token_linear_ok(linear, x):
        return False
    tokens = 1
    for s in x.shape[:-1]:
        tokens *= int(s)
    w = linear.weight
    return bool(_lib.lib().orp_token_linear_pays(tokens, int(w.shape[1]), int(w.shape[0]), epilogue_bits(linear, act, residual)))


def token_linear(x, linear, act=None, residual=None, force=False):
    """act(linear(x)) + residual as ONE launch and a new contiguous tensor [..., N]; x [..., K] with any leading dimensions, residual
    (optional) a contiguous fp32 tensor of the output's shape, act None or 'gelu'.  force=False asks the routing table and raises
    ValueError where it says no -- the caller decides what runs instead; force=True launches at every shape the kernel takes.
    ValueError where `token_linear_ok` is false."""
    if act not in ACTS:
        raise ValueError("token_linear: act must be None or 'gelu', got %r" % (act,))
    if not token_linear_ok(linear, x):
        raise ValueError("token_linear: not an fp32 inference call on contiguous CUDA tokens of a supported shape")
    if not force and not token_linear_routed(linear, x, act, residual):
        raise ValueError("token_linear: this shape is not routed (force=True launches it anyway)")
    w, b = linear.weight, linear.bias
    K, N = int(w.shape[1]), int(w.shape[0])
    x = x.detach()
    y = torch.empty(tuple(x.shape[:-1]) + (N,), dtype=torch.float32, device=x.device)
    if residual is not None:
        residual = residual.detach()
        if not (isinstance(residual, torch.Tensor) and residual.shape == y.shape and residual.is_contiguous() and
                residual.dtype == torch.float32 and residual.device == x.device):
            raise ValueError("token_linear: residual must be a contiguous fp32 tensor of the output's shape on x's device")
    tokens = x.numel() // K
    if tokens == 0:
        return y
    planes = _packed_weight(w)
    _lib.call("orp_token_linear", x.device, _lib.ptr(x), _lib.ptr(planes), _lib.ptr(None if b is None else b.detach()), _lib.ptr(residual),
              _lib.ptr(y), tokens, K, N, ACTS[act], _lib.stream_of(x))
    return y


def token_linear_reference(x, weight, bias=None, act=None, residual=None):
    """the operator in plain torch, any dtype and device: act(x @ weight^T + bias) + residual, GELU = 0.5 u (1 + erf(u / sqrt(2)))"""
    if act not in ACTS:
        raise ValueError("token_linear_reference: act must be None or 'gelu', got %r" % (act,))
    u = x @ weight.transpose(-1, -2)
    if bias is not None:
        u = u + bias
    if act == 'gelu':
        u = 0.5 * u * (1.0 + torch.erf(u * (0.5 ** 0.5)))
    return u if residual is None else u + residual


def stock_linear(linear, x, act=None, residual=None):
    """the stock span `token_linear` replaces: F.linear (+ F.gelu) (+ addition), three library launches"""
    y = F.linear(x, linear.weight, linear.bias)
    if act == 'gelu':
        y = F.gelu(y)
    return y if residual is None else residual + y
