"""Fused normalisation + activation passes (include/orp_hip.h `orp_groupnorm_act_multi`, `orp_affine_act`,
`orp_bias_act_multi`): the GroupNorm+ReLU of the dense-head ConvModules for all FPN levels in one launch pair, the
eval-mode BatchNorm (+ residual) + ReLU of the ResNet bottlenecks as one pass, and the bias / ReLU / residual / base-offset
passes around the head's output convolutions for all levels in one launch.  Those are inference-only (callers use them
under torch.no_grad()).  Training: `group_norm_act_train` is the autograd-capable GroupNorm(+ReLU) over a list of tensors
(one launch pair forward, one pair + a parameter reduction backward, `orp_groupnorm_act_multi_train / _backward`);
`bn_act_train` the autograd-capable eval-mode BatchNorm (+ residual) + ReLU of the bottlenecks (the inference pass forward, one
pass + a per-channel reduction backward, `orp_affine_act_backward` / `orp_affine2_act_backward`)."""
import collections
import ctypes
import functools

import torch

from .. import _lib, _packcache


_NormLevel = _lib.struct("orp_norm_level")


def _norm_levels(ins, outs):
    """the `orp_norm_level` array of a launch: logical [B,C,H,W] tensors, outs[i] None = no such output"""
    levels = (_NormLevel * len(ins))()
    for i, (x, y) in enumerate(zip(ins, outs)):
        levels[i] = _NormLevel(x.data_ptr(), y.data_ptr() if y is not None else None, x.size(2), x.size(3))
    return levels


def _gn_modules(gn, n, who):
    """gn: one nn.GroupNorm for n tensors or a list with one per tensor (modules may repeat) -> (the n modules, the distinct
    ones in order of first use, owner[i] = index of tensor i's module among the distinct ones)"""
    gns = list(gn) if isinstance(gn, (list, tuple)) else [gn] * n
    if len(gns) != n or any(g.num_groups != gns[0].num_groups or g.eps != gns[0].eps for g in gns):
        raise ValueError(who + ": one GroupNorm per tensor, equal num_groups / eps")
    index, distinct, owner = {}, [], []
    for g in gns:
        if id(g) not in index:
            index[id(g)] = len(distinct)
            distinct.append(g)
        owner.append(index[id(g)])
    return gns, distinct, owner


def _ptrs(tensors, owner=None):
    """a pointer per launch tensor: tensors[owner[i]] for tensor i (owner None: tensors[i])"""
    owner = range(len(tensors)) if owner is None else owner
    return (ctypes.c_void_p * len(owner))(*[tensors[k].data_ptr() for k in owner])


def _param_ptrs(weights, biases, owner):
    """(gamma pointers, beta pointers) per tensor -- tensor i reads parameter set owner[i] -- and the fp32 contiguous parameter
    tensors themselves, made once per set: the caller keeps them alive until the launch is queued"""
    gs = [w.detach().float().contiguous() for w in weights]
    bs = [b.detach().float().contiguous() for b in biases]
    return _ptrs(gs, owner), _ptrs(bs, owner), gs, bs


def _affine_ptrs(mods, owner):
    """_param_ptrs of the distinct GroupNorm modules `mods`"""
    return _param_ptrs([m.weight for m in mods], [m.bias for m in mods], owner)


def group_norm_act_multi(xs, gn, relu=True, inplace=True, nhwc=None):
    """[GroupNorm(+ReLU)(x) for x in xs] -- xs: list of [B,C,H,W] fp32 CUDA tensors (FPN levels, possibly of several
    towers: up to 16); gn: one nn.GroupNorm for all of them, or a list with one module per tensor (same num_groups and
    eps).  ONE launch pair.
    nhwc='only': the results come back as channels-last tensors ONLY (same logical shape, memory [B,H,W,C]) -- written
    transposed by the normalisation's second pass; nhwc='both': (NCHW list, channels-last list).  What the head's DeformConv
    consumes without a transposition launch."""
    L = _lib.lib()
    x0 = xs[0]
    B, C = x0.size(0), x0.size(1)
    gns, mods, owner = _gn_modules(gn, len(xs), "group_norm_act_multi")
    ins, outs = [], []
    for x in xs:
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.size(0) == B and x.size(1) == C):
            raise ValueError("group_norm_act_multi expects fp32 CUDA [B,C,H,W] tensors with equal B and C")
        x = x.detach().contiguous()
        ins.append(x); outs.append(x if inplace else torch.empty_like(x))
    levels = _norm_levels(ins, outs)
    gam, bet, _gs, _bs = _affine_ptrs(mods, owner)
    nbytes = L.orp_groupnorm_workspace_bytes(levels, len(xs), B, C, gns[0].num_groups)
    ws = _lib.workspace(x0.device, nbytes)
    if nhwc is not None:
        if nhwc not in ('only', 'both') or C % 32 != 0 or 32 % (C // gns[0].num_groups) != 0:
            raise ValueError("group_norm_act_multi(nhwc=...): 'only' | 'both', channels % 32 == 0, 32 % (channels / groups) == 0")
        cl = [torch.empty(x.shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last) for x in ins]
        cl_ptrs = _ptrs(cl)
        if nhwc == 'only':
            for i in range(len(xs)):
                levels[i].output = None
        _lib.call("orp_groupnorm_act_multi_nhwc", x0.device, levels, gam, bet, cl_ptrs, len(xs), B, C, gns[0].num_groups,
                  float(gns[0].eps), 1 if relu else 0, _lib.ptr(ws), ws.numel(), _lib.stream_of(x0))
        return cl if nhwc == 'only' else (outs, cl)
    _lib.call("orp_groupnorm_act_multi_ex", x0.device, levels, gam, bet, len(xs), B, C, gns[0].num_groups, float(gns[0].eps),
              1 if relu else 0, _lib.ptr(ws), ws.numel(), _lib.stream_of(x0))
    return outs


def group_norm_act_multi_cl(xs, gn, relu=True, inplace=True, amax_slots=None):
    """[GroupNorm(+ReLU)(x) for x in xs] for CHANNELS-LAST fp32 CUDA tensors (logical [B,C,H,W], memory [B,H,W,C]; up to 16:
    both towers' levels), results channels-last -- `orp_groupnorm_act_multi_cl`, three launches for all tensors.  gn: one
    nn.GroupNorm or a list with one per tensor (equal num_groups / eps).  amax_slots (a slot index per tensor): returns
    (outs, int32 tensor of float bits: an upper bound of max |y| per slot, from the statistics pass) for `Amax`."""
    L = _lib.lib()
    x0 = xs[0]
    B, C = x0.size(0), x0.size(1)
    gns, mods, owner = _gn_modules(gn, len(xs), "group_norm_act_multi_cl")
    G = gns[0].num_groups
    if 1024 % C != 0 or C % G != 0 or (C // G) % 4 != 0:
        raise ValueError("group_norm_act_multi_cl: 1024 % channels == 0 and (channels / groups) % 4 == 0")
    ins = [x.detach() for x in xs]
    for x in ins:
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.size(0) == B and x.size(1) == C and _is_cl(x)):
            raise ValueError("group_norm_act_multi_cl expects channels-last fp32 CUDA [B,C,H,W] tensors with equal B and C")
    outs = ins if inplace else [torch.empty_like(x, memory_format=torch.channels_last) for x in ins]
    levels = _norm_levels(ins, outs)
    gam, bet, _gs, _bs = _affine_ptrs(mods, owner)
    nbytes = L.orp_groupnorm_cl_workspace_bytes(levels, len(xs), B, C, G)
    ws = _lib.workspace(x0.device, nbytes)
    if amax_slots is not None and not _ranges_wanted():
        amax_slots, no_ranges = None, True
    else:
        no_ranges = False
    if amax_slots is not None:
        slots = (ctypes.c_int * len(xs))(*[int(v) for v in amax_slots])
        bits = torch.empty(max(int(v) for v in amax_slots) + 1, dtype=torch.int32, device=x0.device)
        _lib.call("orp_groupnorm_act_multi_cl_amax", x0.device, levels, gam, bet, len(xs), B, C, G, float(gns[0].eps), 1 if relu else 0,
                  slots, bits.data_ptr(), bits.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_of(x0))
        return outs, bits
    _lib.call("orp_groupnorm_act_multi_cl", x0.device, levels, gam, bet, len(xs), B, C, G, float(gns[0].eps), 1 if relu else 0,
              _lib.ptr(ws), ws.numel(), _lib.stream_of(x0))
    return (outs, None) if no_ranges else outs


_affine_cache = _packcache.new_cache("bn_affine")


def _bn_affine(bn):
    """eval-mode BatchNorm as (scale, shift): y = x*scale + shift; cached on the live module (_packcache.OwnerCache:
    weak reference + identity check), keyed by the storage / version state of its four tensors."""
    hit = _bn_affine_stats(bn)
    return _lib.keep_for_graph(hit[0]), _lib.keep_for_graph(hit[1])


def _bn_affine_stats(bn, cache=True):
    """(scale, shift, mean, rstd) of an eval-mode BatchNorm, fp32 and contiguous: `_bn_affine`'s pair and the statistics it is
    made of, which the training backward (`bn_act_train`) reads.  One arithmetic, one cache entry.  cache=False: computed now and not
    kept -- inside a stream capture of a module whose parameters train, so that the replay recomputes them from the live weights."""
    def st(t):
        return _packcache.tensor_state(t) if t is not None else None
    state = (st(bn.weight), st(bn.bias), st(bn.running_mean), st(bn.running_var), float(bn.eps))
    hit = _affine_cache.get(bn, state) if cache else None
    if hit is None:
        with torch.no_grad():
            rstd = torch.rsqrt(bn.running_var.float() + bn.eps)
            w = bn.weight.float() if bn.weight is not None else torch.ones_like(rstd)
            b = bn.bias.float() if bn.bias is not None else torch.zeros_like(rstd)
            mean = bn.running_mean.float().contiguous()
            scale = (w * rstd).contiguous()
            shift = (b - mean * scale).contiguous()
        hit = (scale, shift, mean, rstd.contiguous())
        if cache:
            _affine_cache.put(bn, state, hit)
    return hit


def bn_act(x, bn, residual=None, relu=True, residual_bn=None, want_range=False):
    """relu?(BatchNorm_eval(x) (+ residual)) in ONE pass, in place on x ([B,C,H,W] fp32 CUDA, contiguous).
    want_range (no residual_bn): returns (x, bits) -- bits a one-element int32 tensor the pass leaves holding max range_bits(y)
    as float bits (`orp_affine_act_range`), what `conv3x3_bn_act` takes as `range_bits`.
    residual_bn: the residual is a RAW convolution output and this eval-mode BatchNorm is applied to it while it is read
    (`orp_affine2_act`: the downsample branch of a stage's first bottleneck) -- the values of bn_act(residual, residual_bn,
    relu=False) followed by this call, without that pass over memory."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("bn_act expects a contiguous fp32 CUDA [B,C,H,W] tensor")
    if residual is not None and not (residual.shape == x.shape and residual.is_contiguous()
                                     and residual.dtype == torch.float32):
        raise ValueError("bn_act: residual must match x")
    if residual_bn is not None and residual is None:
        raise ValueError("bn_act: residual_bn without a residual")
    if want_range and residual_bn is not None:
        raise ValueError("bn_act: want_range with residual_bn")
    scale, shift = _bn_affine(bn)
    B, C, H, W = x.shape
    head = (_lib.ptr(x), _lib.ptr(residual), _lib.ptr(scale), _lib.ptr(shift))
    tail = (_lib.ptr(x), B, C, H * W, 1 if relu else 0)
    if want_range:
        bits = torch.empty(1, dtype=torch.int32, device=x.device)
        _lib.call("orp_affine_act_range", x.device, *head, *tail, _lib.ptr(bits), _lib.stream_of(x))
        return x, bits
    if residual_bn is not None:
        scale2, shift2 = _bn_affine(residual_bn)
        _lib.call("orp_affine2_act", x.device, *head, _lib.ptr(scale2), _lib.ptr(shift2), *tail, _lib.stream_of(x))
        return x
    _lib.call("orp_affine_act", x.device, *head, *tail, _lib.stream_of(x))
    return x


_packed_1x1_t = _packcache.new_cache("conv1x1_bn_weight")


def _transposed_1x1_weight(weight):
    """[Cout,Cin,1,1] -> the [Cin][Cout] layout orp_conv1x1_bn_act reads, cached on the live parameter (inference only), keyed
    by the tensor's storage / version state."""
    w = weight.detach()
    return _packcache.packed(_packed_1x1_t, weight, lambda: w.float().reshape(w.size(0), w.size(1)).t().contiguous())


def _plain_conv(conv, w, ksize, strides, padding):
    """conv, an nn.Conv2d (the caller has asked: the 1x1 rules take subclasses, the 3x3 rule the class itself) with weight w, is a
    plain convolution: fp32 4-D weight of kernel ksize x ksize, no bias, groups 1, dilation 1, a stride of `strides`, this padding"""
    return bool(w.dtype == torch.float32 and w.dim() == 4 and w.size(2) == ksize and w.size(3) == ksize and conv.bias is None and
                tuple(conv.stride) in strides and tuple(conv.padding) == (padding, padding) and
                tuple(conv.dilation) == (1, 1) and conv.groups == 1)


def _bn_input(x, bn):
    """bn is an eval-mode BatchNorm2d and x an fp32 CUDA tensor"""
    return bool(isinstance(bn, torch.nn.BatchNorm2d) and not bn.training and x.is_cuda and x.dtype == torch.float32)


def conv1x1_bn_act_ok(x, conv, bn):
    """conv is a bias-free 1x1 / stride 1 / groups 1 nn.Conv2d of a shape `orp_conv1x1_bn_act` takes, bn an eval-mode
    BatchNorm2d, x an fp32 CUDA [B,Cin,H,W] tensor"""
    w = conv.weight
    return bool(isinstance(conv, torch.nn.Conv2d) and _bn_input(x, bn) and x.dim() == 4 and
                _plain_conv(conv, w, 1, ((1, 1),), 0) and x.size(1) == w.size(1) and x.size(2) * x.size(3) > 0 and
                _lib.lib().orp_conv1x1_bn_act_ok(w.size(1), w.size(0)))


_packed_1x1_pieces = _packcache.new_cache("conv1x1_bn_pieces_weight")


def _packed_1x1_planes(weight):
    """[Cout,Cin,1,1] -> the three bf16 planes `orp_conv1x1_bn_act_pieces` reads (`orp_conv1x1_bn_pieces_pack_weight`: 6 bytes per
    weight), cached as `_packcache.packed_planes` says."""
    return _packcache.packed_planes(_packed_1x1_pieces, weight, "orp_conv1x1_bn_pieces_packed_bytes", "orp_conv1x1_bn_pieces_pack_weight",
                          lambda w: w.float().reshape(w.size(0), w.size(1)).contiguous())


def conv1x1_bn_act_pieces_tile(cin, cout, hw, B):
    """(tile channels, tile positions) of an `orp_conv1x1_bn_act_pieces` launch of this shape, or None"""
    return _lib.tile_query("orp_conv1x1_bn_act_pieces_tile", 2, cin, cout, hw, B)


def _conv1x1_route(shape, force, pieces):
    """'pieces' | 'fp32' | None: the kernel `conv1x1_bn_act` launches.  shape = (Cin, Cout, H*W, B, has_residual) of supported
    arguments, None otherwise.  The bf16-pieces kernel is asked first: never with pieces=False or with force alone; pieces=True: at
    every shape it takes; None: where ORP_BN_CONV1X1_PIECES is on and its table says so.  Then the fp32 kernel: force, or its table."""
    if shape is None:
        return None
    L = _lib.lib()
    if not (force and pieces is None) and pieces is not False:
        if pieces is None:
            from .. import switches
            pieces = bool(switches.BN_CONV1X1_PIECES) and bool(L.orp_conv1x1_bn_act_pieces_pays(*shape))
        if bool(pieces) and bool(L.orp_conv1x1_bn_act_pieces_ok(shape[0], shape[1])):
            return 'pieces'
    return 'fp32' if force or bool(L.orp_conv1x1_bn_act_pays(*shape)) else None


def conv1x1_bn_act(x, conv, bn, residual=None, residual_bn=None, relu=True, force=False, want_range=False, pieces=None):
    """relu?(BatchNorm_eval(conv(x)) (+ residual)) for a bottleneck's 1x1 convolution, as a new contiguous tensor.  Two fused
    kernels carry the BatchNorm, the residual (residual_bn: the residual is a RAW convolution output and this eval-mode BatchNorm is
    applied to it, as in `bn_act`) and the ReLU in their epilogue.  Asked first: `orp_conv1x1_bn_act_pieces_pays` -- the six-product
    bf16-pieces kernel `orp_conv1x1_bn_act_pieces` where it was measured fastest (pieces=True: at any supported shape; pieces=False:
    never; None: where the table says so and ORP_BN_CONV1X1_PIECES is on).  Then, unchanged, `orp_conv1x1_bn_act_pays` -- the
    exact-fp32 MFMA kernel `orp_conv1x1_bn_act` (force=True: at any supported shape, and the pieces table is not asked).  Everywhere
    else this is `bn_act(conv(x).contiguous(), ...)`: the library's convolution and the pass.  Inference only.
    want_range (no residual): returns (y, bits), bits = a one-element int32 tensor with max range_bits(y) as float bits, left by
    whichever kernel wrote y (`orp_conv1x1_bn_act_pieces` / `orp_conv1x1_bn_act_range` / `orp_affine_act_range`) --
    `conv3x3_bn_act`'s `range_bits`."""
    if residual_bn is not None and residual is None:
        raise ValueError("conv1x1_bn_act: residual_bn without a residual")
    if want_range and residual is not None:
        raise ValueError("conv1x1_bn_act: want_range with a residual")
    fused = conv1x1_bn_act_ok(x, conv, bn) and (residual_bn is None or not residual_bn.training)
    shape = (x.size(1), conv.weight.size(0), x.size(2) * x.size(3), x.size(0), 1 if residual is not None else 0) if fused else None
    route = _conv1x1_route(shape, force, pieces)
    if route is None:
        return bn_act(conv(x).contiguous(), bn, residual=residual, relu=relu, residual_bn=residual_bn, want_range=want_range)
    x = x.detach().contiguous()
    B, cin, H, W = x.shape
    cout = conv.weight.size(0)
    if residual is not None:
        residual = residual.detach()
        if not (tuple(residual.shape) == (B, cout, H, W) and residual.is_contiguous() and residual.dtype == torch.float32):
            raise ValueError("conv1x1_bn_act: residual must be a contiguous fp32 tensor of the output's shape")
    weight = _packed_1x1_planes(conv.weight) if route == 'pieces' else _transposed_1x1_weight(conv.weight)
    scale, shift = _bn_affine(bn)
    scale2, shift2 = _bn_affine(residual_bn) if residual_bn is not None else (None, None)
    y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    bits = torch.empty(1, dtype=torch.int32, device=x.device) if want_range else None
    args = (_lib.ptr(x), _lib.ptr(weight), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(residual), _lib.ptr(scale2), _lib.ptr(shift2),
            _lib.ptr(y), B, cin, cout, H * W, 1 if relu else 0)
    if route == 'pieces':                                    # (one entry point, its range word optional)
        _lib.call("orp_conv1x1_bn_act_pieces", x.device, *args, _lib.ptr(bits), _lib.stream_of(x))
    elif want_range:
        _lib.call("orp_conv1x1_bn_act_range", x.device, *args, _lib.ptr(bits), _lib.stream_of(x))
    else:
        _lib.call("orp_conv1x1_bn_act", x.device, *args, _lib.stream_of(x))
    return (y, bits) if want_range else y


def conv1x1_bn_act_dual_ok(x, conv, bn, x2, conv2, bn2):
    """`conv1x1_bn_act_dual` takes these: conv / bn as `conv1x1_bn_act_ok` wants them for x; conv2 a bias-free 1x1 / groups 1 / padding
    0 nn.Conv2d of stride (1, 1) or (2, 2) with conv's output channels, bn2 an eval-mode BatchNorm2d, x2 an fp32 CUDA [B,Cin2,h2,w2]
    tensor whose sampled map is x's map; both channel pairs supported (`orp_conv1x1_bn_act_pieces_dual_ok`)"""
    if not conv1x1_bn_act_ok(x, conv, bn):
        return False
    w2 = getattr(conv2, 'weight', None)
    if not (isinstance(conv2, torch.nn.Conv2d) and _bn_input(x2, bn2) and x2.dim() == 4 and x2.device == x.device and
            _plain_conv(conv2, w2, 1, ((1, 1), (2, 2)), 0) and x2.size(1) == w2.size(1) and
            w2.size(0) == conv.weight.size(0) and x2.size(0) == x.size(0)):
        return False
    s = conv2.stride[0]
    return bool(x2.size(2) > 0 and x2.size(3) > 0 and (x2.size(2) - 1) // s + 1 == x.size(2) and (x2.size(3) - 1) // s + 1 == x.size(3)
                and _lib.lib().orp_conv1x1_bn_act_pieces_dual_ok(conv.weight.size(1), w2.size(1), w2.size(0)))


def conv1x1_bn_act_dual_pays(x, conv, x2, conv2):
    """the closed table of the dual launch (`orp_conv1x1_bn_act_pieces_dual_pays`) for these shapes"""
    return bool(_lib.lib().orp_conv1x1_bn_act_pieces_dual_pays(conv.weight.size(1), conv2.weight.size(1), conv.weight.size(0),
                                                               x.size(2) * x.size(3), conv2.stride[0], x.size(0)))


def conv1x1_bn_act_dual_routed(x, conv, bn, x2, conv2, bn2):
    """`conv1x1_bn_act_dual` takes these (`conv1x1_bn_act_dual_ok`) and was measured faster than what it replaces
    (`conv1x1_bn_act_dual_pays`): what a caller asks, as `conv3x3_bn_act_routed`"""
    return conv1x1_bn_act_dual_ok(x, conv, bn, x2, conv2, bn2) and conv1x1_bn_act_dual_pays(x, conv, x2, conv2)


def conv1x1_bn_act_dual_tile(cin, cin2, cout, hw, B):
    """(tile channels, tile positions) of an `orp_conv1x1_bn_act_pieces_dual` launch of this shape, or None"""
    return _lib.tile_query("orp_conv1x1_bn_act_pieces_dual_tile", 2, cin, cin2, cout, hw, B)


def conv1x1_bn_act_dual(x, conv, bn, x2, conv2, bn2, relu=True):
    """relu?(BatchNorm_eval(conv(x)) + BatchNorm2_eval(conv2(x2))) as a new contiguous tensor in ONE launch of the bf16-pieces kernel
    (`orp_conv1x1_bn_act_pieces_dual`): a bottleneck's conv3 / bn3 on x with the block's downsample convolution conv2 (bias-free 1x1,
    stride (1, 1) or (2, 2), padding 0) and its eval-mode BatchNorm bn2 on the block input x2 contracted in front of it; the
    downsample output is never written.  The bits of `conv1x1_bn_act(x2[:, :, ::s, ::s].contiguous(), conv2, bn2, relu=False,
    pieces=True)` followed by `conv1x1_bn_act(x, conv, bn, residual=that, relu=relu, pieces=True)`.  Inference only; unsupported
    arguments are a ValueError (the caller asks `conv1x1_bn_act_dual_routed` first)."""
    if not conv1x1_bn_act_dual_ok(x, conv, bn, x2, conv2, bn2):
        raise ValueError("conv1x1_bn_act_dual: unsupported modules or shapes (conv1x1_bn_act_dual_ok)")
    x, x2 = x.detach().contiguous(), x2.detach().contiguous()
    B, cin, H, W = x.shape
    cout, cin2 = conv.weight.size(0), conv2.weight.size(1)
    packed, packed2 = _packed_1x1_planes(conv.weight), _packed_1x1_planes(conv2.weight)
    scale, shift = _bn_affine(bn)
    scale2, shift2 = _bn_affine(bn2)
    y = torch.empty((B, cout, H, W), dtype=torch.float32, device=x.device)
    _lib.call("orp_conv1x1_bn_act_pieces_dual", x.device, _lib.ptr(x), _lib.ptr(packed), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(x2),
              _lib.ptr(packed2), _lib.ptr(scale2), _lib.ptr(shift2), cin2, x2.size(2), x2.size(3), conv2.stride[0], _lib.ptr(y),
              B, cin, cout, H, W, 1 if relu else 0, _lib.stream_of(x))
    return y


_Conv3x3Kernel = collections.namedtuple("_Conv3x3Kernel", "kind strides ok pays packed_bytes pack_weight launch takes_stride "
                                                           "switch fuse_attr force_attr")
# The fused fp16-pieces kernels of a bottleneck's conv2, in the order they are asked: the first that says yes runs.  Per kernel: the
# conv strides it takes; the library's names of its channel rule, its routing table, its packer pair and its launch; whether those
# calls carry the stride -- behind (c_in, c_out) in `ok`, behind (height, width) in `pays` and in the launch; the switch (a name in
# `switches`) and the block attributes that turn it off / route every supported shape.  A shape is taken by at most one `ok`
# (tests/test_conv3x3_route_table.py).  To add a kernel: its .hip file, a row here, a switch.
CONV3X3_KERNELS = (
    _Conv3x3Kernel("act", ((1, 1),), "orp_conv3x3_bn_act_ok", "orp_conv3x3_bn_act_pays", "orp_conv3x3_bn_packed_bytes",
                   "orp_conv3x3_bn_pack_weight", "orp_conv3x3_bn_act", False, "BN_CONV3X3_FUSE", "fuse_conv3x3", "force_conv3x3"),
    _Conv3x3Kernel("deep", ((1, 1), (2, 2)), "orp_conv3x3_bn_deep_ok", "orp_conv3x3_bn_deep_pays", "orp_conv3x3_bn_deep_packed_bytes",
                   "orp_conv3x3_bn_deep_pack_weight", "orp_conv3x3_bn_deep", True, "BN_CONV3X3_DEEP_FUSE", "fuse_conv3x3_deep",
                   "force_conv3x3_deep"),
    _Conv3x3Kernel("s2", ((2, 2),), "orp_conv3x3_bn_s2_ok", "orp_conv3x3_bn_s2_pays", "orp_conv3x3_bn_s2_packed_bytes",
                   "orp_conv3x3_bn_s2_pack_weight", "orp_conv3x3_bn_s2", False, "BN_CONV3X3_S2_FUSE", "fuse_conv3x3_s2", "force_conv3x3_s2"),
)
_CONV3X3 = {k.kind: k for k in CONV3X3_KERNELS}


def conv3x3_kernel(kind):
    """the row of `CONV3X3_KERNELS` of this kind ('act' | 'deep' | 's2')"""
    return _CONV3X3[kind]


def _stride_arg(k, conv):
    return (conv.stride[0],) if k.takes_stride else ()


def _conv3x3_ok(kind, x, conv, bn, shape=None):
    """conv is a bias-free 3x3 / padding 1 / dilation 1 / groups 1 nn.Conv2d of a stride and a shape the kernel `kind` takes (its `ok`
    symbol), bn an eval-mode BatchNorm2d, x an fp32 CUDA [B,Cin,H,W] tensor (shape: the input's shape where x is only a tensor of its
    device and dtype)"""
    k = _CONV3X3[kind]
    w = getattr(conv, 'weight', None)
    shape = tuple(x.shape) if shape is None else tuple(shape)
    # (the class itself: a subclass, which the 1x1 rules take, may have another forward)
    return bool(type(conv) is torch.nn.Conv2d and _bn_input(x, bn) and len(shape) == 4 and
                _plain_conv(conv, w, 3, k.strides, 1) and shape[1] == w.size(1) and shape[0] * shape[2] * shape[3] > 0 and
                getattr(_lib.lib(), k.ok)(w.size(1), w.size(0), *_stride_arg(k, conv)))


def _conv3x3_routed(kind, x, conv, bn, force=False, shape=None):
    """`_conv3x3_launch` would run the kernel `kind` for this input, given its range: supported (`_conv3x3_ok`) and either forced or
    measured faster (its `pays` symbol).  A caller asks BEFORE it produces the input (shape = its shape, x any tensor of its device and
    dtype), so that the producer leaves the range word."""
    if not _conv3x3_ok(kind, x, conv, bn, shape):
        return False
    k = _CONV3X3[kind]
    B, _c, H, W = tuple(x.shape) if shape is None else tuple(shape)
    return bool(force or getattr(_lib.lib(), k.pays)(conv.weight.size(1), conv.weight.size(0), H, W, *_stride_arg(k, conv), B))


def conv3x3_bn_route(x, conv, bn, shape, enabled, forced):
    """the kind of the first kernel of `CONV3X3_KERNELS` that is switched on (enabled(kind)) and whose `_conv3x3_routed` says yes for an
    input of this shape (forced(kind): its force), or None.  A kernel's table is asked only where every kernel before it said no."""
    for k in CONV3X3_KERNELS:
        if enabled(k.kind) and _conv3x3_routed(k.kind, x, conv, bn, forced(k.kind), shape):
            return k.kind
    return None


_packed_3x3_cache = _packcache.new_cache("conv3x3_bn_weight")


def _packed_3x3(kind, weight):
    """[C,C,3,3] -> the two fp16 planes + scale the kernel `kind` reads (its packer: 4 bytes per weight + 16), cached as `_packcache.packed_planes`
    says.  One cache for every kind: the packers write one format, and a weight's shape is taken by one kind only."""
    k = _CONV3X3[kind]
    return _packcache.packed_planes(_packed_3x3_cache, weight, k.packed_bytes, k.pack_weight, lambda w: w.float().contiguous())


def _conv3x3_launch(kind, x, conv, bn, relu=True, force=False, range_bits=None):
    """relu?(BatchNorm_eval(conv(x))) for a bottleneck's conv2 as a new contiguous tensor.  Where `_conv3x3_routed` says so and the
    input's range is known -- range_bits: the one-element int32 tensor its producer left (`conv1x1_bn_act(want_range=True)`,
    `bn_act(want_range=True)`) -- this is ONE launch of the kernel `kind`: the fp16-pieces arithmetic of the towers' convolutions with
    the BatchNorm and the ReLU in the epilogue, NCHW in and out, [B,C,(H-1)//s+1,(W-1)//s+1] for stride s.  Everywhere else it is
    `bn_act(conv(x).contiguous(), bn)`: the library's convolution and the pass.  The weight planes are packed once per weight
    (`_packed_3x3`: cached on the live parameter by storage / version state); nothing else is cached.  Inference only."""
    if range_bits is None or not _conv3x3_routed(kind, x, conv, bn, force):
        return bn_act(conv(x).contiguous(), bn, relu=relu)
    k = _CONV3X3[kind]
    x = x.detach().contiguous()
    B, cin, H, W = x.shape
    cout, s = conv.weight.size(0), conv.stride[0]
    packed = _packed_3x3(kind, conv.weight)
    scale, shift = _bn_affine(bn)
    y = torch.empty((B, cout, (H - 1) // s + 1, (W - 1) // s + 1), dtype=torch.float32, device=x.device)
    _lib.call(k.launch, x.device, _lib.ptr(x), _lib.ptr(packed), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(range_bits), _lib.ptr(y),
              B, cin, cout, H, W, *_stride_arg(k, conv), 1 if relu else 0, _lib.stream_of(x))
    return y


def _of_kind(fn, kind, doc):
    """fn with its first argument bound to `kind`, under a docstring of its own"""
    bound = functools.partial(fn, kind)
    bound.__doc__ = doc
    return bound


conv3x3_bn_act_ok = _of_kind(_conv3x3_ok, "act", "`_conv3x3_ok` of `orp_conv3x3_bn_act`: Cin == Cout in {64, 128, 256}, stride 1")
conv3x3_bn_act_routed = _of_kind(_conv3x3_routed, "act", "`_conv3x3_routed` of `orp_conv3x3_bn_act` (`orp_conv3x3_bn_act_pays`)")
conv3x3_bn_act = _of_kind(_conv3x3_launch, "act", "`_conv3x3_launch` of `orp_conv3x3_bn_act`: 64 / 128 / 256 channels, stride 1")
_packed_3x3_planes = _of_kind(_packed_3x3, "act", "`_packed_3x3` by `orp_conv3x3_bn_pack_weight`")
conv3x3_bn_deep_ok = _of_kind(_conv3x3_ok, "deep", "`_conv3x3_ok` of `orp_conv3x3_bn_deep`: Cin == Cout == 512, stride 1 or 2")
conv3x3_bn_deep_routed = _of_kind(_conv3x3_routed, "deep", "`_conv3x3_routed` of `orp_conv3x3_bn_deep` (`orp_conv3x3_bn_deep_pays`)")
conv3x3_bn_deep = _of_kind(_conv3x3_launch, "deep", "`_conv3x3_launch` of `orp_conv3x3_bn_deep`: stage 4's 512 channels, stride 1 and 2")
_packed_3x3_deep_planes = _of_kind(_packed_3x3, "deep", "`_packed_3x3` by `orp_conv3x3_bn_deep_pack_weight`")
conv3x3_bn_s2_ok = _of_kind(_conv3x3_ok, "s2", "`_conv3x3_ok` of `orp_conv3x3_bn_s2`: Cin == Cout in {128, 256}, stride 2")
conv3x3_bn_s2_routed = _of_kind(_conv3x3_routed, "s2", "`_conv3x3_routed` of `orp_conv3x3_bn_s2` (`orp_conv3x3_bn_s2_pays`)")
conv3x3_bn_s2 = _of_kind(_conv3x3_launch, "s2", "`_conv3x3_launch` of `orp_conv3x3_bn_s2`: block 0 of stages 2 and 3, 128 / 256 channels, stride 2")
_packed_3x3_s2_planes = _of_kind(_packed_3x3, "s2", "`_packed_3x3` by `orp_conv3x3_bn_s2_pack_weight`")


def conv3x3_bn_act_tile(cin, cout, H, W, B):
    """(tile_h, tile_w, waves over positions, waves over channels) of an `orp_conv3x3_bn_act` launch of this shape, or None"""
    return _lib.tile_query("orp_conv3x3_bn_act_tile", 4, cin, cout, H, W, B)


def bn_relu_maxpool(x, bn):
    """max_pool2d(relu(BatchNorm_eval(x)), kernel 3, stride 2, padding 1) as ONE kernel (`orp_affine_relu_maxpool`, the ResNet
    stem): x [B,C,H,W] fp32 CUDA, contiguous, left as it is; returns a new [B,C,(H-1)//2+1,(W-1)//2+1] tensor."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("bn_relu_maxpool expects a contiguous fp32 CUDA [B,C,H,W] tensor")
    scale, shift = _bn_affine(bn)
    B, C, H, W = x.shape
    y = torch.empty((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    _lib.call("orp_affine_relu_maxpool", x.device, _lib.ptr(x), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), B, C, H, W, _lib.stream_of(x))
    return y


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def is_maxpool_3_2_1(mp):
    """mp is exactly MaxPool2d(3, 2, 1): dilation 1, floor mode, no indices"""
    return bool(type(mp) is torch.nn.MaxPool2d and _pair(mp.kernel_size) == (3, 3) and _pair(mp.stride) == (2, 2) and
                _pair(mp.padding) == (1, 1) and _pair(mp.dilation) == (1, 1) and not mp.ceil_mode and not mp.return_indices)


def stem_conv_ok(x, conv, bn=None, maxpool=None):
    """conv is the bias-free 7x7 / stride 2 / padding 3 fp32 nn.Conv2d 3 -> 64 that `orp_stem_conv_bn_relu_pool` takes and x an fp32 CUDA
    [B,3,H,W] tensor; bn (where given) an eval-mode BatchNorm2d; maxpool (where given) exactly MaxPool2d(3, 2, 1): dilation 1, floor mode,
    no indices"""
    w = getattr(conv, 'weight', None)
    if not (type(conv) is torch.nn.Conv2d and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0 and
            _plain_conv(conv, w, 7, ((2, 2),), 3) and x.size(1) == w.size(1) and
            _lib.lib().orp_stem_ok(w.size(1), w.size(0), 7, 2, 3)):
        return False
    if bn is not None and not _bn_input(x, bn):
        return False
    return maxpool is None or is_maxpool_3_2_1(maxpool)


def stem_conv_routed(x, conv, bn, maxpool, force=False):
    """`stem_conv_bn_relu_maxpool` is what runs for this stem and input: supported (`stem_conv_ok`), no gradient wanted, and either
    forced or measured faster than library convolution + `bn_relu_maxpool` (`orp_stem_pays`)"""
    if torch.is_grad_enabled() or not stem_conv_ok(x, conv, bn, maxpool):
        return False
    return bool(force or _lib.lib().orp_stem_pays(x.size(2), x.size(3), x.size(0)))


_packed_stem = _packcache.new_cache("stem_weight")


def _packed_stem_weight(weight):
    """[64,3,7,7] -> the per-lane MFMA operand order `orp_stem_conv_bn_relu_pool` reads (`orp_stem_pack_weight`), cached as
    `_packcache.packed_planes` says."""
    return _packcache.packed_planes(_packed_stem, weight, "orp_stem_packed_bytes", "orp_stem_pack_weight", lambda w: w.float().contiguous())


def _stem_launch(x, conv, bn, pool):
    if not stem_conv_ok(x, conv, bn):
        raise ValueError("the stem kernel takes a bias-free 7x7 / 2 / 3 fp32 convolution 3 -> 64 (and an eval-mode BatchNorm2d) on an "
                         "fp32 CUDA [B,3,H,W] tensor")
    x = x.detach().contiguous()
    B, cin, H, W = x.shape
    cout = conv.weight.size(0)
    packed = _packed_stem_weight(conv.weight)
    scale, shift = _bn_affine(bn) if pool else (None, None)
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if pool:
        ho, wo = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
    y = torch.empty((B, cout, ho, wo), dtype=torch.float32, device=x.device)
    _lib.call("orp_stem_conv_bn_relu_pool", x.device, _lib.ptr(x), _lib.ptr(packed), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), B, cin,
              cout, H, W, 7, 2, 3, 1 if pool else 0, _lib.stream_of(x))
    return y


def stem_conv_bn_relu_maxpool(x, conv, bn):
    """max_pool2d(relu(BatchNorm_eval(conv(x))), 3, 2, 1) of the ResNet stem as ONE launch of `orp_stem_conv_bn_relu_pool` (exact fp32
    MFMA; the raw conv map stays on the CU): x [B,3,H,W] fp32 CUDA; returns a new [B,64,Hp,Wp] tensor.  The caller has asked
    `stem_conv_routed`; an unsupported stem is an error here."""
    return _stem_launch(x, conv, bn, True)


def stem_conv_raw(x, conv):
    """conv(x) by the same launch in raw mode (no BatchNorm / ReLU / pooling): what the tests compare contraction and epilogue through"""
    return _stem_launch(x, conv, None, False)


def fpn_topdown_ok(xs, gns):
    """the laterals (raw convolution outputs, finest first) and their GroupNorms are what `fpn_topdown_cl` takes: at most four
    fp32 CUDA [B,C,H,W] tensors, each exactly twice the next in H and W, channel tiles of 32 that hold whole groups"""
    x0, g0 = xs[0], gns[0]
    B, C = x0.size(0), x0.size(1)
    if not (1 <= len(xs) <= 4 and len(gns) == len(xs) and C % 32 == 0 and C % g0.num_groups == 0 and 32 % (C // g0.num_groups) == 0):
        return False
    for i, (x, g) in enumerate(zip(xs, gns)):
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.size(0) == B and x.size(1) == C and
                isinstance(g, torch.nn.GroupNorm) and g.affine and g.num_groups == g0.num_groups and g.eps == g0.eps):
            return False
        if i and (xs[i - 1].size(2) != 2 * x.size(2) or xs[i - 1].size(3) != 2 * x.size(3)):
            return False
    return True


def fpn_topdown_cl(xs, gns, amax=True):
    """The FPN's top-down path from the RAW lateral convolution outputs xs (finest level first) as ONE pass over the laterals
    behind their statistics (`orp_fpn_topdown_nhwc`: chunk statistics, their merge, the pass): outs[i] = GN_i(xs[i]) + up2(outs[i + 1]) in channels-last memory -- the values of
    group_norm_act_multi, `a + F.interpolate(b, size=a.shape[2:], mode='nearest')` per level and to_channels_last_multi.
    Returns (outs, bits): bits = a one-element int32 tensor with max |out| over all levels as float bits when the library's
    arithmetic reads ranges (as to_channels_last_multi(amax_slots=[0] * n)), else None."""
    if not fpn_topdown_ok(xs, gns):
        raise ValueError("fpn_topdown_cl: see fpn_topdown_ok")
    L = _lib.lib()
    x0 = xs[0]
    B, C = x0.size(0), x0.size(1)
    n = len(xs)
    gns, mods, owner = _gn_modules(gns, n, "fpn_topdown_cl")
    ins = [x.detach().contiguous() for x in xs]
    outs = [torch.empty(x.shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last) for x in ins]
    levels = _norm_levels(ins, outs)
    gam, bet, _gs, _bs = _affine_ptrs(mods, owner)
    bits = torch.empty(1, dtype=torch.int32, device=x0.device) if (amax and _ranges_wanted()) else None
    nbytes = L.orp_fpn_topdown_workspace_bytes(levels, n, B, C, gns[0].num_groups)
    ws = _lib.workspace(x0.device, nbytes)
    _lib.call("orp_fpn_topdown_nhwc", x0.device, levels, gam, bet, n, B, C, gns[0].num_groups, float(gns[0].eps),
              bits.data_ptr() if bits is not None else None, _lib.ptr(ws), ws.numel(), _lib.stream_of(x0))
    return outs, bits


_BiasLevel = _lib.struct("orp_bias_level")


def bias_act_multi(xs, bias, relu=False, residuals=None, sub=None):
    """ys[i] = relu?(xs[i] + bias[c] (+ residuals[i])), in place on xs; with `sub` ([C]) additionally returns
    zs[i] = ys[i] - sub[c].  xs: fp32 CUDA [B,C,H,W] tensors (one per FPN level), ONE launch for all of them.
    Same per-element operation order as the separate framework passes (bias add, residual add, ReLU, subtraction)."""
    x0 = xs[0]
    B, C = x0.size(0), x0.size(1)
    levels = (_BiasLevel * len(xs))()
    ys, zs = [], []
    keep = []
    for i, x in enumerate(xs):
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.size(0) == B and x.size(1) == C):
            raise ValueError("bias_act_multi expects fp32 CUDA [B,C,H,W] tensors with equal B and C")
        x = x.detach().contiguous()
        r = None
        if residuals is not None:
            r = residuals[i].detach().contiguous()
            if r.shape != x.shape or r.dtype != torch.float32:
                raise ValueError("bias_act_multi: residual must match x")
            keep.append(r)
        z = torch.empty_like(x) if sub is not None else None
        ys.append(x); zs.append(z)
        levels[i] = _BiasLevel(x.data_ptr(), r.data_ptr() if r is not None else None, x.data_ptr(),
                               z.data_ptr() if z is not None else None, x.size(2), x.size(3))
    b = bias.detach().float().contiguous() if bias is not None else None
    s = sub.detach().float().reshape(-1).contiguous() if sub is not None else None
    if (b is not None and b.numel() != C) or (s is not None and s.numel() != C):
        raise ValueError("bias_act_multi: bias / sub must have C elements")
    _lib.call("orp_bias_act_multi", x0.device, levels, len(xs), B, C, _lib.ptr(b), _lib.ptr(s), 1 if relu else 0, _lib.stream_of(x0))
    return (ys, zs) if sub is not None else ys


_packed_1x1 = _packcache.new_cache("conv1x1_weight")


def _packed_1x1_weight(weight):
    """[Cout,Cin,1,1] -> the [Cin][32] pack of orp_conv1x1_multi, cached on the live parameter (inference only)."""
    def build():
        w = weight.detach()
        cout, cin = w.size(0), w.size(1)
        w2 = w.float().reshape(cout, cin).contiguous()
        packed = torch.empty((_lib.lib().orp_conv1x1_packed_floats(cin),), dtype=torch.float32, device=w.device)
        _lib.call("orp_conv1x1_pack_weight", w.device, _lib.ptr(w2), cout, cin, _lib.ptr(packed), _lib.stream_of(w2))
        return packed
    return _packcache.packed(_packed_1x1, weight, build)


def conv1x1_ok(conv, x):
    w = conv.weight
    return bool(x.is_cuda and x.dtype == torch.float32 and w.dim() == 4 and w.size(2) == 1 and w.size(3) == 1 and
                tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (0, 0) and conv.groups == 1 and
                _lib.lib().orp_conv1x1_ok(w.size(1), w.size(0)))


def conv1x1_multi(xs, conv, relu=False, residuals=None, sub=None):
    """ys[i] = relu?(conv(xs[i]) (+ residuals[i])) for a 1x1 nn.Conv2d with at most 32 output channels (bias included),
    all FPN levels in ONE launch; with `sub` ([Cout]) also returns zs[i] = ys[i] - sub.  Inference only (no autograd).
    Same epilogue order as the framework passes it replaces (bias add, residual add, ReLU, subtraction)."""
    x0 = xs[0]
    B, cin = x0.size(0), x0.size(1)
    cout = conv.weight.size(0)
    packed = _packed_1x1_weight(conv.weight)
    levels = (_BiasLevel * len(xs))()
    ys, zs, keep = [], [], []
    for i, x in enumerate(xs):
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.size(0) == B and x.size(1) == cin):
            raise ValueError("conv1x1_multi expects fp32 CUDA [B,Cin,H,W] tensors with equal B and Cin")
        x = x.detach().contiguous()
        y = torch.empty((B, cout, x.size(2), x.size(3)), dtype=torch.float32, device=x.device)
        r = None
        if residuals is not None:
            r = residuals[i].detach().contiguous()
            if r.shape != y.shape or r.dtype != torch.float32:
                raise ValueError("conv1x1_multi: residual must match the output")
        z = torch.empty_like(y) if sub is not None else None
        keep += [x, r]
        ys.append(y); zs.append(z)
        levels[i] = _BiasLevel(x.data_ptr(), r.data_ptr() if r is not None else None, y.data_ptr(),
                               z.data_ptr() if z is not None else None, x.size(2), x.size(3))
    b = conv.bias.detach().float().contiguous() if conv.bias is not None else None
    s = sub.detach().float().reshape(-1).contiguous() if sub is not None else None
    if s is not None and s.numel() != cout:
        raise ValueError("conv1x1_multi: sub must have Cout elements")
    _lib.call("orp_conv1x1_multi", x0.device, levels, len(xs), B, cin, cout, _lib.ptr(packed), _lib.ptr(b), _lib.ptr(s),
              1 if relu else 0, _lib.stream_of(x0))
    return (ys, zs) if sub is not None else ys


SMALL_LEVEL_POSITIONS = 1024        # H*W up to which a level goes through conv3x3_multi's HIP kernel (32 x 32 at 1024^2)


def conv3x3_multi(xs, conv, split_k=False):
    """[conv(x) without bias for x in xs] for 3x3 / stride 1 or 2 / pad 1 / groups 1 nn.Conv2d modules, inference only
    (split_k: launches with few positions also split K over the grid, fixed-order sum of the partial images);
    conv: one module for all tensors or a list with one module per tensor (equal channel counts).  The small levels
    (H*W <= SMALL_LEVEL_POSITIONS) share ONE launch of the exact-fp32 MFMA kernel `orp_conv3x3_small_multi_strided` (the
    framework would issue an im2col + GEMM pair per level), the big levels stay on the library (Winograd)."""
    import torch.nn.functional as F
    from .deform_conv import _packed_weight
    convs = list(conv) if isinstance(conv, (list, tuple)) else [conv] * len(xs)
    w0 = convs[0].weight
    cout, cin = w0.size(0), w0.size(1)
    L = _lib.lib()

    def eligible(c):
        w = c.weight
        return (tuple(w.shape) == (cout, cin, 3, 3) and tuple(c.stride) in ((1, 1), (2, 2)) and tuple(c.padding) == (1, 1)
                and tuple(c.dilation) == (1, 1) and c.groups == 1 and w.dtype == torch.float32)
    ok = bool(L.orp_conv3x3_small_ok(cin, cout)) and all(eligible(c) for c in {id(c): c for c in convs}.values())
    outs = [None] * len(xs)
    small = []
    for i, x in enumerate(xs):
        if ok and x.is_cuda and x.dtype == torch.float32 and x.size(2) * x.size(3) <= SMALL_LEVEL_POSITIONS:
            small.append(i)
        else:
            c = convs[i]
            outs[i] = F.conv2d(x, c.weight, None, c.stride, c.padding, c.dilation, c.groups)
    if small:
        B = xs[small[0]].size(0)
        wts = (ctypes.c_void_p * len(small))()
        strides = (ctypes.c_int * len(small))()
        keep, seen, ins = [], {}, []
        for k, i in enumerate(small):
            x = xs[i].detach().contiguous()
            st = int(convs[i].stride[0])
            y = torch.empty((B, cout, (x.size(2) - 1) // st + 1, (x.size(3) - 1) // st + 1), dtype=torch.float32,
                            device=x.device)
            wp = seen.get(id(convs[i]))
            if wp is None:                                 # once per distinct module
                packed = _packed_weight(convs[i].weight)
                keep.append(packed)
                wp = seen[id(convs[i])] = packed.data_ptr()
            ins.append(x); outs[i] = y
            wts[k] = wp
            strides[k] = st
        levels = _norm_levels(ins, [outs[i] for i in small])
        x0 = xs[small[0]]
        nbytes = L.orp_conv3x3_small_workspace_bytes(levels, strides, len(small), B, cout) if split_k else 0
        ws = _lib.workspace(x0.device, nbytes) if nbytes else None
        _lib.call("orp_conv3x3_small_multi_strided", x0.device, levels, wts, strides, len(small), B, cin, cout, _lib.ptr(ws),
                  ws.numel() if ws is not None else 0, _lib.stream_of(x0))
    return outs


class _GroupNormActTrain(torch.autograd.Function):
    """ys[i] = relu?(GroupNorm(xs[i])) for n tensors (the FPN levels of one tower layer) with autograd: forward = the
    inference launch pair + stored (mean, rstd); backward = two launches for every grad_input + one per distinct module
    for (dgamma, dbeta), all sums in a fixed order.  Inputs: n, groups, eps, relu, owner (tensor i uses parameter set
    owner[i]), then the n tensors, then the distinct gammas, then the distinct betas."""

    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)   # under autocast: fp32 inputs, autocast off inside
    def forward(ctx, n, groups, eps, relu, owner, *tensors):
        L = _lib.lib()
        xs = [t.detach().contiguous() for t in tensors[:n]]
        m = (len(tensors) - n) // 2
        gam, bet, gammas, betas = _param_ptrs(tensors[n:n + m], tensors[n + m:], owner)
        x0 = xs[0]
        B, C = x0.size(0), x0.size(1)
        for x in xs:
            if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.size(0) == B and x.size(1) == C):
                raise ValueError("group_norm_act_train expects fp32 CUDA [B,C,H,W] tensors with equal B and C")
        ys = [torch.empty_like(x) for x in xs]
        levels = _norm_levels(xs, ys)
        stats = torch.empty((n * B * groups, 2), dtype=torch.float32, device=x0.device)
        nbytes = L.orp_groupnorm_workspace_bytes(levels, n, B, C, groups)
        ws = _lib.workspace(x0.device, nbytes)
        _lib.call("orp_groupnorm_act_multi_train", x0.device, levels, gam, bet, n, B, C, groups, float(eps), 1 if relu else 0,
                  _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_of(x0))
        ctx.save_for_backward(stats, *xs, *gammas, *betas, *ys)      # ys: the ReLU mask (the next layer keeps them alive anyway)
        ctx.meta = (n, m, groups, bool(relu), tuple(owner))
        return tuple(ys)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        L = _lib.lib()
        n, m, groups, relu, owner = ctx.meta
        saved = ctx.saved_tensors
        stats, xs, gammas, betas = saved[0], saved[1:1 + n], saved[1 + n:1 + n + m], saved[1 + n + m:1 + n + 2 * m]
        ys = saved[1 + n + 2 * m:]
        x0 = xs[0]
        B, C = x0.size(0), x0.size(1)
        gys = [torch.zeros_like(x) if g is None else g.detach().float().contiguous() for x, g in zip(xs, grads)]
        gxs = [torch.empty_like(x) for x in xs]
        dys, dxs = _ptrs(gys), _ptrs(gxs)
        levels = _norm_levels(xs, ys)
        gam, bet, _gs, _bs = _param_ptrs(gammas, betas, owner)
        dgam = [torch.empty_like(g) for g in gammas]
        dbet = [torch.empty_like(b) for b in betas]
        dg, db = _ptrs(dgam, owner), _ptrs(dbet, owner)
        nbytes = L.orp_groupnorm_backward_workspace_bytes(levels, n, B, C, groups)
        ws = _lib.workspace(x0.device, nbytes)
        _lib.call("orp_groupnorm_act_multi_backward", x0.device, levels, dys, dxs, gam, bet, dg, db, n, B, C, groups, 1 if relu else 0,
                  _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_of(x0))
        return (None, None, None, None, None) + tuple(gxs) + tuple(dgam) + tuple(dbet)


def group_norm_act_train(xs, gn, relu=True):
    """[relu?(GroupNorm(x)) for x in xs] with autograd, ONE launch pair forward for all tensors (up to 16).  gn: one
    nn.GroupNorm for all of them or a list with one module per tensor (equal num_groups / eps; modules may repeat)."""
    gns, distinct, owner = _gn_modules(gn, len(xs), "group_norm_act_train")
    outs = _GroupNormActTrain.apply(len(xs), gns[0].num_groups, gns[0].eps, bool(relu), tuple(owner), *xs,
                                    *[d.weight for d in distinct], *[d.bias for d in distinct])
    return list(outs)


def bn_act_train_ok(x, bn):
    """`bn_act_train` takes these: x a contiguous fp32 CUDA [B,C,H,W] tensor with elements, bn an eval-mode nn.BatchNorm2d of C
    channels with fp32 running statistics (and parameters, where it has them)"""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and
            x.numel() > 0):
        return False
    if not (isinstance(bn, torch.nn.BatchNorm2d) and not bn.training and bn.running_var is not None and
            bn.running_mean is not None and bn.num_features == x.size(1)):
        return False
    return all(t is None or (t.dtype == torch.float32 and t.device == x.device)
               for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))


class _BnActTrain(torch.autograd.Function):
    """y = relu?(BatchNorm_eval(x) (+ residual | + BatchNorm2_eval(residual))) with autograd: forward = the inference pass
    (`orp_affine_act` / `orp_affine2_act`) into a new tensor; backward = one pass for grad_x, the residual's gradient and the
    workgroups' partial sums, one small kernel for dweight / dbias (`orp_affine_act_backward` / `orp_affine2_act_backward`).
    Inputs: x, residual | None, bn.weight, bn.bias, residual_bn.weight, residual_bn.bias (None where there is none: autograd sees the
    parameters here), then bn, residual_bn | None, relu."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, weight2, bias2, bn, residual_bn, relu):
        # inside a capture (dist_utils.graph_backbone) the affine of parameters that train is computed in the graph, not cached
        capturing = torch.cuda.is_current_stream_capturing()
        needs = ctx.needs_input_grad
        want1, want2 = bool(needs[2] or needs[3]), bool(needs[4] or needs[5])
        scale, shift, mean, rstd = _bn_affine_stats(bn, cache=not (capturing and want1))
        B, C, H, W = x.shape
        y = torch.empty_like(x)
        head = (_lib.ptr(x), _lib.ptr(residual), _lib.ptr(scale), _lib.ptr(shift))
        tail = (_lib.ptr(y), B, C, H * W, 1 if relu else 0, _lib.stream_of(x))
        keep = [scale, mean, rstd]
        if residual_bn is not None:
            scale2, shift2, mean2, rstd2 = _bn_affine_stats(residual_bn, cache=not (capturing and want2))
            _lib.call("orp_affine2_act", x.device, *head, _lib.ptr(scale2), _lib.ptr(shift2), *tail)
            keep += [scale2, mean2, rstd2]
        else:
            _lib.call("orp_affine_act", x.device, *head, *tail)
        # only what the backward reads: y is the ReLU mask, x / the raw residual feed that BatchNorm's dweight
        ctx.save_for_backward(y if relu else None, x if want1 else None, residual if want2 else None, *keep)
        ctx.meta = (bool(relu), residual_bn is not None, want1, want2)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        relu, two, want1, want2 = ctx.meta
        saved = ctx.saved_tensors
        y, x, x2 = saved[:3]
        scale, mean, rstd = saved[3:6]
        scale2, mean2, rstd2 = saved[6:9] if two else (None, None, None)
        gy = gy.detach().float().contiguous()
        B, C, H, W = gy.shape
        want_res = ctx.needs_input_grad[1]
        gx = torch.empty_like(gy)
        gx2 = torch.empty_like(gy) if (two and want_res) else None
        # without the ReLU the residual's gradient IS grad_y: no copy; with it, a new tensor (a gradient is never written in place)
        gres = torch.empty_like(gy) if (want_res and not two and relu) else None
        dw = torch.empty_like(scale) if want1 else None
        db = torch.empty_like(scale) if want1 else None
        dw2 = torch.empty_like(scale) if want2 else None
        db2 = torch.empty_like(scale) if want2 else None
        ws, nbytes = None, 0
        if want1 or want2:
            # torch's allocator, so that a capture of the backward (make_graphed_callables) owns it
            nbytes = _lib.lib().orp_affine_act_backward_workspace_bytes(B, C, H * W)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=gy.device)
        p = _lib.ptr
        dims = (B, C, H * W, p(ws), nbytes, _lib.stream_of(gy))
        if two:
            _lib.call("orp_affine2_act_backward", gy.device, p(gy), p(y), p(x), p(scale), p(mean), p(rstd), p(x2), p(scale2), p(mean2),
                      p(rstd2), p(gx), p(gx2), None, p(dw), p(db), p(dw2), p(db2), *dims)
        else:
            _lib.call("orp_affine_act_backward", gy.device, p(gy), p(y), p(x), p(scale), p(mean), p(rstd), p(gx), p(gres), p(dw), p(db),
                      *dims)
        if two:
            gr = gx2
        else:
            gr = (gres if relu else gy) if want_res else None
        needs = ctx.needs_input_grad
        return (gx, gr, dw if needs[2] else None, db if needs[3] else None, dw2 if needs[4] else None, db2 if needs[5] else None,
                None, None, None)


def bn_act_train(x, bn, residual=None, relu=True, residual_bn=None):
    """relu?(BatchNorm_eval(x) (+ residual)) with autograd, as a NEW tensor: the values of `bn_act` on a copy of x, bit for bit, one pass
    forward; one pass (+ a per-channel reduction where bn.weight / bn.bias require a gradient) backward, giving the gradients of x, of
    the residual and of the BatchNorm's parameters.  residual_bn: the residual is a RAW convolution output with this eval-mode
    BatchNorm applied while it is read (`orp_affine2_act`), whose parameters get their gradients from the same launch.
    x (and the residual): contiguous fp32 CUDA [B,C,H,W]; bn (residual_bn): eval-mode nn.BatchNorm2d.  Anything else -- 16-bit
    tensors under autocast, float64, channels-last, a BatchNorm in training mode -- is a ValueError: the caller keeps the stock route."""
    if not bn_act_train_ok(x, bn):
        raise ValueError("bn_act_train expects a contiguous fp32 CUDA [B,C,H,W] tensor and an eval-mode BatchNorm2d of its channels")
    if residual_bn is not None and residual is None:
        raise ValueError("bn_act_train: residual_bn without a residual")
    if residual is not None and not (isinstance(residual, torch.Tensor) and residual.shape == x.shape and residual.is_cuda and
                                     residual.device == x.device and residual.dtype == torch.float32 and residual.is_contiguous()):
        raise ValueError("bn_act_train: residual must be a contiguous fp32 tensor of x's shape and device")
    if residual_bn is not None and not bn_act_train_ok(residual, residual_bn):
        raise ValueError("bn_act_train: residual_bn must be an eval-mode BatchNorm2d of the residual's channels")
    return _BnActTrain.apply(x, residual, bn.weight, bn.bias, residual_bn.weight if residual_bn is not None else None,
                             residual_bn.bias if residual_bn is not None else None, bn, residual_bn, bool(relu))


# ---- channels-last tower path (round 4): conv_split_multi -> group_norm_act_multi_cl -> ... -----------------------------------

_ConvLevel = _lib.struct("orp_conv_level")


def _is_cl(x):
    """memory is [B, H, W, C] (channels-last strides of the logical [B, C, H, W] tensor)"""
    return x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)


def _ranges_wanted():
    """the library's arithmetic mode is the fp16-pieces one (orp_dcn_get_split_mode() == 3): producers leave their ranges"""
    return _lib.lib().orp_dcn_get_split_mode() == 3


class Amax(object):
    """Device-side range hand-over between a producer and the fp16-pieces convolution that reads its outputs: `bits` is an int32
    CUDA tensor of float bits (upper bounds of max |x| per slot, written by atomicMax), `stride` 0 = both layers of a pair
    launch read slot 0, 1 = layer b reads slot 1.  None anywhere in the chain simply means the convolution takes the maximum
    itself (a pre-pass over its inputs)."""
    __slots__ = ('bits', 'stride', 'count')

    def __new__(cls, bits, stride=0, count=1):
        if bits is None:
            return None
        return object.__new__(cls)

    def __init__(self, bits, stride=0, count=1):
        # count > 1 (conv_split_gn's hand-over): layer k's range is the maximum of `count` words at bits[k * stride]
        self.bits, self.stride, self.count = bits, stride, count


def to_channels_last_multi(xs, amax_slots=None, amax_into=None, force_ranges=False):
    """[x in channels-last memory for x in xs] -- NCHW-contiguous fp32 CUDA tensors [B,C,H,W] with equal B and C, ONE launch
    (`orp_nchw_to_nhwc_multi`); tensors that already are channels-last pass through.
    amax_slots (one slot index per tensor): also returns an int32 tensor with max |x| per slot as float bits, or None when a
    tensor passed through untouched (its range is not known here); amax_into = (bits tensor, slots): accumulate into an
    existing one instead (all tensors of xs must then be converted here or the result is None again)."""
    todo = [i for i, x in enumerate(xs) if not _is_cl(x)]
    outs = list(xs)
    want_amax = amax_slots is not None or amax_into is not None
    ranges = want_amax and (force_ranges or _ranges_wanted())      # (only the fp16-pieces kernels read them)
    if not todo:
        return (outs, None) if want_amax else outs
    x0 = xs[todo[0]]
    B, C = x0.size(0), x0.size(1)
    ins = []
    for i in todo:
        x = xs[i].detach()
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.size(0) == B and x.size(1) == C):
            raise ValueError("to_channels_last_multi expects fp32 CUDA [B,C,H,W] tensors with equal B and C")
        x = x.contiguous()
        ins.append(x)
        outs[i] = torch.empty(x.shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    levels = _norm_levels(ins, [outs[i] for i in todo])
    if ranges and len(todo) == len(xs):
        if amax_into is not None:
            bits, slots_all, reset = amax_into[0], amax_into[1], 0
        else:
            slots_all, reset = list(amax_slots), 1
            bits = torch.empty(max(slots_all) + 1, dtype=torch.int32, device=x0.device)
        slots = (ctypes.c_int * len(todo))(*[int(slots_all[i]) for i in todo])
        _lib.call("orp_nchw_to_nhwc_multi_amax", x0.device, levels, len(todo), B, C, slots, bits.data_ptr(), bits.numel(), reset,
                  _lib.stream_of(x0))
        return outs, bits
    _lib.call("orp_nchw_to_nhwc_multi", x0.device, levels, len(todo), B, C, _lib.stream_of(x0))
    return (outs, None) if want_amax else outs


def conv_split_ok(conv, x=None):
    """the module is a bias-free-or-not kh x kw nn.Conv2d (groups 1, fp32) of a shape `orp_conv_split_multi` takes"""
    w = conv.weight
    ok = (isinstance(conv, torch.nn.Conv2d) and conv.groups == 1 and w.dtype == torch.float32 and w.is_cuda and
          isinstance(conv.padding, tuple) and
          bool(_lib.lib().orp_conv_split_ok(w.size(1), w.size(0), w.size(2), w.size(3))))
    if ok and x is not None:
        ok = x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.size(1) == w.size(1)
    return ok


def conv_split_set_halo(on):
    """The halo kernel of the 3x3 stride-1 fp16-pieces convolutions on (1) / off (0: the linear-tile kernel) / -1: back to the
    default (ORP_CONV_HALO, 1).  A captured graph keeps the kernel it was captured with."""
    _lib.check(_lib.lib().orp_conv_split_set_halo(int(on)), "orp_conv_split_set_halo")


def conv_split_halo_tile(sizes, batch, cin, cout, kh=3, kw=3, stride=1, pad=1, dil=1, nprod=3):
    """[(th, tw)] per level of the sizes [(H, W)] when a convolution launch of these arguments runs the halo kernel, else None
    (`orp_conv_split_halo_tile`)."""
    n = len(sizes)
    levels = (_ConvLevel * n)()
    for i, (h, w) in enumerate(sizes):
        levels[i] = _ConvLevel(None, None, None, None, int(h), int(w))
    th, tw = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    if not _lib.lib().orp_conv_split_halo_tile(levels, n, int(batch), int(cin), int(cout), kh, kw, stride, pad, dil, int(nprod), th, tw):
        return None
    return [(th[i], tw[i]) for i in range(n)]


def conv_split_weights(xs_a, weights_a, xs_b=None, weight_b=None, biases_a=None, bias_b=None, stride=(1, 1), padding=(1, 1),
                       dilation=(1, 1), relu=False, out_channels_last=True, nprod=None, cache_pack=True, amax=None):
    """The launch behind conv_split_multi, on tensors: weights_a = one [Cout,Cin,kh,kw] weight for all of xs_a, or a list with
    one weight per tensor (then no second layer); cache_pack=False re-packs the weights on every call (training: the
    optimizer writes them between calls); amax: an `Amax` from the producer of the inputs (fp16-pieces mode: no range
    pre-pass), or None."""
    from .deform_conv import _packed_weight
    L = _lib.lib()
    pair = xs_b is not None
    per_level = list(weights_a) if isinstance(weights_a, (list, tuple)) else None
    w = per_level[0] if per_level is not None else weights_a
    cout, cin, kh, kw = w.shape
    if per_level is not None and (pair or len(per_level) != len(xs_a) or any(tuple(t.shape) != tuple(w.shape) for t in per_level)):
        raise ValueError("conv_split: one weight per tensor, equal shapes, no second layer")
    if pair and (tuple(weight_b.shape) != tuple(w.shape) or len(xs_b) != len(xs_a)):
        raise ValueError("conv_split: the two layers must have equal shapes")
    if nprod is None:
        nprod = L.orp_dcn_get_split_mode() or 6
    x0 = xs_a[0]
    B = x0.size(0)
    n = len(xs_a)
    levels = (_ConvLevel * n)()
    keep, outs_a, outs_b = [], [], []
    st, pd, dl = tuple(stride), tuple(padding), tuple(dilation)
    fmt = torch.channels_last if out_channels_last else torch.contiguous_format
    for i in range(n):
        xa = xs_a[i].detach()
        xb = xs_b[i].detach() if pair else None
        for x in (xa, xb):
            if x is None:
                continue
            if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.size(0) == B and x.size(1) == cin and _is_cl(x)):
                raise ValueError("conv_split expects channels-last fp32 CUDA [B,%d,H,W] tensors" % cin)
            if xb is not None and x.shape != xa.shape:
                raise ValueError("conv_split: the two layers' inputs must have equal shapes")
        H, W = xa.size(2), xa.size(3)
        ho = (H + 2 * pd[0] - (dl[0] * (kh - 1) + 1)) // st[0] + 1
        wo = (W + 2 * pd[1] - (dl[1] * (kw - 1) + 1)) // st[1] + 1
        oa = torch.empty((B, cout, ho, wo), dtype=torch.float32, device=xa.device, memory_format=fmt)
        ob = torch.empty((B, cout, ho, wo), dtype=torch.float32, device=xa.device, memory_format=fmt) if pair else None
        keep += [xa, xb]; outs_a.append(oa); outs_b.append(ob)
        levels[i] = _ConvLevel(xa.data_ptr(), xb.data_ptr() if pair else None, oa.data_ptr(), ob.data_ptr() if pair else None, H, W)

    def f32(t):
        return t.detach().float().contiguous() if t is not None else None
    ws = _lib.workspace(x0.device, 256)                    # nprod = 3: max |x| of the inputs (a pre-pass writes it there)
    am_ptr = amax.bits.data_ptr() if amax is not None else None
    am_stride = int(amax.stride) if amax is not None else 0
    keep.append(amax.bits if amax is not None else None)
    if per_level is not None:
        wts = (ctypes.c_void_p * n)()
        bs = (ctypes.c_void_p * n)()
        for i, wt in enumerate(per_level):
            pk = _packed_weight(wt, cache_pack)
            bi = f32(biases_a[i]) if biases_a is not None else None
            keep += [pk, bi]
            wts[i] = pk.data_ptr()
            bs[i] = bi.data_ptr() if bi is not None else None
        _lib.call("orp_conv_split_multi_ex", x0.device, levels, wts, bs, n, B, cin, cout, 1 if relu else 0, kh, kw, st[0], st[1], pd[0],
                  pd[1], dl[0], dl[1], 1 if out_channels_last else 0, int(nprod), _lib.ptr(ws), ws.numel(), am_ptr, _lib.stream_of(x0))
        return outs_a
    pa = _packed_weight(w, cache_pack)
    pb = _packed_weight(weight_b, cache_pack) if pair else None
    ba, bb = f32(biases_a), f32(bias_b) if pair else None
    _lib.call("orp_conv_split_multi", x0.device, levels, n, B, cin, cout, _lib.ptr(pa), _lib.ptr(pb), _lib.ptr(ba), _lib.ptr(bb),
              1 if relu else 0, kh, kw, st[0], st[1], pd[0], pd[1], dl[0], dl[1], 1 if out_channels_last else 0, int(nprod),
              _lib.ptr(ws), ws.numel(), am_ptr, am_stride, _lib.stream_of(x0))
    return (outs_a, outs_b) if pair else outs_a


def conv_split_multi(xs_a, conv_a, xs_b=None, conv_b=None, bias=False, relu=False, out_channels_last=True, nprod=None, amax=None):
    """[conv_a(x) for x in xs_a] (and [conv_b(x) for x in xs_b]: two layers of equal shape in ONE launch -- the two towers'
    layer k) over all FPN levels, `orp_conv_split_multi`: fp32 on the bf16 matrix pipe with every operand split exactly
    into three bf16 pieces, fp32 accumulation.  xs_*: channels-last fp32 CUDA tensors (logical [B,C,H,W]); conv_a: one
    nn.Conv2d for all tensors, or a list with one per tensor (the FPN's output convolutions; no second layer then); bias=True
    adds the modules' biases in the epilogue, relu fuses the activation; outputs channels-last or NCHW.  No autograd
    (training: conv_split_train).  nprod: 6 | 9 partial products (None: the library's DeformConv split mode, 6 when off)."""
    per_level = list(conv_a) if isinstance(conv_a, (list, tuple)) else None
    c0 = per_level[0] if per_level is not None else conv_a
    mods = (per_level or [c0]) + ([conv_b] if conv_b is not None else [])
    if any(c.stride != c0.stride or c.padding != c0.padding or c.dilation != c0.dilation for c in mods):
        raise ValueError("conv_split_multi: equal strides / paddings / dilations")
    if per_level is not None:
        return conv_split_weights(xs_a, [c.weight for c in per_level], None, None,
                                  [c.bias for c in per_level] if bias else None, None, c0.stride, c0.padding, c0.dilation,
                                  relu, out_channels_last, nprod, amax=amax)
    return conv_split_weights(xs_a, c0.weight, xs_b, conv_b.weight if conv_b is not None else None,
                              c0.bias if bias else None, conv_b.bias if (bias and conv_b is not None) else None,
                              c0.stride, c0.padding, c0.dilation, relu, out_channels_last, nprod, amax=amax)


def conv_split_gn_ok(conv_a, conv_b, gn_a, gn_b, x):
    """the two towers' layer k can run as `conv_split_gn`: stride-1 'same' bias-free convolutions of one shape that
    orp_conv_split_multi takes, at most 512 input channels, affine GroupNorms with equal groups / eps whose group size divides 32"""
    import torch.nn as nn
    for c in (conv_a, conv_b):
        if not (conv_split_ok(c, x) and c.bias is None and tuple(c.stride) == (1, 1) and c.weight.size(1) <= 512 and
                tuple(c.weight.shape) == tuple(conv_a.weight.shape) and c.padding == conv_a.padding and c.dilation == conv_a.dilation and
                2 * c.padding[0] == c.dilation[0] * (c.weight.size(2) - 1) and 2 * c.padding[1] == c.dilation[1] * (c.weight.size(3) - 1)):
            return False
    cout = conv_a.weight.size(0)
    for g in (gn_a, gn_b):
        if not (isinstance(g, nn.GroupNorm) and g.affine and g.num_groups == gn_a.num_groups and g.eps == gn_a.eps and
                g.num_channels == cout and cout % g.num_groups == 0 and 32 % (cout // g.num_groups) == 0 and 1024 % cout == 0):
            return False
    return True


def conv_split_gn(xs_a, conv_a, xs_b, conv_b, gn_a, gn_b, coef_in=None, amax=None, nprod=None, materialize=False):
    """One layer of BOTH towers -- conv -> GroupNorm -> ReLU over all FPN levels (reference head :91-113, ConvModule) -- with the
    normalisation fused AROUND the convolution launch (`orp_conv_split_multi_gn`): the statistics leave the convolution's epilogue
    per tile, `orp_conv_split_gn_finish` merges them into per-(tensor, image, channel) coefficients (a, b), and the NEXT layer
    applies relu(x a + b) while it reads.  xs_*: channels-last fp32 tensors; coef_in: the previous layer's coefficients (None: the
    inputs are taken as they are).  Returns (outs_a, outs_b, coef, amax): RAW convolution outputs + their coefficients -- or, with
    materialize=True (the towers' last layer), the normalised + ReLU'd outputs (in place) and coef None.  amax: `Amax` of the
    normalised outputs for the fp16-pieces arithmetic (None in the other modes)."""
    from .deform_conv import _packed_weight
    L = _lib.lib()
    n = len(xs_a)
    w = conv_a.weight
    cout, cin, kh, kw = w.shape
    if nprod is None:
        nprod = L.orp_dcn_get_split_mode() or 6
    x0 = xs_a[0]
    B = x0.size(0)
    levels = (_ConvLevel * n)()
    outs_a, outs_b, keep = [], [], []
    for i in range(n):
        xa, xb = xs_a[i].detach(), xs_b[i].detach()
        for x in (xa, xb):
            if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.size(0) == B and x.size(1) == cin and _is_cl(x) and
                    x.shape == xa.shape):
                raise ValueError("conv_split_gn expects channels-last fp32 CUDA [B,%d,H,W] tensors" % cin)
        H, W = xa.size(2), xa.size(3)
        oa = torch.empty((B, cout, H, W), dtype=torch.float32, device=xa.device, memory_format=torch.channels_last)
        ob = torch.empty((B, cout, H, W), dtype=torch.float32, device=xa.device, memory_format=torch.channels_last)
        keep += [xa, xb]; outs_a.append(oa); outs_b.append(ob)
        levels[i] = _ConvLevel(xa.data_ptr(), xb.data_ptr(), oa.data_ptr(), ob.data_ptr(), H, W)
    G = gn_a.num_groups
    pf = int(L.orp_conv_split_gn_partial_floats(levels, n, B, G, 2))
    partials = torch.empty((pf,), dtype=torch.float32, device=x0.device)
    ws = _lib.workspace(x0.device, 256)
    pa, pb = _packed_weight(conv_a.weight), _packed_weight(conv_b.weight)
    am_ptr = amax.bits.data_ptr() if amax is not None else None
    pd, dl = conv_a.padding, conv_a.dilation
    _lib.call("orp_conv_split_multi_gn", x0.device, levels, n, B, cin, cout, _lib.ptr(pa), _lib.ptr(pb), kh, kw, pd[0], pd[1], dl[0],
              dl[1], int(nprod), _lib.ptr(coef_in), 1, _lib.ptr(partials), pf, G, _lib.ptr(ws), ws.numel(), am_ptr,
              int(amax.stride) if amax is not None else 0, int(amax.count) if amax is not None else 0, _lib.stream_of(x0))
    coef = torch.empty((2 * n, B, cout, 2), dtype=torch.float32, device=x0.device)
    ranges = _ranges_wanted()
    per_set = n * B * G
    bound = torch.empty((2, per_set), dtype=torch.int32, device=x0.device) if ranges else None
    gam, bet, _gs, _bs = _affine_ptrs((gn_a, gn_b), [0] * n + [1] * n)
    _lib.call("orp_conv_split_gn_finish", x0.device, levels, n, B, cout, G, 2, float(gn_a.eps), gam, bet, _lib.ptr(partials),
              _lib.ptr(coef), bound.data_ptr() if bound is not None else None, _lib.stream_of(x0))
    if not materialize:
        return outs_a, outs_b, coef, (Amax(bound, per_set, per_set) if bound is not None else None)
    nl = _norm_levels(outs_a + outs_b, outs_a + outs_b)
    slots = torch.empty((2,), dtype=torch.int32, device=x0.device) if bound is not None else None
    _lib.call("orp_affine_act_multi_cl", x0.device, nl, 2 * n, B, cout, _lib.ptr(coef), 1,
              bound.data_ptr() if bound is not None else None, 2, per_set, slots.data_ptr() if slots is not None else None,
              _lib.stream_of(x0))
    return outs_a, outs_b, None, (Amax(slots, 1) if slots is not None else None)


_WgradLevel = _lib.struct("orp_wgrad_level")


def conv_wgrad_split_ok(weight, padding, dilation):
    cout, cin, kh, kw = weight.shape
    return (bool(_lib.lib().orp_conv_wgrad_split_ok(cin, cout, kh, kw)) and weight.is_cuda and weight.dtype == torch.float32 and
            2 * padding[0] == dilation[0] * (kh - 1) and 2 * padding[1] == dilation[1] * (kw - 1))


def conv_wgrad_split(xs, grad_outs, weight_shape, padding=(1, 1), dilation=(1, 1), amax_x=None, amax_g=None):
    """grad_weight [Cout,Cin,kh,kw] of a stride-1 'same' 256 -> 256 convolution summed over a list of (input, grad_output) pairs
    (the FPN levels of one layer), `orp_conv_wgrad_split`: NCHW fp32 CUDA tensors, ONE launch, fixed summation order.
    amax_x / amax_g: one-element int32 tensors (float bits of an upper bound of max |input| / max |grad_output|), or None."""
    L = _lib.lib()
    cout, cin, kh, kw = weight_shape
    x0 = xs[0]
    B = x0.size(0)
    n = len(xs)
    levels = (_WgradLevel * n)()
    keep = []
    for i in range(n):
        x, g = xs[i].detach().float().contiguous(), grad_outs[i].detach().float().contiguous()
        if not (x.is_cuda and x.dim() == 4 and x.size(0) == B and x.size(1) == cin and tuple(g.shape) == (B, cout, x.size(2), x.size(3))):
            raise ValueError("conv_wgrad_split expects NCHW fp32 CUDA inputs [B,%d,H,W] and grad_outputs [B,%d,H,W]" % (cin, cout))
        keep += [x, g]
        levels[i] = _WgradLevel(x.data_ptr(), g.data_ptr(), x.size(2), x.size(3))
    gw = torch.empty((cout, cin, kh, kw), dtype=torch.float32, device=x0.device)
    nbytes = L.orp_conv_wgrad_split_workspace_bytes(levels, n, B, kh, kw)
    ws = _lib.workspace(x0.device, nbytes)
    have = amax_x is not None and amax_g is not None
    _lib.call("orp_conv_wgrad_split", x0.device, levels, n, B, cin, cout, kh, kw, padding[0], padding[1], dilation[0], dilation[1],
              amax_x.data_ptr() if have else None, amax_g.data_ptr() if have else None, gw.data_ptr(), _lib.ptr(ws), ws.numel(),
              _lib.stream_of(x0))
    return gw


class _ConvSplitTrain(torch.autograd.Function):
    """ys = [conv(x, W_k)] for the levels of one tower layer (or of the two towers' layer k, or of the FPN's output
    convolutions with a weight per level) as ONE autograd node on the bf16-split kernel.  forward: inputs transposed to
    channels-last in one launch, one convolution launch writing NCHW.  backward: grad_input = the same kernel on the
    transposed grad_outputs with the flipped, transposed weights (stride 1: correlation with W[o][c][kh-1-i][kw-1-j] as
    [c][o], padding dil*(k-1) - pad); grad_weight = the library's weight-gradient kernel per level on the channels-last
    tensors (torch.ops.aten.convolution_backward), summed over the levels that share a weight."""

    @staticmethod
    def forward(ctx, meta, *tensors):
        n, nw, groups, padding, dilation = meta             # n inputs, nw weights, groups[i] = weight index of input i
        ws, xs = tensors[:nw], tensors[nw:]
        def key(x):                                           # the towers' first layer reads the same FPN output twice
            return (x.data_ptr(), tuple(x.shape), tuple(x.stride()))
        seen = {}
        for x in xs:
            seen.setdefault(key(x), len(seen))
        uniq = [None] * len(seen)
        for x in xs:
            uniq[seen[key(x)]] = x
        # the transposition also leaves max |x| (fp16-pieces mode: no range pre-pass in the convolution): one slot per layer
        # of a pair launch -- or one for everything when the two layers read the same tensors
        pair = nw == 2 and n % 2 == 0 and list(groups) == [0] * (n // 2) + [1] * (n // 2)
        split_slots = pair and len(uniq) == n
        slots = [(1 if (split_slots and i >= n // 2) else 0) for i in range(len(uniq))]
        uniq_cl, bits = to_channels_last_multi([u.detach().float() for u in uniq], amax_slots=slots, force_ranges=True)
        cl = [uniq_cl[seen[key(x)]] for x in xs]
        amax = Amax(bits, 1 if split_slots else 0) if bits is not None else None
        outs = _ConvSplitTrain._run(cl, ws, groups, padding, dilation, nw, amax)
        ctx.meta = meta
        ctx.x_bits = (bits, split_slots)                      # ranges of the inputs, for the weight-gradient kernel
        # the weight gradient reads ONE copy of the inputs: NCHW for the layers that take orp_conv_wgrad_split, channels-last for
        # the library's kernel -- only what the chosen routes need is kept (both copies doubled the saved activations)
        routes = [_ConvSplitTrain._wgrad_split_route(ws[k], [i for i in range(n) if groups[i] == k], padding, dilation) for k in range(nw)]
        ctx.routes = tuple(routes)
        keep_cl = cl if not all(routes) else []
        keep_x = [x.detach() for x in xs] if any(routes) else []
        ctx.kept = (len(keep_cl), len(keep_x))
        ctx.save_for_backward(*ws, *keep_cl, *keep_x)
        return tuple(outs)

    @staticmethod
    def _wgrad_split_route(w, idx, padding, dilation):
        return len(idx) <= 8 and conv_wgrad_split_ok(w, padding, dilation)

    @staticmethod
    def _run(cl, ws, groups, padding, dilation, nw, amax=None):
        """one launch: a single weight, two weights (pair: first / second half of the tensors), or one weight per tensor"""
        n = len(cl)
        if nw == 1:
            return conv_split_weights(cl, ws[0], padding=padding, dilation=dilation, out_channels_last=False, cache_pack=False,
                                      amax=amax)
        if nw == 2 and n % 2 == 0 and list(groups) == [0] * (n // 2) + [1] * (n // 2):
            a, b = conv_split_weights(cl[:n // 2], ws[0], cl[n // 2:], ws[1], padding=padding, dilation=dilation,
                                      out_channels_last=False, cache_pack=False, amax=amax)
            return a + b
        if amax is not None and amax.stride != 0:
            amax = None                                      # (a layer per tensor reads one slot for all of them)
        return conv_split_weights(cl, [ws[g] for g in groups], padding=padding, dilation=dilation, out_channels_last=False,
                                  cache_pack=False, amax=amax)

    @staticmethod
    def backward(ctx, *grads):
        n, nw, groups, padding, dilation = ctx.meta
        saved = ctx.saved_tensors
        ncl, nx = ctx.kept
        ws, cl, xs_nchw = saved[:nw], saved[nw:nw + ncl], saved[nw + ncl:nw + ncl + nx]
        kh, kw = ws[0].size(2), ws[0].size(3)
        pair = nw == 2 and n % 2 == 0 and list(groups) == [0] * (n // 2) + [1] * (n // 2)
        g_cl, bits = to_channels_last_multi([g.detach().float() for g in grads],
                                            amax_slots=[(1 if (pair and i >= n // 2) else 0) for i in range(n)], force_ranges=True)
        gxs = [None] * n
        if any(ctx.needs_input_grad[1 + nw:]):
            wt = [w.detach().flip(2, 3).transpose(0, 1).contiguous() for w in ws]
            pad_t = (dilation[0] * (kh - 1) - padding[0], dilation[1] * (kw - 1) - padding[1])
            gxs = _ConvSplitTrain._run(g_cl, wt, groups, pad_t, dilation, nw,
                                       Amax(bits, 1 if pair else 0) if bits is not None else None)
        gws = [None] * nw
        for k in range(nw):
            if not ctx.needs_input_grad[1 + k]:
                continue
            idx = [i for i in range(n) if groups[i] == k]
            if ctx.routes[k]:
                # one launch for the layer's levels, straight from the NCHW tensors (positions = the contraction axis)
                xb, x_split = ctx.x_bits
                sx = 1 if (x_split and idx[0] >= n // 2) else 0
                sg = 1 if (pair and idx[0] >= n // 2) else 0
                have = xb is not None and bits is not None
                gws[k] = conv_wgrad_split([xs_nchw[i] for i in idx], [grads[i] for i in idx], tuple(ws[k].shape), padding, dilation,
                                          xb[sx:sx + 1] if have else None, bits[sg:sg + 1] if have else None)
                continue
            acc = None
            for i in idx:
                gw = torch.ops.aten.convolution_backward(g_cl[i], cl[i], ws[k], None, [1, 1], list(padding), list(dilation), False,
                                                         [0, 0], 1, [False, True, False])[1]
                acc = gw if acc is None else acc + gw
            gws[k] = acc
        return (None, *gws, *gxs)


def conv_split_train_ok(convs, x, allow_bias=False):
    """the modules' convolutions can run as a conv_split_train node: split mode on (ORP_TRAIN_SPLIT=0 switches the training
    route off for A/B timing), no autocast, stride 1, fp32 nn.Conv2d of one shape that `orp_conv_split_multi` takes (bias-free
    unless the caller adds the bias itself), fp32 CUDA input"""
    from .. import switches
    if not switches.TRAIN_SPLIT or _lib.lib().orp_dcn_get_split_mode() == 0 or torch.is_autocast_enabled():
        return False
    c0 = convs[0]
    for c in convs:
        if not (conv_split_ok(c, x) and (allow_bias or c.bias is None) and tuple(c.stride) == (1, 1) and tuple(c.weight.shape) == tuple(c0.weight.shape)
                and c.padding == c0.padding and c.dilation == c0.dilation and c.weight.size(0) % 64 == 0 and c.weight.size(1) % 64 == 0
                and c.dilation[0] * (c.weight.size(2) - 1) >= c.padding[0] and c.dilation[1] * (c.weight.size(3) - 1) >= c.padding[1]):
            return False
    return True


def conv_split_train(xs, convs):
    """[convs[i](x_i)] with autograd as one node; xs: NCHW fp32 CUDA tensors (up to 8 per distinct layer in a pair / single
    launch, see _ConvSplitTrain._run), convs: one module, or a list with one module per tensor (tensors sharing a module are
    one layer).  Layouts a launch takes: all tensors one layer; first half / second half two layers (the two towers' layer
    k); a layer per tensor (the FPN)."""
    convs = list(convs) if isinstance(convs, (list, tuple)) else [convs] * len(xs)
    order, groups = {}, []
    for c in convs:
        if id(c) not in order:
            order[id(c)] = len(order)
        groups.append(order[id(c)])
    mods = [None] * len(order)
    for c in convs:
        mods[order[id(c)]] = c
    c0 = mods[0]
    meta = (len(xs), len(mods), tuple(groups), tuple(c0.padding), tuple(c0.dilation))
    return list(_ConvSplitTrain.apply(meta, *[m.weight for m in mods], *xs))
