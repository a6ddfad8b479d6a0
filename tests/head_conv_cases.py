"""Helper of the head / FPN plain-convolution tests (not a conftest, no tests in here): exact-arithmetic cases, random cases and
float64 references in plain torch for three inference kernels --
  * the small-level 3x3 convolution (csrc/orp_conv_small.hip, through fused_norm.conv3x3_multi),
  * the head's 1x1 output convolution with its epilogue (csrc/orp_conv1x1.hip, through fused_norm.conv1x1_multi),
  * both DeformConvs + ReLU + the 1x1 heads in one launch (the HEADS instantiation of csrc/orp_dcn.hip, through
    deform_conv.deform_conv_forward_pair_heads).

The idea, as in tests/dcn_half_cases.py.  With small-integer features and weights (and, for the DeformConvs, offsets whose
fractional part is 0 or 1/2), biases and `sub` values that are multiples of 1/8 and integer residuals, every term of every sum is
a multiple of one unit (1/8) and the sum of the terms' MAGNITUDES stays below 2^24 units at every output.  Then every partial sum,
in any order and with or without fused multiply-adds, is an fp32 number: nothing rounds, and the expected bits are the float64
result's .float().  tests/test_head_conv_cases.py asserts these premises (and that a case is not vacuous) on the generated data
without a GPU; tests/test_gpu_head_convs_exact.py runs the kernels.

Nothing here calls an orp_* entry point."""
import collections
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_half_cases as D  # noqa: E402

X_MAX, W_MAX = 15, 7                     # |x| <= 15, |w| <= 7: 9 * 2048 * 105 < 2^24
UNIT = 1.0 / 8                           # biases and `sub` are multiples of it
LIMIT = 2.0 ** 24 * UNIT                 # sum of magnitudes an exact case must stay below, at every output
BATCHES = (1, 2, 3)


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _ints(g, bound, shape):
    """float64 integers in [-bound, bound]"""
    return torch.randint(-bound, bound + 1, tuple(shape), generator=g).double()


def _eighths(g, bound, shape):
    """float64 multiples of 1/8 in [-bound, bound]"""
    return torch.randint(-8 * bound, 8 * bound + 1, tuple(shape), generator=g).double() / 8


def conv64(x, w, stride=1, magnitudes=False):
    """The convolution (k x k, pad k // 2, no bias) in float64 by columns and a matrix product, on x's device: [B, Cout, Ho, Wo].
    magnitudes: of |x| and |w| -- sum_k |x_k w_k| at every output."""
    import torch.nn.functional as F
    xd, wd = x.double(), w.double().to(x.device)
    if magnitudes:
        xd, wd = xd.abs(), wd.abs()
    B, _, H, W = xd.shape
    k = wd.size(2)
    if k == 1 and stride == 1:
        return torch.einsum('oc,bchw->bohw', wd.flatten(1), xd)
    ho, wo = out_hw(H, W, stride)
    cols = F.unfold(xd, (k, k), 1, k // 2, stride)
    return torch.einsum('ok,bkl->bol', wd.flatten(1), cols).reshape(B, wd.size(0), ho, wo)


def same_bits(a, b):
    """fp32 tensors of equal shape and equal BITS (0.0 and -0.0 differ, NaNs compare by payload)"""
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and \
        torch.equal(a.contiguous().reshape(-1).view(torch.int32), b.contiguous().reshape(-1).view(torch.int32))


def is_fp32(t):
    return bool((t.float().double() == t).all())


def straddling_tiles(batch, per_image, rows):
    """Number of `rows`-position tiles of one level ([batch * per_image] positions, tiles counted from the level's first position) that
    hold positions of two or more images."""
    n = 0
    for t in range(-(-batch * per_image // rows)):
        first, last = t * rows, min(t * rows + rows, batch * per_image) - 1
        n += first // per_image != last // per_image
    return n


# ---- the small-level 3x3 convolution ------------------------------------------------------------------------------------------------
SMALL_LEVEL_POSITIONS = 1024             # fused_norm.SMALL_LEVEL_POSITIONS (the GPU test asserts that the two agree)
TILE_POSITIONS = 32                      # positions of one workgroup of the kernel

Conv3 = collections.namedtuple("Conv3", "name cin cout stride split_k seed")
CONV3_CASES = [
    Conv3("c128_64", 128, 64, 1, False, 301),            # 18 chunks per wave: every wave's K slice spans two taps
    Conv3("c256_256", 256, 256, 1, False, 302),          # the towers
    Conv3("c384_64", 384, 64, 1, False, 303),
    Conv3("c128_192", 128, 192, 1, False, 304),          # three N blocks
    Conv3("c2048_256_s2_split", 2048, 256, 2, True, 305),    # P6: 8 K slices at one 32 x 32 image
    Conv3("c256_256_s2_split", 256, 256, 2, True, 306),      # P7: 2 slices
    Conv3("c256_128_s2", 256, 128, 2, False, 307),
]
CONV3_BY_NAME = {c.name: c for c in CONV3_CASES}
LEVELS_S1 = ((1, 1), (1, 2), (1, 31), (1, 32), (1, 33), (3, 3), (5, 7))
LEVELS_EDGE = ((31, 33), (32, 32), (25, 41))             # 1023, 1024 and 1025 positions: the last one stays on the library
LEVELS_S2 = ((31, 17), (32, 32), (16, 16), (2, 5), (1, 1))
LEVELS_P6 = ((32, 32),)
LEVELS_THIN = ((5, 1), (1, 5))                           # one-pixel axes: the window classes the sets above cannot reach


def conv3_level_sets(case):
    return (LEVELS_S1, LEVELS_EDGE, LEVELS_THIN) if case.stride == 1 else (LEVELS_S2, LEVELS_P6, LEVELS_THIN)


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def routed_small(levels):
    """indices of the levels conv3x3_multi hands to the HIP launch"""
    return [i for i, (h, w) in enumerate(levels) if h * w <= SMALL_LEVEL_POSITIONS]


def conv3_weight(case, salt=0):
    """[Cout, Cin, 3, 3] float64 integers, |w| <= 7"""
    return _ints(_gen(case.seed * 100 + salt), W_MAX, (case.cout, case.cin, 3, 3))


def conv3_inputs(cin, levels, batch, seed):
    """one [batch, cin, H, W] float64 integer tensor per level, |x| <= 15"""
    g = _gen(seed)
    return [_ints(g, X_MAX, (batch, cin, h, w)) for h, w in levels]


def window_classes(h, w, stride):
    """{(row class, column class)} over the outputs of one level: which rows / columns of the 3 x 3 window lie in the padding --
    'in' (none), 'low' (the first), 'high' (the last), 'both' (a 1-pixel axis)."""
    def axis(n):
        out = set()
        for o in range((n - 1) // stride + 1):
            low, high = o * stride - 1 < 0, o * stride + 1 >= n
            out.add('both' if low and high else 'low' if low else 'high' if high else 'in')
        return out
    return {(r, c) for r in axis(h) for c in axis(w)}


ALL_WINDOW_CLASSES = {(r, c) for r in ('in', 'low', 'high', 'both') for c in ('in', 'low', 'high', 'both')}


def ksplit_of(levels, strides, batch, cin, cout, slices_that_fit=16):
    """The number of grid-level K slices of a launch WITH a workspace, after the rule in csrc/orp_conv_small.hip (pick_ksplit and the
    launcher's `while`): the largest power of two <= 16 that keeps an even number >= 4 of 8-channel chunks per wave, at most 320
    workgroups, and the partial images inside the workspace.  Documentation of what a case is built to reach; the launcher has no
    query for it."""
    tiles = sum(-(-batch * out_hw(h, w, s)[0] * out_hw(h, w, s)[1] // TILE_POSITIONS) for (h, w), s in zip(levels, strides))
    chunks, best, s = 9 * (cin // 8), 1, 2
    while s <= 16:
        per_wave = chunks // (8 * s)
        if chunks % (8 * s) or per_wave % 2 or per_wave < 4 or tiles * (cout // 64) * s > 320:
            break
        best, s = s, 2 * s
    while best > 1 and slices_that_fit < best:
        best //= 2
    return best


# ---- the 1x1 output convolution -------------------------------------------------------------------------------------------------------
CONV1_CINS = (8, 256, 264)               # Cin / 8 channels per wave: 1, 32 and 33 (no multiple of the unroll of 8)
CONV1_COUTS = (1, 15, 16, 17, 18, 19, 32)    # the kernel's templates hold 16, 18 and 32 accumulators
CONV1_LEVELS = ((1, 1), (7, 9), (8, 8), (5, 13), (37, 41))          # hw = 1, 63, 64, 65, 1517: 64 positions per workgroup
CONV1_LEVELS8 = CONV1_LEVELS + ((2, 3), (16, 16), (1, 129))         # kMaxLevels of this kernel
CONV1_BATCHES = (1, 3)
CONV1_FORMS = [(b, r, a, s) for b in (False, True) for r in (False, True) for a in (False, True) for s in (False, True)]


def conv1_data(cin, cout, levels, batch, seed):
    """dict(xs, weight [Cout, Cin, 1, 1], bias [Cout], sub [Cout], residuals), float64: integer x (|x| <= 15), w (|w| <= 7) and
    residuals (|r| <= 15), bias and sub multiples of 1/8 up to 15"""
    g = _gen(seed)
    return dict(xs=[_ints(g, X_MAX, (batch, cin, h, w)) for h, w in levels], weight=_ints(g, W_MAX, (cout, cin, 1, 1)),
                bias=_eighths(g, 15, (cout,)), sub=_eighths(g, 15, (cout,)),
                residuals=[_ints(g, X_MAX, (batch, cout, h, w)) for h, w in levels])


def conv1_reference(x, weight, bias=None, residual=None, relu=False, sub=None):
    """(y, z) in float64 in the head's order: convolution, + bias, + residual, ReLU; z = y - sub (None without sub)"""
    y = conv64(x, weight)
    if bias is not None:
        y = y + bias.to(y.device).double().view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.double()
    if relu:
        y = y.clamp_min(0.0)
    return y, (y - sub.to(y.device).double().view(1, -1, 1, 1)) if sub is not None else None


def conv1_magnitude(x, weight, bias=None, residual=None):
    """sum_k |x_k w_k| + |b| + |r| at every output, float64"""
    t = conv64(x, weight, magnitudes=True)
    if bias is not None:
        t = t + bias.to(t.device).double().abs().view(1, -1, 1, 1)
    if residual is not None:
        t = t + residual.double().abs()
    return t


# ---- both DeformConvs + ReLU + the 1x1 heads ----------------------------------------------------------------------------------------
# dcn: a dcn_half_cases.Case (256 -> 256, 3 x 3, ReLU, no modulation, |x| <= 3); its `rows` is what the library's tile-height query
# answers for the launch (32 * pick_tile_rows).  rows: the tile height the HEADS launch runs -- it has no 32-row instantiation and
# raises 32 to 64.
HeadsCase = collections.namedtuple("HeadsCase", "name dcn rows")


def _h(name, levels, batch, seed, query_rows, rows):
    return HeadsCase(name, D._c("heads_" + name, levels, batch=batch, relu=True, x_max=3, seed=seed, rows=query_rows), rows)


HEADS_CASES = [
    _h("seams_64", [(21, 19), (8, 8), (3, 5), (1, 1)], 2, 401, 32, 64),        # 958 positions: level seams, levels below one tile
    _h("wide_64", [(89, 97), (5, 5)], 1, 402, 64, 64),                          # 8658 positions
    _h("single_96", [(127, 129)], 1, 403, 96, 96),                              # 16383 positions, 171 tiles, the last one ragged
    _h("multi_96", [(90, 91), (9, 11), (3, 5), (1, 2)], 2, 404, 96, 96),        # 16612 positions: tiles straddle the images
]
HEADS_BY_NAME = {c.name: c for c in HEADS_CASES}
HEAD_KS = ((15, 18), (1, 20), (20, 4))   # (k_a, k_b): the production pair, the edges of the 20-channel pack
HEAD_W_MAX = 3
HEADS_FORMS = [(res, bias) for res in (False, True) for bias in (False, True)]


def heads_generate(hc):
    """dict(xs_a, xs_b, offs, weight_a, weight_b), float64 on the CPU: two layers with their own features and weights over ONE set
    of offsets (steered by dcn_half_cases so that every border class of the sampler occurs)"""
    a = D.generate(hc.dcn)
    b = D.generate(hc.dcn._replace(seed=hc.dcn.seed + 1000))
    return dict(xs_a=a["xs"], xs_b=b["xs"], offs=a["offs"], weight_a=a["weight"], weight_b=b["weight"])


def heads_layers(data):
    """the two layers as dcn_half_cases data dicts"""
    return (dict(xs=data["xs_a"], offs=data["offs"], masks=None, weight=data["weight_a"], bias=None),
            dict(xs=data["xs_b"], offs=data["offs"], masks=None, weight=data["weight_b"], bias=None))


def head_params(k_a, k_b, seed):
    """dict(weight_a [k_a, 256, 1, 1], weight_b, bias_a [k_a], bias_b), float64: integer weights in [-3, 3], biases multiples of 1/8"""
    g = _gen(seed)
    return dict(weight_a=_ints(g, HEAD_W_MAX, (k_a, 256, 1, 1)), weight_b=_ints(g, HEAD_W_MAX, (k_b, 256, 1, 1)),
                bias_a=_eighths(g, 15, (k_a,)), bias_b=_eighths(g, 15, (k_b,)))


def heads_residuals(hc, k_b, seed):
    """one [B, k_b, Ho, Wo] float64 integer tensor per level, |r| <= 15 (the cases are stride 1, pad 1: Ho x Wo = H x W)"""
    g = _gen(seed)
    return [_ints(g, X_MAX, (hc.dcn.batch, k_b, h, w)) for h, w in hc.dcn.levels]


def head64(d, weight, bias=None, residual=None):
    """1x1 head over d = relu(DeformConv(x)) ([B, 256, Ho, Wo] float64): + bias, + residual, float64 on d's device"""
    y = torch.einsum('kc,bchw->bkhw', weight.to(d.device).double().flatten(1), d)
    if bias is not None:
        y = y + bias.to(d.device).double().view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.to(d.device).double()
    return y


def head_magnitude(d, weight, bias=None, residual=None):
    """sum_c relu(d_c) |wh_kc| + |b_k| + |r| at every output (d >= 0 already)"""
    return head64(d, weight.abs(), bias.abs() if bias is not None else None, residual.abs() if residual is not None else None)


_heads_expected = {}


def heads_expected(hc, device):
    """(heads_generate(hc), relu(DeformConv_a) per level, relu(DeformConv_b) per level) in float64 on `device`, computed once per
    case and process and never modified."""
    if hc.name not in _heads_expected:
        data = heads_generate(hc)
        la, lb = heads_layers(data)
        _heads_expected[hc.name] = (data, D.reference(hc.dcn, la, device), D.reference(hc.dcn, lb, device))
    return _heads_expected[hc.name]


# ---- random data ------------------------------------------------------------------------------------------------------------------------
RANDOM_LEVELS = ((13, 16), (3, 5))
RANDOM_BATCH = 2
U = 2.0 ** -24                           # unit roundoff of fp32


def random_conv(cin, cout, k, levels, batch, seed):
    """dict(xs, weight, bias, residuals) as fp32 tensors: N(0, 1) features and residuals, He-scale weights, N(0, 1) bias"""
    g = _gen(seed)
    return dict(xs=[torch.randn((batch, cin, h, w), generator=g) for h, w in levels],
                weight=torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5,
                bias=torch.randn((cout,), generator=g), sub=torch.randn((cout,), generator=g),
                residuals=[torch.randn((batch, cout, h, w), generator=g) for h, w in levels])


def conv3_bound(x, w, stride):
    """(9 Cin + 2) 2^-24 sum |x_k w_k|: 9 Cin products and sums of an fp32 contraction in any order, each one rounding of at most
    2^-24 relative to a partial result that the sum of magnitudes bounds"""
    return (9 * w.size(1) + 2) * U * conv64(x, w, stride, magnitudes=True)


def conv1_bound(x, w, bias, residual):
    """(Cin + 3) 2^-24 (sum |x_k w_k| + |b| + |r|): the chain, the sum of the eight slices, the bias and the residual add"""
    return (w.size(1) + 3) * U * conv1_magnitude(x, w, bias, residual)


RANDOM_HEADS = D._c("heads_random", RANDOM_LEVELS, batch=RANDOM_BATCH, relu=True, seed=501)


def random_heads(seed):
    """dict(xs_a, xs_b, offs, weight_a, weight_b) as fp32 tensors.  Offsets are N(0, 2) rounded to multiples of 2^-8, so that the
    sampling coordinates and the bilinear weights are fp32 numbers and the float64 reference samples at the kernel's coordinates."""
    g = _gen(seed)
    lv, B = RANDOM_LEVELS, RANDOM_BATCH
    he = (2.0 / (9 * 256)) ** 0.5
    return dict(xs_a=[torch.randn((B, 256, h, w), generator=g) for h, w in lv],
                xs_b=[torch.randn((B, 256, h, w), generator=g) for h, w in lv],
                offs=[torch.round(torch.randn((B, 18, h, w), generator=g) * 2.0 * 256) / 256 for h, w in lv],
                weight_a=torch.randn((256, 256, 3, 3), generator=g) * he, weight_b=torch.randn((256, 256, 3, 3), generator=g) * he)


def dcn_magnitude(case, x, off, weight):
    """sum |sample| |w| of the DeformConv at every output, float64 [B, Cout, Ho, Wo] on x's device (bilinear weights are >= 0)"""
    B, Ho, Wo = x.shape[0], off.shape[2], off.shape[3]
    t = torch.zeros((B * Ho * Wo, case.cout), dtype=torch.float64, device=x.device)
    for tap in range(case.kh * case.kw):
        idx, wgt, _, _ = D.tap_samples(case, x, off, None, tap)
        t += D.tap_columns(x.abs(), idx, wgt.abs()) @ weight[:, :, tap // case.kw, tap % case.kw].abs().t()
    return t.reshape(B, Ho, Wo, case.cout).permute(0, 3, 1, 2).contiguous()


def heads_bound(case, x, off, weight, d, head_w, head_b, residual):
    """sum_c |wh_kc| e_c + (256 + 3) 2^-24 (sum_c relu(d_c) |wh_kc| + |b_k| + |r|), with e_c = (9 * 256 + 2) 2^-24 sum |sample w|
    the DeformConv's own bound; ReLU does not enlarge a difference.  All arguments float64 on one device."""
    e = (9 * 256 + 2) * U * dcn_magnitude(case, x, off, weight)
    return head64(e, head_w.abs()) + (256 + 3) * U * head_magnitude(d, head_w, head_b, residual)
