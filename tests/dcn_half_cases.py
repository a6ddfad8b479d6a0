"""Helper of the half DeformConv tests (not a conftest, no tests in here): exact-arithmetic cases for the fp16 / bf16 forward
(csrc/orp_dcn_half.hip) and a float64 reference of the operator written in plain torch indexing.

The idea.  With small-integer features and weights, offsets whose fractional part is 0 or 1/2 and a few dyadic modulation
values, NOTHING in the operator rounds before the final conversion to the storage type T:
  * every bilinear weight is in {0, 1/4, 1/2, 1}, times a mask in {0, 1/2, 1, 3/2}: a multiple of 1/8, exact in fp16;
  * every product weight x neighbour and every sum of such products, in any order, is a multiple of 2^x_exp / 8 of magnitude
    below 256 of those units: 8 significand bits, exact in bf16 AND fp16 (so the fp16 kernel's packed half combine and the
    bf16 kernel's fp32 combine must both be exact);
  * every partial sum of the contraction is a multiple of 2^(x_exp + w_exp) / 8 below 2^24 of those units: exact in fp32 in any
    order.
So the expected output is the float64 result converted once with torch.Tensor.to(T) (round to nearest even), and the kernel must
produce the same BITS.  tests/test_dcn_half_cases.py asserts these premises (and that a case is not vacuous) on the generated
data without a GPU; tests/test_gpu_dcn_half.py runs the kernels.

Offsets are not merely random: per axis a sample draws a MODE (small offset / integer offset / exactly between -1 and 0 /
exactly between N-1 and N / exactly -1 / exactly N-1 / at or beyond N / a small odd half / beyond -1), so that every border class of the
bilinear sampler holds a few percent of the samples at every level size, 128 x 128 included (where unsteered offsets would
reach the border in 0.3 % of the samples).  An offset the storage types cannot hold exactly (|offset| > 120) falls back to a
small one.

Nothing here calls an orp_* DeformConv entry point."""
import collections

import numpy as np
import torch

Case = collections.namedtuple(
    "Case", "name levels batch cin cout kh kw stride pad dil mask bias relu x_exp w_exp x_max bias_step seed rows")
# levels: ((H, W), ...) input sizes; stride / pad / dil: one int for both axes; mask: DCNv2 modulation; rows: the tile height
# (32 * MT) the case CLAIMS to run -- asserted with the library's query, never derived here; x_max: |x| <= x_max <= X_MAX;
# bias_step: the bias is an integer multiple of it, |multiple| <= 120 (16: up to +-1920, still 8 significand bits for bf16).


def _c(name, levels, batch=1, cin=256, cout=256, k=(3, 3), stride=1, pad=1, dil=1, mask=False, bias=False, relu=False,
       x_exp=0, w_exp=0, x_max=15, bias_step=16, seed=0, rows=32):
    return Case(name, tuple(levels), batch, cin, cout, k[0], k[1], stride, pad, dil, mask, bias, relu, x_exp, w_exp, x_max,
                bias_step, seed, rows)


HEAD = ((128, 128), (64, 64), (32, 32), (16, 16), (8, 8))          # the five levels of a 1024 x 1024 image

# ---- tile heights, single level: position counts that are no multiple of the tile, tile counts = 1, 3, 7 (mod 8) -------------
TILE_CASES = [
    _c("mt1_t9", [(15, 19)], cout=256, mask=True, seed=11, rows=32),             # 285 positions, 9 tiles
    _c("mt1_t11", [(18, 19)], cout=64, mask=True, seed=12, rows=32),             # 342 positions, 11 tiles
    _c("mt1_t7", [(13, 17)], cout=128, mask=True, bias=True, seed=13, rows=32),  # 221 positions, 7 tiles
    _c("mt1_t249", [(73, 109)], cout=256, mask=True, seed=14, rows=32),          # 7957 positions, 249 tiles
    _c("mt2_t129", [(133, 62)], cout=256, mask=True, seed=21, rows=64),          # 8246 positions, 129 tiles
    _c("mt2_t131", [(92, 91)], cout=64, mask=True, bias=True, seed=22, rows=64),  # 8372 positions, 131 tiles
    _c("mt2_t135", [(89, 97)], cout=128, mask=True, seed=23, rows=64),           # 8633 positions, 135 tiles
    _c("mt3_t177", [(140, 121)], cout=256, mask=True, seed=31, rows=96),         # 16940 positions, 177 tiles
    _c("mt3_t171", [(100, 164)], cout=64, mask=True, bias=True, seed=32, rows=96),  # 16400 positions, 171 tiles
    _c("mt3_t175", [(130, 129)], cout=128, mask=True, seed=33, rows=96),         # 16770 positions, 175 tiles
]
# ---- the production head: 256 -> 256, all five levels in one launch -------------------------------------------------------------
HEAD_CASES = [
    _c("head_b1", HEAD, batch=1, mask=True, seed=41, rows=96),
    _c("head_b2", HEAD, batch=2, mask=True, seed=42, rows=96),                   # 16384 positions per image: tiles straddle images
]
# ---- seams: tiles that straddle two images, levels smaller than one tile.  (A 1 x 1 level is contiguous in BOTH memory formats, and
# the wrapper then takes the whole launch as NCHW: the *_1x2 siblings have no such level, so their channels-last run IS channels-last.)
SEAM_CASES = [
    _c("seam_b3", [(9, 12), (5, 5), (1, 1), (2, 3), (7, 9)], batch=3, cout=128, mask=True, seed=51, rows=32),
    _c("seam_b3_1x2", [(9, 12), (5, 5), (1, 2), (2, 3), (7, 9)], batch=3, cout=128, mask=True, bias=True, seed=53, rows=32),
    _c("seam_b2_mt2", [(67, 63), (9, 11), (1, 1), (2, 3)], batch=2, cout=64, mask=True, seed=52, rows=64),
    _c("seam_b2_mt2_1x2", [(67, 63), (9, 11), (1, 2), (2, 3)], batch=2, cout=64, mask=True, bias=True, seed=54, rows=64),
]
# ---- depth: more than one channel block per tap, two N blocks, partial last N block ----------------------------------------------
_DL = [(20, 24), (7, 5)]
DEPTH_CASES = [
    _c("depth_256_64", _DL, batch=2, cin=256, cout=64, mask=True, seed=61),
    _c("depth_256_192", _DL, batch=2, cin=256, cout=192, mask=True, seed=62),
    _c("depth_512_128", _DL, batch=2, cin=512, cout=128, mask=True, seed=63),
    _c("depth_512_320", _DL, batch=2, cin=512, cout=320, mask=True, seed=64),
    _c("depth_512_512", _DL, batch=2, cin=512, cout=512, mask=True, seed=65),
    _c("depth_1024_256", _DL, batch=2, cin=1024, cout=256, mask=True, seed=66),
    _c("depth_1024_320", [(11, 13)], batch=1, cin=1024, cout=320, mask=True, bias=True, seed=67),
]
# ---- geometry ---------------------------------------------------------------------------------------------------------------
_GL = [(23, 31), (9, 6)]
GEOMETRY_CASES = [
    _c("geo_3x3_s2", _GL, batch=2, cout=128, stride=2, pad=1, mask=True, seed=71),
    _c("geo_3x3_d2", _GL, batch=2, cout=128, pad=2, dil=2, mask=True, seed=72),
    _c("geo_1x1", _GL, batch=2, cin=1024, cout=128, k=(1, 1), pad=0, mask=True, bias=True, seed=73),
    _c("geo_1x3", _GL, batch=2, cout=128, k=(1, 3), pad=0, mask=True, bias=True, seed=74),
    _c("geo_3x1", _GL, batch=2, cout=128, k=(3, 1), pad=0, mask=True, bias=True, seed=75),
    _c("geo_2x2", _GL, batch=2, cout=128, k=(2, 2), pad=0, mask=True, bias=True, seed=76),
    _c("geo_512_s2", _GL, batch=2, cin=512, cout=512, stride=2, pad=1, mask=True, seed=77),   # a ResNet DCNv2 stage transition
]
# ---- DCNv2 epilogue on a multi-level launch -------------------------------------------------------------------------------------
_VL = [(40, 40), (20, 20), (7, 9)]
DCNV2_CASES = [
    _c("v2_mask_bias_relu", _VL, batch=2, mask=True, bias=True, relu=True, seed=81),
    _c("v1_bias_relu", _VL, batch=2, cin=1024, mask=False, bias=True, relu=True, seed=82),
    _c("v1_plain", _VL, batch=2, mask=False, seed=83),
]
# ---- range: the same integer case, scaled by powers of two (same seed: same integers).  |x| <= 7 and a bias step of 4 keep the
# unscaled outputs below 4094, so that the case scaled by 2^4 stays finite in fp16 -------------------------------------------------
_RL = [(24, 20), (6, 7)]
RANGE_CASES = [
    _c("range_unit", _RL, batch=2, cout=128, mask=True, bias=True, x_max=7, bias_step=4, seed=91),
    _c("range_down", _RL, batch=2, cout=128, mask=True, bias=True, x_max=7, bias_step=4, x_exp=-8, w_exp=-4, seed=91),
    _c("range_up", _RL, batch=2, cout=128, mask=True, bias=True, x_max=7, bias_step=4, x_exp=4, seed=91),
]
# ---- fp16 saturation: exact results beyond 65504 at some outputs (bf16 runs it too and must not saturate) ------------------------
SATURATION_CASES = [
    _c("saturate", [(6, 7)], batch=1, cout=64, mask=True, x_exp=6, seed=95),
]

FAMILIES = collections.OrderedDict([
    ("tile heights", TILE_CASES), ("production head", HEAD_CASES), ("seams", SEAM_CASES), ("depth", DEPTH_CASES),
    ("geometry", GEOMETRY_CASES), ("DCNv2", DCNV2_CASES), ("range", RANGE_CASES), ("saturation", SATURATION_CASES)])
ALL_CASES = [c for fam in FAMILIES.values() for c in fam]
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)
SYMMETRIC_KERNEL_CASES = [c.name for c in ALL_CASES if c.rows > 32]   # every MT = 2 / MT = 3 case runs again with ORP_DCNH_WS=0

X_MAX, W_MAX = 15, 7                       # |x| <= 15, |w| <= 7 (integers, before the power-of-two scale)
MASK_VALUES, MASK_P = (0.0, 0.5, 1.0, 1.5), (0.1, 0.3, 0.3, 0.3)
OFFSET_LIMIT = 120.0                       # halves up to 127.5 are exact in bf16 (8 significand bits); stay inside
_MODES = ("small", "integer", "low_half", "high_half", "minus_one", "last", "beyond_high", "half", "beyond_low")
_MODE_P = (0.25, 0.10, 0.07, 0.07, 0.04, 0.08, 0.07, 0.25, 0.07)


def out_size(n, case, k):
    return (n + 2 * case.pad - (case.dil * (k - 1) + 1)) // case.stride + 1


def positions(case):
    """Output positions of the launch, all levels: batch x Ho x Wo summed."""
    return sum(case.batch * out_size(h, case, case.kh) * out_size(w, case, case.kw) for h, w in case.levels)


def _axis_offsets(rng, base, n):
    """Offsets along one axis for the un-deformed coordinates `base` (float64 array) on an axis of n pixels."""
    mode = rng.choice(len(_MODES), size=base.shape, p=_MODE_P)
    small = base + rng.randint(-4, 5, size=base.shape) / 2.0
    target = np.select(
        [mode == 0, mode == 1, mode == 2, mode == 3, mode == 4, mode == 5, mode == 6, mode == 7],
        [small, base + rng.randint(-2, 3, size=base.shape), np.full(base.shape, -0.5), np.full(base.shape, n - 0.5),
         np.full(base.shape, -1.0), np.full(base.shape, n - 1.0), n + rng.choice([0.0, 0.5, 1.0, 2.5], size=base.shape),
         base + rng.randint(-2, 2, size=base.shape) + 0.5],
        -1.0 - rng.choice([0.5, 1.0, 2.5], size=base.shape))
    off = target - base
    return np.where(np.abs(off) > OFFSET_LIMIT, small - base, off)


def generate(case):
    """The case's tensors as float64 torch tensors on the CPU (NCHW): dict(xs, offs, masks | None, weight, bias | None).  Every
    value is exactly representable in fp16 and in bf16 (asserted)."""
    rng = np.random.RandomState(case.seed)
    taps = case.kh * case.kw
    xs, offs, masks = [], [], []
    for (H, W) in case.levels:
        Ho, Wo = out_size(H, case, case.kh), out_size(W, case, case.kw)
        assert Ho > 0 and Wo > 0
        xs.append(rng.randint(-min(case.x_max, X_MAX), min(case.x_max, X_MAX) + 1, size=(case.batch, case.cin, H, W)) * 2.0 ** case.x_exp)
        ki, kj = np.divmod(np.arange(taps), case.kw)
        base_h = (np.arange(Ho)[None, :] * case.stride - case.pad + ki[:, None] * case.dil).astype(np.float64)     # [taps, Ho]
        base_w = (np.arange(Wo)[None, :] * case.stride - case.pad + kj[:, None] * case.dil).astype(np.float64)     # [taps, Wo]
        shape = (case.batch, taps, Ho, Wo)
        off = np.empty((case.batch, 2 * taps, Ho, Wo))
        off[:, 0::2] = _axis_offsets(rng, np.broadcast_to(base_h[None, :, :, None], shape), H)
        off[:, 1::2] = _axis_offsets(rng, np.broadcast_to(base_w[None, :, None, :], shape), W)
        offs.append(off)
        masks.append(rng.choice(MASK_VALUES, size=shape, p=MASK_P))
    weight = rng.randint(-W_MAX, W_MAX + 1, size=(case.cout, case.cin, case.kh, case.kw)) * 2.0 ** case.w_exp
    bias = rng.randint(-120, 121, size=(case.cout,)) * float(case.bias_step) * 2.0 ** (case.x_exp + case.w_exp)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))           # noqa: E731
    data = dict(xs=[t(a) for a in xs], offs=[t(a) for a in offs], masks=[t(a) for a in masks] if case.mask else None,
                weight=t(weight), bias=t(bias) if case.bias else None)
    for v in data["xs"] + data["offs"] + (data["masks"] or []) + [data["weight"]] + ([data["bias"]] if case.bias else []):
        for dt in (torch.float16, torch.bfloat16):
            assert torch.equal(v.to(dt).double(), v), "%s: a generated value is not exact in %s" % (case.name, dt)
    return data


def representable(v, dtype):
    """Elementwise: does the float64 value survive the round trip through `dtype` unchanged?"""
    return v.to(dtype).double() == v


def tap_samples(case, x, off, mask, tap):
    """Bilinear sampling of one kernel tap at every output position of one level, float64, from the definition
    (deform_conv_cuda_kernel.cu:84-115,190-243: a sample at or beyond -1 / H / W is zero, a neighbour outside the image
    contributes nothing).  x [B, C, H, W], off [B, 2 taps, Ho, Wo], mask [B, taps, Ho, Wo] or None.
    Returns (idx [N, 4] rows of the [B*H*W, C] pixel table, wgt [N, 4] modulated weights, h [N], w [N]) with
    N = B * Ho * Wo in (b, ho, wo) order."""
    B, _, H, W = x.shape
    Ho, Wo = off.shape[2], off.shape[3]
    ki, kj = divmod(tap, case.kw)
    dev = x.device
    ho = torch.arange(Ho, device=dev, dtype=torch.float64)[None, :, None]
    wo = torch.arange(Wo, device=dev, dtype=torch.float64)[None, None, :]
    h = (ho * case.stride - case.pad + ki * case.dil + off[:, 2 * tap]).reshape(-1)
    w = (wo * case.stride - case.pad + kj * case.dil + off[:, 2 * tap + 1]).reshape(-1)
    valid = (h > -1) & (w > -1) & (h < H) & (w < W)
    h0, w0 = torch.floor(h), torch.floor(w)
    lh, lw = h - h0, w - w0
    b = torch.arange(B, device=dev).repeat_interleave(Ho * Wo)
    m = mask[:, tap].reshape(-1) if mask is not None else torch.ones_like(h)
    idx, wgt = [], []
    for dh, dw in ((0, 0), (0, 1), (1, 0), (1, 1)):
        hh, ww = h0 + dh, w0 + dw
        ok = valid & (hh >= 0) & (hh <= H - 1) & (ww >= 0) & (ww <= W - 1)
        wt = (lh if dh else 1 - lh) * (lw if dw else 1 - lw) * m
        wgt.append(torch.where(ok, wt, torch.zeros_like(wt)))
        idx.append(torch.where(ok, (b * H + hh.long()) * W + ww.long(), torch.zeros_like(b)))
    return torch.stack(idx, 1), torch.stack(wgt, 1), h, w


def tap_columns(x, idx, wgt):
    """[N, C] modulated bilinear samples of one tap."""
    table = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])
    col = wgt[:, 0, None] * table[idx[:, 0]]
    for i in (1, 2, 3):
        col += wgt[:, i, None] * table[idx[:, i]]
    return col


def reference_level(case, x, off, mask, weight, bias):
    """float64 DeformConv / ModulatedDeformConv forward of one level by gather and matmul: [B, Cout, Ho, Wo], on x's device."""
    B, Ho, Wo = x.shape[0], off.shape[2], off.shape[3]
    out = torch.zeros((B * Ho * Wo, case.cout), dtype=torch.float64, device=x.device)
    for tap in range(case.kh * case.kw):
        idx, wgt, _, _ = tap_samples(case, x, off, mask, tap)
        out += tap_columns(x, idx, wgt) @ weight[:, :, tap // case.kw, tap % case.kw].t()
    if bias is not None:
        out += bias[None, :]
    if case.relu:
        out = out.clamp_min(0.0)
    return out.reshape(B, Ho, Wo, case.cout).permute(0, 3, 1, 2).contiguous()


def reference(case, data, device="cpu"):
    """The expected outputs before the final rounding: a list of float64 [B, Cout, Ho, Wo] tensors on `device`."""
    outs = []
    for i in range(len(case.levels)):
        mv = lambda t: t.to(device) if t is not None else None           # noqa: E731
        outs.append(reference_level(case, mv(data["xs"][i]), mv(data["offs"][i]), mv(data["masks"][i]) if case.mask else None,
                                    mv(data["weight"]), mv(data["bias"])))
    return outs


_expected = {}


def expected(case, device):
    """(generate(case), reference(case, data, device)), computed once per case name and process and never modified: the GPU test
    files that run the same case (half and fp32) share it."""
    if case.name not in _expected:
        data = generate(case)
        _expected[case.name] = (data, reference(case, data, device))
    return _expected[case.name]


SAMPLE_CLASSES = ("inside", "h_low=-1", "h_high=H", "w_low=-1", "w_high=W", "on -1", "on H-1 / W-1", "at or beyond H / W",
                  "at or beyond -1", "strictly beyond -1", "integer coordinates")


def sample_class_counts(case, data):
    """{class: number of (position, tap) samples}, and the total, over all levels of the case -- from the coordinates alone."""
    counts = collections.OrderedDict((k, 0) for k in SAMPLE_CLASSES)
    total = 0
    for x, off in zip(data["xs"], data["offs"]):
        H, W = x.shape[2], x.shape[3]
        for tap in range(case.kh * case.kw):
            _, _, h, w = tap_samples(case, x, off, None, tap)
            valid = (h > -1) & (w > -1) & (h < H) & (w < W)
            h0, w0 = torch.floor(h), torch.floor(w)
            n = lambda t: int(t.sum())                                    # noqa: E731
            counts["inside"] += n(valid & (h0 >= 0) & (h0 + 1 <= H - 1) & (w0 >= 0) & (w0 + 1 <= W - 1))
            counts["h_low=-1"] += n(valid & (h0 == -1))
            counts["h_high=H"] += n(valid & (h0 + 1 == H))
            counts["w_low=-1"] += n(valid & (w0 == -1))
            counts["w_high=W"] += n(valid & (w0 + 1 == W))
            counts["on -1"] += n((h == -1) | (w == -1))
            counts["on H-1 / W-1"] += n(valid & ((h == H - 1) | (w == W - 1)))
            counts["at or beyond H / W"] += n((h >= H) | (w >= W))
            counts["at or beyond -1"] += n((h <= -1) | (w <= -1))
            counts["strictly beyond -1"] += n((h < -1) | (w < -1))
            counts["integer coordinates"] += n(valid & (h == h0) & (w == w0))
            total += h.numel()
    return counts, total


def device_inputs(case, data, dtype, device, channels_last):
    """The case's tensors in the storage type on the device, features NCHW-contiguous or channels-last."""
    q = lambda t: t.to(device).to(dtype)                                  # noqa: E731  (exact: generate() asserted it)
    xs = [q(x) for x in data["xs"]]
    if channels_last:
        xs = [x.contiguous(memory_format=torch.channels_last) for x in xs]
    return dict(xs=xs, offs=[q(o) for o in data["offs"]], masks=[q(m) for m in data["masks"]] if case.mask else None,
                weight=q(data["weight"]), bias=q(data["bias"]) if case.bias else None)


def bits(t):
    """The storage of a 2-byte tensor as int16, NCHW order."""
    return t.contiguous().view(torch.int16)


def count_differing(got, want64, dtype):
    """(outputs compared, outputs whose BITS differ from want64.to(dtype))."""
    want = want64.to(dtype)
    assert got.dtype == dtype and got.shape == want.shape
    return want.numel(), int((bits(got) != bits(want)).sum())
