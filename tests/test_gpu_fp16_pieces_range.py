"""GPU: range edges of the fp16-pieces kernels (ORP_DCN_SPLIT=3, the default arithmetic of every fp32 contraction).  Each operand
TENSOR is multiplied by one power of two that puts its largest magnitude into [2^14, 2^15) (csrc/orp_range.hpp), split into
hi = fp16(v), lo = fp16(v - hi), contracted in fp32 and scaled back.  Six kernels share that rule:

  K1  DeformConv forward                (deform_conv_forward_multi)           operands x, W        vs oracle.dcn_forward
  K2  tower / FPN 3x3 convolution       (conv_split_multi)                    operands x, W        vs float64 conv2d
  K3  its grad_input                    (conv_split_train backward)           operands grad, W     vs float64 conv2d_input
  K4  tower / FPN weight gradient       (conv_wgrad_split)                    operands x, grad     vs float64 conv2d_weight
  K5  DeformConv grad_input / offset    (backward_mfma, dense and sparse)     operands grad, W     vs oracle.dcn_backward
  K6  DeformConv grad_weight            (backward_mfma, need_weight)          operands x, grad     vs oracle.dcn_backward

Scenarios, each case against float64:
  S1  one outlier channel (or weight row) 2^R above the rest of its tensor; the outputs that do not read it ("quiet") are
      measured on their own scale.  Gate: 1e-5 for R <= 16, the analytic 2^-(38 - R) beyond (the quiet data keep ~22 - R bits of
      the call's scale; the low piece goes subnormal from R ~ 17) -- and 1e-5 at every R for the exact paths (split mode 6 / 0,
      ORP_DCN_BWD_SPLIT=0 with ORP_DCN_BWD_W16=0 in a child process; K4 has none).  A kernel that took the wrong tensor's range,
      lost one operand's lo plane or flushed fp16 denormals fails here.
  S2  levels 2^R apart in one launch (K1, K2, K3, K5): each level on its own scale, same gates; K2 also with the range handed
      over by the producers (to_channels_last_multi, group_norm_act_multi_cl).
  S3  one NaN, +Inf or -Inf in one operand (where the other operand is dense and non-zero): where float64 is finite the output
      meets the clean tolerance, where float64 is not the output is not either (the kind may differ).  The bad element sits
      inside the map, away from the border pixels a clamped bilinear corner (weight 0) points at; a bad weight sits on the centre tap,
      whose samples stay inside the map: a zero-padded term or a sample outside the map is 0 x NaN in one formulation and
      absent in another (float64 conv2d_input / the DeformConv oracle's col2im_coord vs the kernels), so neither is asserted.  K6 skips grad_out chunks
      that are exactly zero (its active list), so a 0 x NaN there would stay finite; the gradients here are dense.
  S4  operand maxima (2^-80, 2^-40), (2^116, 2^-60), (~2^-130 = fp32 subnormals, 2^100), (2^50, 2^40): the result is a normal
      float and must be finite and within 1e-5 of the float64 output's scale.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

C = 256
SHAPES = [(9, 11), (5, 6), (1, 1)]
CO = 5                                                   # the outlier's channel / row
BAD = (0, 7, 4, 5)                                       # (level, channel, h, w) of a non-finite element: inside the 9 x 11 map
BAD_W = (11, 13, 1, 1)                                   # (the centre tap: see S3)
BWD_EXACT = os.environ.get("ORP_DCN_BWD_SPLIT", "1") == "0"
W16_EXACT = BWD_EXACT or os.environ.get("ORP_DCN_BWD_W16", "1") == "0"
ERRS = {}                                                # kernel -> [(scenario, R, path, error)] for the session summary


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    yield torch.device("cuda:0")
    import conftest
    for k in sorted(ERRS):
        rows = ERRS[k]
        parts = []
        for scen in ("S1", "S2"):
            for path in sorted({r[2] for r in rows if r[0] == scen}):
                worst = {}
                for r in rows:
                    if r[0] == scen and r[2] == path:
                        worst[r[1]] = max(worst.get(r[1], 0.0), r[3])
                vals = ", ".join("R=%d %.2e" % (R, worst[R]) for R in sorted(worst))
                parts.append("%s %s: %s" % (scen, path, vals))
        conftest.REPORT.append("fp16-pieces range edges, %s, worst quiet-output error / own scale -- %s" % (k, "; ".join(parts)))


@pytest.fixture
def split(dev):
    from orientedreppoints_amd import _lib
    L = _lib.lib()

    def set_mode(m):                        # 0 exact fp32 MFMA | 6 products of three bf16 pieces | 3 two fp16 pieces
        assert L.orp_dcn_set_split_mode(int(m)) == 0
        assert L.orp_dcn_get_split_mode() == int(m)
    yield set_mode
    L.orp_dcn_set_split_mode(-1)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().contiguous().cpu().numpy()


def _gate(R, exact):
    return 1e-5 if (exact or R <= 16) else 2.0 ** -(38 - R)


def _pieces(ts, amax=None):
    """float64 model of what the kernels carry of a tensor set: the same range rule (from max |v|, or from the range word a
    producer handed over), hi = fp16(2^k v), lo = fp16(2^k v - hi)"""
    one = not isinstance(ts, list)
    ts = [ts] if one else ts
    k = 14 - (int(np.frexp(amax if amax is not None else max(float(np.abs(t).max()) for t in ts))[1]) - 1)
    out = []
    for t in ts:
        sv = t * np.float32(2.0 ** k)
        hi = sv.astype(np.float16)
        lo = (sv - hi.astype(np.float32)).astype(np.float16)
        out.append((hi.astype(np.float64) + lo.astype(np.float64)) * 2.0 ** -k)
    return out[0] if one else out


def _model_errors(kernel, d, oracle, want, sel):
    """the error of the two-piece representation itself (float64 contraction of the pieces) on the quiet outputs.  At R = 24 the
    quiet data keep about one bit in the low piece and the worst output can pass 2^-(38 - R) on the representation alone (e.g.
    7.1e-5 for the weight gradient with an outlier grad_out channel); there the kernel is held to that model instead.  For the
    DeformConv forward the model splits the bilinear samples as the kernel does; the weight gradient's x side is split after
    sampling too, there the model splits x (a stand-in: interpolated samples are smaller than x and keep fewer bits), hence the
    allowance of 2 for that case."""
    m = dict(d)
    for name in OPERANDS[kernel]:
        m[name] = _pieces(d[name], d.get("_amax_" + name))
    if kernel == "K1":                                   # the forward splits the bilinear samples, scaled by the range of x
        cols = [oracle.dcn_im2col(x, o, 3, 3, 1, 1, 1) for x, o in zip(d["xs"], d["offs"])]
        cols = _pieces(cols, max(float(np.abs(x).max()) for x in d["xs"]))
        wm = m["w"].reshape(C, -1)
        got = [np.einsum("ok,kbhw->bohw", wm, c) for c in cols]
    else:
        with np.errstate(all="ignore"):
            got = REF[kernel](m, oracle)
    return [(_rel(g, w, q) if q is not None else 0.0) for g, w, q in zip(got, want, sel)]


def _check_quiet(e, R, exact, kernel, d, oracle, want, sel, i, cache, floor=0.0):
    """S1 / S2 gate: 1e-5 (R <= 16, exact paths), 2^-(38 - R) beyond -- or, where the representation alone passes that, the
    float64 model of the representation (x 1.5 where the model is the stand-in)"""
    gate = max(floor, _gate(R, exact))
    if e <= gate:
        return
    assert R > 20 and not exact, (kernel, i, R, e, gate)
    if "model" not in cache:
        cache["model"] = _model_errors(kernel, d, oracle, want, sel)
    em = cache["model"][i]
    allow = 2.0 if kernel == "K6" else 1.05
    assert e <= allow * max(em, gate), (kernel, i, R, e, gate, em)


def _case(seed, B, shapes=SHAPES):
    rng = np.random.RandomState(seed)
    xs = [rng.normal(size=(B, C, h, w)).astype(np.float32) for h, w in shapes]
    offs = [rng.uniform(-2.5, 2.5, size=(B, 18, h, w)).astype(np.float32) for h, w in shapes]
    gos = [rng.normal(size=(B, C, h, w)).astype(np.float32) for h, w in shapes]
    w = rng.normal(0, 0.05, size=(C, C, 3, 3)).astype(np.float32)
    return dict(xs=xs, offs=offs, gos=gos, w=w)


def _conv_mod(w, dev):
    m = nn.Conv2d(C, C, 3, padding=1, bias=False)
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(w))
    return m.to(dev)


# ---- the kernels: (operands as numpy) -> list of output arrays; the float64 references --------------------------------------
def run_k1(d, dev, mode):
    from orientedreppoints_amd.mmdet_ops import deform_conv_forward_multi
    return [_np(o) for o in deform_conv_forward_multi([_t(x, dev) for x in d["xs"]], [_t(o, dev) for o in d["offs"]], _t(d["w"], dev),
                                                        1, 1, 1, cache_pack=False)]


def ref_k1(d, oracle):
    return [oracle.dcn_forward(x, o, d["w"], stride=1, pad=1, dil=1).astype(np.float64) for x, o in zip(d["xs"], d["offs"])]


def run_k2(d, dev, mode, producer=None):
    from orientedreppoints_amd.mmdet_ops.fused_norm import Amax, conv_split_multi, to_channels_last_multi
    conv = _conv_mod(d["w"], dev).eval()
    xs = [_t(x, dev) for x in d["xs"]]
    with torch.no_grad():
        if producer == "groupnorm":                     # the GroupNorm's outputs and its bound (_groupnorm_levels)
            return [_np(o) for o in conv_split_multi(d["_ys"], conv, nprod=mode, amax=Amax(d["_bits"], 0))]
        if producer == "transposition":
            cl, bits = to_channels_last_multi(xs, amax_slots=[0] * len(xs), force_ranges=True)
            assert bits is not None
            return [_np(o) for o in conv_split_multi(cl, conv, nprod=mode, amax=Amax(bits, 0))]
        cl = [x.contiguous(memory_format=torch.channels_last) for x in xs]
        return [_np(o) for o in conv_split_multi(cl, conv, nprod=mode)]


def ref_k2(d, oracle=None):
    w = torch.from_numpy(d["w"]).double()
    return [F.conv2d(torch.from_numpy(x).double(), w, padding=1).numpy() for x in d["xs"]]


def run_k3(d, dev, mode):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv_split_train, conv_split_train_ok
    from orientedreppoints_amd import switches
    if not switches.TRAIN_SPLIT:
        pytest.skip("ORP_TRAIN_SPLIT=0: the training convolutions are routed to the library")
    conv = _conv_mod(d["w"], dev)
    conv.weight.requires_grad_(False)
    xs = [_t(x, dev).requires_grad_(True) for x in d["xs"]]
    assert conv_split_train_ok([conv], xs[0])
    outs = conv_split_train(xs, [conv] * len(xs))
    torch.autograd.backward(outs, [_t(g, dev) for g in d["gos"]])
    return [_np(x.grad) for x in xs]


def ref_k3(d, oracle=None):
    w = torch.from_numpy(d["w"]).double()
    return [torch.nn.grad.conv2d_input(x.shape, w, torch.from_numpy(g).double(), padding=1).numpy() for x, g in zip(d["xs"], d["gos"])]


def run_k4(d, dev, mode):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv_wgrad_split
    return [_np(conv_wgrad_split([_t(x, dev) for x in d["xs"]], [_t(g, dev) for g in d["gos"]], (C, C, 3, 3), (1, 1), (1, 1)))]


def ref_k4(d, oracle=None):
    return [sum(torch.nn.grad.conv2d_weight(torch.from_numpy(x).double(), (C, C, 3, 3), torch.from_numpy(g).double(), padding=1)
                for x, g in zip(d["xs"], d["gos"])).numpy()]


def _bwd(d, dev, need_input, need_weight, sparse=False):
    from orientedreppoints_amd.mmdet_ops import deform_conv_backward as bw
    return bw.backward_mfma([_t(x, dev) for x in d["xs"]], [_t(o, dev) for o in d["offs"]], _t(d["w"], dev), [_t(g, dev) for g in d["gos"]],
                            (1, 1), (1, 1), (1, 1), need_input=need_input, need_weight=need_weight, sparse_grad=sparse)


def run_k5(d, dev, mode, sparse=False):
    gis, goffs, _ = _bwd(d, dev, True, False, sparse)
    return [_np(g) for g in gis] + [_np(g) for g in goffs]


def ref_k5(d, oracle):
    r = [oracle.dcn_backward(x, o, d["w"], g) for x, o, g in zip(d["xs"], d["offs"], d["gos"])]
    return [a[0].astype(np.float64) for a in r] + [a[1].astype(np.float64) for a in r]


def run_k6(d, dev, mode):
    return [_np(_bwd(d, dev, False, True)[2])]


def ref_k6(d, oracle):
    return [sum(oracle.dcn_backward(x, o, d["w"], g)[2].astype(np.float64) for x, o, g in zip(d["xs"], d["offs"], d["gos"]))]


RUN = {"K1": run_k1, "K2": run_k2, "K3": run_k3, "K4": run_k4, "K5": run_k5, "K6": run_k6}
REF = {"K1": ref_k1, "K2": ref_k2, "K3": ref_k3, "K4": ref_k4, "K5": ref_k5, "K6": ref_k6}
OPERANDS = {"K1": ("xs", "w"), "K2": ("xs", "w"), "K3": ("gos", "w"), "K4": ("xs", "gos"), "K5": ("gos", "w"), "K6": ("xs", "gos")}
# the paths a case runs: (label, split mode, exact?) -- K5 / K6 take the library's backward switches (read at load: a child process)
PATHS = {"K1": [("pieces", 3, False), ("6 products", 6, True), ("exact fp32", 0, True)],
         "K2": [("pieces", 3, False), ("6 products", 6, True)],
         "K3": [("pieces", 3, False), ("6 products", 6, True)],
         "K4": [("pieces", 3, False)],
         "K5": [("exact fp32" if BWD_EXACT else "pieces", 3, BWD_EXACT)],
         "K6": [("exact fp32" if W16_EXACT else "pieces", 3, W16_EXACT)]}


def _rel(got, want, sel=None):
    g, w = got.astype(np.float64), want
    if sel is not None:
        g, w = g[sel], w[sel]
    return float(np.max(np.abs(g - w))) / max(1e-300, float(np.max(np.abs(w))))


def _is_offset(kernel, i, nlev):
    return kernel == "K5" and i >= nlev                  # K5 returns grad_input of every level, then grad_offset of every level


def _clean_tol(kernel, i, nlev):
    return 1e-4 if _is_offset(kernel, i, nlev) else 1e-5   # grad_offset: the coordinate derivatives' tolerance vs the oracle


# ---- S1: one outlier channel / weight row --------------------------------------------------------------------------------------
def _outlier(kernel, which, R, seed):
    """operands with one outlier, and per output tensor the index of its quiet part (outputs that do not read the outlier)"""
    d = _case(seed, 1 if R % 8 else 2)
    s = np.float32(2.0 ** R)
    name = OPERANDS[kernel][which]
    n_out = len(SHAPES) if kernel in ("K1", "K2", "K3") else (2 * len(SHAPES) if kernel == "K5" else 1)
    if kernel in ("K4", "K6"):                           # grad_weight [o][c]: the outlier's column (x) or row (grad) is loud
        for t in d[name]:
            t[:, CO] *= s
        quiet = [(slice(None), np.arange(C) != CO)] if name == "xs" else [(np.arange(C) != CO,)]
        return d, quiet
    if name == "w":                                      # one row of the weights: W[o] (forward), W[:, c] (grad_input: W^T)
        if kernel in ("K1", "K2"):
            d["w"][CO] *= s
        else:
            d["w"][:, CO] *= s
        quiet = [(slice(None), np.arange(C) != CO)] * n_out
    else:                                                # x / grad_out channel CO: half of the outputs get zero weights for it
        for t in d[name]:
            t[:, CO] *= s
        if kernel in ("K1", "K2"):
            d["w"][:C // 2, CO] = 0.0
        else:
            d["w"][CO, :C // 2] = 0.0
        quiet = [(slice(None), slice(0, C // 2))] * n_out
    if kernel == "K5":                                   # grad_offset sums over every input channel: measured whole
        quiet = quiet[:len(SHAPES)] + [None] * len(SHAPES)
    return d, quiet


@pytest.mark.parametrize("R", [12, 16, 20, 24])
@pytest.mark.parametrize("which", [0, 1], ids=["first_operand", "second_operand"])
@pytest.mark.parametrize("kernel", ["K1", "K2", "K3", "K4", "K5", "K6"])
def test_s1_one_outlier_channel(dev, oracle, split, kernel, which, R):
    d, quiet = _outlier(kernel, which, R, 1000 + 10 * R + which)
    want = REF[kernel](d, oracle)
    cache = {}
    for label, mode, exact in PATHS[kernel]:
        split(mode)
        got = RUN[kernel](d, dev, mode)
        worst = 0.0
        for i, (g, w, q) in enumerate(zip(got, want, quiet)):
            assert np.isfinite(g).all(), (kernel, label, i)
            assert _rel(g, w) <= _clean_tol(kernel, i, len(SHAPES)), (kernel, label, i, _rel(g, w))          # whole tensor, tensor scale
            if q is not None:
                e = _rel(g, w, q)
                worst = max(worst, e)
                _check_quiet(e, R, exact, kernel, d, oracle, want, quiet, i, cache)
        ERRS.setdefault(kernel, []).append(("S1", R, label, worst))


# ---- S2: levels 2^R apart in one launch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [8, 16, 24])
@pytest.mark.parametrize("kernel", ["K1", "K2", "K3", "K5", "K2-transposition", "K2-groupnorm"])
def test_s2_levels_apart(dev, oracle, split, kernel, R):
    base = kernel.split("-")[0]
    # (a tensor that already is channels-last -- the 1 x 1 level -- passes the transposition untouched: its range is not known there)
    d = _case(2000 + R, 2, [(9, 11), (7, 5), (3, 3)] + ([] if kernel == "K2-transposition" else [(1, 1)]))
    name = OPERANDS[base][0]
    d[name][0] *= np.float32(2.0 ** R)                   # level 0 is loud, the others quiet
    paths = PATHS[base]
    if kernel == "K2-groupnorm":
        split(3)
        d["xs"] = _groupnorm_levels(d, dev, R)
    want = REF[base](d, oracle)
    nlev = len(d["xs"])
    cache = {}
    for label, mode, exact in paths:
        if kernel != base and mode != 3:
            continue                                     # (the producers leave ranges for the fp16-pieces mode)
        split(mode)
        got = run_k2(d, dev, mode, producer=kernel.split("-")[1]) if kernel != base else RUN[base](d, dev, mode)
        worst = 0.0
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.isfinite(g).all(), (kernel, label, i)
            e = _rel(g, w)
            lvl = i % nlev
            if lvl == 0:
                assert e <= _clean_tol(base, i, nlev), (kernel, label, i, R, e)
            else:
                _check_quiet(e, R, exact, base, d, oracle, want, [None if j % nlev == 0 else () for j in range(len(want))], i, cache,
                             floor=_clean_tol(base, i, nlev))
            if _is_offset(base, i, nlev):
                continue
            if lvl:
                worst = max(worst, e)
        ERRS.setdefault(kernel, []).append(("S2", R, label, worst))


def _groupnorm_levels(d, dev, R):
    """the tower's inputs as the channels-last GroupNorm leaves them: level 0 through a GroupNorm whose affine is 2^R larger;
    the range word is its statistics' bound (group_norm_act_multi_cl), the tensors handed on are what it wrote"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import group_norm_act_multi_cl
    g = torch.Generator().manual_seed(R)
    gns = []
    for i in range(len(d["xs"])):
        gn = nn.GroupNorm(32, C)
        with torch.no_grad():
            gn.weight.copy_(torch.rand(C, generator=g) * 1.8 + 0.2)
            gn.bias.copy_(torch.randn(C, generator=g) * 0.5)
            if i == 0:
                gn.weight.mul_(2.0 ** R); gn.bias.mul_(2.0 ** R)
        gns.append(gn.to(dev))
    with torch.no_grad():
        cl = [_t(x / np.float32(2.0 ** R) if i == 0 else x, dev).contiguous(memory_format=torch.channels_last) for i, x in enumerate(d["xs"])]
        ys, bits = group_norm_act_multi_cl(cl, gns, relu=False, inplace=False, amax_slots=[0] * len(cl))
        assert bits is not None
        d["_ys"], d["_bits"] = ys, bits
        d["_amax_xs"] = float(bits[:1].cpu().view(torch.float32))          # the bound the convolution scales by (>= max |y|)
    return [_np(y) for y in ys]


# ---- S3: non-finite elements -------------------------------------------------------------------------------------------------
def _plant(d, kernel, which, value):
    name = OPERANDS[kernel][which]
    if name == "w":
        d["w"][BAD_W] = value
    else:
        lvl, c, h, w = BAD
        d[name][lvl][d[name][lvl].shape[0] - 1, c, h, w] = value


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("which", [0, 1], ids=["first_operand", "second_operand"])
@pytest.mark.parametrize("kernel", ["K1", "K2", "K3", "K4", "K5", "K5-sparse", "K6"])
def test_s3_non_finite_elements(dev, oracle, split, kernel, which, value):
    base = kernel.split("-")[0]
    d = _case(3000 + which, 2, SHAPES[:2])
    for o in d["offs"]:                                  # the centre tap samples inside the map
        o[:, 8:10] = np.clip(o[:, 8:10], -0.4, 0.4)
    _plant(d, base, which, np.float32(value))
    with np.errstate(invalid="ignore", over="ignore"):
        want = REF[base](d, oracle)
    assert any(not np.isfinite(w).all() for w in want) and any(np.isfinite(w).any() for w in want)
    split(3)
    got = run_k5(d, dev, 3, sparse=True) if kernel == "K5-sparse" else RUN[base](d, dev, 3)
    for i, (g, w) in enumerate(zip(got, want)):
        fin = np.isfinite(w)
        assert not np.isfinite(g[~fin]).any(), (kernel, i, "finite where float64 is not", int(np.isfinite(g[~fin]).sum()))
        if fin.any() and np.abs(w[fin]).max() > 0:
            tol = _clean_tol(base, i, 2)
            assert np.isfinite(g[fin]).all(), (kernel, i, "non-finite where float64 is finite", int((~np.isfinite(g[fin])).sum()))
            assert _rel(g, w, fin) <= tol, (kernel, i, _rel(g, w, fin))


# ---- S4: operand magnitudes at the ends of the float range ---------------------------------------------------------------
@pytest.mark.parametrize("amax", [(-80, -40), (116, -60), (-130, 100), (50, 40)], ids=["2^-80,2^-40", "2^116,2^-60", "2^-130,2^100", "2^50,2^40"])
@pytest.mark.parametrize("kernel", ["K1", "K2", "K3", "K4", "K5", "K5-sparse", "K6"])
def test_s4_magnitude_extremes(dev, oracle, split, kernel, amax):
    base = kernel.split("-")[0]
    d = _case(4000, 2, SHAPES[:2])
    for name, e in zip(OPERANDS[base], amax):
        ts = d[name] if isinstance(d[name], list) else [d[name]]
        m = max(float(np.abs(t).max()) for t in ts)
        k = np.ldexp(1.0, e) / m
        if name == "w":
            d["w"] = (d["w"].astype(np.float64) * k).astype(np.float32)
        else:
            d[name] = [(t.astype(np.float64) * k).astype(np.float32) for t in ts]
    want = REF[base](d, oracle)
    split(3)
    got = run_k5(d, dev, 3, sparse=True) if kernel == "K5-sparse" else RUN[base](d, dev, 3)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(w).all() and float(np.abs(w).max()) > 1e-37
        assert np.isfinite(g).all(), (kernel, i, "non-finite output")
        tol = _clean_tol(base, i, 2)
        assert _rel(g, w) <= tol, (kernel, i, _rel(g, w))


# ---- the exact backward kernels, behind the library's load-time switches ---------------------------------------------------
def test_s1_backward_exact_switches_in_a_child(dev):
    """ORP_DCN_BWD_SPLIT=0 / ORP_DCN_BWD_W16=0 are read when the library loads: S1 for K5 and K6 in a child pytest with both at 0,
    where the gate is 1e-5 at every R."""
    if BWD_EXACT:
        pytest.skip("this process already runs the exact backward kernels")
    env = dict(os.environ, ORP_DCN_BWD_SPLIT="0", ORP_DCN_BWD_W16="0")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                          "-k", "test_s1_one_outlier_channel and (K5 or K6)"],
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=900)
    assert out.returncode == 0, out.stdout[-4000:]
    assert " passed" in out.stdout and "failed" not in out.stdout
    import conftest
    conftest.REPORT.extend("(child, ORP_DCN_BWD_SPLIT=0 ORP_DCN_BWD_W16=0) " + ln for ln in out.stdout.splitlines()
                           if ln.startswith("fp16-pieces range edges"))
