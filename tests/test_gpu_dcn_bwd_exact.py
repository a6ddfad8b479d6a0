"""GPU: the MFMA DeformConv backward (csrc/orp_dcn_bwd_mfma.hip: chunk flags and compaction, kernel A in its four instantiations,
the region pass -- binning, radix sort, bounds, descriptors, scatter --, both weight kernels and the partial reduction), the column
route (csrc/orp_dcn_bwd.hip) and the autograd entry points BIT FOR BIT against the float64 reference of tests/dcn_bwd_cases.py.

Under the cases' premises (small-integer x, W and grad_out, offsets with fractional part 0 or 1/2, dyadic modulation values; asserted
without a GPU by tests/test_dcn_bwd_cases.py) every product and every partial sum of all four gradients is an fp32 number in any
summation order, the fp16 pieces have lo = 0 and the range scalings are powers of two.  So every route has to return the float64
result converted once to the storage type: EVERY element of every gradient is compared, with no tolerance and nothing masked out.
One thing is not compared: the sign of a zero (0 x negative is -0, and whether a sum of zeros keeps that sign depends on the
association; torch.equal does not see it either) -- got + 0 and want + 0 are compared in their bits.

Before every call the call's workspace is filled with 0xFF bytes and blocks of the outputs' sizes are filled with NaN and freed, so an
element that no kernel writes shows as NaN (the region route runs no memset)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_half_cases as D  # noqa: E402
import dcn_bwd_cases as B  # noqa: E402

GRADS = ("grad_input", "grad_offset", "grad_weight", "grad_mask")
FP32_CASES = [c for c in B.ALL_CASES if c not in B.HALF_CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    assert os.environ.get("ORP_DCN_BWD_SPLIT", "1") != "0", "this file expects the library's default routes"
    return torch.device("cuda:0")


def _bits(t):
    t = t.contiguous().reshape(-1) + 0.0                                  # (-0 -> +0; everything else unchanged)
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _where(case, data, name, level, index):
    """For the message: the sample classes of a grad_offset / grad_mask element, the region of a grad_input element."""
    if name == "grad_input":
        b, _, h, w = index
        return "region %d (image %d, rows %d.., columns %d..)" % (B.region_of(case, level, b, h, w), b, h // 8 * 8, w // 8 * 8)
    if name in ("grad_offset", "grad_mask"):
        b, ch, ho, wo = index
        tap = ch // 2 if name == "grad_offset" else ch
        ki, kj = divmod(tap, case.kw)
        off = data["offs"][level]
        h = ho * case.stride - case.pad + ki * case.dil + float(off[b, 2 * tap, ho, wo])
        w = wo * case.stride - case.pad + kj * case.dil + float(off[b, 2 * tap + 1, ho, wo])
        return "tap %d sampled at (%g, %g): %s" % (tap, h, w, ", ".join(B.sample_class_of(case, level, h, w)))
    return ""


def _assert_bits(case, data, got, want, dtype, what, names=GRADS):
    for name in names:
        w64s, gs = want[name], got[name]
        if w64s is None:
            assert gs is None
            continue
        per_level = isinstance(w64s, list)
        for level, (g, w64) in enumerate(zip(gs if per_level else [gs], w64s if per_level else [w64s])):
            w = w64.to(dtype)
            assert g is not None and g.dtype == dtype and g.shape == w.shape, (case.name, what, name, level)
            diff = _bits(g) != _bits(w)
            bad = int(diff.sum())
            if bad:
                first = int(torch.nonzero(diff)[0])
                index = tuple(int(i) for i in np.unravel_index(first, tuple(w.shape)))
                raise AssertionError("%s, %s, %s%s: %d of %d elements differ in their bits; first at %s: got %r, want %r; %s" % (
                    case.name, what, name, " level %d" % level if per_level else "", bad, w.numel(), index,
                    float(g.reshape(-1)[first]), float(w.reshape(-1)[first]), _where(case, data, name, level, index)))


def _inputs(case, data, gos, dtype, dev):
    t = D.device_inputs(case, data, dtype, dev, False)
    t["gos"] = [g.to(dev).to(dtype) for g in gos]
    return t


def _poison(t, dev):
    """0xFF bytes (NaN in every float type) over the cached workspace, NaN over freed blocks of the outputs' sizes."""
    from orientedreppoints_amd import _lib
    _lib.workspace(dev, 1).fill_(255)
    junk = [torch.full_like(v, float("nan")) for v in t["xs"] + t["offs"] + (t["masks"] or []) + [t["weight"]]]
    junk += [torch.full_like(v, float("nan"), dtype=torch.float32) for v in t["offs"] + (t["masks"] or []) + [t["weight"]]]
    del junk


def _call(case, t, dev, **kw):
    from orientedreppoints_amd.mmdet_ops import deform_conv_backward as bw
    g3 = lambda v: (v, v)                                                 # noqa: E731
    _poison(t, dev)
    out = bw.backward_mfma(t["xs"], t["offs"], t["weight"], t["gos"], g3(case.stride), g3(case.pad), g3(case.dil),
                           masks=t["masks"], **kw)
    none = lambda v: None if v is None or (isinstance(v, list) and all(e is None for e in v)) else v   # noqa: E731
    return dict(grad_input=none(out[0]), grad_offset=none(out[1]), grad_weight=out[2],
                grad_mask=none(out[3]) if case.mask else None)


@pytest.mark.parametrize("case", FP32_CASES, ids=lambda c: c.name)
def test_backward_mfma_is_bitwise_the_float64_reference(dev, case):
    """One backward_mfma call over all levels of the case, four ways: the default route (region pass, fp16 pieces), sparse_grad=True
    (atomic scatter: exact arithmetic has no order), without the weight gradient, without the input gradients."""
    from orientedreppoints_amd import _lib
    assert _lib.lib().orp_dcn_backward_mfma_ok(case.cin, case.cout, case.kh, case.kw, 1, 1) == 1
    data, gos, want = B.expected(case, dev)
    t = _inputs(case, data, gos, torch.float32, dev)
    _assert_bits(case, data, _call(case, t, dev), want, torch.float32, "region route")
    _assert_bits(case, data, _call(case, t, dev, sparse_grad=True), want, torch.float32, "atomic route")
    got = _call(case, t, dev, need_weight=False)
    assert got["grad_weight"] is None
    _assert_bits(case, data, got, want, torch.float32, "need_weight=False", ("grad_input", "grad_offset", "grad_mask"))
    got = _call(case, t, dev, need_input=False)
    assert got["grad_input"] is None and got["grad_offset"] is None and got["grad_mask"] is None
    _assert_bits(case, data, got, want, torch.float32, "need_input=False", ("grad_weight",))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", B.HALF_CASES, ids=lambda c: c.name)
def test_backward_mfma_half_io_is_one_rounding_of_the_float64_reference(dev, case, dtype):
    """fp16 / bf16 tensors in and out: every gradient is the exact value rounded ONCE to the type.  |x| <= 3 and |grad_out| <= 1 keep
    every expected value finite in fp16 (asserted)."""
    data, gos, want = B.expected(case, dev)
    for name in GRADS:
        for w64 in (want[name] if isinstance(want[name], list) else [want[name]] if want[name] is not None else []):
            assert bool(torch.isfinite(w64.to(torch.float16)).all()), "%s: %s is not finite in fp16" % (case.name, name)
    assert any(not bool(D.representable(w64, dtype).all()) for w64 in want["grad_offset"]), "no gradient rounds in the conversion"
    t = _inputs(case, data, gos, dtype, dev)
    _assert_bits(case, data, _call(case, t, dev), want, dtype, "region route, %s" % dtype)
    _assert_bits(case, data, _call(case, t, dev, sparse_grad=True), want, dtype, "atomic route, %s" % dtype)


_CHILD = """
import sys, torch
sys.path.insert(0, %(root)r)
from orientedreppoints_amd.mmdet_ops import deform_conv_backward as bw
dev = torch.device('cuda:0')
cases = torch.load(%(inp)r)
out = {}
for name, c in cases.items():
    mv = lambda v: [t.to(dev) for t in v] if v is not None else None
    for sparse in (False, True):
        r = bw.backward_mfma(mv(c['xs']), mv(c['offs']), c['weight'].to(dev), mv(c['gos']), c['stride'], c['pad'], c['dil'],
                             masks=mv(c['masks']), sparse_grad=sparse)
        out['%%s|%%d' %% (name, sparse)] = [[t.cpu() for t in v] if isinstance(v, list) else v.cpu() for v in r]
torch.cuda.synchronize()
torch.save(out, %(outp)r)
"""


def test_exact_fp32_kernels_are_bitwise_the_float64_reference(dev):
    """ORP_DCN_BWD_SPLIT=0 (read once per process, so ONE child process runs the subset): kernel A's v_mfma_f32_32x32x2_f32 contraction
    on both routes and the exact-fp32 weight kernel."""
    cases = [B.BY_NAME[n] for n in B.SUBSET]
    payload = {}
    for case in cases:
        data, gos, _ = B.expected(case, dev)
        f = lambda v: [t.float() for t in v] if v is not None else None   # noqa: E731
        g3 = lambda v: (v, v)                                             # noqa: E731
        payload[case.name] = dict(xs=f(data["xs"]), offs=f(data["offs"]), masks=f(data["masks"]), weight=data["weight"].float(),
                                  gos=f(gos), stride=g3(case.stride), pad=g3(case.pad), dil=g3(case.dil))
    with tempfile.TemporaryDirectory() as tmp:
        inp, outp = os.path.join(tmp, "in.pt"), os.path.join(tmp, "out.pt")
        torch.save(payload, inp)
        code = _CHILD % dict(root=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), inp=inp, outp=outp)
        run = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ORP_DCN_BWD_SPLIT="0"), stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
        assert run.returncode == 0, run.stdout[-2000:]
        out = torch.load(outp)
    for case in cases:
        data, _, want = B.expected(case, dev)
        for sparse in (False, True):
            r = out['%s|%d' % (case.name, sparse)]
            got = dict(grad_input=[t.to(dev) for t in r[0]], grad_offset=[t.to(dev) for t in r[1]], grad_weight=r[2].to(dev),
                       grad_mask=[t.to(dev) for t in r[3]] if case.mask else None)
            _assert_bits(case, data, got, want, torch.float32, "exact fp32, %s route" % ("atomic" if sparse else "region"))


@pytest.mark.parametrize("name", B.SUBSET)
def test_column_route_is_bitwise_the_float64_reference(dev, name):
    """USE_MFMA = False: the sampling kernels of csrc/orp_dcn_bwd.hip around two library GEMMs, level by level."""
    from orientedreppoints_amd.mmdet_ops import deform_conv_backward as bw
    case = B.BY_NAME[name]
    data, gos, want = B.expected(case, dev)
    t = _inputs(case, data, gos, torch.float32, dev)
    g3 = lambda v: (v, v)                                                 # noqa: E731
    geo = (g3(case.stride), g3(case.pad), g3(case.dil), 1, 1)
    bw.USE_MFMA = False
    try:
        for i in range(len(case.levels)):
            x, off, go = t["xs"][i], t["offs"][i], t["gos"][i]
            if case.mask:
                gi, goff, gm, gw, _ = bw.modulated_backward(x, off, t["masks"][i], t["weight"], go, *geo, False)
            else:
                gi, goff = bw.backward_input(x, off, t["weight"], go, *geo)
                gw, gm = bw.backward_parameters(x, off, t["weight"], go, *geo), None
            got = dict(grad_input=[gi], grad_offset=[goff], grad_weight=gw, grad_mask=[gm] if case.mask else None)
            lvl = dict(grad_input=[want["grad_input"][i]], grad_offset=[want["grad_offset"][i]],
                       grad_weight=want["grad_weight_levels"][i], grad_mask=[want["grad_mask"][i]] if case.mask else None)
            one = case._replace(levels=(case.levels[i],))
            _assert_bits(one, dict(offs=[data["offs"][i]]), got, lvl, torch.float32, "column route, level %d" % i)
    finally:
        bw.USE_MFMA = True


@pytest.mark.parametrize("modulated", [False, True], ids=["deform_conv", "modulated_deform_conv"])
@pytest.mark.parametrize("name", ["geo_3x3_s2", "geo_1x1"])
def test_autograd_entry_points_are_bitwise_the_float64_reference(dev, name, modulated):
    """deform_conv(...).backward and modulated_deform_conv(...).backward at stride 2 and at 1 x 1, level by level: the routes a model
    takes (backward_input + backward_parameters, modulated_backward)."""
    from orientedreppoints_amd.mmdet_ops import deform_conv, modulated_deform_conv, deform_conv_backward as bw
    case = B.BY_NAME[name]._replace(mask=modulated)
    assert bw.USE_MFMA and bw.mfma_ok(torch.empty((256, 256, case.kh, case.kw)), 1, 1)
    if modulated:
        data = B.generate(case)
        gos = B.grad_outputs(case, data)
        for k, (v, unit) in B.premise_bounds(case, data, gos, dev).items():
            assert v < 2.0 ** 24, (name, k, v, unit)
        want = B.reference_backward(case, data, gos, dev)
    else:
        data, gos, want = B.expected(case, dev)
    t = _inputs(case, data, gos, torch.float32, dev)
    for i in range(len(case.levels)):
        leaves = [v.clone().requires_grad_(True) for v in [t["xs"][i], t["offs"][i], t["weight"]] + ([t["masks"][i]] if modulated else [])]
        _poison(t, dev)
        if modulated:
            y = modulated_deform_conv(leaves[0], leaves[1], leaves[3], leaves[2], None, case.stride, case.pad, case.dil, 1, 1)
        else:
            y = deform_conv(leaves[0], leaves[1], leaves[2], case.stride, case.pad, case.dil, 1, 1)
        y.backward(t["gos"][i])
        got = dict(grad_input=[leaves[0].grad], grad_offset=[leaves[1].grad], grad_weight=leaves[2].grad,
                   grad_mask=[leaves[3].grad] if modulated else None)
        lvl = dict(grad_input=[want["grad_input"][i]], grad_offset=[want["grad_offset"][i]],
                   grad_weight=want["grad_weight_levels"][i], grad_mask=[want["grad_mask"][i]] if modulated else None)
        one = case._replace(levels=(case.levels[i],))
        _assert_bits(one, dict(offs=[data["offs"][i]]), got, lvl, torch.float32, "autograd, level %d" % i)
