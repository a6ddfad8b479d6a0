"""GPU: the fused GroupNorm(+ReLU) family of csrc/orp_norm.hip through orientedreppoints_amd/mmdet_ops/fused_norm.py --
group_norm_act_multi (NCHW, and its nhwc= entries), group_norm_act_train (forward and backward) and group_norm_act_multi_cl
(channels-last, with and without the range word) -- on every case of tests/norm_cases.py: levels exactly on, one below and one
above a 4096-float chunk, spans of one and two elements, tails of one, two and eight, channels that straddle a chunk border for
1, 2, 3, 8 and 32 channels per group, sixteen tensors with two modules in turn; data whose fp32 statistics are hard (mean a
thousand deviations out, variance far below eps, a span without variance).

Checker: the float64 reference of tests/norm_cases.py, judged by norm_cases.judge_launch -- forward within
max(4 * 2^-23 * (max |x| max rstd max |gamma| + max |beta|), 2 e_stock), gradients within max(2e-5 of scale, 2 e_stock), where
e_stock is the stock fp32 torch GroupNorm's own error against the same reference on the same tensor (taken on the CPU: the very
figures tests/test_norm_cases.py holds the emulation to).  The backward reference takes the kernel's own `y > 0` as its gate,
and the gate is compared with the reference's wherever the forward bound decides it.  tests/test_norm_cases.py shows without a
GPU that this judge fails a tail chunk counted as full, a channel index one element early and a gate read from x.

Under ReLU the kernels give +0 for a NaN (fmaxf), the framework NaN: DESIGN.md, fused-norm contract.  Nothing here asserts a
poisoned span's forward value under ReLU; without ReLU, and in every gradient, the poison must show."""
import os
import sys

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import norm_cases as N  # noqa: E402

ALL = [(s.name, B, kind) for s in N.SETS for B in N.BATCHES for kind in N.KINDS]
ALL_CL = [(s.name, B, kind) for s in N.CL_SETS for B in N.BATCHES for kind in N.KINDS]
_id = lambda v: "-".join(str(t) for t in v)          # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture()
def ranges_mode():
    """the fp16-pieces mode: the one in which producers leave range words (fused_norm._ranges_wanted)"""
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    assert L.orp_dcn_set_split_mode(3) == 0
    yield
    L.orp_dcn_set_split_mode(-1)


def _modules(c, dev):
    """(distinct modules, one per tensor)"""
    mods = []
    for ga, be in zip(c.gammas, c.betas):
        m = nn.GroupNorm(c.set.G, c.set.C, eps=N.EPS).to(dev)
        with torch.no_grad():
            m.weight.copy_(ga); m.bias.copy_(be)
        mods.append(m)
    return mods, [mods[o] for o in c.owner]


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


_FIG, _LINE = {}, {}


def _report(route, kind, fig):
    """one line per (route, data kind) in the session's report: the maxima over every case judged so far"""
    import conftest
    key = (route, kind)
    acc = _FIG.setdefault(key, {})
    for k, v in fig.items():
        acc[k] = max(acc.get(k, 0.0), v)
    if key in _LINE and _LINE[key] in conftest.REPORT:
        conftest.REPORT.remove(_LINE[key])
    _LINE[key] = N.figures_line("GroupNorm %s, %s data, max over cases (kernel err / stock fp32 err / bound terms)" % key, acc)
    conftest.REPORT.append(_LINE[key])


def _judged(c, relu, ys, grads, route):
    rep = N.judge_launch(c, relu, ys, grads)
    _report(route, c.kind, rep.figures)
    assert not rep.fails, "%s %s B=%d %s relu=%s: (what, tensor / module, err, bound) %s | %s" % (
        route, c.set.name, c.B, c.kind, relu, rep.fails[:6], N.figures_line("figures", rep.figures))
    return rep


# ---- group_norm_act_multi ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=_id)
def test_multi_vs_float64(dev, case):
    from orientedreppoints_amd.mmdet_ops.fused_norm import group_norm_act_multi
    c = N.make_case(*case)
    mods, gns = _modules(c, dev)
    gn = gns if len(mods) > 1 else mods[0]
    xs = [x.to(dev) for x in c.xs]
    keep = [x.clone() for x in xs]
    with torch.no_grad():
        for relu in (True, False):
            out = group_norm_act_multi(xs, gn, relu=relu, inplace=False)
            for x, k, y in zip(xs, keep, out):
                assert _same_bits(x, k) and y.data_ptr() != x.data_ptr() and y.shape == x.shape and y.is_contiguous()
            _judged(c, relu, out, None, "multi")
            ins = [x.clone() for x in xs]
            inp = group_norm_act_multi(ins, gn, relu=relu)                       # in place is the default
            again = group_norm_act_multi(xs, gn, relu=relu, inplace=False)
            for a, b, y, z in zip(inp, ins, out, again):
                assert a.data_ptr() == b.data_ptr() and _same_bits(a, y) and _same_bits(z, y)


@pytest.mark.parametrize("kind", ("plain", "const"))
@pytest.mark.parametrize("B", N.BATCHES)
@pytest.mark.parametrize("name", N.NHWC_SETS)
def test_multi_nhwc_entries_have_the_nchw_bits(dev, name, B, kind):
    """nhwc='only' / 'both': channels-last results with the bits of the NCHW entry ("Same arithmetic as gn_apply_kernel:
    identical values"); with 'both' the NCHW tensors are the in-place results."""
    from orientedreppoints_amd.mmdet_ops.fused_norm import group_norm_act_multi
    c = N.make_case(name, B, kind)
    mods, gns = _modules(c, dev)
    xs = [x.to(dev) for x in c.xs]
    with torch.no_grad():
        for relu in (True, False):
            base = group_norm_act_multi(xs, gns, relu=relu, inplace=False)
            only = group_norm_act_multi([x.clone() for x in xs], gns, relu=relu, nhwc='only')
            ins = [x.clone() for x in xs]
            both = group_norm_act_multi(ins, gns, relu=relu, nhwc='both')
            assert isinstance(only, list) and isinstance(both, tuple) and len(both) == 2
            for i, y in enumerate(base):
                for t in (only[i], both[1][i]):
                    assert t.shape == y.shape and t.is_contiguous(memory_format=torch.channels_last), (i, t.stride())
                    assert torch.equal(_bits(_cl(y)), _bits(t)), (name, B, kind, relu, i)
                assert both[0][i].data_ptr() == ins[i].data_ptr() and _same_bits(both[0][i], y), (name, B, kind, relu, i)


# ---- group_norm_act_train -----------------------------------------------------------------------------------------------------------------
def _step(c, dev, mods, gns, relu, xs=None, dys=None):
    from orientedreppoints_amd.mmdet_ops.fused_norm import group_norm_act_train
    for m in mods:
        m.weight.grad = None; m.bias.grad = None
    xs = [x.to(dev).requires_grad_(True) for x in c.xs] if xs is None else xs
    ys = group_norm_act_train(xs, gns if len(mods) > 1 else mods[0], relu=relu)
    torch.autograd.backward(ys, [d.to(dev) for d in (c.dys if dys is None else dys)])
    return ys, ([x.grad for x in xs], [m.weight.grad.clone() for m in mods], [m.bias.grad.clone() for m in mods])


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_train_forward_backward_vs_float64(dev, case):
    from orientedreppoints_amd.mmdet_ops.fused_norm import group_norm_act_multi
    c = N.make_case(*case)
    s = c.set
    mods, gns = _modules(c, dev)
    zero, minus, _ = N.gate_channels(s.C)
    for relu in (True, False):
        ys, grads = _step(c, dev, mods, gns, relu)
        with torch.no_grad():
            base = group_norm_act_multi([x.to(dev) for x in c.xs], gns, relu=relu, inplace=False)
        for y, b in zip(ys, base):
            assert y.dtype == torch.float32 and _same_bits(y, b)
        _judged(c, relu, ys, grads, "train")
        for dg, db in zip(grads[1], grads[2]):
            if relu:                              # y == 0 in both channels (gamma = beta = 0; gamma = 0, beta = -1): the gate is shut
                assert float(dg[zero]) == 0.0 and float(db[zero]) == 0.0 and float(dg[minus]) == 0.0 and float(db[minus]) == 0.0
        for lv, dx in zip(s.levels, grads[0]):
            if lv.span == 1:
                assert not bool(dx.any()), "a span of one element has no gradient: %s" % dx.flatten()[:8]
        ys2, grads2 = _step(c, dev, mods, gns, relu)
        for a, b in zip(list(ys) + grads[0] + grads[1] + grads[2], list(ys2) + grads2[0] + grads2[1] + grads2[2]):
            assert _same_bits(a, b), "a repeated step must give the same bits"


@pytest.mark.parametrize("B", N.BATCHES)
def test_train_loss_forms(dev, B):
    """One level's .sum() as the whole loss (its incoming gradient is a stride-0 expansion, every other level's output is unused
    and must get an all-zero gradient); one level handed in with channels-last memory; half inputs under autocast."""
    from orientedreppoints_amd.mmdet_ops.fused_norm import group_norm_act_train
    c = N.make_case("T2", B, "plain")
    mods, gns = _modules(c, dev)
    used = 2                                                                      # (3, 683): a tail of two
    for relu in (True, False):
        xs = [x.to(dev).requires_grad_(True) for x in c.xs]
        ys = group_norm_act_train(xs, mods[0], relu=relu)
        for m in mods:
            m.weight.grad = None; m.bias.grad = None
        ys[used].sum().backward()
        dys = tuple(torch.ones_like(d) if i == used else torch.zeros_like(d) for i, d in enumerate(c.dys))
        grads = ([x.grad for x in xs], [mods[0].weight.grad], [mods[0].bias.grad])
        for i, x in enumerate(xs):
            assert x.grad is not None and x.grad.shape == x.shape
            if i != used:
                assert not bool(x.grad.any()), "level %d does not enter the loss" % i
        _judged(c._replace(dys=dys), relu, ys, grads, "train")
        # channels-last memory for one level: the values and gradients of the contiguous call
        ref_y, ref_g = _step(c, dev, mods, gns, relu)
        xs = [x.to(dev) for x in c.xs]
        xs[0] = _cl(xs[0])
        assert not xs[0].is_contiguous()
        xs = [x.requires_grad_(True) for x in xs]
        got_y, got_g = _step(c, dev, mods, gns, relu, xs=xs)
        for a, b in zip(list(ref_y) + ref_g[0] + ref_g[1] + ref_g[2], list(got_y) + got_g[0] + got_g[1] + got_g[2]):
            assert a.shape == b.shape and torch.equal(a, b)
        # autocast: half in, fp32 out, inside the forward bound of the half-rounded inputs
        xh = [x.to(dev).half() for x in c.xs]
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            yh = group_norm_act_train(xh, mods[0], relu=relu)
        assert all(y.dtype == torch.float32 for y in yh)
        _judged(c._replace(xs=tuple(x.float().cpu() for x in xh)), relu, yh, None, "train under autocast")


# ---- group_norm_act_multi_cl ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CL, ids=_id)
def test_channels_last_vs_float64(dev, ranges_mode, case):
    from orientedreppoints_amd.mmdet_ops.fused_norm import group_norm_act_multi_cl
    c = N.make_case(*case)
    mods, gns = _modules(c, dev)
    xs = [_cl(x.to(dev)) for x in c.xs]
    keep = [x.clone() for x in xs]
    slots = [i % 2 for i in range(len(xs))]
    with torch.no_grad():
        for relu in (True, False):
            out = group_norm_act_multi_cl(xs, mods[0], relu=relu, inplace=False)
            for x, k, y in zip(xs, keep, out):
                assert _same_bits(x, k) and y.data_ptr() != x.data_ptr() and y.is_contiguous(memory_format=torch.channels_last)
            _judged(c, relu, out, None, "channels-last")
            ins = [x.clone() for x in xs]
            inp, bits = group_norm_act_multi_cl(ins, mods[0], relu=relu, amax_slots=slots)
            assert bits is not None and bits.dtype == torch.int32 and bits.numel() == max(slots) + 1
            for a, b, y in zip(inp, ins, out):
                assert a.data_ptr() == b.data_ptr() and torch.equal(a, y)
            word = bits.view(torch.float32).cpu()
            for sl in set(slots):
                true_max = max(float(y.abs().max()) for y, s_ in zip(out, slots) if s_ == sl)
                assert bool(torch.isfinite(word[sl])) and float(word[sl]) >= true_max, (sl, float(word[sl]), true_max)
            again, bits2 = group_norm_act_multi_cl([x.clone() for x in xs], mods[0], relu=relu, amax_slots=slots)
            assert torch.equal(bits, bits2) and all(torch.equal(a, y) for a, y in zip(again, out))


# ---- one NaN, one +inf: nothing else changes -------------------------------------------------------------------------------------------------
def _span_mask(shape, G, b, g):
    m = torch.zeros(shape, dtype=torch.bool)
    cg = shape[1] // G
    m[b, g * cg:(g + 1) * cg] = True
    return m


@pytest.mark.parametrize("route", ("multi", "nhwc", "train", "cl"))
def test_non_finite_stays_in_its_span(dev, ranges_mode, route):
    from orientedreppoints_amd.mmdet_ops import fused_norm as fn
    B = 3
    if route == "cl":
        c = N.make_case("CL256", B, "plain")
        nan_at, inf_at = (3, 1, 5), (1, 2, 31)            # hw 32: the NaN sits in the second chunk; hw 17: the inf in the tail
        pos = {3: (2, 4), 1: (0, 16)}
    else:
        c = N.make_case("T1", B, "plain")
        nan_at, inf_at = (6, 1, 5), (1, 2, 31)            # nine chunks, the NaN in one of them; the inf is the span's last element
        pos = {6: (9, 100), 1: (26, 18)}
    s = c.set
    cg = s.C // s.G
    mods, gns = _modules(c, dev)
    salted = [x.clone() for x in c.xs]
    (ln, bn, gn_), (li, bi, gi) = nan_at, inf_at
    salted[ln][bn, gn_ * cg + cg // 2, pos[ln][0], pos[ln][1]] = float("nan")
    salted[li][bi, gi * cg + cg - 1, pos[li][0], pos[li][1]] = float("inf")
    hit = [torch.zeros(x.shape, dtype=torch.bool) for x in c.xs]
    hit[ln] |= _span_mask(c.xs[ln].shape, s.G, bn, gn_)
    hit[li] |= _span_mask(c.xs[li].shape, s.G, bi, gi)

    def run(data, relu):
        """-> {name: list of tensors per level}, range words or None"""
        if route == "train":
            xs = [x.to(dev).requires_grad_(True) for x in data]
            ys = fn.group_norm_act_train(xs, mods[0], relu=relu)
            torch.autograd.backward(ys, [d.to(dev) for d in c.dys])
            return {"y": [y.detach() for y in ys], "dx": [x.grad for x in xs]}, None
        with torch.no_grad():
            xs = [x.to(dev) for x in data]
            if route == "multi":
                return {"y": fn.group_norm_act_multi(xs, mods[0], relu=relu)}, None
            if route == "nhwc":
                nchw, cl = fn.group_norm_act_multi(xs, mods[0], relu=relu, nhwc='both')
                return {"y": nchw, "y_nhwc": cl}, None
            outs, bits = fn.group_norm_act_multi_cl([_cl(x) for x in xs], mods[0], relu=relu, amax_slots=list(range(len(xs))))
            return {"y": outs}, bits.cpu()

    for relu in (True, False):
        clean, cw = run(c.xs, relu)
        dirty, dw = run(salted, relu)
        for name in clean:
            for i, (a, b) in enumerate(zip(clean[name], dirty[name])):
                a, b = a.cpu(), b.cpu()
                same = a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)
                assert bool(same[~hit[i]].all()), "%s %s level %d: a span without poison changed" % (route, name, i)
                assert bool(torch.isfinite(a).all())
                if name == "dx" or not relu:                                 # (the forward under ReLU: module docstring)
                    assert bool(torch.isnan(b[hit[i]]).all()), "%s %s level %d relu=%s: the poisoned span must be NaN" % (route, name, i, relu)
        if cw is not None:
            # range words: a poisoned span hands in 0 = "no bound" and the word stays the bound of the slot's other spans
            # (atomicMax; orp_range.hpp: a non-finite element spreads to the outputs that read it and to no other)
            cwf, dwf = cw.view(torch.float32), dw.view(torch.float32)
            for i in range(len(c.xs)):
                if i in (ln, li):
                    rest = float(clean["y"][i].cpu()[~hit[i]].abs().max())
                    assert bool(torch.isfinite(dwf[i])) and rest <= float(dwf[i]) <= float(cwf[i]), (i, float(dwf[i]), rest)
                else:
                    assert int(dw[i]) == int(cw[i]) and int(cw[i]) > 0
    if route == "cl":
        # ... and where the poisoned span is the slot's only one (one image, one group), the word IS 0
        c1 = N.make_case("CL32", 1, "plain")
        m1, _ = _modules(c1, dev)
        xs = [x.clone() for x in c1.xs]
        xs[0][0, 7, 3, 5] = float("nan")
        xs[1][0, 31, 2, 42] = float("inf")                   # the last position: the one-position tail chunk
        with torch.no_grad():
            for relu in (True, False):
                ys, bits = fn.group_norm_act_multi_cl([_cl(x.to(dev)) for x in xs], m1[0], relu=relu, amax_slots=[0, 1])
                assert bits.cpu().tolist() == [0, 0], "the range word of a slot whose only span is poisoned: 0 = no bound"
                if not relu:
                    assert all(bool(torch.isnan(y).all()) for y in ys)


# ---- argument edges: raise, and launch nothing ------------------------------------------------------------------------------------------------
def test_argument_edges_raise_and_do_not_launch(dev):
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops import fused_norm as fn
    g = torch.Generator().manual_seed(5)

    def data(n, B, C, cl=False):
        xs = [torch.randn(B, C, 3, 4, generator=g).to(dev) for _ in range(n)]
        return [_cl(x) for x in xs] if cl else xs

    def refused(call, xs, errors=(ValueError,)):
        keep = [x.clone() for x in xs]
        with pytest.raises(errors):
            call(xs)
        torch.cuda.synchronize()
        for x, k in zip(xs, keep):
            assert _same_bits(x, k), "a refused call must not have launched"

    def gn(G, C, eps=1e-5):
        return nn.GroupNorm(G, C, eps=eps).to(dev)

    any_err = (ValueError, _lib.OrpHipError)
    # cg = 3 (T5): the NCHW entry only
    t5 = N.SET["T5"]
    m96 = gn(t5.G, t5.C)
    for mode in ('only', 'both'):
        refused(lambda xs: fn.group_norm_act_multi(xs, m96, nhwc=mode), data(3, 2, t5.C))
    refused(lambda xs: fn.group_norm_act_multi(xs, m96, nhwc='neither'), data(3, 2, t5.C))
    refused(lambda xs: fn.group_norm_act_multi_cl(xs, m96), data(3, 2, t5.C, cl=True))
    # kGnMaxLevels + 1 tensors
    m64 = gn(8, 64)
    n = N.MAX_LEVELS + 1
    refused(lambda xs: fn.group_norm_act_multi(xs, m64), data(n, 2, 64), any_err)
    refused(lambda xs: fn.group_norm_act_multi(xs, m64, nhwc='both'), data(n, 2, 64), any_err)
    refused(lambda xs: fn.group_norm_act_multi_cl(xs, m64), data(n, 2, 64, cl=True), any_err)
    refused(lambda xs: fn.group_norm_act_train(xs, m64), data(n, 2, 64), any_err)
    with torch.no_grad():
        assert len(fn.group_norm_act_multi(data(N.MAX_LEVELS, 2, 64), m64)) == N.MAX_LEVELS        # sixteen are taken
    # unequal B or C
    for other in ((3, 64), (2, 128)):
        for cl in (False, True):
            xs = data(2, 2, 64, cl) + data(1, other[0], other[1], cl)
            if cl:
                refused(lambda t: fn.group_norm_act_multi_cl(t, m64), xs)
            else:
                refused(lambda t: fn.group_norm_act_multi(t, m64), xs)
                refused(lambda t: fn.group_norm_act_train(t, m64), xs)
    # modules that disagree in eps or in the number of groups
    for bad in (gn(8, 64, eps=1e-3), gn(16, 64)):
        refused(lambda t: fn.group_norm_act_multi(t, [m64, bad]), data(2, 2, 64))
        refused(lambda t: fn.group_norm_act_train(t, [m64, bad]), data(2, 2, 64))
        refused(lambda t: fn.group_norm_act_multi_cl(t, [m64, bad]), data(2, 2, 64, cl=True))
    # channels-last entry handed NCHW memory
    refused(lambda t: fn.group_norm_act_multi_cl(t, m64), data(2, 2, 64))
