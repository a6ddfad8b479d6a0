"""No GPU: the case tables of tests/norm_cases.py hold what tests/test_gpu_norm.py relies on.

* every level sits on the chunk edge it declares (re-derived from C, G, H, W);
* the float64 reference is torch's float64 autograd of the stock operator to 1e-12 of scale, ReLU both ways, on every case;
* the gate band (elements whose ReLU gate the forward bound cannot decide) stays under norm_cases.BAND_CAP of every tensor;
* the table notices faults: a numpy fp32 emulation of the chunked scheme passes the judge as it is, and fails it by at least ten
  times the bound with each of three planted faults (a tail chunk counted as full, a channel index one element early, the gate
  read from x).

The `offset` kind (x ~ N(1000, 1)) is outside the band cap by its own arithmetic, not by a choice of seed: the forward bound is
4 * 2^-23 * 1000 * rstd * gamma ~ 1e-3 of an output of unit deviation, whose density at zero is ~0.4, so ~8e-4 of the elements lie
inside whatever the seed (measured 3e-4 .. 1e-3 on the large levels).  Its share is bounded by that reasoning instead (see
test_gate_band_cap) and the gate is still compared everywhere outside the band."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_cases as N  # noqa: E402

ALL = [(s.name, B, kind) for s in N.SETS for B in N.BATCHES for kind in N.KINDS]
ALL_CL = [(s.name, B, kind) for s in N.CL_SETS for B in N.BATCHES for kind in N.KINDS]
_id = lambda v: "-".join(str(t) for t in v)          # noqa: E731


def test_every_level_sits_on_its_declared_edge():
    for s in N.SETS:
        cg = s.C // s.G
        assert s.C % s.G == 0 and len(s.levels) <= N.MAX_LEVELS
        for lv in s.levels:
            hw = lv.h * lv.w
            span = cg * hw
            cpg = (span + N.CHUNK - 1) // N.CHUNK
            assert span == lv.span, (s.name, lv)
            assert span - N.CHUNK * (cpg - 1) == lv.tail and 1 <= lv.tail <= N.CHUNK, (s.name, lv)
            assert (span % 4 == 0) == lv.stat_vec and (hw % 4 == 0) == lv.apply_vec, (s.name, lv)
        eligible = s.C % 32 == 0 and 32 % cg == 0                      # what the nhwc= entry takes
        assert eligible == (s.name in N.NHWC_SETS or s.name == "T6") and eligible != s.nchw_only, s.name
    spans = {s.name: [lv.span for lv in s.levels] for s in N.SETS}
    tails = {s.name: [lv.tail for lv in s.levels] for s in N.SETS}
    # the edges the table exists for: exactly on / one below / one above a chunk, spans of 1 and 2, tails of 1, 2 and 8, both
    # disagreements of the two passes' vector conditions, a channel that straddles a chunk border for cg = 1, 2, 3, 8 and 32
    assert {4096, 4104, 4088, 8192, 8, 32776} <= set(spans["T1"]) and {4096, 4050, 4098, 4, 2} <= set(spans["T2"])
    assert spans["T3"] == [4096, 4095, 4097, 1] and 1 in tails["T3"] and 2 in tails["T2"] and 8 in tails["T1"]
    assert {4096, 4128, 32} == set(spans["T4"]) and {4095, 4098, 48} == set(spans["T5"])
    assert any(lv.stat_vec and not lv.apply_vec for lv in N.SET["T1"].levels)
    for name in ("T1", "T2", "T3", "T4", "T5"):
        s = N.SET[name]
        assert any(lv.span > N.CHUNK and N.CHUNK % (lv.h * lv.w) != 0 for lv in s.levels), name + ": no channel crosses a chunk border"
    t6 = N.SET["T6"]
    assert len(t6.levels) == N.MAX_LEVELS and set(N.owners(t6)) == {0, 1} and N.owners(t6)[0] != N.owners(t6)[1]
    for s in N.CL_SETS:
        ppc = N.CHUNK // s.C
        assert 1024 % s.C == 0 and (s.C // s.G) % 4 == 0, s.name
        for lv in s.levels:
            assert lv.h * lv.w == lv.hw and lv.hw - ppc * ((lv.hw + ppc - 1) // ppc - 1) == lv.tail, (s.name, lv)
        hws = [lv.hw for lv in s.levels]
        assert ppc in hws and ppc + 1 in hws, s.name                         # exactly one chunk, and one position more
    assert [lv.hw for lv in N.CL_SET["CL256"].levels] == [16, 17, 15, 32, 1]
    assert [lv.hw for lv in N.CL_SET["CL1024"].levels] == [4, 5, 3, 1]
    assert N.CL_SET["CL128"].C // N.CL_SET["CL128"].G == 4


def test_case_data_is_what_the_kinds_say():
    for name in ("T2", "CL64"):
        for kind in N.KINDS:
            c = N.make_case(name, 3, kind)
            s = c.set
            z, m1, h5 = N.gate_channels(s.C)
            for ga, be in zip(c.gammas, c.betas):
                assert ga[z] == 0 and be[z] == 0 and ga[m1] == 0 and be[m1] == -1 and ga[h5] == 0 and be[h5] == 0.5
            x = c.xs[0]
            if kind == "offset":
                assert abs(float(x.mean()) - 1000) < 0.1 and 0.9 < float(x.std()) < 1.1
            if kind == "flat":
                assert float(x.var()) < 1e-2 * N.EPS
            if kind == "const":
                b, g = N.const_span(3, s.G)
                cg = s.C // s.G
                for t in c.xs:
                    assert bool((t[b, g * cg:(g + 1) * cg] == N.CONST_VALUE).all())
                    assert float(N.ref_forward(t, c.gammas[0], c.betas[0], s.G).var[b, g]) == 0.0


@pytest.mark.parametrize("case", ALL + ALL_CL, ids=_id)
def test_reference_is_float64_autograd(case):
    c = N.make_case(*case)
    s = c.set
    for relu in (True, False):
        for i in range(len(s.levels)):
            ga, be = c.gammas[c.owner[i]], c.betas[c.owner[i]]
            x = c.xs[i].double().requires_grad_(True)
            g64, b64 = ga.double().requires_grad_(True), be.double().requires_grad_(True)
            y = torch.group_norm(x, s.G, g64, b64, N.EPS)
            y = F.relu(y) if relu else y
            y.backward(c.dys[i].double())
            fwd = N.ref_forward(c.xs[i], ga, be, s.G)
            dx, dg, db = N.ref_backward(fwd, ga, c.dys[i], (fwd.z > 0) if relu else None, s.G)
            # 1e-12 of scale, or where that is beyond float64 itself (x ~ 1000 +- 1, a span of one or two elements): 64
            # roundings of a float64 mean carried through rstd, once for y and once more through rstd for the gradients.
            # Measured: at most 0.8 and 1.9 of 2^-53 * cond (* rstd) per element, more on dgamma, which sums a span's common shift.
            cond = 64 * 2.0 ** -53 * float(c.xs[i].abs().max()) * float(fwd.rstd.max())
            rel_y, rel_g = max(1e-12, cond), max(1e-12, cond * max(1.0, float(fwd.rstd.max())))
            for got, want, rel in ((N.relu_of(fwd.z, relu), y.detach(), rel_y), (dx, x.grad, rel_g), (dg, g64.grad, rel_g),
                                   (db, b64.grad, rel_g)):
                assert float((got - want).abs().max()) <= rel * max(1.0, float(want.abs().max())), (case, relu, i, rel)


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_gate_band_cap(case):
    """The condition the backward comparison stands on: all but BAND_CAP of a tensor's elements have a gate the forward bound
    decides.  `offset`: the band is as wide as the bound the data's mean forces (module docstring); there the share must stay
    under the density argument's figure, 2 * bound * 0.5 per unit of output, i.e. under the widest span bound itself."""
    c = N.make_case(*case)
    s = c.set
    for i in range(len(s.levels)):
        ga, be = c.gammas[c.owner[i]], c.betas[c.owner[i]]
        fwd = N.ref_forward(c.xs[i], ga, be, s.G)
        stock = N.stock_forward(c.xs[i], ga, be, s.G, False)
        outside, share = N.gate_band(c.xs[i], fwd, stock, ga, be, s.G)
        if c.kind == "offset":
            numel = c.xs[i].numel()
            widest = float(N.span_bounds(c.xs[i], fwd, stock, ga, be, s.G).max())
            assert share <= widest + 3.0 * (widest / numel) ** 0.5, (case, i, share, widest)   # + 3 deviations of such a count
        else:
            assert share <= N.BAND_CAP, (case, i, share)
        # and the stock module, a correct fp32 implementation, has the reference's gate outside the band
        assert not bool((((stock > 0) != (fwd.z > 0)) & outside).any()), (case, i)


EMU = [(s.name, B, kind) for s in N.SETS for B in N.BATCHES for kind in N.KINDS]


@pytest.mark.parametrize("case", EMU, ids=_id)
def test_emulation_passes_the_judge(case):
    c = N.make_case(*case)
    for relu in ((True, False) if c.B == 1 else (True,)):
        ys, dxs, dgs, dbs = N.emulate(c, relu)
        rep = N.judge_launch(c, relu, ys, (dxs, dgs, dbs))
        assert not rep.fails, (case, relu, rep.fails[:4], N.figures_line("figures", rep.figures))


@pytest.mark.parametrize("fault", [f for f in N.FAULTS if f])
def test_planted_fault_is_caught(fault):
    caught = []
    for s in N.SETS:
        c = N.make_case(s.name, 1, "plain")
        ys, dxs, dgs, dbs = N.emulate(c, True, fault=fault)
        rep = N.judge_launch(c, True, ys, (dxs, dgs, dbs))
        if rep.fails and rep.worst >= 10.0:
            caught.append("%s %s at %.0f x the bound" % (s.name, sorted({(w, i) for w, i, _, _ in rep.fails})[:6], min(rep.worst, 1e9)))
    assert caught, "no case of the table fails the judge by 10 x the bound with the fault '%s'" % fault
    print("fault '%s' caught by: %s" % (fault, "; ".join(caught)))
