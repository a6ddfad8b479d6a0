"""Helper of the DeformConv backward tests (not a conftest, no tests in here): exact-arithmetic cases for the MFMA backward
(csrc/orp_dcn_bwd_mfma.hip) and a float64 reference of all four gradients written from the definition in plain torch indexing.

The idea is dcn_half_cases.py's, carried to the gradients.  With small-integer x, W and grad_out, offsets whose fractional part
is 0 or 1/2 and modulation values in {0, 1/2, 1, 3/2}:
  * G_t = grad_out . W[:, :, tap] is an integer; every bilinear weight (times the modulation) is a multiple of 1/8 (1/4 without
    modulation); every term of grad_input and grad_weight is a multiple of 1/8, every term of grad_offset and grad_mask a multiple
    of 1/4 (the coordinate derivative has ONE bilinear factor, grad_mask none of the modulation);
  * `premise_bounds` adds up the ABSOLUTE values of the terms of every output element, per corner; below 2^24 units every partial
    sum is an fp32 number in any summation order and any association of the products;
  * the fp16 pieces of grad_out, W and the sampled columns have lo = 0 (a few significand bits) and the range scalings are powers
    of two.
So the fp16-pieces kernels, the exact-fp32 kernels, the region route, the atomic route and the column route all have to return
the BITS of the float64 result.  tests/test_dcn_bwd_cases.py asserts the premises and that no case is vacuous, without a GPU;
tests/test_gpu_dcn_bwd_exact.py runs the kernels.

The structure the cases aim at (csrc/orp_dcn_bwd_mfma.hip): 32-position chunks that straddle images but not levels, the list of
ACTIVE chunks (any non-zero grad_out value) cut into 8 slabs, 8 x 8-pixel regions of grad_input whose (sample, region) lists are
walked 64 entries at a time in steps of 16, empty regions that still write zeros, up to 8 levels per call.

Every case is 256 -> 256: the MFMA route accepts nothing else.  Nothing here calls an orp_* entry point."""
import collections
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcn_half_cases as D  # noqa: E402

Case = D.Case
Meta = collections.namedtuple("Meta", "pattern steer go_max")
META = {}
# pattern (grad_out): "dense" | "rows" (a few non-zero rows per level) | "level_zero" | "image_zero" | "channel_edge" (rows whose
#   only non-zero value is in channel 0 or in channel 255) | "zero" | ("chunks", n) (exactly n active chunks)
# steer (offsets): None = dcn_half_cases' steered generator | "one_region" (every sample's footprint inside region (0, 0) of its
#   image) | "outside" (every sample at or beyond H)
GO_MAX = 3                                 # |grad_out| <= 3 (7 would leave grad_offset less than one bit below 2^24 units)


def _b(name, levels, pattern="dense", steer=None, go_max=GO_MAX, **kw):
    assert name not in META
    META[name] = Meta(pattern, steer, go_max)
    return D._c(name, levels, **kw)


# ---- chunks: level sizes around the 32-position chunk, chunks across images, MAXL levels, active-chunk counts around the 8 slabs --
_AL = [(9, 11), (12, 13)]                  # B = 2: 7 + 10 = 17 chunks
CHUNK_CASES = [
    _b("chunk_sizes", [(1, 1), (1, 31), (4, 8), (3, 11), (5, 13)], seed=201),             # 1, 31, 32, 33, 65 positions
    _b("chunk_straddle", [(5, 5)], batch=3, mask=True, seed=202),                          # 25 positions per image, 3 chunks
    _b("chunk_8levels", [(1, 1), (2, 3), (3, 3), (1, 2), (5, 5), (4, 7), (2, 2), (6, 5)], batch=2, seed=203),
    _b("active_1", _AL, batch=2, pattern=("chunks", 1), seed=204),
    _b("active_7", _AL, batch=2, pattern=("chunks", 7), seed=205),
    _b("active_8", _AL, batch=2, pattern=("chunks", 8), mask=True, seed=206),
    _b("active_9", _AL, batch=2, pattern=("chunks", 9), seed=207),
    _b("active_17", _AL, batch=2, seed=208),                                               # dense: all 17
]
# ---- regions: maps around the 8 x 8 region, region counts 1, 2, 6, 18, 42; lists of exactly 64 and 65 entries; a pile-up -----------
_RM = [(1, 1), (7, 9), (8, 8), (9, 8), (16, 17), (19, 21)]
REGION_CASES = [
    _b("reg_1x1", [(1, 1)], batch=2, seed=211),
    _b("reg_7x9", [(7, 9)], seed=212),
    _b("reg_8x8", [(8, 8)], mask=True, seed=213),
    _b("reg_9x8", [(9, 8)], batch=3, seed=214),
    _b("reg_16x17", [(16, 17)], mask=True, seed=215),
    _b("reg_19x21", [(19, 21)], batch=2, seed=216),
    _b("reg_all_maps", _RM, batch=2, mask=True, seed=217),
    _b("reg_one_64", [(8, 8)], steer="one_region", k=(1, 1), pad=0, seed=218),             # 64 samples -> one list of 64
    _b("reg_one_65", [(5, 13)], steer="one_region", k=(1, 1), pad=0, mask=True, seed=219),  # 65 samples -> one list of 65, one empty
    _b("reg_pileup", [(19, 21)], steer="one_region", seed=220),                             # 3591 entries in 1 of 9 regions
    _b("reg_outside", [(9, 11), (8, 8)], batch=2, steer="outside", mask=True, seed=221),    # nothing lands: every gradient is zero
]
# ---- borders: every class of the bilinear sampler, DCNv1 and DCNv2 ------------------------------------------------------------------
BORDER_CASES = [
    _b("bord_9x11_v1", [(9, 11)], batch=2, seed=231),
    _b("bord_9x11_v2", [(9, 11)], batch=2, mask=True, seed=232),
    _b("bord_40x40_v1", [(40, 40)], batch=2, seed=233),
    _b("bord_40x40_v2", [(40, 40)], batch=2, mask=True, seed=234),
]
# ---- geometry: what a backbone's dcn= stage and the general kh x kw signature can send down the MFMA route -------------------------
_GL = [(23, 31), (9, 6)]
GEOMETRY_CASES = [
    _b("geo_3x3_s2", _GL, batch=2, stride=2, pad=1, seed=241),
    _b("geo_3x3_d2", _GL, batch=2, pad=2, dil=2, mask=True, seed=242),
    _b("geo_3x3_p0", _GL, batch=2, pad=0, seed=243),
    _b("geo_1x1", _GL, batch=2, k=(1, 1), pad=0, seed=244),                                # one tap: the exact-fp32 weight kernel
    _b("geo_1x3", _GL, batch=2, k=(1, 3), pad=0, mask=True, seed=245),
    _b("geo_3x1", _GL, batch=2, k=(3, 1), pad=0, seed=246),
    _b("geo_2x2", _GL, batch=2, k=(2, 2), pad=0, mask=True, seed=247),
]
# ---- sparsity: the grad_out patterns on a three-level call -----------------------------------------------------------------------------
_SL = [(12, 13), (9, 11), (5, 5)]
SPARSITY_CASES = [
    _b("sparse_dense", _SL, batch=2, pattern="dense", seed=251),
    _b("sparse_rows", _SL, batch=2, pattern="rows", seed=252),
    _b("sparse_level_zero", _SL, batch=2, pattern="level_zero", mask=True, seed=253),
    _b("sparse_image_zero", _SL, batch=2, pattern="image_zero", seed=254),
    _b("sparse_channel_edge", _SL, batch=2, pattern="channel_edge", mask=True, seed=255),
    _b("sparse_zero", _SL, batch=2, pattern="zero", seed=256),
]
# ---- half I/O: |x| <= 3 and |grad_out| <= 1 keep every gradient finite in fp16 (asserted where they run) ---------------------------------
HALF_CASES = [
    _b("half_bord_9x11_v2", [(9, 11)], batch=2, mask=True, x_max=3, go_max=1, seed=261),
    _b("half_geo_3x3_s2", _GL, batch=2, stride=2, pad=1, x_max=3, go_max=1, seed=262),
    _b("half_reg_19x21", [(19, 21)], batch=2, x_max=3, go_max=1, seed=263),
]

FAMILIES = collections.OrderedDict([
    ("chunks", CHUNK_CASES), ("regions", REGION_CASES), ("borders", BORDER_CASES), ("geometry", GEOMETRY_CASES),
    ("sparsity", SPARSITY_CASES), ("half", HALF_CASES)])
ALL_CASES = [c for fam in FAMILIES.values() for c in fam]
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES) and all(c.cin == 256 and c.cout == 256 and not c.bias and not c.relu for c in ALL_CASES)
ZERO_CASES = ("reg_outside", "sparse_zero")                           # built to have all-zero gradients
SUBSET = ("bord_9x11_v2", "geo_3x3_s2", "reg_19x21")                  # the routes that run on a subset: one of each kind


def out_hw(case, level):
    H, W = case.levels[level]
    return D.out_size(H, case, case.kh), D.out_size(W, case, case.kw)


def _steer_offsets(case, level, rng, mode):
    """Offsets [B, 2 taps, Ho, Wo] that put every sample at a coordinate drawn per axis from `targets(n)` (halves)."""
    H, W = case.levels[level]
    Ho, Wo = out_hw(case, level)
    taps = case.kh * case.kw
    ki, kj = np.divmod(np.arange(taps), case.kw)
    base_h = (np.arange(Ho)[None, :] * case.stride - case.pad + ki[:, None] * case.dil).astype(np.float64)[None, :, :, None]
    base_w = (np.arange(Wo)[None, :] * case.stride - case.pad + kj[:, None] * case.dil).astype(np.float64)[None, :, None, :]
    shape = (case.batch, taps, Ho, Wo)

    def target(n):
        if mode == "outside":
            return n + rng.randint(0, 5, size=shape) / 2.0                       # n, n + 1/2, ... n + 2
        hi = n - 1.0 if n <= 8 else 6.5                                          # both corners of the axis in pixels 0 .. 7
        return rng.randint(0, int(2 * hi) + 1, size=shape) / 2.0
    off = np.empty((case.batch, 2 * taps, Ho, Wo))
    off[:, 0::2] = target(H) - base_h
    off[:, 1::2] = target(W) - base_w
    assert np.abs(off).max() <= D.OFFSET_LIMIT
    return torch.from_numpy(off)


def generate(case):
    """dcn_half_cases.generate(case), with the offsets of a steered case replaced."""
    data = D.generate(case)
    steer = META[case.name].steer
    if steer is not None:
        rng = np.random.RandomState(case.seed + 5000)
        data["offs"] = [_steer_offsets(case, i, rng, steer) for i in range(len(case.levels))]
    return data


def level_chunks(case):
    """[(first chunk, number of chunks, positions)] per level: chunks of 32 positions (b, ho, wo order) never cross a level."""
    out, c0 = [], 0
    for i in range(len(case.levels)):
        Ho, Wo = out_hw(case, i)
        npos = case.batch * Ho * Wo
        out.append((c0, (npos + 31) // 32, npos))
        c0 += (npos + 31) // 32
    return out


def grad_outputs(case, data):
    """Integer grad_out per level (float64 [B, 256, Ho, Wo], |g| <= go_max) in the case's pattern."""
    meta = META[case.name]
    rng = np.random.RandomState(case.seed + 9000)
    g = meta.go_max
    gos = []
    chunks = level_chunks(case)
    total_chunks = sum(n for _, n, _ in chunks)
    pattern = meta.pattern
    pick = None
    if isinstance(pattern, tuple):
        # the first chunk and the last (partial) chunk of the call take part whenever two or more are active
        forced = [0, total_chunks - 1] if pattern[1] >= 2 else []
        rest = [c for c in range(total_chunks) if c not in forced]
        pick = set(forced + rng.choice(rest, size=pattern[1] - len(forced), replace=False).tolist())
        assert len(pick) == pattern[1]
    for i in range(len(case.levels)):
        Ho, Wo = out_hw(case, i)
        npos = case.batch * Ho * Wo
        dense = rng.randint(-g, g + 1, size=(npos, case.cout)).astype(np.float64)
        dense[:, 0] = np.where(dense[:, 0] == 0, 1.0, dense[:, 0])               # no accidental all-zero row
        rows = np.zeros_like(dense)
        if pattern == "dense":
            rows = dense
        elif pattern == "rows":
            keep = rng.choice(npos, size=min(npos, 3), replace=False)
            rows[keep] = dense[keep]
        elif pattern == "level_zero":
            rows = dense if i != 1 else rows
        elif pattern == "image_zero":
            rows = dense.copy()
            rows[:Ho * Wo] = 0.0                                                 # image 0
        elif pattern == "channel_edge":
            keep = rng.choice(npos, size=max(2, npos // 7), replace=False)
            rows[keep[0::2], 0] = rng.choice([-g, -1.0, 1.0, g], size=len(keep[0::2]))
            rows[keep[1::2], case.cout - 1] = rng.choice([-g, -1.0, 1.0, g], size=len(keep[1::2]))
        elif pattern == "zero":
            pass
        else:
            c0, n, _ = chunks[i]
            for c in range(n):
                if c0 + c in pick:
                    lo, hi = 32 * c, min(32 * c + 32, npos)
                    keep = rng.choice(np.arange(lo, hi), size=min(2, hi - lo), replace=False)
                    keep = np.union1d(keep, [hi - 1])                            # the chunk's last row always
                    rows[keep] = dense[keep]
        gos.append(torch.from_numpy(np.ascontiguousarray(
            rows.reshape(case.batch, Ho, Wo, case.cout).transpose(0, 3, 1, 2))))
    return gos


def _rows(go):
    """[B, C, Ho, Wo] -> [B * Ho * Wo, C] in (b, ho, wo) order."""
    return go.permute(0, 2, 3, 1).reshape(-1, go.shape[1])


def active_chunks(case, gos):
    """Ascending list of the call's active chunks: a 32-position chunk with any non-zero grad_out value."""
    act = []
    for (c0, n, npos), go in zip(level_chunks(case), gos):
        nz = (_rows(go) != 0).any(dim=1)
        act += [c0 + c for c in range(n) if bool(nz[32 * c:32 * c + 32].any())]
    return act


def straddling_chunks(case):
    """Chunks whose 32 positions belong to more than one image."""
    out = []
    for i, (c0, n, npos) in enumerate(level_chunks(case)):
        Ho, Wo = out_hw(case, i)
        out += [c0 + c for c in range(n) if (32 * c) // (Ho * Wo) != (min(32 * c + 31, npos - 1)) // (Ho * Wo)]
    return out


def corner_predicates(case, h, w, H, W):
    """(valid [N], ok [N, 4]) of the samples at (h, w): the point is inside (-1, H) x (-1, W), and per corner in the order
    (low, low), (low, high), (high, low), (high, high): low >= 0 / high <= N - 1 on both axes (deform_conv_cuda_kernel.cu:145-188)."""
    valid = (h > -1) & (w > -1) & (h < H) & (w < W)
    h0, w0 = torch.floor(h), torch.floor(w)
    t_ok, b_ok, l_ok, r_ok = h0 >= 0, h0 + 1 <= H - 1, w0 >= 0, w0 + 1 <= W - 1
    return valid, torch.stack([valid & t_ok & l_ok, valid & t_ok & r_ok, valid & b_ok & l_ok, valid & b_ok & r_ok], 1)


def _level_backward(case, x, off, mask, weight, go):
    """One level, float64, from the definition.  Returns (grad_input, grad_offset, grad_weight, grad_mask | None) and the
    sums of absolute terms (same shapes, plus max |go| . |W|) for premise_bounds."""
    B, C, H, W = x.shape
    Ho, Wo = off.shape[2], off.shape[3]
    taps = case.kh * case.kw
    table = x.permute(0, 2, 3, 1).reshape(-1, C)
    g2 = _rows(go)
    gi = torch.zeros_like(table)
    gi_abs = torch.zeros_like(table)
    goff = torch.zeros((B * Ho * Wo, 2 * taps), dtype=torch.float64, device=x.device)
    s_abs = torch.zeros((B * Ho * Wo, taps), dtype=torch.float64, device=x.device)
    gm = torch.zeros((B * Ho * Wo, taps), dtype=torch.float64, device=x.device)
    gw = torch.zeros_like(weight)
    gw_abs = torch.zeros_like(weight)
    g_abs = 0.0
    for tap in range(taps):
        wt = weight[:, :, tap // case.kw, tap % case.kw]                         # [o, c]
        G = g2 @ wt                                                              # G_t[p, c]
        Gabs = g2.abs() @ wt.abs()                                               # bounds G's own partial sums; G itself is then exact,
                                                                                 # and the terms below are products with the finished G
        g_abs = max(g_abs, float(Gabs.max()))
        idx, wgt, h, w = D.tap_samples(case, x, off, mask, tap)
        for k in range(4):                                                       # invalid corners: weight 0 into pixel 0
            gi.index_add_(0, idx[:, k], wgt[:, k, None] * G)
            gi_abs.index_add_(0, idx[:, k], wgt[:, k, None].abs() * G.abs())
        gw[:, :, tap // case.kw, tap % case.kw] = g2.t() @ D.tap_columns(x, idx, wgt)
        gw_abs[:, :, tap // case.kw, tap % case.kw] = g2.abs().t() @ D.tap_columns(x.abs(), idx, wgt.abs())
        # the coordinate derivative: S_k = sum_c G[p, c] x[corner k, c], zero for a corner outside the map
        valid, ok = corner_predicates(case, h, w, H, W)
        lh, lw = h - torch.floor(h), w - torch.floor(w)
        uh, uw = 1 - lh, 1 - lw
        m = mask[:, tap].reshape(-1) if mask is not None else torch.ones_like(h)
        S = []
        for k in range(4):
            v = torch.where(ok[:, k, None], table[idx[:, k]], torch.zeros_like(G))
            S.append((G * v).sum(1))
            s_abs[:, tap] += (G.abs() * v.abs()).sum(1)
        goff[:, 2 * tap] = m * (uw * (S[2] - S[0]) + lw * (S[3] - S[1]))         # right-sided slope at integer coordinates
        goff[:, 2 * tap + 1] = m * (uh * (S[1] - S[0]) + lh * (S[3] - S[2]))
        if mask is not None:
            _, wgt1, _, _ = D.tap_samples(case, x, off, None, tap)
            gm[:, tap] = (G * D.tap_columns(x, idx, wgt1)).sum(1)
        s_abs[:, tap] *= torch.clamp(m.abs(), min=1.0)
    nchw = lambda t, ch: t.reshape(B, Ho, Wo, ch).permute(0, 3, 1, 2).contiguous()           # noqa: E731
    grads = (gi.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous(), nchw(goff, 2 * taps), gw,
             nchw(gm, taps) if mask is not None else None)
    return grads, (float(gi_abs.max()), float(s_abs.max()), gw_abs, g_abs)


def _on(data, i, case, device):
    mv = lambda t: t.to(device)                                                  # noqa: E731
    return mv(data["xs"][i]), mv(data["offs"][i]), (mv(data["masks"][i]) if case.mask else None), mv(data["weight"])


def reference_backward(case, data, gos, device="cpu"):
    """dict(grad_input=[...], grad_offset=[...], grad_weight=tensor, grad_weight_levels=[...], grad_mask=[...] | None), float64 on
    `device`: the gradients of sum_levels <DeformConv(x, off[, mask]; W), grad_out>."""
    gis, goffs, gws, gms = [], [], [], []
    for i in range(len(case.levels)):
        x, off, mask, w = _on(data, i, case, device)
        (gi, goff, gw, gm), _ = _level_backward(case, x, off, mask, w, gos[i].to(device))
        gis.append(gi); goffs.append(goff); gws.append(gw); gms.append(gm)
    total = gws[0].clone()
    for g in gws[1:]:
        total += g
    return dict(grad_input=gis, grad_offset=goffs, grad_weight=total, grad_weight_levels=gws,
                grad_mask=gms if case.mask else None)


def premise_bounds(case, data, gos, device="cpu"):
    """{gradient: (largest sum of |terms| of any output element, in units; the unit)} and "G" for G_t = grad_out . W itself.
    grad_input / grad_weight: unit 1/8 under modulation, 1/4 without; per corner, so any association of weight x G (x value) is
    covered.  grad_offset / grad_mask: unit 1/4; the sum is sum_corners sum_c |G| |x| times max(|m|, 1), WITHOUT the bilinear
    factors: it also bounds the four channel sums S_k the kernels form before they apply the factors."""
    u_in = 0.125 if case.mask else 0.25
    b_in = b_off = b_g = 0.0
    gw_abs = None
    for i in range(len(case.levels)):
        x, off, mask, w = _on(data, i, case, device)
        _, (a_in, a_off, a_gw, a_g) = _level_backward(case, x, off, mask, w, gos[i].to(device))
        b_in, b_off, b_g = max(b_in, a_in), max(b_off, a_off), max(b_g, a_g)
        gw_abs = a_gw if gw_abs is None else gw_abs + a_gw
    out = collections.OrderedDict([("G", (b_g, 1.0)), ("grad_input", (b_in / u_in, u_in)), ("grad_offset", (b_off / 0.25, 0.25)),
                                   ("grad_weight", (float(gw_abs.max()) / u_in, u_in))])
    if case.mask:
        out["grad_mask"] = (b_off / 0.25, 0.25)
    return out


def region_of(case, level, b, h, w):
    """Number of the 8 x 8 region of pixel (b, h, w) of a level, counted over the call (levels, images, region rows, columns)."""
    r0 = 0
    for i in range(level):
        H, W = case.levels[i]
        r0 += case.batch * ((H + 7) // 8) * ((W + 7) // 8)
    H, W = case.levels[level]
    return r0 + (b * ((H + 7) // 8) + h // 8) * ((W + 7) // 8) + w // 8


def region_list_lengths(case, data, gos):
    """Per level an int64 tensor [B, RH, RW]: how many (sample, region) entries the region's list holds -- one entry per
    (position, tap) sample of an ACTIVE chunk and per distinct region that one of its valid corners falls into."""
    act = set(active_chunks(case, gos))
    out = []
    for i, ((c0, n, npos), x, off) in enumerate(zip(level_chunks(case), data["xs"], data["offs"])):
        B, _, H, W = x.shape
        RH, RW = (H + 7) // 8, (W + 7) // 8
        live = torch.tensor([c0 + p // 32 in act for p in range(npos)])
        counts = torch.zeros(B * RH * RW, dtype=torch.int64)
        for tap in range(case.kh * case.kw):
            idx, _, h, w = D.tap_samples(case, x, off, None, tap)
            _, ok = corner_predicates(case, h, w, H, W)
            q = idx                                                              # (b * H + h) * W + w
            reg = ((q // (H * W)) * RH + (q // W) % H // 8) * RW + (q % W) // 8
            reg = torch.where(ok & live[:, None], reg, torch.full_like(reg, -1))
            for k in range(4):
                new = reg[:, k] >= 0
                for j in range(k):
                    new &= reg[:, k] != reg[:, j]
                counts.index_add_(0, reg[new, k], torch.ones(int(new.sum()), dtype=torch.int64))
        out.append(counts.reshape(B, RH, RW))
    return out


def sample_class_of(case, level, h, w):
    """The border classes (dcn_half_cases.SAMPLE_CLASSES) of ONE sample at coordinates (h, w) of a level, for messages."""
    H, W = case.levels[level]
    valid = h > -1 and w > -1 and h < H and w < W
    h0, w0 = np.floor(h), np.floor(w)
    tests = (("inside", valid and h0 >= 0 and h0 + 1 <= H - 1 and w0 >= 0 and w0 + 1 <= W - 1),
             ("h_low=-1", valid and h0 == -1), ("h_high=H", valid and h0 + 1 == H), ("w_low=-1", valid and w0 == -1),
             ("w_high=W", valid and w0 + 1 == W), ("on -1", h == -1 or w == -1),
             ("on H-1 / W-1", valid and (h == H - 1 or w == W - 1)), ("at or beyond H / W", h >= H or w >= W),
             ("at or beyond -1", h <= -1 or w <= -1), ("strictly beyond -1", h < -1 or w < -1),
             ("integer coordinates", valid and h == h0 and w == w0))
    return [k for k, t in tests if t]


_expected = {}


def expected(case, device):
    """(data, grad_outs, reference_backward on `device`), computed once per case name and process and never modified."""
    if case.name not in _expected:
        data = generate(case)
        gos = grad_outputs(case, data)
        _expected[case.name] = (data, gos, reference_backward(case, data, gos, device))
    return _expected[case.name]
