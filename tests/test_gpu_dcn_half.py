"""GPU: the fp16 / bf16 DeformConv forward (csrc/orp_dcn_half.hip: the wave-specialised kernel, the default, and the symmetric
one) at every tile height, depth and geometry it admits.

1. Exact-arithmetic cases (tests/dcn_half_cases.py), compared BIT FOR BIT with a float64 gather-and-matmul reference converted
   once to the storage type.  The premises that make this legitimate, and the conditions that keep it from passing vacuously,
   are asserted without a GPU in tests/test_dcn_half_cases.py.  No tolerance: one wrong neighbour, bilinear weight, tap index,
   tile row or output rounding changes bits.  Which tile height a case ran is ASSERTED with the library's query
   (orp_dcn_forward_h_tile_rows), not derived here.
2. Random data at the shapes the older tests do not reach, against the fp32 oracle on the same rounded inputs, at the
   project's stated tolerance (2e-3 fp16 / 1.6e-2 bf16 of the output scale; csrc/orp_dcn_half.hip, head comment).
3. The wrapper's contract at the edge of the half path, and the C entry's error returns.

Measured (MI355X): see docs/notebook/round7.md section 2."""
import collections
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dcn_half_cases as D  # noqa: E402

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


_family_stats = collections.OrderedDict()          # family -> [cases run, outputs compared, outputs differing, tile heights]


def _expected(case, dev):
    """(CPU float64 tensors of the case, float64 reference outputs on the device), computed once per case."""
    return D.expected(case, dev)


def _launch(case, data, dtype, channels_last, dev):
    from orientedreppoints_amd.mmdet_ops import deform_conv_forward_multi
    t = D.device_inputs(case, data, dtype, dev, channels_last)
    outs = deform_conv_forward_multi(t["xs"], t["offs"], t["weight"], case.stride, case.pad, case.dil, masks=t["masks"],
                                     bias=t["bias"], relu=case.relu)
    # a [B, C, 1, 1] tensor is contiguous in both memory formats; the wrapper then runs the whole launch as NCHW
    nhwc = channels_last and all(not x.is_contiguous() for x in t["xs"])
    for o in outs:
        assert o.dtype == dtype, "the half path did not run: output dtype %s" % o.dtype
        assert o.is_contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format)
    if channels_last and (1, 1) not in case.levels:
        assert nhwc, "the channels-last run of %s was not channels-last" % case.name
    return outs, nhwc


def _describe(case, level, got, want64, dtype):
    """Where the bits differ: for reading a failure (which rows of a tile, which channels), not for deciding it."""
    want = want64.to(dtype)
    bad = (D.bits(got) != D.bits(want)).nonzero()
    B, C, Ho, Wo = want.shape
    pos = bad[:, 0] * Ho * Wo + bad[:, 2] * Wo + bad[:, 3]
    first = ["(b %d, c %d, h %d, w %d): got %r want %r" % (b, c, h, w, float(got[b, c, h, w]), float(want[b, c, h, w]))
             for b, c, h, w in bad[:6].tolist()]
    return ("%s level %d (%dx%d -> %dx%d): %d of %d outputs differ; positions %d..%d, %d distinct, position mod %d in %s; "
            "channels %d..%d, %d distinct; first: %s"
            % (case.name, level, case.levels[level][0], case.levels[level][1], Ho, Wo, bad.shape[0], want.numel(), int(pos.min()),
               int(pos.max()), pos.unique().numel(), case.rows, sorted(set((pos % case.rows).tolist()))[:40], int(bad[:, 1].min()),
               int(bad[:, 1].max()), bad[:, 1].unique().numel(), "; ".join(first)))


def _compare_case(case, dtype, dev):
    """Both layouts of one case in one storage type: (outputs compared, outputs differing, descriptions of the differences,
    launches that ran NCHW, launches that ran NHWC -- a case with a 1 x 1 level runs NCHW twice, see _launch)."""
    data, want = _expected(case, dev)
    total = differing = 0
    notes, ran = [], [0, 0]
    for channels_last in (False, True):
        outs, nhwc = _launch(case, data, dtype, channels_last, dev)
        ran[1 if nhwc else 0] += 1
        for level, (got, w64) in enumerate(zip(outs, want)):
            n, bad = D.count_differing(got, w64, dtype)
            total += n
            differing += bad
            if bad and len(notes) < 4:
                notes.append(("NHWC " if nhwc else "NCHW ") + _describe(case, level, got, w64, dtype))
    return total, differing, notes, ran[0], ran[1]


@pytest.fixture(scope="module", autouse=True)
def _report_families():
    yield
    import conftest
    for fam, (cases, total, differing, rows, nchw, nhwc) in _family_stats.items():
        conftest.REPORT.append("half DeformConv, exact cases bit for bit vs float64, %-15s: %d case runs (fp16 + bf16), launches %d NCHW + "
                               "%d NHWC, tile heights %s, %d outputs compared, %d differ"
                               % (fam, cases, nchw, nhwc, sorted(rows), total, differing))


_CASE_PARAMS = [pytest.param(fam, c, id=c.name) for fam, cs in D.FAMILIES.items() for c in cs]


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("family,case", _CASE_PARAMS)
def test_exact_case_is_bitwise_the_float64_reference(dev, family, case, dtype):
    """The default (wave-specialised) kernel, NCHW and channels-last in / out: the storage of every output equals the float64
    reference converted with .to(T), +-inf of the fp16 saturation case included.  The tile height the case claims is the one
    the launcher picks (same host function)."""
    from orientedreppoints_amd.mmdet_ops.deform_conv import half_tile_rows, half_path_ok
    assert half_tile_rows(D.positions(case), len(case.levels)) == case.rows
    assert half_path_ok(torch.empty((case.cout, case.cin, case.kh, case.kw), dtype=DTYPES[dtype]), 1, 1)
    from orientedreppoints_amd import _lib
    assert _lib.lib().orp_dcn_forward_h_wave_specialised() == 1, "this process runs the symmetric kernel"
    total, differing, notes, nchw, nhwc = _compare_case(case, DTYPES[dtype], dev)
    st = _family_stats.setdefault(family, [0, 0, 0, set(), 0, 0])
    st[0] += 1; st[1] += total; st[2] += differing; st[3].add(case.rows); st[4] += nchw; st[5] += nhwc
    assert differing == 0, "\n".join(notes)
    if case in D.SATURATION_CASES and dtype == "float16":
        assert any(torch.isinf(w.to(torch.float16)).any() for w in _expected(case, dev)[1])


def test_float64_helper_is_bitwise_the_oracle(dev, oracle):
    """The reference of this file (tests/dcn_half_cases.py: plain torch indexing, float64, run on the device) against the CPU
    oracle (oracle.dcn_forward / dcn_v2_forward: the reference's float sampler, contracted in double) on small cases of every
    geometry, with and without modulation: the same values exactly (the oracle returns fp32; under the premises of the cases
    every output is an fp32 number)."""
    small = [D.BY_NAME[n] for n in ("seam_b3", "geo_3x3_s2", "geo_3x3_d2", "geo_1x1", "geo_1x3", "geo_3x1", "geo_2x2", "mt1_t7")]
    small += [D.BY_NAME["seam_b3"]._replace(name="seam_b3_v1", mask=False, bias=True, relu=True)]
    for case in small:
        data = D.generate(case)
        ref = D.reference(case, data, dev)
        assert all(torch.equal(r.cpu(), c) for r, c in zip(ref, D.reference(case, data, "cpu"))), "device and host float64 differ"
        w = data["weight"].numpy()
        b = data["bias"].numpy() if case.bias else None
        for i, r in enumerate(ref):
            x, off = data["xs"][i].numpy(), data["offs"][i].numpy()
            m = data["masks"][i].numpy() if case.mask else None
            want = oracle.dcn_forward(x, off, w, case.stride, case.pad, case.dil, mask=m, bias=b)
            if case.relu:
                want = np.maximum(want, 0.0)
            assert np.array_equal(r.cpu().numpy(), want.astype(np.float64)), (case.name, i)
            if case.mask:
                want2 = oracle.dcn_v2_forward(x, off, m, w, b, case.stride, case.pad, case.dil)
                assert np.array_equal(r.cpu().numpy(), want2.astype(np.float64)), (case.name, i)


def _child_main(names):
    """Body of the child process of the test below: the named cases, both types, both layouts; prints one RESULT line."""
    from orientedreppoints_amd import _lib
    dev = torch.device("cuda:0")
    assert _lib.lib().orp_dcn_forward_h_wave_specialised() == 0, "ORP_DCNH_WS=0 did not select the symmetric kernel"
    cases = total = differing = nchw = nhwc = 0
    for n in names:
        for dt in DTYPES.values():
            t, bad, notes, a, b = _compare_case(D.BY_NAME[n], dt, dev)
            cases += 1; total += t; differing += bad; nchw += a; nhwc += b
            for ln in notes:
                print("DIFF", ln)
    print("RESULT cases %d outputs %d differing %d launches %d NCHW + %d NHWC" % (cases, total, differing, nchw, nhwc))


def test_symmetric_kernel_exact_cases_at_tile_heights_2_and_3(dev):
    """ORP_DCNH_WS=0 selects the symmetric kernel (dcn_fwd_half_kernel) when the library is loaded: a fresh process runs
    EVERY case of tile height 2 or 3, the production head at batch 1 and 2 included (both types, both layouts), against the
    same float64 reference, and asserts with the library's query that it is the symmetric kernel it launches.  One process, one time limit,
    no retry."""
    import conftest
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_dcn_half as t; t._child_main(%r)" % (
        os.path.dirname(HERE), HERE, D.SYMMETRIC_KERNEL_CASES)
    assert sorted(D.SYMMETRIC_KERNEL_CASES) == sorted(c.name for c in D.ALL_CASES if c.rows in (64, 96))
    assert {D.BY_NAME[n].rows for n in D.SYMMETRIC_KERNEL_CASES} == {64, 96}
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ORP_DCNH_WS="0"), stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:]
    res = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
    assert len(res) == 1, out.stdout[-4000:]
    conftest.REPORT.append("half DeformConv, exact cases bit for bit vs float64, symmetric kernel (child, ORP_DCNH_WS=0), tile heights "
                           "[64, 96]: " + res[0][7:])
    f = res[0].split()
    assert int(f[2]) == 2 * len(D.SYMMETRIC_KERNEL_CASES) and int(f[4]) > 0
    assert int(f[6]) == 0, "\n".join(ln for ln in out.stdout.splitlines() if ln.startswith("DIFF"))[-4000:]


# shapes for ordinary data: (levels, batch, c_in, c_out, stride, pad, dil, tile rows claimed)
_RANDOM_SHAPES = [
    pytest.param([(40, 40), (20, 20)], 2, 256, 64, 1, 1, 1, 32, id="mt1"),
    pytest.param([(92, 91)], 1, 256, 64, 1, 1, 1, 64, id="mt2"),
    pytest.param([(100, 164)], 1, 256, 64, 1, 1, 1, 96, id="mt3"),
    pytest.param([(20, 24), (7, 5)], 2, 512, 128, 1, 1, 1, 32, id="cin512"),
    pytest.param([(23, 31), (9, 6)], 2, 256, 128, 2, 1, 1, 32, id="stride2"),
    pytest.param([(23, 31), (9, 6)], 2, 256, 128, 1, 2, 2, 32, id="dilation2"),
]


@pytest.mark.parametrize("dtype,tol", [("float16", 2e-3), ("bfloat16", 1.6e-2)])
@pytest.mark.parametrize("levels,B,cin,cout,stride,pad,dil,rows", _RANDOM_SHAPES)
def test_random_data_vs_fp32_oracle_at_the_new_shapes(dev, oracle, levels, B, cin, cout, stride, pad, dil, rows, dtype, tol):
    """The comparison of test_dcn_forward_half_precision_vs_fp32_oracle (normal features and offsets, weights of std 0.05,
    the fp32 oracle on the SAME rounded inputs, the project's stated tolerance of the output scale, unchanged) at one shape per
    tile height, at c_in = 512, with stride 2 and with dilation 2.  The exact cases carry the precision of this file; this shows
    that ordinary data behaves the same there."""
    from orientedreppoints_amd.mmdet_ops import deform_conv_forward_multi
    from orientedreppoints_amd.mmdet_ops.deform_conv import half_tile_rows
    dt = DTYPES[dtype]
    rng = np.random.RandomState(41 + cin + stride + 2 * dil + rows)
    od = lambda n: (n + 2 * pad - (dil * 2 + 1)) // stride + 1           # noqa: E731
    assert half_tile_rows(sum(B * od(h) * od(w) for h, w in levels), len(levels)) == rows
    q = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev).to(dt)   # noqa: E731  (round to the storage type)
    f = lambda t: t.float().cpu().numpy()                                # noqa: E731
    xs = [q(rng.normal(size=(B, cin, h, w))) for h, w in levels]
    offs = [q(rng.normal(0, 2.0, size=(B, 18, od(h), od(w)))) for h, w in levels]
    w = q(rng.normal(0, 0.05, size=(cout, cin, 3, 3)))
    outs = deform_conv_forward_multi(xs, offs, w, stride, pad, dil)
    for x, o, got in zip(xs, offs, outs):
        assert got.dtype == dt
        want = oracle.dcn_forward(f(x), f(o), f(w), stride, pad, dil)
        assert np.max(np.abs(f(got) - want)) <= tol * np.max(np.abs(want))


def test_half_path_boundary_and_what_a_refused_half_tensor_gets(dev):
    """`half_path_ok` across its boundary, and the PINNED behaviour of `deform_conv_forward_multi` for half tensors the half path
    refuses: they are converted, computed by the fp32 path and returned as FP32 tensors (bitwise what the fp32 call on the
    converted tensors returns) -- not a half result; DeformConvFunction casts back itself.  A shape the fp32 MFMA path refuses
    as well (c_out = 96) is ORP_EINVAL for half and fp32 tensors alike: callers ask `fast_path_ok` first.  Pinned, not changed:
    callers rely on it."""
    from orientedreppoints_amd.mmdet_ops import deform_conv_forward_multi
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.deform_conv import half_path_ok, fast_path_ok
    for dt in DTYPES.values():
        wt = lambda *s: torch.empty(s, dtype=dt, device=dev)               # noqa: E731
        assert [half_path_ok(wt(256, c, 3, 3), 1, 1) for c in (128, 256, 384)] == [False, True, False]
        assert [half_path_ok(wt(c, 256, 3, 3), 1, 1) for c in (32, 64, 96)] == [False, True, False]
        assert half_path_ok(wt(64, 256, 1, 9), 1, 1) and not half_path_ok(wt(64, 256, 2, 5), 1, 1)      # 9 taps, 10 taps
        assert not half_path_ok(wt(256, 128, 3, 3), 2, 1) and not half_path_ok(wt(256, 256, 3, 3), 1, 2)
        assert not half_path_ok(torch.empty((256, 256, 3, 3), device=dev), 1, 1)                       # an fp32 weight
        torch.manual_seed(3)
        for cin, cout in ((128, 64), (384, 128), (256, 96)):
            x = torch.randn(2, cin, 9, 7, device=dev).to(dt)
            off = torch.randn(2, 18, 9, 7, device=dev).to(dt)
            w = (torch.randn(cout, cin, 3, 3, device=dev) * 0.05).to(dt)
            if not fast_path_ok(w, 1, 1):                     # c_out = 96: the fp32 MFMA path refuses it too -> loud, both ways
                for args in (([x], [off], w), ([x.float()], [off.float()], w.float())):
                    with pytest.raises(_lib.OrpHipError, match="ORP_EINVAL"):
                        deform_conv_forward_multi(*args, 1, 1, 1)
                continue
            got = deform_conv_forward_multi([x], [off], w, 1, 1, 1)[0]
            assert got.dtype == torch.float32 and got.shape == (2, cout, 9, 7)
            assert torch.equal(got, deform_conv_forward_multi([x.float()], [off.float()], w.float(), 1, 1, 1)[0])
        x = torch.randn(1, 256, 5, 5, device=dev).to(dt)                                                # admitted shape, fp32 weight
        got = deform_conv_forward_multi([x], [torch.zeros(1, 18, 5, 5, device=dev, dtype=dt)], torch.randn(64, 256, 3, 3, device=dev), 1, 1, 1)[0]
        assert got.dtype == torch.float32


def test_forward_multi_h_error_returns(dev):
    """orp_dcn_forward_multi_h refuses, before it launches anything: a workspace one byte short for NCHW inputs
    (ORP_EWORKSPACE), a dtype code other than 1 / 2, more than 8 levels, a level whose output size is not positive, and a
    shape orp_dcn_half_path_ok refuses (all ORP_EINVAL).  The output buffer keeps its contents."""
    from orientedreppoints_amd import _lib
    L = _lib.lib()

    class Level(ctypes.Structure):
        _fields_ = [("input", ctypes.c_void_p), ("offset", ctypes.c_void_p), ("output", ctypes.c_void_p),
                    ("height", ctypes.c_int), ("width", ctypes.c_int)]
    B, cin, cout, H, W = 1, 256, 64, 6, 5
    x = torch.zeros(B, cin, H, W, device=dev, dtype=torch.float16)
    off = torch.zeros(B, 18, H, W, device=dev, dtype=torch.float16)
    out = torch.full((B, cout, H, W), 7.0, device=dev, dtype=torch.float16)
    wp = torch.zeros(cout * cin * 9, device=dev, dtype=torch.float16)
    lv = (Level * 9)(*[Level(x.data_ptr(), off.data_ptr(), out.data_ptr(), H, W) for _ in range(9)])
    need = L.orp_dcn_forward_h_workspace_bytes(lv, 1, B, cin, 0)
    assert need >= 2 * B * cin * H * W
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def call(nlev=1, c_in=cin, c_out=cout, kh=3, kw=3, pad=1, dtype=1, ws_bytes=need, levels=lv):
        return L.orp_dcn_forward_multi_h(levels, None, nlev, B, c_in, c_out, _lib.ptr(wp), None, 0, kh, kw, 1, 1, pad, pad, 1, 1, 0, 0,
                                         dtype, _lib.ptr(ws), ws_bytes, _lib.stream_of(x))
    assert call(ws_bytes=need - 1) == _lib.ORP_EWORKSPACE and call(ws_bytes=0) == _lib.ORP_EWORKSPACE
    assert call(dtype=0) == _lib.ORP_EINVAL and call(dtype=3) == _lib.ORP_EINVAL
    assert call(nlev=9) == _lib.ORP_EINVAL and call(nlev=0) == _lib.ORP_EINVAL
    small = (Level * 1)(Level(x.data_ptr(), off.data_ptr(), out.data_ptr(), 2, 5))                       # 3x3, pad 0: Ho = 0
    assert call(pad=0, levels=small) == _lib.ORP_EINVAL
    assert call(c_in=128) == _lib.ORP_EINVAL and call(c_out=32) == _lib.ORP_EINVAL and call(kh=2, kw=5) == _lib.ORP_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == _lib.ORP_OK                                                                        # the same call, valid
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
