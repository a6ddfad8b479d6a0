"""CPU: the host side of orp_token_linear -- what its queries answer and refuse without a device, the plain-torch statement of the
operator, where the Swin modules send their linears, and what the kernels cost in registers and LDS when the source is compiled for
gfx950 (no launch)."""
import contextlib
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

torch = pytest.importorskip("torch")
F = torch.nn.functional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAX = 163840
WORKGROUPS_PER_CU = 2
WAVES_PER_WORKGROUP = 4
SWIN_K = (96, 192, 384, 768, 1536, 3072)
SWIN_N = (96, 192, 288, 384, 576, 768, 1152, 1536, 2304, 3072)


def _lib():
    from orientedreppoints_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def test_ok_and_packed_bytes():
    L = _lib()
    for k in SWIN_K + (32, 64, 160):
        for n in SWIN_N + (32, 160):
            assert L.orp_token_linear_ok(k, n) == 1, (k, n)
            assert L.orp_token_linear_packed_bytes(k, n) == 6 * k * n
    for k, n in ((24, 96), (96, 20), (24, 20), (0, 96), (96, 0), (-96, 96), (96, -96), (48, 96), (96, 48), (16, 32), (1 << 20, 96),
                 (96, 1 << 20)):
        assert L.orp_token_linear_ok(k, n) == 0, (k, n)
        assert L.orp_token_linear_packed_bytes(k, n) == 0, (k, n)


def test_pays_is_a_closed_table():
    """whatever the table holds, it answers 0 or 1 at the Swin-T shapes and 0 everywhere else: refused shapes, shapes nobody timed, token
    counts beyond a 1536^2 image's or below a 1024^2 image's last stage, unknown epilogue bits"""
    L = _lib()
    for k in SWIN_K:
        for n in SWIN_N:
            for t in (1024, 65536, 147456):
                for epi in range(8):
                    assert L.orp_token_linear_pays(t, k, n, epi) in (0, 1)
    for t, k, n, epi in ((65536, 24, 96, 1), (65536, 96, 20, 1), (65536, 32, 32, 1), (65536, 160, 160, 5), (65536, 96, 320, 1),
                         (0, 96, 288, 1), (-1, 96, 288, 1), (1, 96, 288, 1), (1023, 768, 2304, 1), (147457, 96, 288, 1),
                         (1 << 40, 96, 288, 1), (65536, 96, 288, 8), (65536, 96, 288, -1), (65536, 96, 288, 6), (65536, 96, 96, 2)):
        assert L.orp_token_linear_pays(t, k, n, epi) == 0, (t, k, n, epi)
    # the tiny shapes of the existing Swin tests are outside it: those tests run the library's launches as before
    for t in (70, 196, 300, 1938):
        for k, n in ((24, 72), (24, 24), (24, 96), (96, 24), (96, 288), (96, 96), (96, 384), (384, 96), (384, 192)):
            for epi in (0, 1, 3, 5):
                assert L.orp_token_linear_pays(t, k, n, epi) == 0


def test_launch_and_pack_refuse_bad_arguments_without_a_device():
    """the argument checks come before any device call: ORP_EINVAL for null or misaligned pointers, a negative token count, a refused
    shape, an unknown activation, and y aliasing x or the residual; no tokens is ORP_OK"""
    from orientedreppoints_amd import _lib as lib_mod
    L = _lib()
    x, w, b, r, y = (ctypes.c_void_p(4096 * (i + 1)) for i in range(5))
    odd = ctypes.c_void_p(4096 + 4)
    E = lib_mod.ORP_EINVAL
    good = (64, 96, 96, 0)
    assert L.orp_token_linear(x, w, b, r, y, 0, 96, 96, 0, None) == lib_mod.ORP_OK
    assert L.orp_token_linear(x, w, None, None, y, 0, 96, 288, 1, None) == lib_mod.ORP_OK
    for ptrs in ((None, w, b, r, y), (x, None, b, r, y), (x, w, b, r, None), (odd, w, b, r, y), (x, odd, b, r, y), (x, w, odd, r, y),
                 (x, w, b, odd, y), (x, w, b, r, odd), (x, w, b, r, x), (x, w, b, r, r)):
        assert L.orp_token_linear(*ptrs, *good, None) == E, ptrs
        assert L.orp_token_linear(*ptrs, 0, 96, 96, 0, None) == E, ptrs
    for bad in ((-1, 96, 96, 0), (64, 24, 96, 0), (64, 96, 20, 0), (64, 0, 96, 0), (64, 96, 96, 2), (64, 96, 96, -1)):
        assert L.orp_token_linear(x, w, b, r, y, *bad, None) == E, bad
    assert L.orp_token_linear_pack_weight(None, 96, 96, w, None) == E
    assert L.orp_token_linear_pack_weight(x, 96, 96, None, None) == E
    assert L.orp_token_linear_pack_weight(x, 96, 96, odd, None) == E
    assert L.orp_token_linear_pack_weight(x, 24, 96, w, None) == E
    assert L.orp_token_linear_pack_weight(x, 96, 20, w, None) == E


@pytest.mark.parametrize("act", [None, 'gelu'])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("res", [True, False])
def test_reference_in_float64_is_the_stock_modules(act, bias, res):
    from orientedreppoints_amd.mmdet_ops.token_linear import token_linear_reference
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 37, 96), generator=g, dtype=torch.float64)
    w = torch.randn((160, 96), generator=g, dtype=torch.float64)
    b = torch.randn((160,), generator=g, dtype=torch.float64) if bias else None
    r = torch.randn((2, 37, 160), generator=g, dtype=torch.float64) if res else None
    want = F.linear(x, w, b)
    if act == 'gelu':
        want = F.gelu(want)
    if res:
        want = want + r
    got = token_linear_reference(x, w, b, act, r)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 37, 160)
    assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))
    with pytest.raises(ValueError):
        token_linear_reference(x, w, b, 'relu', r)


class _Described(object):
    """what the routing predicates ask of a tensor, for devices this machine does not have"""

    def __init__(self, is_cuda, dtype, shape=(1, 300, 96), contiguous=True, device=None):
        self.is_cuda, self.dtype, self.shape, self._contiguous = is_cuda, dtype, tuple(shape), contiguous
        self.device = torch.device('cpu') if device is None else device           # (where this machine's parameters live)

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._contiguous


@contextlib.contextmanager
def _cuda_autocast():
    """the CUDA autocast flag as the predicates read it, set without a device"""
    was = torch.is_autocast_enabled()
    torch.set_autocast_enabled(True)
    try:
        yield
    finally:
        torch.set_autocast_enabled(was)


def test_token_linear_ok_on_described_tensors():
    from orientedreppoints_amd.mmdet_ops.token_linear import token_linear, token_linear_ok, token_linear_routed
    lin = torch.nn.Linear(96, 288)
    x32 = dict(is_cuda=True, dtype=torch.float32)
    assert not token_linear_ok(lin, _Described(**x32))                         # gradients are enabled
    with torch.no_grad():
        assert token_linear_ok(lin, _Described(**x32))
        assert token_linear_ok(lin, _Described(shape=(96,), **x32)) and token_linear_ok(lin, _Described(shape=(2, 3, 5, 96), **x32))
        assert token_linear_ok(torch.nn.Linear(96, 288, bias=False), _Described(**x32))
        assert not token_linear_ok(lin, _Described(is_cuda=False, dtype=torch.float32))
        assert not token_linear_ok(lin, torch.zeros(1, 300, 96))                                 # a CPU tensor
        assert not token_linear_ok(lin, _Described(is_cuda=True, dtype=torch.float16))
        assert not token_linear_ok(lin, _Described(is_cuda=True, dtype=torch.float64))
        assert not token_linear_ok(lin, _Described(contiguous=False, **x32))
        assert not token_linear_ok(lin, _Described(device=torch.device('meta'), **x32))         # parameters on another device
        assert not token_linear_ok(lin, _Described(shape=(1, 300, 192), **x32))                   # not this layer's input
        assert not token_linear_ok(torch.nn.Linear(24, 96), _Described(shape=(1, 300, 24), **x32))   # K the kernel refuses
        assert not token_linear_ok(torch.nn.Linear(96, 20), _Described(**x32))                    # N the kernel refuses
        assert not token_linear_ok(torch.nn.Linear(96, 288).half(), _Described(**x32))            # a model.half() layer
        assert not token_linear_ok(torch.nn.Conv2d(96, 288, 1), _Described(**x32))
        with _cuda_autocast():
            assert not token_linear_ok(lin, _Described(**x32))
        # outside the table nothing is routed, whatever the predicate says
        assert not token_linear_routed(lin, _Described(**x32), None, None)
        assert not token_linear_routed(lin, _Described(**x32), 'relu', None)
        with pytest.raises(ValueError):
            token_linear(torch.zeros(1, 300, 96), lin, force=True)              # never a fall-back
    with torch.enable_grad():
        assert not token_linear_ok(lin, _Described(**x32))


def test_swin_block_routes(monkeypatch):
    """`SwinBlock.fuses_linears`: an eval-mode block whose attention takes the fp32 inference kernel, under the switch or the block's own
    attribute; everything else keeps the modules as written"""
    from orientedreppoints_amd import switches
    from orientedreppoints_amd.mmdet_models.swin import SwinBlock
    blk = SwinBlock(96, 3, 7, 0, 4., True, None, 0., 0., 0.1).eval()
    x = _Described(True, torch.float32)
    asked = []
    monkeypatch.setattr(blk, "fuses_attention", lambda t: asked.append(t) or True, raising=False)
    monkeypatch.setattr(switches, "SWIN_LINEAR_FUSE", True)
    assert blk.fuses_linears(x) is True and asked == [x]
    assert blk.fuses_linears(_Described(True, torch.float32, contiguous=False)) is False
    blk.train()
    assert blk.fuses_linears(x) is False                      # dropout / drop_path are not identities
    blk.eval()
    blk.fuse_token_linear = False
    assert blk.fuses_linears(x) is False
    monkeypatch.setattr(switches, "SWIN_LINEAR_FUSE", False)
    blk.fuse_token_linear = None
    assert blk.fuses_linears(x) is False                      # the switch
    blk.fuse_token_linear = True
    assert blk.fuses_linears(x) is True                       # the attribute overrides it
    monkeypatch.setattr(blk, "fuses_attention", lambda t: False, raising=False)
    assert blk.fuses_linears(x) is False                      # the stock attention branch
    blk.force_token_linear = True
    assert blk.fuses_linears(x) is False                      # force skips the table, not the conditions
    # the real predicate: gradients, autocast, 16-bit tokens and CPU tensors all keep the stock branch
    monkeypatch.undo()
    blk.fuse_token_linear = True
    for t in (torch.zeros(1, 49, 96), torch.zeros(1, 49, 96, dtype=torch.float16)):
        with torch.no_grad():
            assert blk.fuses_linears(t) is False
        assert blk.fuses_linears(t) is False


def test_cpu_modules_keep_their_bits(monkeypatch):
    """CPU tensors run the modules as written, bit for bit, whatever the switch and the attributes say"""
    from orientedreppoints_amd import switches
    from orientedreppoints_amd.mmdet_models.swin import PatchMerging, SwinStage
    torch.manual_seed(0)
    st = SwinStage(32, 2, 2, 7, 4., True, None, 0., 0., [0., 0.], True, False).eval()
    x = torch.randn(1, 15 * 20, 32)
    with torch.no_grad():
        monkeypatch.setattr(switches, "SWIN_LINEAR_FUSE", False)
        want = st(x, 15, 20)
        monkeypatch.setattr(switches, "SWIN_LINEAR_FUSE", True)
        for m in list(st.blocks) + [st.downsample]:
            m.force_token_linear = True
        got = st(x, 15, 20)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2:] == want[2:]
    pm = PatchMerging(32).eval()
    with torch.no_grad():
        y = pm(x, 15, 20)
        xs = F.pad(x.view(1, 15, 20, 32), (0, 0, 0, 0, 0, 1))
        cat = torch.cat([xs[:, 0::2, 0::2], xs[:, 1::2, 0::2], xs[:, 0::2, 1::2], xs[:, 1::2, 1::2]], -1)
        assert torch.equal(y, pm.reduction(pm.norm(cat.view(1, -1, 128))))


def test_kernels_compile_without_spills_or_scratch_inside_the_lds_plan():
    """compiles csrc/orp_token_linear.hip with the library's flags and reads the compiler's resource remarks: all twelve instantiations
    (three token tiles x GELU x residual) spill nothing, use no scratch, and fit two workgroups of four waves on a CU both ways: two
    waves per SIMD in registers (at most 256 each) and twice the static LDS inside 163 840 B"""
    from orientedreppoints_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not found")
    assert "orp_token_linear.hip" in [s for s, _ in build.SOURCES]
    src = os.path.join(build.CSRC, "orp_token_linear.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC] + build.COMMON + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "tl.o")]
        r = subprocess.run(cmd, cwd=build.CSRC, stderr=subprocess.PIPE, stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    seen = {}
    for blk in blocks:
        name = blk.split()[0]
        if "token_linear_kernel" not in name:
            continue

        def num(key):
            return int(re.search(re.escape(key) + r":\s+(\d+)", blk).group(1))
        seen[name] = dict(vgprs=num("VGPRs"), agprs=num("AGPRs"), scratch=num("ScratchSize [bytes/lane]"), sgpr_spill=num("SGPRs Spill"),
                          vgpr_spill=num("VGPRs Spill"), lds=num("LDS Size [bytes/block]"), occupancy=num("Occupancy [waves/SIMD]"))
    assert len(seen) == 12, sorted(seen)
    waves_per_simd = WORKGROUPS_PER_CU * WAVES_PER_WORKGROUP // 4
    for name, u in seen.items():
        assert u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0 and u["scratch"] == 0, (name, u)
        assert u["vgprs"] + u["agprs"] <= 256 and u["occupancy"] >= waves_per_simd, (name, u)
        assert 0 < u["lds"] and WORKGROUPS_PER_CU * u["lds"] <= LDS_MAX, (name, u)
