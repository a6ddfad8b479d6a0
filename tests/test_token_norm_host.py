"""CPU: the host side of orp_token_layernorm -- what its queries answer and refuse without a device, the plain-torch statement of the
four layouts, where the Swin modules send their LayerNorms, and what the kernels cost in registers and LDS when the source is compiled
for gfx950 (no launch)."""
import contextlib
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

torch = pytest.importorskip("torch")
F = torch.nn.functional

LDS_MAX = 163840
LAYOUTS = ('tokens', 'merge', 'from_nchw', 'to_nchw')
SWIN_C = (96, 192, 384, 768, 1536)


def _lib():
    from orientedreppoints_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def test_ok_over_the_width_grid():
    L = _lib()
    for c, want in ((31, 0), (32, 1), (96, 1), (100, 0), (4096, 1), (4128, 0), (0, 0), (-96, 0), (64, 1), (3072, 1)):
        assert L.orp_token_layernorm_ok(c) == want, c


def test_plan_is_a_function_of_the_width():
    """lanes per row: the fewest of 8 / 16 / 32 / 64 with at most four float4 per lane; 256 / lanes rows per workgroup; the NCHW variants'
    tile is 32, 16 or 8 tokens of c channels plus one padding column, inside the CU's 160 KB, and no LDS at all for TOKENS and MERGE"""
    from orientedreppoints_amd import _lib as lib_mod
    _lib()
    for c, lanes in ((32, 8), (96, 8), (128, 8), (160, 16), (192, 16), (384, 32), (768, 64), (1536, 64), (4096, 64)):
        for layout in (0, 1):
            assert lib_mod.tile_query("orp_token_layernorm_plan", 3, 1, 64, 64, c, layout) == (lanes, 256 // lanes, 0), (c, layout)
        for layout in (2, 3):
            for hw in ((256, 256), (32, 32), (5, 3)):
                got = lib_mod.tile_query("orp_token_layernorm_plan", 3, 1, hw[0], hw[1], c, layout)
                assert got[0] == lanes and got[1] in (32, 16, 8) and got[2] == c * (got[1] + 1) * 4 <= LDS_MAX, (c, layout, hw, got)
                assert got[2] <= 65536 or got[1] == 8
    # the widest tile that still gives 256 workgroups, else the narrowest
    assert lib_mod.tile_query("orp_token_layernorm_plan", 3, 1, 256, 256, 96, 3)[1] == 32
    assert lib_mod.tile_query("orp_token_layernorm_plan", 3, 1, 32, 32, 768, 3)[1] == 8
    assert lib_mod.tile_query("orp_token_layernorm_plan", 3, 1, 64, 64, 768, 3)[1] == 16
    for bad in ((1, 8, 8, 100, 0), (1, 8, 8, 96, 4), (1, 8, 8, 96, -1), (-1, 8, 8, 96, 0), (1, -8, 8, 96, 0), (1, 8, -8, 96, 2)):
        assert lib_mod.tile_query("orp_token_layernorm_plan", 3, *bad) is None, bad


def test_pays_is_a_closed_table():
    """whatever the table holds, it answers 0 or 1 at the Swin-T spans and 0 everywhere else: refused widths, unknown layouts, token
    counts beyond a 1536^2 image's or below a 1024^2 image's last stage, and the 300- and 80-token shapes of the existing Swin tests"""
    L = _lib()
    for c in SWIN_C:
        for layout in range(4):
            for t in (1024, 2304, 4096, 9216, 16384, 36864, 65536, 147456):
                assert L.orp_token_layernorm_pays(t, c, layout) in (0, 1)
            for t in (0, -1, 1, 80, 300, 1023, 147457, 1 << 40):
                assert L.orp_token_layernorm_pays(t, c, layout) == 0, (t, c, layout)
    for t, c, layout in ((65536, 100, 0), (65536, 31, 0), (65536, 4128, 0), (65536, 96, 4), (65536, 96, -1), (65536, 32, 0), (65536, 160, 0),
                         (65536, 4096, 0), (300, 96, 0), (80, 384, 1), (300, 96, 3), (300, 24, 0), (80, 96, 1)):
        assert L.orp_token_layernorm_pays(t, c, layout) == 0, (t, c, layout)


def test_launch_refuses_bad_arguments_without_a_device():
    """the argument checks come before any device call: ORP_EINVAL for null or misaligned pointers, a refused width, an unknown layout, a
    negative extent and y aliasing x; no rows is ORP_OK"""
    from orientedreppoints_amd import _lib as lib_mod
    L = _lib()
    x, g, b, y = (ctypes.c_void_p(4096 * (i + 1)) for i in range(4))
    odd = ctypes.c_void_p(4096 + 4)
    E = lib_mod.ORP_EINVAL
    eps = ctypes.c_float(1e-5)
    for layout in range(4):
        for empty in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
            assert L.orp_token_layernorm(x, g, b, y, *empty, 96, eps, layout, None) == lib_mod.ORP_OK
        for ptrs in ((None, g, b, y), (x, None, b, y), (x, g, None, y), (x, g, b, None), (odd, g, b, y), (x, odd, b, y), (x, g, odd, y),
                     (x, g, b, odd), (x, g, b, x)):
            assert L.orp_token_layernorm(*ptrs, 2, 8, 8, 96, eps, layout, None) == E, (ptrs, layout)
            assert L.orp_token_layernorm(*ptrs, 0, 8, 8, 96, eps, layout, None) == E, (ptrs, layout)
        for bad in ((-1, 8, 8, 96), (2, -8, 8, 96), (2, 8, -8, 96), (2, 8, 8, 100), (2, 8, 8, 31), (2, 8, 8, 0), (2, 8, 8, 4128)):
            assert L.orp_token_layernorm(x, g, b, y, *bad, eps, layout, None) == E, (bad, layout)
    for layout in (-1, 4, 17):
        assert L.orp_token_layernorm(x, g, b, y, 2, 8, 8, 96, eps, layout, None) == E


def _sources(layout, dtype=torch.float64):
    """(x, hw) with odd H and W and B = 2, C = 64"""
    g = torch.Generator().manual_seed(5)
    if layout == 'tokens':
        return torch.randn((2, 15 * 21, 64), generator=g, dtype=dtype), None
    if layout == 'merge':
        return torch.randn((2, 15 * 21, 16), generator=g, dtype=dtype), (15, 21)
    if layout == 'from_nchw':
        return torch.randn((2, 64, 15, 21), generator=g, dtype=dtype), None
    return torch.randn((2, 15 * 21, 64), generator=g, dtype=dtype), (15, 21)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_reference_in_float64_is_the_lines_of_swin(layout):
    from orientedreppoints_amd.mmdet_ops.token_norm import token_layernorm_reference
    g = torch.Generator().manual_seed(3)
    w = torch.randn((64,), generator=g, dtype=torch.float64)
    b = torch.randn((64,), generator=g, dtype=torch.float64)
    x, hw = _sources(layout)
    if layout == 'tokens':
        want = F.layer_norm(x, (64,), w, b, 1e-5)
    elif layout == 'merge':
        v = F.pad(x.view(2, 15, 21, 16), (0, 0, 0, 1, 0, 1))
        v = torch.cat([v[:, 0::2, 0::2], v[:, 1::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 1::2]], -1)
        want = F.layer_norm(v.view(2, -1, 64), (64,), w, b, 1e-5)
        assert tuple(want.shape) == (2, 8 * 11, 64)
    elif layout == 'from_nchw':
        want = F.layer_norm(x.flatten(2).transpose(1, 2), (64,), w, b, 1e-5)
    else:
        want = F.layer_norm(x, (64,), w, b, 1e-5).view(-1, 15, 21, 64).permute(0, 3, 1, 2).contiguous()
        assert tuple(want.shape) == (2, 64, 15, 21)
    got = token_layernorm_reference(x, w, b, 1e-5, layout, hw)
    assert got.dtype == torch.float64 and got.shape == want.shape and got.stride() == want.stride() and torch.equal(got, want)
    if layout == 'merge':       # the 4-D source carries H and W itself
        assert torch.equal(token_layernorm_reference(x.view(2, 15, 21, 16), w, b, 1e-5, layout), want)
    with pytest.raises(ValueError):
        token_layernorm_reference(x, w, b, 1e-5, 'nhwc', hw)
    with pytest.raises(ValueError):
        token_layernorm_reference(x, w[:32], b[:32], 1e-5, layout, hw)


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


def test_token_layernorm_ok_on_described_tensors():
    from orientedreppoints_amd.mmdet_ops.token_norm import token_layernorm, token_layernorm_ok, token_layernorm_routed
    ln = torch.nn.LayerNorm(96)
    x32 = dict(is_cuda=True, dtype=torch.float32)
    assert not token_layernorm_ok(ln, _Described(**x32))                       # gradients are enabled
    with torch.no_grad():
        assert token_layernorm_ok(ln, _Described(**x32))
        assert token_layernorm_ok(ln, _Described(shape=(96,), **x32)) and token_layernorm_ok(ln, _Described(shape=(2, 3, 5, 96), **x32))
        assert token_layernorm_ok(ln, _Described(shape=(2, 300, 24), **x32), 'merge', (15, 20))
        assert token_layernorm_ok(ln, _Described(shape=(2, 15, 20, 24), **x32), 'merge')
        assert token_layernorm_ok(ln, _Described(shape=(2, 96, 300), **x32), 'from_nchw')
        assert token_layernorm_ok(ln, _Described(shape=(2, 96, 15, 20), **x32), 'from_nchw')
        assert token_layernorm_ok(ln, _Described(shape=(2, 300, 96), **x32), 'to_nchw', (15, 20))
        # shapes that are not the layout's source
        assert not token_layernorm_ok(ln, _Described(shape=(2, 300, 24), **x32), 'merge')              # no H, W
        assert not token_layernorm_ok(ln, _Described(shape=(2, 300, 24), **x32), 'merge', (15, 21))
        assert not token_layernorm_ok(ln, _Described(shape=(2, 300, 96), **x32), 'merge', (15, 20))    # 4 x 96 is not this norm's width
        assert not token_layernorm_ok(ln, _Described(shape=(2, 300, 96), **x32), 'from_nchw')
        assert not token_layernorm_ok(ln, _Described(shape=(2, 300, 96), **x32), 'to_nchw')
        assert not token_layernorm_ok(ln, _Described(shape=(2, 300, 96), **x32), 'to_nchw', (15, 21))
        assert not token_layernorm_ok(ln, _Described(shape=(1, 300, 192), **x32))
        assert not token_layernorm_ok(ln, _Described(**x32), 'nhwc')
        # tensors and modules the kernel does not take
        assert not token_layernorm_ok(ln, _Described(is_cuda=False, dtype=torch.float32))
        assert not token_layernorm_ok(ln, torch.zeros(1, 300, 96))                                # a CPU tensor
        assert not token_layernorm_ok(ln, _Described(is_cuda=True, dtype=torch.float16))
        assert not token_layernorm_ok(ln, _Described(is_cuda=True, dtype=torch.float64))
        assert not token_layernorm_ok(ln, _Described(contiguous=False, **x32))
        assert not token_layernorm_ok(ln, _Described(device=torch.device('meta'), **x32))          # parameters on another device
        assert not token_layernorm_ok(torch.nn.LayerNorm(100), _Described(shape=(1, 300, 100), **x32))     # a width the kernel refuses
        assert not token_layernorm_ok(torch.nn.LayerNorm(96).half(), _Described(**x32))            # a model.half() layer
        assert not token_layernorm_ok(torch.nn.LayerNorm(96, elementwise_affine=False), _Described(**x32))
        assert not token_layernorm_ok(torch.nn.LayerNorm((300, 96)), _Described(**x32))            # two normalised axes
        assert not token_layernorm_ok(torch.nn.GroupNorm(1, 96), _Described(**x32))
        with _cuda_autocast():
            assert not token_layernorm_ok(ln, _Described(**x32))
        # outside the table nothing is routed, whatever the predicate says
        assert not token_layernorm_routed(ln, _Described(**x32))
        assert not token_layernorm_routed(ln, _Described(shape=(2, 300, 96), **x32), 'to_nchw', (15, 20))
        with pytest.raises(ValueError):
            token_layernorm(torch.zeros(1, 300, 96), ln, force=True)            # never a fall-back
        with pytest.raises(ValueError):
            token_layernorm(torch.zeros(1, 300, 96), ln, layout='nhwc', force=True)
    with torch.enable_grad():
        assert not token_layernorm_ok(ln, _Described(**x32))


def test_modules_carry_the_switch_attributes():
    from orientedreppoints_amd import switches
    from orientedreppoints_amd.mmdet_models.swin import PatchEmbed, PatchMerging, SwinBlock, SwinTransformer
    assert isinstance(switches.SWIN_NORM_FUSE, bool)
    mods = (SwinBlock(96, 3, 7, 0, 4., True, None, 0., 0., 0.1), PatchMerging(96), PatchEmbed(),
            SwinTransformer(embed_dim=32, depths=(1, 1), num_heads=(1, 2), out_indices=(0, 1)))
    for m in mods:
        assert m.fuse_token_norm is None and m.force_token_norm is False, type(m).__name__


def _randomise_norms(model):
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.normal_(1.0, 0.3)
                m.bias.normal_(0.0, 0.3)


def test_cpu_modules_keep_their_bits(monkeypatch):
    """CPU tensors run the modules as written, bit for bit, whatever the switch and the attributes say: a stage with its merge against
    the lines of the modules spelled out here, and a whole backbone with the switch off and on"""
    from orientedreppoints_amd import switches
    from orientedreppoints_amd.mmdet_models.swin import SwinStage, SwinTransformer
    torch.manual_seed(0)
    st = SwinStage(32, 2, 2, 7, 4., True, None, 0., 0., [0., 0.], True, False).eval()
    _randomise_norms(st)
    x = torch.randn(2, 15 * 21, 32)
    with torch.no_grad():
        monkeypatch.setattr(switches, "SWIN_NORM_FUSE", False)
        want = st(x, 15, 21)
        monkeypatch.setattr(switches, "SWIN_NORM_FUSE", True)
        for m in list(st.blocks) + [st.downsample]:
            m.force_token_norm = True
        got = st(x, 15, 21)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2:] == want[2:] == (8, 11)
        # the merge is the lines PatchMerging always ran
        pm = st.downsample
        v = F.pad(want[0].view(2, 15, 21, 32), (0, 0, 0, 1, 0, 1))
        cat = torch.cat([v[:, 0::2, 0::2], v[:, 1::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 1::2]], -1)
        assert torch.equal(want[1], pm.reduction(pm.norm(cat.view(2, -1, 128))))
        # a block is x + proj(attention(norm1 x)), then + mlp(norm2 .): norm1 / norm2 are the modules themselves
        blk = st.blocks[0]
        seen = []
        hooks = [n.register_forward_hook(lambda mod, args, out: seen.append(mod)) for n in (blk.norm1, blk.norm2)]
        blk(x, 15, 21, None)
        for h in hooks:
            h.remove()
        assert seen == [blk.norm1, blk.norm2]

        torch.manual_seed(1)
        net = SwinTransformer(embed_dim=32, depths=(2, 2), num_heads=(2, 4), out_indices=(0, 1), drop_path_rate=0.).eval()
        _randomise_norms(net)
        img = torch.randn(2, 3, 61, 83)
        monkeypatch.setattr(switches, "SWIN_NORM_FUSE", False)
        want = net(img)
        # the embedding and an output norm, spelled out
        e = net.patch_embed
        p = e.proj(F.pad(img, (0, 1, 0, 3)))
        assert torch.equal(e(img), e.norm(p.flatten(2).transpose(1, 2)).transpose(1, 2).reshape(2, 32, 16, 21))
        monkeypatch.setattr(switches, "SWIN_NORM_FUSE", True)
        for m in net.modules():
            if hasattr(m, 'force_token_norm'):
                m.force_token_norm = True
        got = net(img)
        assert len(got) == len(want) == 2
        for a, b in zip(got, want):
            assert a.shape == b.shape and a.stride() == b.stride() and a.is_contiguous() and torch.equal(a, b)
        assert tuple(got[0].shape) == (2, 32, 16, 21) and tuple(got[1].shape) == (2, 64, 8, 11)


def test_kernels_compile_without_spills_or_scratch_inside_the_lds_plan():
    """compiles csrc/orp_token_layernorm.hip with the library's flags and reads the compiler's resource remarks: all twenty-four
    instantiations (four layouts x six (lanes, float4 per lane) shapes) spill nothing, use no scratch, declare no static LDS (the NCHW
    tile is dynamic: `orp_token_layernorm_plan`, at most 147 456 B of the CU's 163 840) and fit 256 threads in registers; the shapes
    Swin-T to Swin-L launch (at most eight float4 per lane) keep at least four waves per SIMD"""
    from orientedreppoints_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not found")
    assert ("orp_token_layernorm.hip", []) in build.SOURCES                  # the library's flags: no packed fp32, contraction on
    src = os.path.join(build.CSRC, "orp_token_layernorm.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC] + build.COMMON + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "ln.o")]
        r = subprocess.run(cmd, cwd=build.CSRC, stderr=subprocess.PIPE, stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    seen = {}
    for blk in blocks:
        name = blk.split()[0]
        if "token_layernorm_kernel" not in name:
            continue

        def num(key):
            return int(re.search(re.escape(key) + r":\s+(\d+)", blk).group(1))
        seen[name] = dict(vgprs=num("VGPRs"), agprs=num("AGPRs"), scratch=num("ScratchSize [bytes/lane]"), sgpr_spill=num("SGPRs Spill"),
                          vgpr_spill=num("VGPRs Spill"), lds=num("LDS Size [bytes/block]"), occupancy=num("Occupancy [waves/SIMD]"))
    assert len(seen) == 24, sorted(seen)
    for name, u in seen.items():
        assert u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0 and u["scratch"] == 0, (name, u)
        assert u["vgprs"] + u["agprs"] <= 256 and u["occupancy"] >= 1 and u["lds"] == 0, (name, u)
        if "ELi16EEE" not in name:                                            # (sixteen float4 per lane: c beyond 2048)
            assert u["occupancy"] >= 4, (name, u)
    with open(src) as f:
        assert "atomic" not in f.read().replace("No atomics", "").replace("no atomics", "")
