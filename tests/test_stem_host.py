"""CPU: the host side of orp_stem_conv_bn_relu_pool -- what its queries answer and refuse without a device, and what its kernels cost in
registers and LDS when the source is compiled for gfx950 (no launch)."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAX = 163840
WORKGROUPS_PER_CU = 2                 # the plan of csrc/orp_stem.hip: one workgroup stages while the other multiplies
WAVES_PER_WORKGROUP = 4
TILE_LDS = 64 * 9 * 33 * 4            # the conv tile of the epilogue, [64 channels][9 x 33 positions] fp32; the patch lies inside it


def _lib():
    from orientedreppoints_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def test_ok_takes_the_stem_convolution_only():
    L = _lib()
    assert L.orp_stem_ok(3, 64, 7, 2, 3) == 1
    for args in ((4, 64, 7, 2, 3), (3, 32, 7, 2, 3), (64, 3, 7, 2, 3), (3, 64, 3, 2, 3), (3, 64, 5, 2, 2), (3, 64, 7, 1, 3),
                 (3, 64, 7, 2, 2), (3, 64, 7, 2, 0), (0, 0, 0, 0, 0), (-3, -64, -7, -2, -3)):
        assert L.orp_stem_ok(*args) == 0, args


def test_packed_bytes():
    L = _lib()
    assert L.orp_stem_packed_bytes(3, 64) == 2 * 74 * 64 * 4          # two channel blocks x 74 steps of two taps x 64 lanes
    for cin, cout in ((3, 32), (4, 64), (64, 3), (64, 64), (0, 0), (-3, 64)):
        assert L.orp_stem_packed_bytes(cin, cout) == 0


def test_pays_is_a_closed_table():
    """one image from 1024^2 to 1536^2 (both sides inside), two images at 1024^2, nothing beyond a timed corner and no degenerate size"""
    L = _lib()
    inside = [(1024, 1024, 1), (1536, 1536, 1), (1024, 1536, 1), (1200, 1100, 1), (1024, 1024, 2)]
    outside = [(1023, 1024, 1), (1024, 1023, 1), (1537, 1536, 1), (1536, 1537, 1), (2048, 2048, 1), (512, 512, 1), (76, 68, 1),
               (1025, 1024, 2), (1536, 1536, 2), (1024, 1024, 3), (1, 1024 * 1024, 1), (0, 1024, 1), (1024, 0, 1), (-1024, 1024, 1),
               (1024, 1024, 0), (1024, 1024, -1)]
    paid = [L.orp_stem_pays(*a) for a in inside]
    assert paid[2] == paid[3] == (1 if paid[0] and paid[1] else 0)
    assert all(p in (0, 1) for p in paid)
    for a in outside:
        assert L.orp_stem_pays(*a) == 0, a


def test_launch_and_pack_refuse_bad_arguments_without_a_device():
    """the argument checks come before any device call: ORP_EINVAL for null pointers, other shapes and non-positive sizes"""
    import ctypes
    from orientedreppoints_amd import _lib as lib_mod
    L = _lib()
    p = ctypes.c_void_p(4096)
    q = ctypes.c_void_p(8192)
    good = (1, 3, 64, 16, 64, 7, 2, 3, 1)
    for k, v in ((0, 0), (1, 4), (2, 32), (3, 0), (4, -1), (5, 3), (6, 1), (7, 1), (8, 2)):
        bad = list(good)
        bad[k] = v
        assert L.orp_stem_conv_bn_relu_pool(p, p, p, p, q, *bad, None) == lib_mod.ORP_EINVAL, (k, v)
    for ptrs in ((None, p, p, p, q), (p, None, p, p, q), (p, p, None, p, q), (p, p, p, None, q), (p, p, p, p, None), (p, p, p, p, p)):
        assert L.orp_stem_conv_bn_relu_pool(*ptrs, *good, None) == lib_mod.ORP_EINVAL
    assert L.orp_stem_pack_weight(None, 3, 64, p, None) == lib_mod.ORP_EINVAL
    assert L.orp_stem_pack_weight(p, 3, 64, None, None) == lib_mod.ORP_EINVAL
    assert L.orp_stem_pack_weight(p, 3, 32, q, None) == lib_mod.ORP_EINVAL


def test_kernels_compile_without_spills_or_scratch_inside_the_lds_plan():
    """compiles csrc/orp_stem.hip with the library's flags and reads the compiler's resource remarks: both modes of the kernel spill
    nothing, use no scratch, and fit WORKGROUPS_PER_CU workgroups of four waves on a CU both ways: two waves per SIMD in registers (at
    most 256 each) and twice the static LDS -- the 76 032 B conv tile, nothing beside it -- inside 163 840 B"""
    from orientedreppoints_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not found")
    src = os.path.join(build.CSRC, "orp_stem.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC] + build.COMMON + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "stem.o")]
        r = subprocess.run(cmd, cwd=build.CSRC, stderr=subprocess.PIPE, stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    seen = {}
    for blk in blocks:
        name = blk.split()[0]
        if "stem_kernel" not in name:
            continue

        def num(key):
            return int(re.search(re.escape(key) + r":\s+(\d+)", blk).group(1))
        seen[name] = dict(vgprs=num("VGPRs"), agprs=num("AGPRs"), scratch=num("ScratchSize [bytes/lane]"), sgpr_spill=num("SGPRs Spill"),
                          vgpr_spill=num("VGPRs Spill"), lds=num("LDS Size [bytes/block]"), occupancy=num("Occupancy [waves/SIMD]"))
    assert len(seen) == 2, sorted(seen)                            # pool = 1 and pool = 0
    waves_per_simd = WORKGROUPS_PER_CU * WAVES_PER_WORKGROUP // 4
    assert TILE_LDS == 76032
    for name, u in seen.items():
        assert u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0 and u["scratch"] == 0, (name, u)
        assert u["vgprs"] + u["agprs"] <= 512 // waves_per_simd and u["occupancy"] >= waves_per_simd, (name, u)
        assert u["lds"] == TILE_LDS, (name, u)
        assert WORKGROUPS_PER_CU * u["lds"] <= LDS_MAX, (name, u)
