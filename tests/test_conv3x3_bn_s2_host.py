"""CPU: the host side of orp_conv3x3_bn_s2 -- what its queries answer (and that the other two 3x3 routes answer what they did), and what
its two kernels cost in registers and LDS when the source is compiled for gfx950 (no launch)."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAX = 163840
WORKGROUPS_PER_CU = 2                 # the plan of csrc/orp_conv3x3_bn_s2.hip: one workgroup stages while the other multiplies
PASS_LDS = 5 * 33 * (64 + 8) * 2 * 2  # a 64-channel pass of the 5 x 33 halo, two fp16 planes


def _lib():
    from orientedreppoints_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def test_ok_takes_128_and_256_channels_only():
    L = _lib()
    for cin in (-128, 0, 64, 128, 192, 256, 512, 1024):
        for cout in (0, 64, 128, 256, 512):
            assert L.orp_conv3x3_bn_s2_ok(cin, cout) == (1 if cin == cout and cin in (128, 256) else 0)


def test_the_other_routes_answer_what_they_did():
    L = _lib()
    assert [L.orp_conv3x3_bn_act_ok(c, c) for c in (64, 128, 256, 512)] == [1, 1, 1, 0]
    assert L.orp_conv3x3_bn_act_pays(512, 512, 32, 32, 1) == 0
    for c in (64, 128, 256, 512):
        for s in (1, 2):
            assert L.orp_conv3x3_bn_deep_ok(c, c, s) == (1 if c == 512 else 0)
    # the deep route's table (docs/notebook/round23.md) and the absence of the new route's channels from it
    assert [L.orp_conv3x3_bn_deep_pays(512, 512, h, h, s, b) for (h, s, b) in
            ((32, 1, 1), (48, 1, 1), (32, 1, 2), (64, 2, 1), (96, 2, 1), (64, 2, 2), (48, 1, 2), (96, 2, 2), (128, 2, 1))] == \
        [1, 1, 1, 1, 1, 1, 0, 0, 0]
    for c, side in ((128, 256), (256, 128)):
        assert L.orp_conv3x3_bn_deep_pays(c, c, side, side, 2, 1) == 0
    assert L.orp_conv3x3_bn_deep_packed_bytes(512, 512) == 4 * 512 * 512 * 9 + 16
    assert L.orp_conv3x3_bn_deep_packed_bytes(256, 256) == 0


def test_packed_bytes():
    L = _lib()
    for c in (128, 256):
        assert L.orp_conv3x3_bn_s2_packed_bytes(c, c) == 4 * c * c * 9 + 16
    for cin, cout in ((64, 64), (512, 512), (128, 256), (256, 128), (0, 0)):
        assert L.orp_conv3x3_bn_s2_packed_bytes(cin, cout) == 0


def test_pays_refuses_what_ok_refuses_and_degenerate_maps():
    L = _lib()
    for args in ((64, 64, 256, 256, 1), (512, 512, 64, 64, 1), (128, 256, 256, 256, 1), (128, 128, 0, 256, 1),
                 (128, 128, 256, -1, 1), (128, 128, 256, 256, 0), (256, 256, 128, 128, -2)):
        assert L.orp_conv3x3_bn_s2_pays(*args) == 0
    # a closed table: nothing below the 1024^2 image's map, above the 1536^2 image's, beyond two images or off the square maps
    for c, side in ((128, 256), (256, 128)):
        for h, w, b in ((side - 1, side - 1, 1), (side * 2, side * 2, 1), (side, side, 3), (side * 3 // 2, side * 3 // 2, 2),
                        (1, side * side, 1), (side // 2, side * 2, 1)):
            assert L.orp_conv3x3_bn_s2_pays(c, c, h, w, b) == 0
        # the other C's map is not this C's
        assert L.orp_conv3x3_bn_s2_pays(c, c, 384 - side, 384 - side, 2) == 0


def test_kernels_compile_without_spills_or_scratch_inside_the_lds_plan():
    """compiles csrc/orp_conv3x3_bn_s2.hip with the library's flags and reads the compiler's resource remarks: both kernels spill
    nothing, use no scratch, and fit WORKGROUPS_PER_CU workgroups of eight waves on a CU both ways: four waves per SIMD in registers
    (at most 128 each), and static LDS + the 47 520 B pass, twice, inside 163 840 B"""
    from orientedreppoints_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not found")
    src = os.path.join(build.CSRC, "orp_conv3x3_bn_s2.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC] + build.COMMON + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "s2.o")]
        r = subprocess.run(cmd, cwd=build.CSRC, stderr=subprocess.PIPE, stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    seen = {}
    for blk in blocks:
        name = blk.split()[0]
        if "conv3x3_bn_s2_kernel" not in name:
            continue

        def num(key):
            return int(re.search(re.escape(key) + r":\s+(\d+)", blk).group(1))
        seen[name] = dict(vgprs=num("VGPRs"), agprs=num("AGPRs"), scratch=num("ScratchSize [bytes/lane]"), sgpr_spill=num("SGPRs Spill"),
                          vgpr_spill=num("VGPRs Spill"), lds=num("LDS Size [bytes/block]"), occupancy=num("Occupancy [waves/SIMD]"))
    assert len(seen) == 2, sorted(seen)
    assert PASS_LDS == 47520
    for name, u in seen.items():
        assert u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0 and u["scratch"] == 0, (name, u)
        assert u["occupancy"] >= 2, (name, u)
        assert u["vgprs"] + u["agprs"] <= 512 // (2 * WORKGROUPS_PER_CU) and u["occupancy"] >= 2 * WORKGROUPS_PER_CU, (name, u)
        assert u["lds"] + PASS_LDS <= LDS_MAX, (name, u)
        assert WORKGROUPS_PER_CU * (u["lds"] + PASS_LDS) <= LDS_MAX, (name, u)
