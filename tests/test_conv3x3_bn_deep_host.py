"""CPU: the host side of orp_conv3x3_bn_deep -- what its queries answer, and what its two kernels cost in registers and LDS when the
source is compiled for gfx950 (no launch)."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAX = 163840


def _lib():
    from orientedreppoints_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def test_ok_takes_512_channels_at_stride_1_and_2_only():
    L = _lib()
    for cin in (64, 128, 256, 512, 1024, 2048):
        for cout in (64, 256, 512, 2048):
            for s in (-1, 0, 1, 2, 3, 4):
                assert L.orp_conv3x3_bn_deep_ok(cin, cout, s) == (1 if (cin, cout) == (512, 512) and s in (1, 2) else 0)
    # the first route's answers are what they were
    assert [L.orp_conv3x3_bn_act_ok(c, c) for c in (64, 128, 256, 512)] == [1, 1, 1, 0]
    assert L.orp_conv3x3_bn_act_pays(512, 512, 32, 32, 1) == 0


def test_packed_bytes():
    L = _lib()
    assert L.orp_conv3x3_bn_deep_packed_bytes(512, 512) == 4 * 512 * 512 * 9 + 16
    for cin, cout in ((256, 256), (512, 256), (256, 512), (0, 0)):
        assert L.orp_conv3x3_bn_deep_packed_bytes(cin, cout) == 0


def test_pays_refuses_what_ok_refuses_and_degenerate_maps():
    L = _lib()
    for args in ((256, 256, 64, 64, 1, 1), (512, 512, 32, 32, 3, 1), (512, 512, 32, 32, 0, 1), (512, 512, 0, 32, 1, 1),
                 (512, 512, 32, -1, 1, 1), (512, 512, 32, 32, 1, 0), (512, 512, 64, 64, 2, -2)):
        assert L.orp_conv3x3_bn_deep_pays(*args) == 0
    # a closed table: nothing below the 1024^2 image's map, above the 1536^2 image's, beyond two images or off the square maps
    for s, side in ((1, 32), (2, 64)):
        for h, w, b in ((side - 1, side - 1, 1), (side * 2, side * 2, 1), (side, side, 3), (side * 3 // 2, side * 3 // 2, 2),
                        (1, side * side, 1), (side // 2, side * 2, 1)):
            assert L.orp_conv3x3_bn_deep_pays(512, 512, h, w, s, b) == 0


def test_kernels_compile_without_spills_or_scratch_inside_the_lds_limit():
    """compiles csrc/orp_conv3x3_bn_deep.hip with the library's flags and reads the compiler's resource remarks: both kernels spill
    nothing, use no scratch and fit two waves per SIMD (512 threads); the halo planes are dynamic LDS, 149 760 B at stride 1 and
    89 760 B per pass at stride 2 (the source's static_assert refuses more than 163 840 B at compile time)"""
    from orientedreppoints_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not found")
    src = os.path.join(build.CSRC, "orp_conv3x3_bn_deep.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC] + build.COMMON + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "deep.o")]
        r = subprocess.run(cmd, cwd=build.CSRC, stderr=subprocess.PIPE, stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    seen = {}
    for blk in blocks:
        name = blk.split()[0]
        if "conv3x3_bn_deep_kernel" not in name:
            continue
        def num(key):
            return int(re.search(re.escape(key) + r":\s+(\d+)", blk).group(1))
        seen[name] = dict(vgprs=num("VGPRs"), agprs=num("AGPRs"), scratch=num("ScratchSize [bytes/lane]"), sgpr_spill=num("SGPRs Spill"),
                          vgpr_spill=num("VGPRs Spill"), lds=num("LDS Size [bytes/block]"), occupancy=num("Occupancy [waves/SIMD]"))
    assert len(seen) == 2, sorted(seen)
    for name, u in seen.items():
        assert u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0 and u["scratch"] == 0, (name, u)
        assert u["vgprs"] + u["agprs"] <= 256 and u["occupancy"] >= 2, (name, u)
    halo = {1: 4 * 18 * (512 + 8) * 2 * 2, 2: 5 * 33 * (128 + 8) * 2 * 2}
    assert halo == {1: 149760, 2: 89760}
    for name, u in seen.items():
        assert u["lds"] + max(halo.values()) <= LDS_MAX, (name, u)
