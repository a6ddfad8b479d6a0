"""The register budget of conv1x1_bn_pieces_kernel, held by a test rather than by a table in a notebook: every instantiation --
the MODE 3 ones above all, whose 128 x 64 tile keeps r next to the accumulators and whose scalar fetch forms its addresses per load
so that sixteen running ones are not held through the loop -- compiles for gfx950 without a spilled register and without scratch,
inside the 256 registers that two workgroups per CU leave a wave.  Device-side compilation only; no GPU."""
import os
import re
import subprocess

import pytest

from orientedreppoints_amd import build


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    assert os.path.exists(build.HIPCC), "hipcc builds the library: it is there wherever the tests run"
    out = tmp_path_factory.mktemp("pieces_resources")
    cmd = [build.HIPCC] + build.COMMON + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                          os.path.join(build.CSRC, "orp_conv1x1_bn_pieces.hip"), "-o", str(out / "k.s")]
    r = subprocess.run(cmd, cwd=build.CSRC, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:\S+: )?\s*(.*?) \[-Rpass-analysis", line) or re.search(r":\d+:\d+:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).replace("remark: ", "").strip()
        t = re.sub(r"^\S+:\d+:\d+:\s*", "", t)
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            rows[cur] = {}
        elif cur and ":" in t:
            k, v = t.rsplit(":", 1)
            rows[cur][k.strip()] = v.strip()
    return {k: v for k, v in rows.items() if "conv1x1_bn_pieces_kernel" in k}


def test_no_instantiation_spills_or_uses_scratch(usage):
    assert len(usage) == 38, sorted(usage)                         # 32 of modes 0 - 2 (+ range) and the 6 of MODE 3
    for name, u in usage.items():
        assert int(u["VGPRs Spill"]) == 0 and int(u["ScratchSize [bytes/lane]"]) == 0, (name, u)     # (SGPRs may spill into VGPR lanes)
        assert int(u["VGPRs"]) + int(u["AGPRs"]) <= 256 and int(u["Occupancy [waves/SIMD]"]) >= 2, (name, u)


def test_the_dual_instantiations_are_there(usage):
    """MODE is the fifth template argument: <4, WN, 64, VEC, 3, false, SAMP> mangles as ...Li64ELb?ELi3ELb0ELb?E"""
    dual = [k for k in usage if re.search(r"Li4ELi[12]ELi64ELb[01]ELi3ELb0ELb[01]E", k)]
    assert len(dual) == 6, dual
