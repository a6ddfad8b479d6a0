"""The code-object metadata of the window-attention kernels in the built library (csrc/orp_window_attn.hip), shared by the three CPU
test files of the route: one scan of the gfx950 code object's notes."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

KERNELS = ("wattn_bwd_kernel", "wattn_fwd_kernel")            # templates over <head dim, operand type>
HEAD_DIMS = tuple(range(4, 33, 4))
OPERANDS = (0, 1, 2)                                          # fp32, fp16, bf16
VGPR_CAP = 168                                                # every instantiation declares amdgpu_waves_per_eu(3)


@functools.lru_cache(maxsize=None)
def instantiations():
    """{(kernel, head dim, operand type): (spilled VGPRs, scratch bytes, VGPRs, LDS bytes)} of every instantiation of the forward and
    the backward kernel; a kernel under one of these names that is no such instantiation, or one met twice, fails here"""
    from orientedreppoints_amd import build, _lib
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(objdump) and os.path.exists(readelf), "the llvm tools of the toolchain that builds the library"
    build.build_hip()
    seen = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "liborp_hip.so")
        shutil.copy(_lib.LIB_PATH, so)
        subprocess.run([objdump, "--offloading", so], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
        for b in [f for f in os.listdir(tmp) if f.endswith("gfx950")]:
            notes = subprocess.run([readelf, "--notes", os.path.join(tmp, b)], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
            for blk in notes.split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                m = re.search(r"(wattn_fwd_kernel|wattn_bwd_kernel)ILi(\d+)ELi(\d+)E", name)
                if not m:
                    assert "wattn_fwd" not in name and "wattn_bwd" not in name and "window_attn" not in name, name
                    continue
                key = (m.group(1), int(m.group(2)), int(m.group(3)))
                assert key not in seen, name
                seen[key] = tuple(int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                                  for k in ("vgpr_spill_count", "private_segment_fixed_size", "vgpr_count", "group_segment_fixed_size"))
    return seen
