"""Golden files for the fast merge from THE REFERENCE'S OWN DOTA_devkit/ResultMerge_multi_process.py, run here on the
CPU: its `mergebase` (the serial loop; `mergebypoly` would spread the files over a 16-process pool) with
`py_cpu_nms_poly_fast` at the module's `nms_thresh = 0.1`, over the raw patch files of tests/golden/merge/raw.  As in
make_golden_merge.py, `dota_utils` imports shapely (absent): a stub `shapely.geometry` is registered before import, and
the reference's `polyiou` SWIG module is built from its own sources into /tmp (its loader falls back to a top-level
`_polyiou` on sys.path).
    python tests/golden/make_golden_merge_mp.py     -> tests/golden/merge_mp/merged/Task1_*.txt
"""
import os
import shutil
import subprocess
import sys
import sysconfig
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("ORP_REFERENCE_ROOT", "/root/reference")
REF = os.path.join(REF_ROOT, "DOTA_devkit")
BUILD = "/tmp/ref_polyiou_build"
os.makedirs(BUILD, exist_ok=True)
so = os.path.join(BUILD, "_polyiou" + sysconfig.get_config_var("EXT_SUFFIX"))
if not os.path.exists(so):
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I" + sysconfig.get_paths()["include"],
                           os.path.join(REF, "polyiou.cpp"), os.path.join(REF, "polyiou_wrap.cxx"), "-o", so])
sys.path.insert(0, BUILD)
sys.path.insert(0, REF_ROOT)
shp = types.ModuleType("shapely"); geo = types.ModuleType("shapely.geometry")
shp.geometry = geo; sys.modules["shapely"] = shp; sys.modules["shapely.geometry"] = geo
import DOTA_devkit.ResultMerge_multi_process as RMP  # noqa: E402  (the reference module)

raw, merged = os.path.join(HERE, "merge", "raw"), os.path.join(HERE, "merge_mp", "merged")
shutil.rmtree(merged, ignore_errors=True)
os.makedirs(merged)
RMP.mergebase(raw, merged, RMP.py_cpu_nms_poly_fast)
print("nms_thresh", RMP.nms_thresh,
      {f: sum(1 for _ in open(os.path.join(raw, f))) for f in sorted(os.listdir(raw))},
      {f: sum(1 for _ in open(os.path.join(merged, f))) for f in sorted(os.listdir(merged))})
