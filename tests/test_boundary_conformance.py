"""CPU: the drop-in boundary -- the mirrors in orientedreppoints_amd/mmdet_ops + dota_devkit expose the
reference wrappers' names, parameter names and defaults, and the reference's own Python files resolve their native operators
through `compat.install_mmdet_aliases()`.  The reference side -- parsed with `ast` / regular expressions from its sources
where they lie -- is recorded in tests/golden/boundary.json by tests/golden/make_golden_boundary.py."""
import importlib
import inspect
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "boundary.json")

# (key, reference file, function, class or None, parameters dropped in front)
SIGNATURES = [
    ("nms_wrapper.rnms", "mmdet/ops/nms/nms_wrapper.py", "rnms", None, 0),
    ("nms_wrapper.soft_rnms", "mmdet/ops/nms/nms_wrapper.py", "soft_rnms", None, 0),
    ("iou_wrapper.convex_giou", "mmdet/ops/iou/iou_wrapper.py", "convex_giou", None, 0),
    ("iou_wrapper.convex_iou", "mmdet/ops/iou/iou_wrapper.py", "convex_iou", None, 0),
    ("iou_wrapper.convex_overlaps", "mmdet/ops/iou/iou_wrapper.py", "convex_overlaps", None, 0),
    ("chamfer_distance.ChamferDistance2D", "mmdet/ops/chamfer_distance.py", "ChamferDistance2D", None, 0),
    ("minarea_rect.minaerarect", "mmdet/ops/minarearect/minarea_rect.py", "minaerarect", None, 0),
] + [("deform_conv.%s.%s" % (c, m), "mmdet/ops/dcn/deform_conv.py", m, c, 1)
     for c in ("DeformConv", "ModulatedDeformConv", "DeformConvPack", "ModulatedDeformConvPack") for m in ("__init__", "forward")] + [
    ("deform_conv.%s.forward" % c, "mmdet/ops/dcn/deform_conv.py", "forward", c, 1) for c in ("DeformConvFunction", "ModulatedDeformConvFunction")] + [
    ("sigmoid_focal_loss.SigmoidFocalLossFunction.forward", "mmdet/ops/sigmoid_focal_loss/sigmoid_focal_loss.py", "forward",
     "SigmoidFocalLossFunction", 1),
    ("sigmoid_focal_loss.SigmoidFocalLoss.__init__", "mmdet/ops/sigmoid_focal_loss/sigmoid_focal_loss.py", "__init__", "SigmoidFocalLoss", 1),
]
# (key, Cython file, function)
PYX = [("poly_gpu_nms", "DOTA_devkit/poly_nms_gpu/poly_nms.pyx", "poly_gpu_nms"),
       ("poly_overlaps", "DOTA_devkit/poly_nms_gpu/poly_overlaps.pyx", "poly_overlaps")]
# (key, C++ file, regular expression of the declaration's parameter list)
PYBIND = [("pointsJf", "mmdet/ops/point_justify/src/points_justify.cpp", r"int\s+pointsJf\s*\((.*?)\)"),
          ("box_iou_rotated", "mmdet/ops/box_iou_rotated/src/box_iou_rotated.h", r"box_iou_rotated\s*\((.*?)\)")]
# reference Python files whose native-operator imports (`from mmdet.ops... import ...`) must resolve through the aliases
IMPORTING_FILES = ["mmdet/core/post_processing/bbox_nms.py", "mmdet/core/bbox/assigners/max_iou_assigner.py",
                   "mmdet/models/losses/iou_loss.py"]


def _decode(v):
    if isinstance(v, dict) and set(v) == {"__tuple__"}:
        return tuple(_decode(x) for x in v["__tuple__"])
    if isinstance(v, list):
        return [_decode(x) for x in v]
    return v


@pytest.fixture(scope="module")
def ref():
    with open(GOLDEN) as f:
        g = json.load(f)
    g["signatures"] = {k: [(n, _decode(d)) for n, d in v] for k, v in g["signatures"].items()}
    g["pyx"] = {k: [(n, _decode(d)) for n, d in v] for k, v in g["pyx"].items()}
    return g


def _sig_from_obj(obj, drop_first=0):
    out = []
    params = list(inspect.signature(obj).parameters.values())[drop_first:]
    for p in params:
        if p.kind == p.VAR_POSITIONAL:
            out.append(('*' + p.name, None))
        elif p.kind == p.VAR_KEYWORD:
            out.append(('**' + p.name, None))
        else:
            out.append((p.name, None if p.default is p.empty else p.default))
    return out


def test_function_wrappers_have_the_reference_signatures(ref):
    from orientedreppoints_amd.mmdet_ops import chamfer_distance, iou_wrapper, minarea_rect, nms_wrapper
    for name in ("rnms", "soft_rnms"):
        assert _sig_from_obj(getattr(nms_wrapper, name)) == ref["signatures"]["nms_wrapper." + name], name
    for name in ("convex_giou", "convex_iou", "convex_overlaps"):
        assert _sig_from_obj(getattr(iou_wrapper, name)) == ref["signatures"]["iou_wrapper." + name], name
    assert _sig_from_obj(chamfer_distance.ChamferDistance2D) == ref["signatures"]["chamfer_distance.ChamferDistance2D"]
    assert _sig_from_obj(minarea_rect.minaerarect) == ref["signatures"]["minarea_rect.minaerarect"]


def test_deform_conv_and_focal_modules_have_the_reference_signatures(ref):
    dc = importlib.import_module("orientedreppoints_amd.mmdet_ops.deform_conv")
    for cls in ("DeformConv", "ModulatedDeformConv", "DeformConvPack", "ModulatedDeformConvPack"):
        for meth in ("__init__", "forward"):
            assert _sig_from_obj(getattr(getattr(dc, cls), meth), 1) == ref["signatures"]["deform_conv.%s.%s" % (cls, meth)], (cls, meth)
    for cls in ("DeformConvFunction", "ModulatedDeformConvFunction"):
        assert _sig_from_obj(getattr(dc, cls).forward, 1) == ref["signatures"]["deform_conv.%s.forward" % cls], cls
    fl = importlib.import_module("orientedreppoints_amd.mmdet_ops.sigmoid_focal_loss")
    assert _sig_from_obj(fl.SigmoidFocalLossFunction.forward, 1) == ref["signatures"]["sigmoid_focal_loss.SigmoidFocalLossFunction.forward"]
    assert _sig_from_obj(fl.SigmoidFocalLoss.__init__, 1) == ref["signatures"]["sigmoid_focal_loss.SigmoidFocalLoss.__init__"]


def test_cython_and_pybind_entry_points(ref):
    from orientedreppoints_amd.dota_devkit import poly_nms_gpu as png
    from orientedreppoints_amd.mmdet_ops import box_iou_rotated, pointsJf
    assert _sig_from_obj(png.poly_gpu_nms) == ref["pyx"]["poly_gpu_nms"]
    assert _sig_from_obj(png.poly_overlaps) == ref["pyx"]["poly_overlaps"]
    # pybind functions: arity from the C++ declarations
    assert ref["pybind_arity"]["pointsJf"] == len(_sig_from_obj(pointsJf)) == 3
    assert ref["pybind_arity"]["box_iou_rotated"] == len(_sig_from_obj(box_iou_rotated)) == 2


def test_reference_python_imports_through_the_aliases(ref):
    """bbox_nms.py, max_iou_assigner.py and iou_loss.py of the reference import their native operators with
    `from mmdet.ops... import ...` (recorded in the golden): through install_mmdet_aliases() each of those imports binds this
    package's operator (the compiled extensions do not exist here)."""
    saved = {k: v for k, v in sys.modules.items() if k == "mmdet" or k.startswith("mmdet.") or k.startswith("DOTA_devkit")}
    try:
        for k in list(saved):
            del sys.modules[k]
        from orientedreppoints_amd.compat import install_mmdet_aliases
        from orientedreppoints_amd.mmdet_ops import iou_wrapper, nms_wrapper
        install_mmdet_aliases()
        want = {"nms_wrapper": nms_wrapper, "convex_overlaps": iou_wrapper.convex_overlaps, "convex_giou": iou_wrapper.convex_giou}
        imports = ref["operator_imports"]
        assert {f for f, _, _ in imports} == set(IMPORTING_FILES)
        for f, module, name in imports:
            bound = getattr(__import__(module, fromlist=[name]), name)          # what `from <module> import <name>` binds
            assert bound is want[name], (f, module, name)
        assert sys.modules["mmdet.ops.nms"].nms_wrapper.rnms is nms_wrapper.rnms
        import DOTA_devkit.poly_nms_gpu.poly_nms as pn
        assert callable(pn.poly_gpu_nms)
        from mmdet.ops import DeformConv, minaerarect, sigmoid_focal_loss  # noqa: F401
    finally:
        for k in [k for k in sys.modules if k == "mmdet" or k.startswith("mmdet.") or k.startswith("DOTA_devkit")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_box_iou_rotated_cpu_branch_matches_reference_golden(golden_dir):
    """box_iou_rotated.h:20-33 dispatches CPU tensors to box_iou_rotated_cpu: the mirror does too (host-compiled same
    source as the device kernel) and reproduces the reference-generated golden exactly."""
    import numpy as np
    import torch
    from orientedreppoints_amd.mmdet_ops import box_iou_rotated
    g = np.load(os.path.join(golden_dir, "box_iou_rotated.npz"))
    got = box_iou_rotated(torch.from_numpy(g["a"]), torch.from_numpy(g["b"]))
    assert not got.is_cuda and got.shape == g["iou"].shape
    assert np.max(np.abs(got.numpy() - g["iou"])) <= 1e-6
    assert box_iou_rotated(torch.zeros(0, 5), torch.from_numpy(g["b"])).shape == (0, g["b"].shape[0])
