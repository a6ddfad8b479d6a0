"""The fast merge of the DOTA evaluation workflow (dota_devkit/result_merge_multi_process.py, mirror of
DOTA_devkit/ResultMerge_multi_process.py) against files produced by the reference's own `mergebase` with
`py_cpu_nms_poly_fast` at nms_thresh = 0.1 (tests/golden/make_golden_merge_mp.py)."""
import filecmp
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RAW = os.path.join(HERE, "golden", "merge", "raw")
MERGED = os.path.join(HERE, "golden", "merge_mp", "merged")


def _same_files(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names
    for n in names:
        assert filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False), n


def test_mergebase_host_logic_with_oracle_fast_nms(tmp_path):
    """patch-name grammar, coordinate mapping, grouping, nms_thresh = 0.1, output format: byte-identical files when the
    NMS is the CPU oracle's py_cpu_nms_poly_fast (no GPU involved)."""
    from orientedreppoints_amd.dota_devkit import result_merge_multi_process as RMP
    from oracle import orp_oracle as O
    assert RMP.nms_thresh == 0.1
    RMP.mergebase(RAW, str(tmp_path), lambda dets, thr: O.py_cpu_nms_poly_fast(dets, thr))
    _same_files(str(tmp_path), MERGED)


def test_goldens_differ_from_the_full_merge():
    """The fast merge at 0.1 is not the ResultMerge.py merge at 0.3: the two golden sets must differ (else the test above
    would not tell the two mirrors apart)."""
    other = os.path.join(HERE, "golden", "merge", "merged")
    assert any(not filecmp.cmp(os.path.join(MERGED, n), os.path.join(other, n), shallow=False) for n in os.listdir(MERGED))


def test_batched_merge_nms_limits_are_errors():
    """orp_poly_nms_f64_batched refuses what it cannot do before touching the device: a segment bound above
    ORP_NMS_MAX_BOXES is ORP_ETOOBIG (never truncated), unknown modes are ORP_EINVAL.  The buffers are real and valid
    (device tensors where a GPU is present, host arrays otherwise), so no ordering of the checks can make this call
    address memory it does not own."""
    import ctypes
    import torch
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    nseg_max = 65536
    seg = np.minimum(np.arange(nseg_max + 1) * 10, 10).astype(np.int32)      # [0, 10, 10, ...]: one segment of 10 rows
    host = dict(dets=np.zeros((10, 9)), seg=seg, keep=np.zeros(10, np.int64), num=np.zeros(nseg_max, np.int32),
                ws=np.zeros(1 << 20, np.uint8))
    if torch.cuda.is_available():
        bufs = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        ptr = {k: ctypes.c_void_p(t.data_ptr()) for k, t in bufs.items()}
    else:
        bufs = host
        ptr = {k: v.ctypes.data_as(ctypes.c_void_p) for k, v in host.items()}

    def call(max_seg, fast=1, presorted=0, nseg=1):
        return L.orp_poly_nms_f64_batched(ptr["dets"], 10, ptr["seg"], nseg, max_seg, 0.1, fast, presorted, ptr["keep"],
                                          ptr["num"], ptr["ws"], 1 << 20, None)
    assert call(_lib.ORP_NMS_MAX_BOXES + 1) == _lib.ORP_ETOOBIG
    assert call(10, nseg=65536) == _lib.ORP_ETOOBIG
    assert call(10, fast=2) == _lib.ORP_EINVAL
    assert call(10, presorted=-1) == _lib.ORP_EINVAL
    assert call(-1) == _lib.ORP_EINVAL
    from orientedreppoints_amd.mmdet_ops.nms_wrapper import poly_nms_f64_batched_device
    with pytest.raises(TypeError):
        poly_nms_f64_batched_device(np.zeros((3, 9)), np.array([0, 3]), 3, 0.1)


@pytest.mark.gpu
def test_mergebypoly_gpu_matches_reference_files(tmp_path):
    """mergebypoly with every image of a class file in ONE orp_poly_nms_f64_batched launch sequence on the MI355X:
    byte-identical to the reference's merged files."""
    import torch
    assert torch.cuda.is_available()
    from orientedreppoints_amd.dota_devkit import result_merge_multi_process as RMP
    RMP.mergebypoly(RAW, str(tmp_path))
    _same_files(str(tmp_path), MERGED)


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,thr", [(1, 0, 0.1), (64, 1, 0.1), (65, 2, 0.3), (700, 3, 0.1), (3000, 4, 0.1)])
def test_py_gpu_nms_poly_fast_vs_oracle(n, seed, thr):
    """Single segment, numpy's argsort()[::-1] order taken on the host (presorted): the oracle's keep list exactly."""
    from orientedreppoints_amd import synthetic as S
    from orientedreppoints_amd.dota_devkit.result_merge_multi_process import py_gpu_nms_poly_fast
    from oracle import orp_oracle as O
    d = S.gen_polys(n, seed, clustered=True)
    d[:, 8] = np.round(d[:, 8], 2)                      # score ties, as in 3-decimal result files
    if n > 100:
        d[5] = d[4]; d[7, :8] = 0.0; d[9, :8] = d[9, 0]  # exact duplicate, all-zero box, single-point box
    assert py_gpu_nms_poly_fast(d, thr) == [int(i) for i in O.py_cpu_nms_poly_fast(d, thr)]
