"""Whole-scene merge on the MI355X: the segmented fp64 merge NMS `orp_poly_nms_f64_batched` (every (class, scene)
segment in one launch sequence) against the CPU oracle's py_cpu_nms_poly_fast / py_cpu_nms_poly given the same visiting
order, and against the existing single-segment `orp_poly_nms_f64`."""
import ctypes

import numpy as np
import pytest
import torch

SIZES = [0, 1, 63, 64, 65, 3000, 9000]                 # > 8192: more than 128 column blocks, the general sweep path


def _oracle_keep(d, thr, fast, order):
    """Kept original indices of the oracle's greedy loop over `order` (fast: HBB pre-filter, else full polyiou)."""
    from oracle import orp_oracle as O
    d = np.ascontiguousarray(d, np.float64)
    order = np.ascontiguousarray(order, np.int64)
    keep = np.empty(max(d.shape[0], 1), np.int64)
    fn = O.lib().orc_py_cpu_nms_poly_fast if fast else O.lib().orc_py_cpu_nms_poly
    n = fn(O._p(d), d.shape[0], O._p(order), ctypes.c_double(thr), O._p(keep))
    return [int(i) for i in keep[:n]]


def _stable_desc(scores):
    """The documented tie rule of presorted = 0: score descending, then index ascending."""
    return np.argsort(-np.asarray(scores, np.float64), kind="stable")


def _segment(n, seed):
    """n scene detections [n, 9] fp64: clustered polygons spread over ~4000 px (mostly far apart, dense hubs), scores
    rounded to 2 decimals (ties), plus exact duplicates, zero-area and single-point boxes and two boxes whose horizontal
    boxes touch (w == 0)."""
    from orientedreppoints_amd import synthetic as S
    d = S.gen_polys(n, seed, clustered=True)
    d[:, :8] *= 4.0
    d[:, 8] = np.round(d[:, 8], 2)
    if n >= 20:
        d[5] = d[4]
        d[7, :8] = 0.0
        d[9, :8] = d[9, 0]
        d[11, :8] = [100.0, 100.0, 110.0, 100.0, 110.0, 120.0, 100.0, 120.0]
        d[12, :8] = [110.0, 100.0, 125.0, 100.0, 125.0, 120.0, 110.0, 120.0]
        d[13, 8] = d[14, 8]
    return d


def _run(segs, thr, fast, presorted, dev):
    from orientedreppoints_amd.mmdet_ops.nms_wrapper import poly_nms_f64_batched_device
    cat = np.concatenate([s.reshape(-1, 9) for s in segs]) if segs else np.zeros((0, 9))
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int32)
    keep, num = poly_nms_f64_batched_device(torch.from_numpy(cat).to(dev), torch.from_numpy(off).to(dev),
                                            max([len(s) for s in segs] + [1]), thr, hbb_prefilter=fast, presorted=presorted)
    keep, num = keep.cpu().numpy(), num.cpu().numpy()
    return [[int(i) - int(off[s]) for i in keep[off[s]:off[s] + num[s]]] for s in range(len(segs))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("fast,thr", [(True, 0.1), (True, 0.3), (False, 0.3), (True, -0.05)])
def test_batched_merge_nms_vs_oracle(dev, fast, thr):
    """Segments of 0 .. 9000 boxes in one call: every segment's keep list (original indices, visiting order) equals the
    oracle's with the documented (score desc, index asc) order.  thr < 0 is evaluated pair by pair (every HBB-disjoint
    pair suppresses then)."""
    segs = [_segment(n, 10 + i) for i, n in enumerate(SIZES)]
    got = _run(segs, thr, fast, False, dev)
    for s, d in enumerate(segs):
        want = _oracle_keep(d, thr, fast, _stable_desc(d[:, 8])) if len(d) else []
        assert got[s] == want, "segment %d (%d boxes)" % (s, len(d))


@pytest.mark.gpu
def test_batched_merge_nms_presorted_is_numpy_order(dev):
    """presorted = 1 with numpy's argsort()[::-1] per segment: O.py_cpu_nms_poly_fast's keep lists exactly (ties as
    numpy breaks them)."""
    from oracle import orp_oracle as O
    segs = [_segment(n, 30 + i) for i, n in enumerate(SIZES)]
    orders = [d[:, 8].argsort()[::-1] for d in segs]
    got = _run([d[o] for d, o in zip(segs, orders)], 0.1, True, True, dev)
    for d, o, g in zip(segs, orders, got):
        want = [int(i) for i in O.py_cpu_nms_poly_fast(d, 0.1)] if len(d) else []
        assert [int(o[i]) for i in g] == want


@pytest.mark.gpu
def test_batched_full_merge_matches_orp_poly_nms_f64(dev):
    """hbb_prefilter = 0 makes the same decisions as the single-segment orp_poly_nms_f64 (py_gpu_nms_poly), which is one
    presorted segment of the same launch sequence: both are held to the CPU oracle's py_cpu_nms_poly."""
    from oracle import orp_oracle as O
    from orientedreppoints_amd.dota_devkit.result_merge import py_gpu_nms_poly
    segs = [_segment(n, 50 + i) for i, n in enumerate([1, 65, 3000])]
    orders = [d[:, 8].argsort()[::-1] for d in segs]
    got = _run([d[o] for d, o in zip(segs, orders)], 0.3, False, True, dev)
    for d, o, g in zip(segs, orders, got):
        single = py_gpu_nms_poly(d, 0.3)
        assert [int(i) for i in O.py_cpu_nms_poly(d, 0.3)] == single
        assert [int(o[i]) for i in g] == single


@pytest.mark.gpu
def test_batched_merge_nms_scene_of_15_classes(dev):
    """A 4000^2 scene as 15 class segments of ~3000 detections (the dense load of 25 tiles): one call, every segment the
    oracle's; a second call gives the same lists."""
    rng = np.random.RandomState(7)
    segs = [_segment(int(rng.randint(1500, 4500)), 70 + c) for c in range(15)]
    got = _run(segs, 0.1, True, False, dev)
    for d, g in zip(segs, got):
        assert g == _oracle_keep(d, 0.1, True, _stable_desc(d[:, 8]))
    assert _run(segs, 0.1, True, False, dev) == got


@pytest.mark.gpu
def test_batched_merge_nms_broken_table_gives_empty_segments(dev):
    """A segment table that breaks the contract (decreasing, past n_total, a segment longer than max_seg) is turned into
    all-empty segments on the device instead of being followed."""
    from orientedreppoints_amd.mmdet_ops.nms_wrapper import poly_nms_f64_batched_device
    d = torch.from_numpy(_segment(100, 3)).to(dev)
    for off, max_seg in (([0, 60, 40, 100], 60), ([0, 50, 101], 51), ([0, 100], 50), ([-1, 100], 101)):
        keep, num = poly_nms_f64_batched_device(d, torch.tensor(off, dtype=torch.int32), max_seg, 0.1)
        assert num.cpu().tolist() == [0] * (len(off) - 1), off
    keep, num = poly_nms_f64_batched_device(d, torch.tensor([0, 40, 100], dtype=torch.int32), 60, 0.1)
    assert num.cpu().numpy().min() > 0                        # the same call with a valid table keeps boxes


@pytest.mark.gpu
def test_batched_merge_nms_signed_zero_scores_tie(dev):
    """-0.0 and +0.0 are one score: the tie goes to the lower index (presorted = 0)."""
    d = np.tile(np.array([[0.0, 0.0, 10.0, 0.0, 10.0, 10.0, 0.0, 10.0, 0.0]]), (3, 1))
    d[0, 8], d[1, 8], d[2, 8] = -0.0, 0.0, -0.0
    for fast in (True, False):
        assert _run([d], 0.1, fast, False, dev) == [[0]]
        assert _oracle_keep(d, 0.1, fast, _stable_desc(d[:, 8])) == [0]
