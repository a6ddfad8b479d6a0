"""Whole-scene inference on the MI355X: the tile kernel `orp_scene_tiles` against numpy's `imnormalize` (bit for bit), the
collect kernel `orp_scene_collect` against its numpy restatement, `SceneInference` end to end against a composition of what
existed before it (numpy crop -> imnormalize -> simple_test_batch -> translate -> CPU oracle NMS), against the files route
(`result_merge_multi_process.mergebypoly`), with the capacity-overflow fallback, and without host synchronisation in the
tile loop.  Every comparison is exact.  The numpy oracles live in this file."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
NUM_CLASSES = 15


# ---- numpy oracles (no device needed: tests/test_scene_inference.py checks them against poly2origpoly) ----------------------
def tile_oracle(scene, left, up, S, mean=MEAN, std=STD, to_rgb=True):
    """float32 [3, S, S]: imnormalize of the crop, CHW, zero where the tile hangs over the scene (Pad after Normalize)."""
    from orientedreppoints_amd.mmdet_datasets.imops import imnormalize
    out = np.zeros((3, S, S), np.float32)
    crop = scene[up:up + S, left:left + S]
    out[:, :crop.shape[0], :crop.shape[1]] = imnormalize(crop, mean, std, to_rgb).transpose(2, 0, 1)
    return out


def translate_rows(rows, left, up, rate):
    """rows [n, >= 9] float32 whose last nine columns are 8 corners + score -> float64 [n, 9]: x = (float64(x) + left) / rate,
    y = (float64(y) + up) / rate (poly2origpoly on the exactly widened value), score widened."""
    r = np.asarray(rows)[:, -9:].astype(np.float64)
    r[:, 0:8:2] = (r[:, 0:8:2] + float(left)) / float(rate)
    r[:, 1:8:2] = (r[:, 1:8:2] + float(up)) / float(rate)
    return r


def collect_oracle(packed, origins, rate, C):
    """packed [T, m + 1, 28] float32 -> (dets [N, 9] float64, seg_offsets [C + 1], src [N, 2], flag): class-major, inside a
    class tile ascending then packed row ascending; overflowed tiles left out and flagged."""
    m = packed.shape[1] - 1
    per_class = [([], []) for _ in range(C)]
    flag = 0
    for t, (p, (left, up)) in enumerate(zip(packed, origins)):
        if p[m, 1] != 0:
            flag = 1
            continue
        n = int(p[m, 0])
        for c in range(C):
            rows = np.nonzero(p[:n, 27] == c)[0]
            per_class[c][0].append(translate_rows(p[rows, 18:27], left, up, rate))
            per_class[c][1].append(np.stack([np.full(len(rows), t), rows], 1).astype(np.int32).reshape(-1, 2))
    dets = np.concatenate([np.concatenate(d) for d, _ in per_class])
    src = np.concatenate([np.concatenate(s) for _, s in per_class])
    off = np.concatenate([[0], np.cumsum([sum(len(x) for x in d) for d, _ in per_class])]).astype(np.int32)
    return dets, off, src, flag


def synthetic_packed(T, m, C, seed, overflow_tile=None, empty_class=4):
    """Random packed results: counts 0 .. m (every third tile empty), labels over the classes but `empty_class`."""
    rng = np.random.RandomState(seed)
    packed = np.zeros((T, m + 1, 28), np.float32)
    labels = np.array([c for c in range(C) if c != empty_class])
    for t in range(T):
        n = 0 if t % 3 == 1 else int(rng.randint(1, m + 1))
        packed[t, :n, :26] = rng.uniform(0, 1024, size=(n, 26)).astype(np.float32)
        packed[t, :n, 26] = rng.uniform(0.05, 1, size=n).astype(np.float32)
        packed[t, :n, 27] = rng.choice(labels, size=n)
        packed[t, m, 0] = n
    if overflow_tile is not None:
        packed[overflow_tile, m, 1] = 1.0
    return packed


def oracle_merge(dets, thr=0.1):
    """Rows of dets [n, 9] float64 kept by the CPU oracle's py_cpu_nms_poly_fast in stable score-descending order."""
    from oracle import orp_oracle as O
    d = np.ascontiguousarray(dets, np.float64)
    if len(d) == 0:
        return d.reshape(0, 9), []
    order = np.ascontiguousarray(np.argsort(-d[:, 8], kind="stable"), np.int64)
    keep = np.empty(len(d), np.int64)
    n = O.lib().orc_py_cpu_nms_poly_fast(O._p(d), len(d), O._p(order), ctypes.c_double(thr), O._p(keep))
    return d[keep[:n]], [int(i) for i in keep[:n]]


def stub_model(num_classes=NUM_CLASSES + 1, training=False, nms_type='rnms'):
    """What SceneInference reads of a model before it touches the device."""
    from orientedreppoints_amd.mmdet_models import ConfigDict
    return types.SimpleNamespace(training=training, bbox_head=types.SimpleNamespace(num_classes=num_classes),
                                 test_cfg=ConfigDict(dict(nms=dict(type=nms_type, iou_thr=0.4), score_thr=0.05, max_per_img=2000)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- (a) tiles, bit-exact --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("S", [64, 256, 1024])
def test_scene_tiles_bit_exact(dev, S):
    """fp32 output array_equal to imnormalize of the crop; fp16 / bf16 output equal to torch's cast of that; to_rgb on and off;
    origins of split_origins plus odd lefts and origins hanging over the right and bottom edges (zeros there); a contiguous
    scene, one of odd width, and a strided view at an odd byte offset."""
    from orientedreppoints_amd.dota_devkit.img_split import split_origins
    from orientedreppoints_amd.mmdet_ops.scene_ops import scene_tiles
    rng = np.random.RandomState(S)
    big = rng.randint(0, 256, size=(1100, 1500 + 7, 3)).astype(np.uint8)
    big_dev = torch.from_numpy(big).to(dev)
    cases = [(big[:, :1500].copy(), None), (rng.randint(0, 256, size=(1031, 1277, 3)).astype(np.uint8), None),
             (big[:, 5:5 + 1500], big_dev[:, 5:5 + 1500])]
    for scene, view in cases:
        H, W = scene.shape[:2]
        origins = split_origins(W, H, S, S // 4)
        origins = origins[:3] + origins[-3:] + [(1, 0), (3, 5), (1023, 7), (W - S // 2 - 1, H - S // 3), (W - 1, H - 1), (W - 3, 1)]
        scene_dev = torch.from_numpy(np.ascontiguousarray(scene)).to(dev) if view is None else view
        assert view is None or not view.is_contiguous()
        o_dev = torch.tensor(origins, dtype=torch.int32).to(dev)
        for to_rgb in (True, False):
            want = np.stack([tile_oracle(scene, l, u, S, to_rgb=to_rgb) for l, u in origins])
            assert (want[9][:, :, -1] == 0).all() and (want[9][:, -1, :] == 0).all()           # (origin 9 does hang over both edges)
            for dtype in (torch.float32, torch.float16, torch.bfloat16):
                out = torch.full((len(origins), 3, S, S), 7.0, dtype=dtype, device=dev)
                scene_tiles(scene_dev, o_dev, out, MEAN, STD, to_rgb)
                got = out.cpu()
                expect = torch.from_numpy(want).to(dtype)
                assert torch.equal(got, expect), (S, W, to_rgb, dtype)
                if dtype == torch.float32:
                    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))     # bits, signed zeros included


@pytest.mark.gpu
def test_scene_tiles_other_mean_std(dev):
    """A second normalisation (no round numbers, a mean above 255): still numpy's bits."""
    from orientedreppoints_amd.mmdet_ops.scene_ops import scene_tiles
    rng = np.random.RandomState(3)
    scene = rng.randint(0, 256, size=(300, 333, 3)).astype(np.uint8)
    mean, std = (0.1, 300.7, 127.5), (0.3, 255.0, 1.7)
    origins = [(0, 0), (13, 11), (333 - 64, 300 - 64)]
    out = torch.empty((3, 3, 64, 64), dtype=torch.float32, device=dev)
    scene_tiles(torch.from_numpy(scene).to(dev), torch.tensor(origins, dtype=torch.int32).to(dev), out, mean, std, True)
    want = np.stack([tile_oracle(scene, l, u, 64, mean, std, True) for l, u in origins])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- (b) collect, exact ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("T,overflow_tile", [(1, None), (7, 2), (40, 17)])
@pytest.mark.parametrize("rate", [1.0, 0.5])
def test_scene_collect_exact(dev, T, overflow_tile, rate):
    """dets, seg_offsets, src and the flag array_equal to the numpy restatement: empty tiles, a tile with its overflow flag
    set, a class with no rows; more rows per tile than one block pass (m = 300 > 256 threads)."""
    from orientedreppoints_amd.mmdet_ops.scene_ops import scene_collect
    m, C = 300, NUM_CLASSES
    packed = synthetic_packed(T, m, C, 100 + T, overflow_tile)
    origins = [(int(824 * (t // 5)), int(824 * (t % 5))) for t in range(T)]
    dets, table, src = scene_collect(torch.from_numpy(packed).to(dev), torch.tensor(origins, dtype=torch.int32).to(dev), rate, C)
    table = table.cpu().numpy()
    w_dets, w_off, w_src, w_flag = collect_oracle(packed, origins, rate, C)
    n = int(w_off[-1])
    assert n > 0 and w_off[5] == w_off[4]                                           # class 4 is empty
    assert np.array_equal(table[:C + 1], w_off)
    assert int(table[C + 1] != 0) == w_flag == int(overflow_tile is not None)
    assert np.array_equal(dets[:n].cpu().numpy(), w_dets)
    assert np.array_equal(src[:n].cpu().numpy(), w_src)


# ---- (c), (e), (f): a detector made to detect ------------------------------------------------------------------------------
SUB, GAP = 256, 64


def _scene(seed=5, H=600, W=700):
    """Noise with structure: 8 x 8 blocks of random colour plus fine noise (uint8 BGR)."""
    rng = np.random.RandomState(seed)
    blocks = np.kron(rng.randint(0, 256, size=((H + 7) // 8, (W + 7) // 8, 3)), np.ones((8, 8, 1)))[:H, :W]
    return np.clip(blocks + rng.normal(0, 12, size=(H, W, 3)), 0, 255).astype(np.uint8)


def _calibrate_head(model, img, target):
    """The head-bias calibration of bench.py:calibrate_head, restated: a 3 x 3 point grid as the init bias, raised weight
    spread, and a per-class classification bias that lets ~target / C (point, class) pairs of `img` pass score_thr."""
    head = model.bbox_head
    with torch.no_grad():
        base = torch.tensor([[-1, -1], [-1, 0], [-1, 1], [0, -1], [0, 0], [0, 1], [1, -1], [1, 0], [1, 1]],
                            dtype=torch.float32, device=img.device).reshape(-1) * 2.0
        head.reppoints_pts_init_out.bias.copy_(base)
        head.reppoints_pts_init_out.weight.normal_(0, 0.05)
        head.reppoints_pts_refine_out.weight.normal_(0, 0.05)
        head.reppoints_cls_out.weight.normal_(0, 0.05)
        cls_outs = head(model.extract_feat(img))[0]
        C = cls_outs[0].size(1)
        logits = torch.cat([c.permute(1, 0, 2, 3).reshape(C, -1) for c in cls_outs], 1)
        thr = model.test_cfg.score_thr
        thr_logit = float(np.log(thr / (1 - thr)))
        for c in range(C):
            k = max(1, min(target // C + (1 if c < target % C else 0), logits.size(1) - 1))
            head.reppoints_cls_out.bias[c] += thr_logit - torch.topk(logits[c], k).values[-1] + 1e-4


@pytest.fixture(scope="module")
def detector(dev):
    """(model, scene): R-50 FPN detector, random weights, calibrated on the scene's first tile; the library's convolutions in
    their reproducible mode for the module (two eager runs of these tiny maps can differ otherwise)."""
    from orientedreppoints_amd.dota_configs import r50_model, test_cfg
    from orientedreppoints_amd.mmdet_models import ConfigDict, build_detector
    det_flag = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    torch.manual_seed(0)
    model = build_detector(ConfigDict(r50_model), train_cfg=None, test_cfg=ConfigDict(dict(test_cfg))).to(dev).eval()
    scene = _scene()
    _calibrate_head(model, torch.from_numpy(tile_oracle(scene, 0, 0, SUB)[None]).to(dev), 300)
    yield model, scene
    torch.backends.cudnn.deterministic = det_flag


def _expected(model, scene, batch, dev, scaled=()):
    """Composed from what existed before SceneInference; scaled = [(resampled scene, rate)] of further rates, in rate order.
    Returns (per-class kept rows, per-class all rows, per-class tile number of each row)."""
    from orientedreppoints_amd.dota_devkit.img_split import split_origins
    metas = [dict(img_shape=(SUB, SUB, 3), pad_shape=(SUB, SUB, 3), scale_factor=1.0, flip=False) for _ in range(batch)]
    rows = [[] for _ in range(NUM_CLASSES)]
    tiles = [[] for _ in range(NUM_CLASSES)]
    first = 0
    for sc, rate in [(scene, 1.0)] + list(scaled):
        origins = split_origins(sc.shape[1], sc.shape[0], SUB, GAP)
        for i in range(0, len(origins), batch):
            group = origins[i:i + batch]
            padded = group + [group[-1]] * (batch - len(group))
            img = torch.from_numpy(np.stack([tile_oracle(sc, l, u, SUB) for l, u in padded])).to(dev)
            with torch.no_grad():
                results = model.simple_test_batch(img, metas)
            for j, (left, up) in enumerate(group):
                for c in range(NUM_CLASSES):
                    rows[c].append(translate_rows(results[j][c], left, up, rate))
                    tiles[c].append(np.full(len(results[j][c]), first + i + j))
        first += len(origins)
    rows = [np.concatenate(r) for r in rows]
    tiles = [np.concatenate(t) for t in tiles]
    return [oracle_merge(r)[0] for r in rows], rows, tiles


@pytest.mark.gpu
@pytest.mark.parametrize("batch,depth", [(1, 1), (1, 3), (2, 1), (2, 3)])
def test_scene_inference_end_to_end_exact(dev, detector, batch, depth):
    """SceneInference's per-class arrays array_equal to numpy crop -> imnormalize -> simple_test_batch (same tile batches, same
    order) -> (float64(c) + origin) / rate -> CPU oracle py_cpu_nms_poly_fast in stable score-descending order.  The scene
    yields detections in at least two classes and at least one suppression across a tile border."""
    from orientedreppoints_amd.mmdet_models import SceneInference
    model, scene = detector
    want, rows, tiles = _expected(model, scene, batch, dev)
    assert sum(len(w) > 0 for w in want) >= 2, "the scene must produce detections in at least two classes"
    crossed = 0
    for r, t in zip(rows, tiles):
        kept_all = set(oracle_merge(r)[1])
        for tile in np.unique(t):
            own = np.nonzero(t == tile)[0]
            # kept when only its own tile is merged, dropped in the scene's merge: some suppression crossed a tile border
            crossed += sum(1 for k in oracle_merge(r[own])[1] if int(own[k]) not in kept_all)
    assert crossed >= 1, "the scene must produce at least one suppression across a tile border"
    si = SceneInference(model, subsize=SUB, gap=GAP, batch=batch, depth=depth)
    for source in (scene, torch.from_numpy(scene).to(dev)):              # a host array and a device tensor; the second call reuses the graphs
        got = si(source)
        assert len(got) == NUM_CLASSES
        for c in range(NUM_CLASSES):
            assert got[c].dtype == np.float64 and got[c].shape == want[c].shape, (c, got[c].shape, want[c].shape)
            assert np.array_equal(got[c], want[c]), c
    assert si.fallback_tiles == 0


@pytest.mark.gpu
def test_scene_inference_two_rates_exact(dev, detector):
    """rates = (1.0, 0.5): the scene resampled once on the device (torch's bicubic; the resampled pixels are taken from the
    device, they are plumbing and not checked against cv2), each rate tiled on its own, coordinates divided by the rate,
    classes concatenated in rate order, one merge.  Composed expectation as above, array_equal."""
    from orientedreppoints_amd.dota_devkit.img_split import scaled_size
    from orientedreppoints_amd.mmdet_models import SceneInference
    model, scene = detector
    w, h = scaled_size(scene.shape[1], scene.shape[0], 0.5)
    half = SceneInference._resample(torch.from_numpy(scene).to(dev), w, h).cpu().numpy()
    assert half.shape == (h, w, 3) and half.dtype == np.uint8 and half.std() > 10
    want, rows, _ = _expected(model, scene, 2, dev, scaled=[(half, 0.5)])
    only_full = _expected(model, scene, 2, dev)[1]
    assert sum(len(r) for r in rows) > sum(len(r) for r in only_full)            # the half-size scene detects too
    got = SceneInference(model, subsize=SUB, gap=GAP, rates=(1.0, 0.5), batch=2, depth=2)(scene)
    assert sum(len(w_) for w_ in want) > 0
    for c in range(NUM_CLASSES):
        assert np.array_equal(got[c], want[c]), c


@pytest.mark.gpu
def test_scene_inference_overflow_fallback(dev, detector):
    """static_capacity low enough that tiles overflow: the result is array_equal to the run with ample capacity."""
    from orientedreppoints_amd.mmdet_models import SceneInference
    model, scene = detector
    want = SceneInference(model, subsize=SUB, gap=GAP, batch=2, depth=2)(scene)
    model.test_cfg['static_capacity'] = 64
    try:
        si = SceneInference(model, subsize=SUB, gap=GAP, batch=2, depth=2)
        got = si(scene)
    finally:
        model.test_cfg['static_capacity'] = 8192
    assert si.fallback_tiles >= 1, "no tile overflowed: the capacity is not low enough for this scene"
    assert sum(len(w) for w in want) > 0
    for c in range(NUM_CLASSES):
        assert np.array_equal(got[c], want[c]), c


@pytest.mark.gpu
def test_scene_inference_tile_loop_does_not_synchronise(dev, detector):
    """With torch's sync debug mode on "error" around the tile loop (not around the upload, the capture or the final fetch) a
    scene of 12 tiles runs without raising, and the mode does fire on this build when something synchronises."""
    from orientedreppoints_amd.mmdet_models import SceneInference
    model, scene = detector
    si = SceneInference(model, subsize=SUB, gap=GAP, batch=1, depth=3)
    want = si(scene)
    plan = si.prepare(torch.from_numpy(scene).to(dev))
    assert len(plan.origins[0]) >= 6
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        si.run_tiles(plan)
        with pytest.raises(RuntimeError):                        # (the mode is live: a D2H copy of a device tensor raises)
            plan.packed[0][0, 0, 0].item()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    got = si.merge(plan)
    for c in range(NUM_CLASSES):
        assert np.array_equal(got[c], want[c])


# ---- (d) agreement with the files route ------------------------------------------------------------------------------------
def exact_fixture(rate, seed=11, T_side=(3, 2), per_tile=14, m=40):
    """Synthetic per-tile results whose text round trip is exact: coordinates multiples of 1/8 below 16 384, scores distinct
    multiples of 1/256 inside every class.  Returns (packed [T, m + 1, 28] float32, origins).  Boxes are rectangles of
    60 .. 200 px spread over 1024 px tiles that overlap by 200 px, so neighbours (and tiles) suppress each other."""
    rng = np.random.RandomState(seed)
    origins = [(824 * i, 824 * j) for i in range(T_side[0]) for j in range(T_side[1])]
    T, C = len(origins), NUM_CLASSES
    packed = np.zeros((T, m + 1, 28), np.float32)
    scores = {c: list(rng.permutation(np.arange(13, 257))) for c in (0, 6, 9)}       # three classes, <= 244 rows each
    for t in range(T):
        for r in range(per_tile):
            c = (0, 6, 9)[int(rng.randint(3))]
            cx, cy = rng.randint(0, 1024 * 8, size=2) / 8.0
            w, h = rng.randint(60 * 8, 200 * 8, size=2) / 8.0
            packed[t, r, 18:26] = [cx, cy, cx + w, cy, cx + w, cy + h, cx, cy + h]
            packed[t, r, 26] = scores[c].pop() / 256.0
            packed[t, r, 27] = c
        packed[t, m, 0] = per_tile
    return packed, origins


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [1, 0.5])
def test_scene_merge_agrees_with_files_route(dev, tmp_path, rate):
    """Patch files written the way parse_pkl_mege_results_for_dota_evaluation.py writes them (`str()` of every field, names
    from patch_name) -> the existing mergebypoly; byte for byte the files write_task1 writes from collect + merge on the same
    rows.  The fixture's values survive the text round trip (asserted), so exact widening and the files agree."""
    from orientedreppoints_amd.dota_devkit.img_split import patch_name
    from orientedreppoints_amd.dota_devkit.result_merge_multi_process import mergebypoly
    from orientedreppoints_amd.mmdet_models.scene_inference import DOTA_CLASSES, SceneInference, _Plan
    packed, origins = exact_fixture(rate)
    m = packed.shape[1] - 1
    live = packed[:, :m, 18:27][packed[:, :m, 26] > 0]
    assert len(live) > 50 and all(float(str(v)) == float(v) for v in live.reshape(-1))       # v: np.float32
    for c in range(NUM_CLASSES):
        s = packed[:, :m, 26][(packed[:, :m, 27] == c) & (packed[:, :m, 26] > 0)]
        assert len(s) <= 256 and len(set(s.tolist())) == len(s)                               # distinct scores per class
    src, dst, ours = tmp_path / "raw", tmp_path / "merged", tmp_path / "ours"
    src.mkdir(), dst.mkdir()
    for t, (left, up) in enumerate(origins):
        name = patch_name("P0001", rate, left, up)
        for r in range(int(packed[t, m, 0])):
            bbox, cls = packed[t, r, :27], DOTA_CLASSES[int(packed[t, r, 27])]
            confidence = float(bbox[-1])
            with open(src / ("Task1_" + cls + ".txt"), "a+") as f:
                f.write(name + ' ' + str(confidence) + ' ' + ' '.join(str(bbox[k]) for k in range(-9, -1)) + '\n')
    mergebypoly(str(src), str(dst))
    si = SceneInference(stub_model(), subsize=1024, gap=200, rates=(rate,))
    plan = _Plan()
    plan.rates, plan.origins = [float(str(rate))], [origins]
    plan.origins_dev = [torch.tensor(origins, dtype=torch.int32).to(dev)]
    plan.packed = [torch.from_numpy(packed).to(dev)]
    per_class = si.merge(plan)
    si.write_task1(str(ours), "P0001", per_class)
    names = sorted(os.listdir(dst))
    assert names == sorted(os.listdir(ours)) and len(names) == 3
    suppressed = 0
    for n in names:
        a, b = open(dst / n, "rb").read(), open(ours / n, "rb").read()
        assert a == b, n
        suppressed += len(open(src / n).readlines()) - len(a.splitlines())
    assert suppressed > 0                                                                     # the merge had work to do
