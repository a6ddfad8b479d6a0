"""SceneInference without a GPU: the argument checks (through a stub model), the Task1 writer against a hand-written file,
and the numpy restatements the GPU tests use against `poly2origpoly` and `imnormalize`."""
import numpy as np
import pytest

from test_gpu_scene_inference import collect_oracle, exact_fixture, stub_model, synthetic_packed, tile_oracle, translate_rows


def test_rejects_what_it_cannot_run():
    from orientedreppoints_amd.mmdet_models import SceneInference
    with pytest.raises(ValueError, match="multiple of 32"):
        SceneInference(stub_model(), subsize=1000)
    with pytest.raises(ValueError, match="eval mode"):
        SceneInference(stub_model(training=True))
    with pytest.raises(ValueError, match="static rnms"):
        SceneInference(stub_model(nms_type='soft_rnms'))
    model = stub_model()
    model.test_cfg['static_postprocess'] = False
    with pytest.raises(ValueError, match="static rnms"):
        SceneInference(model)
    si = SceneInference(stub_model(), subsize=1024, gap=200)
    with pytest.raises(ValueError, match="smaller than a 1024 tile"):
        si(np.zeros((1023, 4000, 3), np.uint8))
    with pytest.raises(ValueError, match="smaller than a 1024 tile"):          # large enough at rate 1, too small at 0.5
        SceneInference(stub_model(), rates=(1.0, 0.5))(np.zeros((2000, 2040, 3), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        si(np.zeros((2000, 2000, 3), np.float32))
    assert si.num_classes == 15 and si.rates == [(1.0, 1.0)]


def test_write_task1_format(tmp_path):
    """`name score x1 .. y4`, `str()` of Python floats, appended per class; nothing for an empty class."""
    from orientedreppoints_amd.mmdet_models import SceneInference
    si = SceneInference(stub_model())
    per_class = [np.zeros((0, 9)) for _ in range(15)]
    per_class[0] = np.array([[1.0, 2.5, 3.0, 2.5, 3.0, 4.125, 1.0, 4.125, 0.75],
                             [10.0, 20.0, 30.0, 20.0, 30.0, 40.0, 10.0, 40.0, 0.1]])
    per_class[14] = np.array([[0.1 + 0.2, 1e-5, 1 / 3, 4.0, 5.0, 6.0, 7.0, 16383.875, float(np.float32(0.3))]])
    si.write_task1(str(tmp_path), "P0001", per_class)
    si.write_task1(str(tmp_path), "P0002", per_class[:1] + [np.zeros((0, 9))] * 14)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["Task1_helicopter.txt", "Task1_plane.txt"]
    assert (tmp_path / "Task1_plane.txt").read_text() == (
        "P0001 0.75 1.0 2.5 3.0 2.5 3.0 4.125 1.0 4.125\n"
        "P0001 0.1 10.0 20.0 30.0 20.0 30.0 40.0 10.0 40.0\n"
        "P0002 0.75 1.0 2.5 3.0 2.5 3.0 4.125 1.0 4.125\n"
        "P0002 0.1 10.0 20.0 30.0 20.0 30.0 40.0 10.0 40.0\n")
    assert (tmp_path / "Task1_helicopter.txt").read_text() == (
        "P0001 0.30000001192092896 0.30000000000000004 1e-05 0.3333333333333333 4.0 5.0 6.0 7.0 16383.875\n")


def test_translate_rows_is_poly2origpoly():
    """The restatement the GPU tests compare the collect kernel with: poly2origpoly's expression on the widened fp32 value."""
    from orientedreppoints_amd.dota_devkit.result_merge import poly2origpoly
    rng = np.random.RandomState(0)
    rows = rng.uniform(-50, 1100, size=(6, 27)).astype(np.float32)
    for left, up, rate in ((0, 0, '1'), (824, 1648, '1'), (3296, 824, '0.5'), (17, 5, '1.5')):
        got = translate_rows(rows, left, up, float(rate))
        for r, g in zip(rows, got):
            want = poly2origpoly([float(v) for v in r[18:26]], left, up, rate)
            assert g[:8].tolist() == want and g[8] == float(r[26])


def test_collect_oracle_order_and_overflow():
    """Class-major, tile ascending, row ascending; an overflowed tile's rows are left out and flagged."""
    packed = synthetic_packed(7, 20, 15, 1, overflow_tile=2)
    origins = [(10 * t, 100 * t) for t in range(7)]
    dets, off, src, flag = collect_oracle(packed, origins, 0.5, 15)
    assert flag == 1 and off[0] == 0 and off[-1] == len(dets) == len(src) and off[5] == off[4]
    assert 2 not in src[:, 0] and (np.diff(off) >= 0).all()
    for c in range(15):
        seg = src[off[c]:off[c + 1]]
        assert (packed[seg[:, 0], seg[:, 1], 27] == c).all()
        key = seg[:, 0].astype(np.int64) * 1000 + seg[:, 1]
        assert (np.diff(key) > 0).all()
    t, r = src[3]
    assert dets[3, 0] == (float(packed[t, r, 18]) + origins[t][0]) / 0.5 and dets[3, 8] == float(packed[t, r, 26])
    total = sum(int(packed[t, 20, 0]) for t in range(7) if t != 2)
    assert len(dets) == total


def test_tile_oracle_pads_with_zeros():
    from orientedreppoints_amd.mmdet_datasets.imops import imnormalize
    scene = np.random.RandomState(2).randint(0, 256, size=(40, 50, 3)).astype(np.uint8)
    out = tile_oracle(scene, 30, 20, 32)
    assert out.shape == (3, 32, 32) and out.dtype == np.float32
    assert np.array_equal(out[:, :20, :20], imnormalize(scene[20:, 30:], (123.675, 116.28, 103.53), (58.395, 57.12, 57.375), True).transpose(2, 0, 1))
    assert (out[:, 20:] == 0).all() and (out[:, :, 20:] == 0).all()


@pytest.mark.parametrize("rate", [1, 0.5])
def test_exact_fixture_survives_the_text_round_trip(rate):
    """Multiples of 1/8 below 16 384 and of 1/256 in (0, 1] are what `str(float32)` -> `float` gives back unchanged; multiples
    of 1/512 already are not."""
    packed, origins = exact_fixture(rate)
    m = packed.shape[1] - 1
    live = packed[:, :m, 18:27][packed[:, :m, 26] > 0]
    assert all(float(str(v)) == float(v) for v in live.reshape(-1))
    assert any(float(str(np.float32(k / 512.0))) != float(np.float32(k / 512.0)) for k in range(1, 512, 2))
