"""GPU (MI355X): every route of the NMS sweep kernel, on inputs whose route is known by construction.

`nms_sweep_kernel` (csrc/orp_nms.hip) has three routes, chosen on the device from the segment's column-block count and from
the number of non-zero mask words the mask kernel filed (`kNzCap` = 8192, `kSmallCb` = 64 blocks):
  small   <= 64 blocks and <= 8192 words: the greedy pass by one wave out of LDS;
  sparse  more blocks, <= 8192 words: the workgroup pass over the bucketed side list;
  dense   more than 8192 words: the block-row pass over the mask in memory.

Construction: axis-aligned 10 x 10 boxes on a 16-pixel grid.  Boxes of different cells never touch, so their IoU is exactly
0 (the fp32 origin-fan arithmetic gives it within 2e-3 at these coordinates); a cell holds m exact
copies with distinct scores, whose IoU (1) is far above the threshold of 0.3.  The keep set is the
best-scored copy of every cell, and mask word (row, 64-column block) is non-zero exactly where the block holds a same-cell
column right of the row -- the tests count those pairs on the host from the visiting order and assert on which side of
8192 the count lies.  Each case goes through `rnms` (ascending-index output), `poly_gpu_nms` (presorted input,
visiting-order output) and the fp64 merge NMS (`py_gpu_nms_poly`, `poly_nms_f64_batched_device`); the dense case through
`py_gpu_nms_poly` is what reaches the dense route with visiting-order output.

Not repeated here, covered elsewhere: the tile maps of the mask kernel.  `test_rnms_vs_oracle` at n = 1000 and 2000 has 16
and 32 column blocks and takes the XCD-aware lists; n = 500 and the batched tests take `decode_diag_last`.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K_NZ_CAP = 8192
THR = 0.3


def _scene(copies, seed):
    """copies[k] boxes in cell k, rows shuffled, distinct scores (exact in fp32).  Returns (dets [n, 9] float64, cell [n])."""
    rng = np.random.RandomState(seed)
    cell = rng.permutation(np.repeat(np.arange(len(copies)), copies))
    n = cell.size
    x0 = 16.0 * (cell % 100 + 1)
    y0 = 16.0 * (cell // 100 + 1)
    d = np.stack([x0, y0, x0 + 10, y0, x0 + 10, y0 + 10, x0, y0 + 10, rng.permutation(n) + 1.0], 1)
    d[:, 8] /= 8192.0
    return d, cell


def _nonzero_mask_words(cell_by_position):
    """(row, 64-column block) pairs whose block holds a same-cell column right of the row."""
    blocks_of = {}
    for pos, c in enumerate(cell_by_position):
        blocks_of.setdefault(int(c), []).append(pos >> 6)           # ascending positions
    count = 0
    for blocks in blocks_of.values():
        for t in range(len(blocks) - 1):
            count += len(set(blocks[t + 1:]))
    return count


CASES = {
    # name: (copies per cell, column blocks, True = more non-zero words than the side list holds)
    "sparse_65_blocks": ([1] * 3860 + [2] * 150, 65, False),
    "dense_65_blocks": ([64] * 65, 65, True),
    "small_64_blocks": ([1] * 3796 + [2] * 150, 64, False),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scenes(oracle):
    """Every case once: boxes, the keep list by construction (visiting order) and the oracle's keep set; the route
    conditions are asserted here, on the host."""
    out = {}
    for i, (name, (copies, blocks, over_cap)) in enumerate(sorted(CASES.items())):
        d, cell = _scene(copies, 20 + i)
        n = d.shape[0]
        assert (n + 63) // 64 == blocks
        order = np.argsort(-d[:, 8], kind="stable")               # scores are distinct: every entry point's visiting order
        words = _nonzero_mask_words(cell[order])
        print("%s: %d boxes, %d cells, %d non-zero mask words" % (name, n, len(copies), words))
        assert (words > K_NZ_CAP) == over_cap, words
        if name != "dense_65_blocks":
            assert words <= 150
        seen, keep = set(), []
        for p in order:                                           # the best-scored copy of every cell
            if cell[p] not in seen:
                seen.add(cell[p])
                keep.append(int(p))
        assert len(keep) == len(copies)
        want = oracle.rnms(d.astype(np.float32), THR)
        assert np.array_equal(np.sort(keep), want)
        out[name] = (d, keep, want)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_rnms_route(dev, scenes, name):
    from orientedreppoints_amd.mmdet_ops import rnms
    d, keep, want = scenes[name]
    _, inds = rnms(torch.from_numpy(d.astype(np.float32)).to(dev), THR)
    got = inds.cpu().numpy()
    assert np.array_equal(got, np.sort(keep))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", sorted(CASES))
def test_poly_gpu_nms_route(dev, scenes, name):
    from orientedreppoints_amd.dota_devkit.poly_nms_gpu import poly_gpu_nms
    d, keep, want = scenes[name]
    got = [int(i) for i in poly_gpu_nms(d.astype(np.float32), THR)]
    assert got == keep
    assert np.array_equal(np.sort(got), want)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp64_merge_route(dev, scenes, name):
    from orientedreppoints_amd.dota_devkit.result_merge import py_gpu_nms_poly
    from orientedreppoints_amd.mmdet_ops.nms_wrapper import poly_nms_f64_batched_device
    d, keep, want = scenes[name]
    got = py_gpu_nms_poly(d, THR)
    assert got == keep
    assert np.array_equal(np.sort(got), want)
    for fast in (False, True):                                     # one segment of the segmented form, sorted on the device
        k, num = poly_nms_f64_batched_device(torch.from_numpy(d).to(dev), torch.tensor([0, d.shape[0]], dtype=torch.int32),
                                             d.shape[0], THR, hbb_prefilter=fast, presorted=False)
        assert [int(i) for i in k[:int(num[0].item())].cpu().numpy()] == keep
