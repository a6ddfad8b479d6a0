"""The split grammar of whole-scene inference (dota_devkit/img_split.py) against a line-by-line restatement of
DOTA_devkit/SplitOnlyImage.py's SplitSingle loop (no GPU)."""
import re

import pytest


def _split_single(weight, height, subsize, gap):
    """SplitOnlyImage.py:40-57, the loop as written there, collecting (left, up) instead of writing files."""
    slide = subsize - gap
    out = []
    left, up = 0, 0
    while (left < weight):
        if (left + subsize >= weight):
            left = max(weight - subsize, 0)
        up = 0
        while (up < height):
            if (up + subsize >= height):
                up = max(height - subsize, 0)
            out.append((left, up))
            if (up + subsize >= height):
                break
            else:
                up = up + slide
        if (left + subsize >= weight):
            break
        else:
            left = left + slide
    return out


@pytest.mark.parametrize("subsize,gap", [(1024, 200), (1024, 500), (512, 200), (1024, 0), (1024, 924)])
def test_split_origins_matches_split_single(subsize, gap):
    from orientedreppoints_amd.dota_devkit.img_split import split_origins
    S = subsize
    extents = [1, S - 1, S, S + 1, 2 * S - gap, 2 * S - gap + 1, 4000, 20000]
    for w in extents:
        for h in extents:
            assert split_origins(w, h, subsize, gap) == _split_single(w, h, subsize, gap), (w, h)


def test_split_origins_counts_and_cover():
    from orientedreppoints_amd.dota_devkit.img_split import split_origins
    o = split_origins(4000, 4000, 1024, 200)
    assert len(o) == 25 and o[0] == (0, 0) and o[-1] == (2976, 2976)
    assert o[:5] == [(0, 0), (0, 824), (0, 1648), (0, 2472), (0, 2976)]       # inner loop over up
    assert split_origins(0, 100) == [] and split_origins(700, 300) == [(0, 0)]


@pytest.mark.parametrize("subsize,gap", [(1024, 1024), (1024, 2000), (512, 512)])
def test_split_origins_rejects_gap_not_below_subsize(subsize, gap):
    from orientedreppoints_amd.dota_devkit.img_split import split_origins
    with pytest.raises(ValueError):
        split_origins(4000, 4000, subsize, gap)


def test_scaled_size_is_cv2_dsize():
    from orientedreppoints_amd.dota_devkit.img_split import scaled_size
    assert scaled_size(4000, 3000, 1.0) == (4000, 3000)
    assert scaled_size(4000, 3000, 0.5) == (2000, 1500)
    assert scaled_size(4000, 3001, 1.5) == (6000, 4502)              # 4501.5 -> 4502 (ties to even)
    assert scaled_size(1001, 1003, 0.5) == (500, 502)                # 500.5 -> 500, 501.5 -> 502
    assert scaled_size(333, 777, 1.5) == (500, 1166)                 # 499.5 -> 500, 1165.5 -> 1166


@pytest.mark.parametrize("rate", [1.0, 0.5, 1.5, 1])
def test_patch_name_round_trips_through_result_merge(rate):
    from orientedreppoints_amd.dota_devkit import result_merge as RM, result_merge_multi_process as RMP
    from orientedreppoints_amd.dota_devkit.img_split import patch_name, split_origins
    for left, up in split_origins(4000, 2500, 1024, 500):
        name = patch_name("P0001", rate, left, up)
        assert name == "P0001__%s__%d___%d" % (rate, left, up)
        for pat_xy, pat_rate in ((RM._PAT_XY, RM._PAT_RATE), (RMP._PAT_XY, RMP._PAT_RATE)):
            assert name.split('__')[0] == "P0001"
            x, y = (int(v) for v in re.findall(r'\d+', re.findall(pat_xy, name)[0]))
            assert (x, y) == (left, up)
            assert float(re.findall(pat_rate, name)[0]) == float(rate)
        # the mapping back to scene coordinates the merge applies
        assert RM.poly2origpoly([1.0, 2.0], left, up, str(rate)) == [(1.0 + left) / float(rate), (2.0 + up) / float(rate)]
