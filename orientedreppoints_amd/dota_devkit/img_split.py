"""Split grammar of the DOTA evaluation workflow (DOTA_devkit/SplitOnlyImage.py:27-57,
SplitOnlyImage_multi_process.py:49-83, prepare_dota1_ms.py:16,83): where the S x S patches of a scene lie, the size a
rate scales the scene to, and the patch names (`<name>__<rate>__<left>___<up>`) that `result_merge` and
`result_merge_multi_process` parse back.  Host code only; no cv2."""


def _axis_origins(extent, subsize, slide):
    """Start positions along one axis: every `slide` pixels, the last one moved back to max(extent - subsize, 0)."""
    out = []
    pos = 0
    while pos < extent:
        if pos + subsize >= extent:
            out.append(max(extent - subsize, 0))
            break
        out.append(pos)
        pos += slide
    return out


def split_origins(width, height, subsize=1024, gap=200):
    """(left, up) of every patch in SplitSingle's loop order: outer loop over `left`, inner loop over `up`.
    `gap >= subsize` raises ValueError (the reference's loop would never end)."""
    width, height, subsize, gap = int(width), int(height), int(subsize), int(gap)
    if subsize <= 0:
        raise ValueError("split_origins: subsize must be positive (got %d)" % subsize)
    if gap >= subsize:
        raise ValueError("split_origins: gap (%d) must be smaller than subsize (%d)" % (gap, subsize))
    slide = subsize - gap
    ups = _axis_origins(height, subsize, slide)
    return [(left, up) for left in _axis_origins(width, subsize, slide) for up in ups]


def scaled_size(width, height, rate):
    """cv2.resize(img, None, fx=rate, fy=rate)'s dsize: (round(width * rate), round(height * rate)), ties to even as
    cv2's saturate_cast<int> of a double rounds them."""
    return int(round(width * rate)), int(round(height * rate))


def patch_name(name, rate, left, up):
    """SplitSingle's patch name: name + '__' + str(rate) + '__' + str(left) + '___' + str(up)."""
    return name + '__' + str(rate) + '__' + str(left) + '___' + str(up)
