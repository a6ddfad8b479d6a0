"""CPU: the table of a bottleneck's fused conv2 kernels (fused_norm.CONV3X3_KERNELS) against the library's host functions: which
kernel answers first at every R-50 conv2 shape, that no shape is taken by two kernels (what makes their one shared pack cache sound),
that every name in the table exists, and the packed size."""
import pytest

FIRST = {(64, 64, 1): "act", (128, 128, 1): "act", (256, 256, 1): "act", (512, 512, 1): "deep", (512, 512, 2): "deep",
         (128, 128, 2): "s2", (256, 256, 2): "s2", (64, 64, 2): None,
         (64, 128, 1): None, (64, 128, 2): None, (512, 256, 1): None, (512, 256, 2): None}


@pytest.fixture(scope="module")
def L():
    from orientedreppoints_amd import build, _lib
    build.build_hip()
    return _lib.lib()


def _table():
    from orientedreppoints_amd.mmdet_ops.fused_norm import CONV3X3_KERNELS
    return CONV3X3_KERNELS


def _ok(L, k, cin, cout, stride):
    """what fused_norm._conv3x3_ok asks of the library for a convolution of this stride: the stride set, then the `ok` symbol"""
    if (stride, stride) not in k.strides:
        return False
    return bool(getattr(L, k.ok)(cin, cout, *((stride,) if k.takes_stride else ())))


def test_the_cases_are_the_issue_s():
    assert {(c, c, s) for c in (64, 128, 256, 512) for s in (1, 2)} <= set(FIRST) and len(FIRST) == 12


@pytest.mark.parametrize("shape", sorted(FIRST))
def test_precedence_and_at_most_one_kernel_per_shape(L, shape):
    takers = [k.kind for k in _table() if _ok(L, k, *shape)]
    assert (takers[0] if takers else None) == FIRST[shape]
    assert len(takers) <= 1, takers


def test_table_names_exist_and_the_order_is_act_deep_s2():
    from orientedreppoints_amd import _lib, switches
    from orientedreppoints_amd.mmdet_ops import fused_norm
    table = _table()
    assert [k.kind for k in table] == ["act", "deep", "s2"]
    for k in table:
        for name in (k.ok, k.pays, k.packed_bytes, k.pack_weight, k.launch):
            assert name in _lib._SIGNATURES, name
        assert isinstance(getattr(switches, k.switch), bool), k.switch
        assert k.fuse_attr == "fuse_" + k.force_attr[len("force_"):] and k.force_attr.startswith("force_conv3x3")
        assert fused_norm.conv3x3_kernel(k.kind) is k
        # the stride travels where the signatures say: one more int in ok / pays / launch
        n = 1 if k.takes_stride else 0
        assert [len(_lib._SIGNATURES[s][1]) for s in (k.ok, k.pays, k.launch)] == [2 + n, 5 + n, 13 + n]


def test_packed_bytes(L):
    """a packer has no stride argument: the size at the channel pairs its kernel takes at some stride, 0 at every other pair"""
    for k in _table():
        for (cin, cout) in sorted({s[:2] for s in FIRST}):
            takes = any(_ok(L, k, cin, cout, s) for s in (1, 2))
            assert getattr(L, k.packed_bytes)(cin, cout) == (4 * cin * cout * 9 + 16 if takes else 0), (k.kind, cin, cout)
