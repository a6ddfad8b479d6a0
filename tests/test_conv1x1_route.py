"""No GPU: the route `conv1x1_bn_act` takes -- bf16-pieces kernel, fp32 kernel or library convolution + pass -- over every combination
of (force, pieces, ORP_BN_CONV1X1_PIECES, pieces table, pieces shape rule, fp32 table, supported or not), against the conditions
the function had before the route was a function of its own, written out below; and `switches.of`."""
import itertools

import pytest

torch = pytest.importorskip("torch")

SHAPE = (256, 64, 65536, 1, 0)


class _Library(object):
    """the four entry points the route asks, with fixed answers"""

    def __init__(self, pieces_pays, pieces_ok, fp32_pays):
        self.asked = []
        self.answers = {'orp_conv1x1_bn_act_pieces_pays': pieces_pays, 'orp_conv1x1_bn_act_pieces_ok': pieces_ok,
                        'orp_conv1x1_bn_act_pays': fp32_pays}

    def __getattr__(self, name):
        if name not in self.answers:
            raise AttributeError(name)

        def entry(*args):
            self.asked.append((name,) + args)
            return 1 if self.answers[name] else 0
        return entry


def _route_of_before(L, switch, shape, force, pieces):
    """conv1x1_bn_act's conditions as they stood inline (fused = the arguments are supported: shape is not None)"""
    fused = shape is not None
    use_pieces = False
    if fused and not (force and pieces is None) and pieces is not False:
        if pieces is None:
            pieces = bool(switch) and bool(L.orp_conv1x1_bn_act_pieces_pays(*shape))
        use_pieces = bool(pieces) and bool(L.orp_conv1x1_bn_act_pieces_ok(shape[0], shape[1]))
    if use_pieces:
        return 'pieces'
    if fused and not force:
        fused = bool(L.orp_conv1x1_bn_act_pays(*shape))
    return 'fp32' if fused else None


def test_route_truth_table(monkeypatch):
    from orientedreppoints_amd import _lib, switches
    from orientedreppoints_amd.mmdet_ops.fused_norm import _conv1x1_route
    cases = list(itertools.product((False, True), (None, True, False), (False, True), (False, True), (False, True), (False, True),
                                   (False, True)))
    assert len(cases) == 192
    seen = set()
    for force, pieces, switch, pieces_pays, pieces_ok, fp32_pays, supported in cases:
        shape = SHAPE if supported else None
        want_lib = _Library(pieces_pays, pieces_ok, fp32_pays)
        want = _route_of_before(want_lib, switch, shape, force, pieces)
        got_lib = _Library(pieces_pays, pieces_ok, fp32_pays)
        monkeypatch.setattr(_lib, 'lib', lambda got_lib=got_lib: got_lib)
        monkeypatch.setattr(switches, 'BN_CONV1X1_PIECES', switch)
        got = _conv1x1_route(shape, force, pieces)
        case = (force, pieces, switch, pieces_pays, pieces_ok, fp32_pays, supported)
        assert got == want, case
        assert got_lib.asked == want_lib.asked, case            # the same questions in the same order
        seen.add(got)
    assert seen == {'pieces', 'fp32', None}


@pytest.mark.parametrize("module_switch", [False, True])
@pytest.mark.parametrize("attribute", [True, False, None])
def test_switches_of(monkeypatch, attribute, module_switch):
    from orientedreppoints_amd import switches

    class Block(object):
        pass
    blk = Block()
    monkeypatch.setattr(switches, 'BN_CONV1X1_FUSE', module_switch)
    assert switches.of(blk, 'fuse_conv1x1', 'BN_CONV1X1_FUSE') is module_switch          # no attribute at all: the module's
    blk.fuse_conv1x1 = attribute
    assert switches.of(blk, 'fuse_conv1x1', 'BN_CONV1X1_FUSE') is (module_switch if attribute is None else attribute)
