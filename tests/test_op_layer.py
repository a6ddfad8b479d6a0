"""CPU: the two helpers every operator wrapper goes through -- `_lib.call` (device guard, entry point looked up at call time, return
code checked) and `_packcache.packed` (the cache protocol of every weight pack, with the hand-over to a graph that is being captured)."""
import gc
import importlib

import pytest
import torch
import torch.nn as nn

from orientedreppoints_amd import _lib, _packcache

NO_DEVICE = -1            # torch.cuda.device(-1) is a no-op guard: these tests launch nothing


class _StandIn(object):
    """a library object with one entry point that records its arguments and returns `rc`"""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def orp_probe(self, *args):
        self.calls.append(args)
        return self.rc


def test_call_passes_the_arguments_and_returns_on_a_zero_status(monkeypatch):
    lib = _StandIn(_lib.ORP_OK)
    monkeypatch.setattr(_lib, "_lib", lib)
    assert _lib.call("orp_probe", NO_DEVICE, 1, None, "x") is None
    assert lib.calls == [(1, None, "x")]


@pytest.mark.parametrize("rc, text", [(_lib.ORP_EINVAL, "ORP_EINVAL"), (_lib.ORP_EWORKSPACE, "ORP_EWORKSPACE"),
                                      (_lib.ORP_ETOOBIG, "ORP_ETOOBIG"), (700, "hipError 700")])
def test_call_raises_with_the_entry_point_and_the_code(monkeypatch, rc, text):
    monkeypatch.setattr(_lib, "_lib", _StandIn(rc))
    with pytest.raises(_lib.OrpHipError) as e:
        _lib.call("orp_probe", NO_DEVICE)
    assert str(e.value) == "orp_probe failed: " + text


def test_call_looks_the_entry_point_up_when_it_is_called(monkeypatch):
    lib = _StandIn()
    monkeypatch.setattr(_lib, "_lib", lib)
    _lib.call("orp_probe", NO_DEVICE, 1)
    seen = []
    monkeypatch.setattr(lib, "orp_probe", lambda *a: seen.append(a) or 0)     # what every `_spy` of the GPU tests does
    _lib.call("orp_probe", NO_DEVICE, 2)
    assert lib.calls == [(1,)] and seen == [(2,)]
    with pytest.raises(AttributeError):
        _lib.call("orp_no_such_entry", NO_DEVICE)


def test_tile_query_fills_integers_or_says_none(monkeypatch):
    class Lib(object):
        @staticmethod
        def orp_some_tile(a, b, t0, t1):
            if a == 0:
                return 0
            t0._obj.value, t1._obj.value = a + b, a * b
            return 1
    monkeypatch.setattr(_lib, "_lib", Lib())
    assert _lib.tile_query("orp_some_tile", 2, 3, 4) == (7, 12)
    assert _lib.tile_query("orp_some_tile", 2, 0, 4) is None


def _counting(payload_of):
    built = []

    def build():
        built.append(payload_of())
        return built[-1]
    return build, built


def test_packed_hits_until_the_owner_changes():
    cache = _packcache.OwnerCache("t")
    p = nn.Parameter(torch.zeros(4, 3))
    build, built = _counting(lambda: p.detach().clone())
    first = _packcache.packed(cache, p, build)
    assert _packcache.packed(cache, p, build) is first and len(built) == 1 and len(cache) == 1
    assert (cache.hits, cache.misses) == (1, 1)
    with torch.no_grad():
        p.add_(1.0)                                          # in-place update: the version moves, the entry is stale
    second = _packcache.packed(cache, p, build)
    assert second is not first and len(built) == 2 and len(cache) == 1
    assert _packcache.packed(cache, p, build) is second and len(built) == 2


def test_packed_takes_a_state_of_the_callers():
    cache = _packcache.OwnerCache("t")
    owner = nn.BatchNorm2d(2)
    build, built = _counting(lambda: object())
    a = _packcache.packed(cache, owner, build, state=("s", 1))
    assert _packcache.packed(cache, owner, build, state=("s", 1)) is a and len(built) == 1
    assert _packcache.packed(cache, owner, build, state=("s", 2)) is not a and len(built) == 2


def test_packed_never_serves_a_dead_owners_entry_to_a_recycled_id():
    cache = _packcache.OwnerCache("t")
    seen, recycled = set(), 0
    for i in range(300):
        p = nn.Parameter(torch.full((18, 256, 1, 1), float(i)))
        recycled += id(p) in seen
        seen.add(id(p))
        build, built = _counting(lambda: i)
        assert _packcache.packed(cache, p, build) == i and len(built) == 1, "a dead parameter's pack served to a new one (%d)" % i
        del p
    assert recycled > 0, "the test did not exercise id() recycling"
    gc.collect()
    assert len(cache) == 0


def test_packed_without_store_builds_every_time_and_keeps_nothing(monkeypatch):
    cache = _packcache.OwnerCache("t")
    p = nn.Parameter(torch.zeros(4))
    kept = []
    monkeypatch.setattr(_lib, "_keepalive", kept)
    build, built = _counting(lambda: p.detach().clone())
    a = _packcache.packed(cache, p, build, store=False)
    b = _packcache.packed(cache, p, build, store=False)
    assert a is not b and len(built) == 2
    assert len(cache) == 0 and (cache.hits, cache.misses) == (0, 0) and kept == []
    stored = _packcache.packed(cache, p, build)              # an entry that exists is neither read nor replaced without store
    assert _packcache.packed(cache, p, build, store=False) is not stored and len(cache) == 1
    assert _packcache.packed(cache, p, build) is stored


def test_packed_hands_misses_and_hits_to_a_capturing_graph(monkeypatch):
    cache = _packcache.OwnerCache("t")
    p = nn.Parameter(torch.zeros(4))
    build, _built = _counting(lambda: p.detach().clone())
    monkeypatch.setattr(_lib, "_keepalive", None)
    outside = _packcache.packed(cache, p, build)             # no capture is collecting: nothing to append to
    kept = []
    monkeypatch.setattr(_lib, "_keepalive", kept)
    assert _packcache.packed(cache, p, build) is outside     # a hit
    assert len(kept) == 1 and kept[0] is outside
    with torch.no_grad():
        p.add_(1.0)
    fresh = _packcache.packed(cache, p, build)               # a miss
    assert len(kept) == 2 and kept[1] is fresh and fresh is not outside
    monkeypatch.setattr(_lib, "_keepalive", None)
    assert _packcache.packed(cache, p, build) is fresh and len(kept) == 2


def test_the_helpers_have_one_home():
    fused_norm = importlib.import_module("orientedreppoints_amd.mmdet_ops.fused_norm")
    token_linear = importlib.import_module("orientedreppoints_amd.mmdet_ops.token_linear")
    for name in ("_call", "_tile_query", "_packed_planes"):  # `_lib.call`, `_lib.tile_query` and `_packcache.packed_planes` now
        assert not hasattr(fused_norm, name) and not hasattr(token_linear, name), name
    assert "fused_norm" not in vars(token_linear)            # a Swin linear layer asks nothing of the normalisation module
    assert callable(_packcache.packed_planes) and callable(_lib.tile_query)
