"""Identity-safe cache of device-side re-layouts of module parameters (DeformConv / 3x3 / 1x1 weight packs, folded
eval-mode BatchNorm affines).

An entry belongs to ONE live Python object (an nn.Parameter or an nn.Module):

* the entry holds a weak reference to its owner and a hit requires `entry.owner() is obj` -- CPython recycles `id()`s
  and the caching allocator recycles device addresses, so `(id, data_ptr, _version, shape)` of a freed parameter can
  all reappear on a new one (build a model, drop it, build another of the same shape);
* the weak reference's callback removes exactly that entry when the owner dies; nothing is ever cleared wholesale and
  there is no size cap to thrash against (the cache is as large as the set of live packed parameters);
* `state` (storage address, version counters, dtype, device) catches in-place updates of a live owner.  Writes through
  `.data` bump no version counter: training-mode callers pass `cache=False` (see deform_conv.py), everything else
  calls `invalidate()`.
"""
import weakref

import torch

from . import _lib


class OwnerCache:
    def __init__(self, name):
        self.name = name
        self._entries = {}          # id(owner) -> (weakref(owner), state, payload)
        self.hits = self.misses = 0

    def get(self, owner, state):
        e = self._entries.get(id(owner))
        if e is not None and e[0]() is owner and e[1] == state:
            self.hits += 1
            return e[2]
        self.misses += 1
        return None

    def put(self, owner, state, payload):
        key = id(owner)
        entries = self._entries

        def _gone(ref, key=key, entries=entries):
            e = entries.get(key)
            if e is not None and e[0] is ref:        # a recycled id may already carry a newer owner's entry
                del entries[key]
        entries[key] = (weakref.ref(owner, _gone), state, payload)
        return payload

    def invalidate(self):
        self._entries.clear()

    def __len__(self):
        return len(self._entries)


_all = []


def new_cache(name):
    c = OwnerCache(name)
    _all.append(c)
    return c


def invalidate_all():
    """Drop every cached pack / affine of every cache (after loading a checkpoint through `.data`, EMA swaps, ...)."""
    for c in _all:
        c.invalidate()


def stats():
    return {c.name: {"entries": len(c), "hits": c.hits, "misses": c.misses} for c in _all}


def tensor_state(t):
    return (t.data_ptr(), t._version, tuple(t.shape), t.dtype, t.device.index)


def packed(cache, owner, build, state=None, store=True):
    """The cache protocol of every pack: `cache`'s entry of the live `owner` in this `state` (default: the tensor's storage / version
    state), made by build() on a miss; hit or miss, handed to a graph that is being captured (`_lib.keep_for_graph`), which must
    outlive the entry.  store=False (training: optimizers write through `.data`): build() now, nothing looked up, kept or registered."""
    if not store:
        return build()
    if state is None:
        state = tensor_state(owner.detach())
    hit = cache.get(owner, state)
    if hit is None:
        hit = cache.put(owner, state, build())
    return _lib.keep_for_graph(hit)


def packed_planes(cache, weight, size_fn, pack_fn, view):
    """weight [Cout,Cin,...] -> the byte buffer the library's `pack_fn` fills from view(weight) (fp32, contiguous), `size_fn`(Cin, Cout)
    bytes; cached on the live parameter as `packed` says (inference only)."""
    def build():
        w = weight.detach()
        cout, cin = w.size(0), w.size(1)
        w32 = view(w)
        planes = torch.empty((getattr(_lib.lib(), size_fn)(cin, cout),), dtype=torch.uint8, device=w.device)
        _lib.call(pack_fn, w.device, _lib.ptr(w32), cin, cout, _lib.ptr(planes), _lib.stream_of(w32))
        return planes
    return packed(cache, weight, build)
