"""svs_hip/tensor_cache.py on the CPU: what a hit and a miss are for the one-slot form (Derived) and the bounded many-entry
form (TensorCache), and the rule both obey -- while an entry can be hit, the storage its key names cannot be handed to
another tensor."""
import weakref

import pytest
import torch

from svs_hip.tensor_cache import Derived, TensorCache, tensor_key


class _Slot:
    """both forms behind one call: lookup(tensors, make)"""

    def __init__(self, form):
        self.form = form
        self.cache = Derived() if form == "slot" else TensorCache()

    def __call__(self, tensors, make):
        return self.cache(tensors, make) if self.form == "slot" else self.cache.get(tensors, make)

    def drop(self):
        self.cache.invalidate() if self.form == "slot" else self.cache.clear()


@pytest.fixture(params=["slot", "many"])
def lookup(request):
    return _Slot(request.param)


def _counter():
    calls = []
    return calls, lambda: calls.append(1) or len(calls)


def test_same_tensor_twice_makes_once(lookup):
    calls, make = _counter()
    t = torch.zeros(3)
    assert lookup([t], make) == 1 and lookup([t], make) == 1 and len(calls) == 1


def test_in_place_write_is_a_miss(lookup):
    calls, make = _counter()
    t = torch.zeros(3)
    assert lookup([t], make) == 1
    with torch.no_grad():
        t.add_(1)
    assert lookup([t], make) == 2 and lookup([t], make) == 2


def test_another_tensor_is_a_miss(lookup):
    calls, make = _counter()
    t, u = torch.zeros(3), torch.zeros(3)
    assert lookup([t], make) == 1 and lookup([u], make) == 2


def test_another_dependency_list_is_a_miss(lookup):
    calls, make = _counter()
    t, u = torch.zeros(3), torch.zeros(3)
    assert lookup([t, u], make) == 1 and lookup([t, u], make) == 1
    assert lookup([t, t], make) == 2
    assert lookup([t], make) == 3
    assert lookup([u, t], make) == 4


def test_another_tag_is_a_miss():
    cache = TensorCache()
    calls, make = _counter()
    t = torch.zeros(3)
    assert cache.get(t, make, tag="a") == 1 and cache.get(t, make, tag="b") == 2 and cache.get(t, make) == 3
    assert cache.get(t, make, tag="a") == 1 and cache.get(t, make, tag="b") == 2 and cache.get(t, make) == 3


def test_one_tensor_and_a_list_of_it_are_the_same_entry():
    cache = TensorCache()
    calls, make = _counter()
    t = torch.zeros(3)
    assert cache.get(t, make) == 1 and cache.get([t], make) == 1 and cache.get((t,), make) == 1


def test_recycled_address(lookup):
    """malloc hands a freed block straight back and a fresh tensor's version is 0 again: with nothing held, the key of trial
    i + 1 is the key of trial i (17 stale hits of 19 with the one-slot form that kept only the key)"""
    calls, make = _counter()
    for i in range(20):
        w = torch.full((64, 64), float(i))
        assert lookup([w], lambda: make() and float(w[0, 0])) == float(i)
        del w
    assert len(calls) == 20


def test_storage_swapped_under_a_parameter(lookup):
    """`p.data = other`: the same object and the same version on another storage is a miss, and the old storage stays alive
    while the entry can be hit (so that its address cannot come back under another tensor)"""
    calls, make = _counter()
    p = torch.nn.Parameter(torch.zeros(64, 64))
    old = weakref.ref(p.untyped_storage())
    assert lookup([p], make) == 1
    version, address = p._version, p.data_ptr()
    p.data = torch.ones(64, 64)
    assert p._version == version and p.data_ptr() != address
    assert old() is not None and old().data_ptr() == address
    assert lookup([p], make) == 2 and lookup([p], make) == 2
    lookup.drop()
    assert old() is None


def test_views_of_one_storage_are_different_entries():
    cache = TensorCache()
    calls, make = _counter()
    w = torch.zeros(3, 5)
    assert w.t().data_ptr() == w.data_ptr() and tensor_key(w.t()) != tensor_key(w)
    assert cache.get(w, make) == 1 and cache.get(w.t(), make) == 2
    assert cache.get(w, make) == 1 and cache.get(w.t(), make) == 2
    assert cache.get(w.view(5, 3), make) == 3 and cache.get(w.view(15), make) == 4


def test_entry_bound_empties_the_cache():
    cache = TensorCache(entries=3)
    calls, make = _counter()
    ts = [torch.zeros(2) for _ in range(4)]
    assert [cache.get(t, make) for t in ts[:3]] == [1, 2, 3]
    assert [cache.get(t, make) for t in ts[:3]] == [1, 2, 3]            # full, and every entry still there
    assert cache.get(ts[3], make) == 4                                  # the fourth empties it and goes in
    assert cache.get(ts[3], make) == 4 and cache.get(ts[0], make) == 5 and cache.get(ts[3], make) == 4


def test_byte_bound_empties_the_cache():
    cache = TensorCache(nbytes=100)
    calls, make = _counter()
    ts = [torch.zeros(2) for _ in range(3)]
    assert cache.get(ts[0], make, nbytes=60) == 1 and cache.get(ts[1], make, nbytes=40) == 2      # 100 of 100
    assert cache.get(ts[0], make, nbytes=60) == 1 and cache.get(ts[1], make, nbytes=40) == 2
    assert cache.get(ts[2], make, nbytes=1) == 3                                                    # 101: emptied first
    assert cache.get(ts[2], make, nbytes=1) == 3 and cache.get(ts[1], make, nbytes=40) == 4 and cache.get(ts[0], make, nbytes=60) == 5
    assert cache.get(ts[0], make, nbytes=60) == 5 and cache.get(ts[2], make, nbytes=1) == 6        # 1 + 40 + 60: emptied again


def test_a_value_that_is_not_cacheable_is_returned_and_not_remembered():
    cache = TensorCache(entries=4)
    calls, make = _counter()
    t = torch.zeros(3)
    assert cache.get(t, make, cacheable=lambda v: v > 2) == 1 and cache.get(t, make, cacheable=lambda v: v > 2) == 2
    assert cache.get(t, make, cacheable=lambda v: v > 2) == 3 and cache.get(t, make, cacheable=lambda v: v > 2) == 3


def test_dropping_lets_go_of_value_and_storage(lookup):
    """clear() / invalidate(): what only the cache held is freed"""
    t = torch.zeros(8)
    value = torch.ones(8)
    storage, made = weakref.ref(t.untyped_storage()), weakref.ref(value)
    assert lookup([t], lambda: value) is value
    del t, value
    assert storage() is not None and made() is not None
    lookup.drop()
    assert storage() is None and made() is None


def test_dropping_forces_a_make(lookup):
    calls, make = _counter()
    t = torch.zeros(3)
    assert lookup([t], make) == 1 and lookup([t], make) == 1
    lookup.drop()
    assert lookup([t], make) == 2 and lookup([t], make) == 2


def test_cached_fold_is_the_one_slot_form():
    from models.blocks import CachedFold
    assert CachedFold is Derived
