"""Values derived from tensors, remembered until a tensor changes: the one home of every cache keyed on a tensor's storage
address and torch version counter (packed weight streams, folded BatchNorm weights, weight fragments, channel-last feature
maps, host copies of camera matrices).

The rule, for both forms: WHILE AN ENTRY CAN BE HIT, THE STORAGE ITS KEY NAMES CANNOT BE HANDED TO ANOTHER TENSOR.  malloc and
torch's caching allocator hand a freed block straight back, and a fresh tensor's `_version` is 0 again.  Holding the tensor
object is not enough for a Parameter: `param.data = other` swaps the storage under the same object and keeps `_version`.  So
an entry holds the storage (`t.untyped_storage()`) of every tensor of its key, taken on a miss only.  The consequence: after
`module.to(...)` the old storage lives until the slot's next miss or the cache's next clear() (a few MB of weights here).
The limit: a writer torch does not see (a kernel of this library, any raw-pointer writer) leaves `_version` alone and
invalidates explicitly, as `invalidate_packed()` and `TrainStep.inputs_changed()` do.
The many-entry form keys on the full `tensor_key`; the one-slot form on (address, version) per tensor, which is sufficient
there -- an owner passes a fixed list of its own parameters and the held storage rules out a recycled address -- and
measurably cheaper: the train step holds with either, a feature extractor's 14 slots per image do not with the full key
(profiles/tensor_caches_refactor.txt).

Not here, on purpose: `captured.CapturedSteps.key` and `train._JobCache` (their keys name addresses a captured graph or a
job table holds: an equal address is the condition itself there, not a proxy for "the same tensor"), `SplitVolume._cache`
(a buffer pool keyed by shape), `scene._CACHE` (keyed by file), `StageLoop`'s fingerprints (keyed by content) and
`VolOpt._mvs_view_cache` (`id()` with the objects held)."""
import torch


def tensor_key(t):
    return (t.data_ptr(), t._version, t.shape, t.stride(), t.device, t.dtype)


class Derived:
    """One value derived from a list of tensors: `slot(tensors, make)` is the remembered value while every tensor of the list
    is unchanged, make() otherwise.  An optimiser step, load_state_dict, .to() and a `.data` swap all change the key."""

    def __init__(self):
        self.invalidate()

    def invalidate(self):
        """forget the value and let go of the storages: the next call makes"""
        self._key, self._held, self.value = None, (), None

    def __call__(self, tensors, make):
        key = tuple([(t.data_ptr(), t._version) for t in tensors])
        if key != self._key:
            self.invalidate()
            self.value = make()
            self._held, self._key = [t.untyped_storage() for t in tensors], key
        return self.value


class TensorCache:
    """Many values, each derived from one tensor or a tuple of tensors (plus an optional tag).  Bounded by entries and / or
    bytes, or unbounded; a full cache is emptied (the working set of a scan fits: the bound is a guard against a leak, not an
    eviction policy)."""

    def __init__(self, entries=None, nbytes=None):
        self.entries, self.nbytes = entries, nbytes
        self.clear()

    def clear(self):
        self._d, self._used = {}, 0

    def get(self, t, make, tag=None, nbytes=0, cacheable=None):
        """the cached make() of tensor t (or of the tensors t).  cacheable(value) false: this value is returned but not
        remembered (a value that turned out to depend on more than its key says)."""
        ts = (t,) if isinstance(t, torch.Tensor) else t
        key = (tag, *map(tensor_key, ts))
        hit = self._d.get(key)
        if hit is None:
            value = make()
            if cacheable is not None and not cacheable(value):
                return value
            if (self.entries is not None and len(self._d) >= self.entries) or (self.nbytes is not None and self._used + nbytes > self.nbytes):
                self.clear()
            hit = self._d[key] = ([x.untyped_storage() for x in ts], value)
            self._used += nbytes
        return hit[1]
