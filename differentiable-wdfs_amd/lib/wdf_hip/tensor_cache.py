"""The per-tensor caches of the host layer: is this the tensor an answer was kept for?  Two rules, one class each.

ObjectMemo, the OBJECT rule: an answer belongs to one tensor object at one version (`_version`, which every in-place change
moves).  Weak references only: the memo keeps no device memory alive and its entries die with the tensors.  A fresh tensor
at a recycled address (same address, shape, strides, version 0) is a miss.  For facts derived from a tensor (max R, is the
pot constant along every sequence) and small copies that must die with it.

EntryCache, the STORAGE rule: an entry belongs to the storage a tensor looks at (tensor_key: address, shape, strides, dtype,
version, device).  Fresh slices X[i:j] of one dataset are the same batch, so a mini-batch loop finds its resident stepper
again every epoch.  Sound only because the cache holds the tensors it was keyed on: their address cannot be handed to other
data while the entry exists.  For resident steppers and their buffers.

Both take `ts`, one tensor or a tuple of tensors (EntryCache keys anything else in it by value), and `extra`, anything
hashable the answer also depends on (layout, shape).
"""
import weakref

import torch


def _dead(refs):
    if type(refs) is not tuple:
        return refs() is None
    return any(w is not None and w() is None for w in refs)


class ObjectMemo:
    """Answers per tensor object and version, at most `max_entries` of them.  A tuple `ts` may hold None (an optional input);
    a hit then needs None in the same place.  put() first drops the entries whose tensors have died, then the oldest.
    values(): (weak reference(s), answer) per entry, oldest first."""

    def __init__(self, max_entries):
        self.d, self.max_entries = {}, int(max_entries)

    def get(self, ts, extra=None):
        if type(ts) is not tuple:                    # (one tensor: one look-up, one dereference, one version compare)
            hit = self.d.get((id(ts), extra))
            return hit[2] if hit is not None and hit[0]() is ts and hit[1] == ts._version else None
        hit = self.d.get((tuple(map(id, ts)), extra))
        ok = hit is not None and all(t is None or (w() is t and t._version == v) for t, w, v in zip(ts, hit[0], hit[1]))
        return hit[2] if ok else None

    def put(self, ts, value, extra=None):
        d = self.d
        for k in [k for k, e in d.items() if _dead(e[0])]:
            del d[k]
        if type(ts) is not tuple:
            d[(id(ts), extra)] = (weakref.ref(ts), ts._version, value)
        else:
            d[(tuple(map(id, ts)), extra)] = (tuple(None if t is None else weakref.ref(t) for t in ts),
                                              tuple(None if t is None else t._version for t in ts), value)
        while len(d) > self.max_entries:
            del d[next(iter(d))]
        return value

    def values(self):
        return [(e[0], e[2]) for e in self.d.values()]

    def clear(self):
        self.d.clear()

    def __len__(self):
        return len(self.d)


def tensor_key(t):
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype, t._version, t.device.type, t.device.index)


class EntryCache:
    """Insertion-ordered cache of resident entries under the storage rule: at most `max_entries`, and -- beyond the first
    four -- at most `max_bytes` of device buffers in total (a full-batch loop keeps a training and a validation set; a
    mini-batch loop keeps every mini-batch of an epoch while they are small).  Holds the tensors of every entry's key."""

    def __init__(self, max_entries=256, max_bytes=16 << 30):
        self.d, self.held, self.nbytes, self.max_entries, self.max_bytes = {}, {}, {}, int(max_entries), int(max_bytes)

    @staticmethod
    def _key(ts, extra):
        with torch._C.DisableTorchFunctionSubclass():           # (plain attribute reads: no subclass dispatch)
            return tuple(tensor_key(t) if isinstance(t, torch.Tensor) else t for t in (ts if type(ts) is tuple else (ts,))), extra

    def get(self, ts, extra=None):
        return self.d.get(self._key(ts, extra))

    def put(self, ts, ent, extra=None, nbytes=0):
        key = self._key(ts, extra)
        self.d[key], self.held[key], self.nbytes[key] = ent, ts, int(nbytes)
        while len(self.d) > self.max_entries or (len(self.d) > 4 and sum(self.nbytes.values()) > self.max_bytes):
            old = next(iter(self.d))
            del self.d[old], self.held[old], self.nbytes[old]
        return ent

    def values(self):
        return self.d.values()

    def __len__(self):
        return len(self.d)
