"""wdf_hip.tensor_cache: the two identity rules every per-tensor cache of the host layer uses.

ObjectMemo (the object rule) answers for one tensor object at one version and keeps nothing alive; EntryCache (the storage
rule) answers for the storage a tensor looks at and holds the tensors it was keyed on.  Two tensors made by torch.from_numpy
on ONE array share address, shape, strides and version -- what the caching allocator produces when a loop builds every batch
anew in the freed block of the previous one.  CPU only.
"""
import gc
import weakref

import numpy as np
import pytest

torch = pytest.importorskip("torch")


@pytest.fixture
def tc():
    from wdf_hip import tensor_cache
    return tensor_cache


def test_object_memo_misses_for_the_second_tensor_at_the_same_address(tc):
    a = np.ones((2, 8), np.float32)
    memo = tc.ObjectMemo(4)
    t1 = torch.from_numpy(a)
    memo.put(t1, "first", "layout")
    assert memo.get(t1, "layout") == "first" and memo.get(t1, "other") is None
    t2 = torch.from_numpy(a)
    assert tc.tensor_key(t1) == tc.tensor_key(t2)              # the collision the storage key cannot see
    assert memo.get(t2, "layout") is None


def test_object_memo_misses_after_an_in_place_change(tc):
    t = torch.zeros(4)
    memo = tc.ObjectMemo(4)
    memo.put(t, 1.0)
    assert memo.get(t) == 1.0
    t.add_(1.0)
    assert memo.get(t) is None
    memo.put(t, 2.0)
    assert memo.get(t) == 2.0 and len(memo) == 1                  # the stale answer was replaced, not kept beside


def test_object_memo_tuples_with_an_optional_tensor(tc):
    x, r = torch.zeros(3), torch.ones(3)
    memo = tc.ObjectMemo(8)
    memo.put((x, None), "x alone", 7)
    memo.put((x, r), "x and r", 7)
    assert memo.get((x, None), 7) == "x alone" and memo.get((x, r), 7) == "x and r"
    assert memo.get((r, None), 7) is None and memo.get((x, r), 8) is None
    r.mul_(2.0)                                                    # any tensor's version moving misses
    assert memo.get((x, r), 7) is None and memo.get((x, None), 7) == "x alone"


def test_object_memo_keeps_no_tensor_alive(tc):
    memo = tc.ObjectMemo(4)
    t, u = torch.zeros(16), torch.zeros(16)
    memo.put(t, "t")
    memo.put((u, None), "u")
    wt, wu = weakref.ref(t), weakref.ref(u)
    del t, u
    gc.collect()
    assert wt() is None and wu() is None


def test_object_memo_evicts_dead_entries_before_live_ones(tc):
    memo = tc.ObjectMemo(3)
    live = [torch.zeros(1), torch.zeros(1)]
    memo.put(live[0], 0)
    dead = torch.zeros(1)
    memo.put(dead, "dead")
    memo.put(live[1], 1)
    del dead
    gc.collect()
    newest = torch.zeros(1)
    memo.put(newest, 2)                                            # full: the dead entry goes, not the oldest live one
    assert len(memo) == 3 and [(w(), v) for w, v in memo.values()] == [(live[0], 0), (live[1], 1), (newest, 2)]
    assert memo.get(live[0]) == 0 and memo.get(live[1]) == 1 and memo.get(newest) == 2
    more = torch.zeros(1)
    memo.put(more, 3)                                              # nothing dead: the oldest goes
    assert memo.get(live[0]) is None and memo.get(more) == 3 and len(memo) == 3
    memo.clear()
    assert len(memo) == 0 and memo.get(more) is None


def test_entry_cache_hits_for_two_slices_of_one_tensor(tc):
    X = torch.arange(24, dtype=torch.float32).reshape(6, 4)
    Y = torch.zeros(6)
    cache = tc.EntryCache()
    ent = cache.put((X[0:2], Y[0:2]), {"stepper": 1}, "mse")
    assert cache.get((X[0:2], Y[0:2]), "mse") is ent              # fresh slice objects, the same storage
    assert cache.get((X[2:4], Y[2:4]), "mse") is None and cache.get((X[0:2], Y[0:2]), "esr") is None
    assert list(cache.values()) == [ent]                          # entries as they were stored
    X[0, 0] += 1.0                                                 # in place: the version moved
    assert cache.get((X[0:2], Y[0:2]), "mse") is None


def test_entry_cache_holds_the_tensors_it_was_keyed_on(tc):
    cache = tc.EntryCache(max_entries=1)
    x = torch.from_numpy(np.arange(8, dtype=np.float32))
    cache.put(x, True)
    wx = weakref.ref(x)
    ptr = x.data_ptr()
    del x
    gc.collect()
    assert wx() is not None and wx().data_ptr() == ptr            # the storage is still the entry's: no other data there
    assert cache.get(wx()) is True
    cache.put(torch.zeros(3), False)                               # the entry is evicted, the tensor with it
    gc.collect()
    assert wx() is None and len(cache) == 1
