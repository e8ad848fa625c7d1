"""The per-tensor caches of the Python layer answer for the tensor they are asked about, not for an earlier tensor that
happened to look the same.

Two tensors made by torch.from_numpy on ONE array share address, shape, strides and version counter (a fresh tensor starts at
version 0) -- exactly what PyTorch's caching allocator produces when a loop builds every batch anew and gets the freed block
of the previous batch back.  Between the two calls the array changes; each cache must then give the second tensor's answer.
Deterministic, no allocator and no GPU involved.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


@pytest.fixture
def binding():
    from wdf_hip import binding
    return binding


@pytest.fixture
def engine():
    from wdf_hip import engine
    return engine


def same_key(a, b):
    return (a.data_ptr(), tuple(a.shape), tuple(a.stride()), a._version) == (b.data_ptr(), tuple(b.shape), tuple(b.stride()), b._version)


@pytest.mark.parametrize("time_major", [False, True])
def test_r_is_per_sequence_answers_for_the_second_tensor_at_the_same_address(binding, time_major):
    B, T = 4, 8
    a = np.full((T, B) if time_major else (B, T), 1.0e3, np.float32)
    if time_major:
        a[:, :] = np.array([1.0e3, 2.0e3, 3.0e3, 4.0e3], np.float32)[None, :]      # one value per sequence (column)
    else:
        a[:, :] = np.array([1.0e3, 2.0e3, 3.0e3, 4.0e3], np.float32)[:, None]      # one value per sequence (row)
    r1 = torch.from_numpy(a)
    assert binding.r_is_per_sequence(r1, time_major)
    # the pot moves inside every sequence: a step half-way
    if time_major:
        a[T // 2:, :] *= 2.0
    else:
        a[:, T // 2:] *= 2.0
    r2 = torch.from_numpy(a)
    assert same_key(r1, r2)                                    # the collision the address-keyed cache could not see
    assert not bool((r2 == (r2[0:1, :] if time_major else r2[:, 0:1])).all())
    assert not binding.r_is_per_sequence(r2, time_major)
    # and back: constant again, a third tensor at the same address
    a[:, :] = 5.0e3
    r3 = torch.from_numpy(a)
    assert same_key(r2, r3) and binding.r_is_per_sequence(r3, time_major)


def test_r_is_per_sequence_hits_on_the_same_object_and_misses_on_a_new_version(binding):
    r = torch.full((3, 16), 2.5e3)
    assert binding.r_is_per_sequence(r, False)
    calls = []
    real_all = torch.Tensor.all

    def counting_all(self, *a, **k):
        calls.append(1)
        return real_all(self, *a, **k)
    torch.Tensor.all = counting_all
    try:
        assert binding.r_is_per_sequence(r, False)             # the same object, same version: cached, nothing compared
        assert not calls
        r[1, 9:] = 7.0e3                                        # in place: the version counter moves
        assert not binding.r_is_per_sequence(r, False)
        assert calls
    finally:
        torch.Tensor.all = real_all
    # a fresh view of the same memory is a new object: looked at again, and answered right
    assert not binding.r_is_per_sequence(r[:, :], False)
    assert binding.r_is_per_sequence(r[:1, :], False) is True and binding.r_is_per_sequence(r[1:, :], False) is False


def test_r_is_per_sequence_switch_and_no_channel(binding, monkeypatch):
    r = torch.full((2, 8), 1.0e3)
    assert binding.r_is_per_sequence(None, False) is False
    monkeypatch.setattr(binding, "R_PER_SEQUENCE", False)
    assert binding.r_is_per_sequence(r, False) is False


def test_r_is_per_sequence_keeps_no_tensor_alive(binding):
    import gc
    import weakref
    r = torch.full((2, 8), 1.0e3)
    binding.r_is_per_sequence(r, True)
    w = weakref.ref(r)
    del r
    gc.collect()
    assert w() is None


@pytest.mark.parametrize("time_major", [False, True])
def test_split_channels_answers_for_the_second_tensor_at_the_same_address(engine, time_major):
    B, T = 3, 10
    a = np.zeros((B, T, 2), np.float32)
    a[..., 0] = np.arange(B * T, dtype=np.float32).reshape(B, T)
    a[..., 1] = 1.0e3
    x1 = torch.from_numpy(a)
    xv1, r1 = engine.split_channels(x1, True, time_major=time_major)
    want = (lambda c: torch.from_numpy(a[..., c].T.copy())) if time_major else (lambda c: torch.from_numpy(a[..., c].copy()))
    assert torch.equal(xv1, want(0)) and torch.equal(r1, want(1))
    a[..., 0] *= -1.0
    a[:, T // 2:, 1] = 4.0e3
    x2 = torch.from_numpy(a)
    assert same_key(x1, x2)
    xv2, r2 = engine.split_channels(x2, True, time_major=time_major)
    assert torch.equal(xv2, want(0)) and torch.equal(r2, want(1))
    # the same object again hits (the same copies), an in-place change misses
    xv3, _ = engine.split_channels(x2, True, time_major=time_major)
    assert xv3 is xv2
    x2.mul_(2.0)
    xv4, r4 = engine.split_channels(x2, True, time_major=time_major)
    assert torch.equal(xv4, want(0)) and torch.equal(r4, want(1)) and float(r4.max()) == 8.0e3


def test_resistance_max_min_answer_for_the_second_tensor_at_the_same_address(engine):
    a = np.full((4, 32), 1.0e3, np.float32)
    a[2, 5] = 9.0e4
    r1 = torch.from_numpy(a)
    assert engine.resistance_max(r1) == 9.0e4 and engine.resistance_min(r1) == 1.0e3
    a[:, :] = 5.0e3
    a[1, 7] = 300.0
    r2 = torch.from_numpy(a)
    assert same_key(r1, r2)
    assert engine.resistance_max(r2) == 5.0e3 and engine.resistance_min(r2) == 300.0
    r2.add_(1.0)                                               # in place: looked at again
    assert engine.resistance_max(r2) == 5.001e3 and engine.resistance_min(r2) == 301.0


def test_warmup_per_wave_answers_for_the_second_tensor_at_the_same_address():
    from wdf_hip import mlp_root
    C, fs = 33.0e-9, 48000.0
    a = np.full((8, 64), 1.0e3, np.float32)
    r1 = torch.from_numpy(a)
    W1, m1 = mlp_root.warmup_per_wave(r1, C, fs)
    a[4:, 10] = 1.0e5                                          # the second group of four sequences now has a slow memory
    r2 = torch.from_numpy(a)
    assert same_key(r1, r2)
    W2, m2 = mlp_root.warmup_per_wave(r2, C, fs)
    Wf, mf = mlp_root.warmup_per_wave(r2.clone(), C, fs)       # (a tensor no cache has seen)
    assert torch.equal(W2, Wf) and m2 == mf
    assert torch.equal(W2[:1], W1[:1]) and int(W2[1]) > int(W1[1]) and m2 > m1
    assert mlp_root.warmup_per_wave(r2, C, fs)[0] is W2        # the same object again hits
