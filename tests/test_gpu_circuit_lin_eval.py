"""GPU: Circuit.mse / mse_esr(..., grad=False) on a resident LINEAR tree through the loss-only evaluation pass
(csrc/wdf_ss_lin_eval.h: wdf_ss_lin_eval, _LinResident.eval_entry / evaluate) with lowering.LIN_EVAL_PASS_SERVES forced on, whatever
the committed flag is -- on tests/test_gpu_circuit_lin_esr.py's three circuits (the RC low-pass of lpf.py, the divider of
voltage_divider.py, a two-capacitor two-source ladder), each to_device(), at (B, T) = (70, 300), skip 50.

The pass is the training step without its tangents, so what it reports is held to the DEFAULT route (grad=True: wdf_ss_lin_step_mse /
wdf_ss_lin_step_esr) on a twin circuit BIT FOR BIT: the loss, last_output, last_state.  Against the forward's float64 composition the
loss is held to that module's bounds for this route: 2e-6 relative (and, where the loss has fallen by an order of magnitude over the
Adam steps, its stated wider bound for its stated reason: the 1.5e-7 by which two fp32 forward kernels differ in y weighs the more
the smaller y - target is), and to the float64 composition of the pass's own y within 32 x 2^-24 + 2^-23.
"""
import contextlib

import numpy as np
import pytest

import test_gpu_circuit_lin_esr as L

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B, T, SKIP = L.B, L.T, L.SKIP
CASES = L.CASES
KINDS = ["mse", "mse+esr"]


@pytest.fixture(scope="module")
def wdf():
    import tf_wdf
    from wdf_hip import binding
    binding.require_gpu()
    return tf_wdf


@contextlib.contextmanager
def serving(on):
    """the evaluation pass routed (or not), and the MSE + ESR step serving the default route as committed code has it"""
    from wdf_hip import lowering
    old = lowering.LIN_EVAL_PASS_SERVES
    lowering.LIN_EVAL_PASS_SERVES = on
    try:
        yield
    finally:
        lowering.LIN_EVAL_PASS_SERVES = old


def loss_of(circ, kind, x, target, **kw):
    return circ.mse(x, target, **kw) if kind == "mse" else circ.mse_esr(x, target, SKIP, **kw)


def bits(v):
    return np.float32(float(v)).tobytes()


_VAL = {}


def validation_pair(wdf, case):
    """a second (x, target) pair: other inputs, and a teacher whose values are all moved UP, by 12 %, 24 %, ... (theta_k (1 + 0.12 (k + 1))):
    the training pair's teacher has the low-pass's R up and its C down, the product nearly where it was, and a validation target of
    that kind would be fitted to nothing by the training itself -- the loss of few 1e-8 then measures the 1.5e-7 by which two fp32
    forward kernels differ, not this route"""
    if case not in _VAL:
        rng = np.random.default_rng(100 + CASES.index(case))
        x = L.cuda(rng.standard_normal((B, T, 2) if case == "ladder" else (B, T)) * 1.2)
        teacher, tv, _ = L.build(wdf, case)
        for k, v in enumerate(tv):
            v.assign(float(v) * (1.0 + 0.12 * (k + 1)))
        with torch.no_grad():
            _VAL[case] = (x, teacher(x).as_subclass(torch.Tensor).detach().clone())
    return _VAL[case]


def composition(y, target, kind):
    if kind == "mse":
        return ((y.as_subclass(torch.Tensor).double() - target.double()) ** 2).mean()
    return L.composition(y, target, SKIP)


def eval_entry_of(circ, x, target):
    return circ._lin.cache.get((x, target), ("eval",))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES)
def test_routing(wdf, case, kind):
    """detached, no gradient attached; loss and last_output the default call's on a twin, bit for bit; an entry of its own"""
    x, target = L.data(wdf, case)
    circ, tv, _ = L.resident(wdf, case)
    twin, _, _ = L.resident(wdf, case)
    with serving(True):
        loss = loss_of(circ, kind, x, target, grad=False)
    y = circ.last_output.clone()
    want = loss_of(twin, kind, x, target)
    assert not loss.requires_grad and loss.grad_fn is None and not hasattr(loss, "_wdf_fused") and hasattr(want, "_wdf_fused")
    assert isinstance(loss, wdf.tf.Tensor)
    assert bits(loss) == bits(want), (float(loss), float(want))
    assert tuple(y.shape) == (T, B) and torch.equal(y.view(torch.int32), twin.last_output.view(torch.int32))
    ent = eval_entry_of(circ, x, target)
    assert ent is not None and ent["y"] is not None and circ.last_output.data_ptr() == ent["y"].data_ptr()
    assert eval_entry_of(twin, x, target) is None
    assert circ._lin.cache.get((x, target), None if kind == "mse" else ("mse+esr", SKIP)) is None      # (no training entry was made)
    # against the forward's float64 composition, and against the composition of its own y
    with torch.no_grad():
        l0 = float(composition(circ(x), target, kind))
    own = float(composition(y, target, kind))
    print(f"FIG {case} {kind}: loss {float(loss):.7e} forward {abs(float(loss) - l0) / l0:.2e} own y {abs(float(loss) - own) / own:.2e}")
    assert abs(float(loss) - l0) <= L.LOSS_BOUND * l0 and abs(float(loss) - own) <= L.LOSS_OWN_BOUND * own


@pytest.mark.parametrize("case", CASES)
def test_without_the_output(wdf, case):
    x, target = L.data(wdf, case)
    circ, _, _ = L.resident(wdf, case)
    with serving(True):
        a = circ.mse_esr(x, target, SKIP, grad=False, store_output=False)
        assert circ.last_output is None
        ent = eval_entry_of(circ, x, target)
        assert ent is not None and ent["y"] is None
        m = circ.mse(x, target, grad=False, store_output=False)
        assert circ.last_output is None and ent["y"] is None
        b = circ.mse_esr(x, target, SKIP, grad=False)
        assert ent["y"] is not None and circ.last_output.data_ptr() == ent["y"].data_ptr() and eval_entry_of(circ, x, target) is ent
        m2 = circ.mse(x, target, grad=False)
    # (each call's loss sits in a row of its own: the first ones are still what they were)
    assert bits(a) == bits(b) and bits(m) == bits(m2) and float(a) > 0.0 and float(m) > 0.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["lpf", "ladder"])
def test_stateful_calls(wdf, case, kind):
    """three carry_state epochs, then an explicit z0: last_state, last_output and the loss are the default route's on a twin"""
    x, target = L.data(wdf, case)
    circ, _, _ = L.resident(wdf, case)
    twin, _, _ = L.resident(wdf, case)
    seen = []
    for epoch in range(3):
        with serving(True):
            loss = loss_of(circ, kind, x, target, carry_state=True, grad=False)
        want = loss_of(twin, kind, x, target, carry_state=True)
        assert not hasattr(loss, "_wdf_fused") and not loss.requires_grad
        assert bits(loss) == bits(want), (epoch, float(loss), float(want))
        assert tuple(circ.last_state.shape) == (circ.ns, B) and torch.equal(circ.last_state, twin.last_state), epoch
        assert torch.equal(circ.last_output, twin.last_output)
        seen.append((float(loss), circ.last_state.clone()))
    assert seen[0][0] != seen[1][0] and not torch.equal(seen[0][1], seen[1][1])          # (the state was handed on)
    with serving(True):
        again = loss_of(circ, kind, x, target, z0=seen[0][1], grad=False)
    want = loss_of(twin, kind, x, target, z0=seen[0][1])
    assert bits(again) == bits(want) and bits(again) == np.float32(seen[1][0]).tobytes()
    assert torch.equal(circ.last_state, twin.last_state) and torch.equal(circ.last_state, seen[1][1])
    assert eval_entry_of(twin, x, target) is None and eval_entry_of(circ, x, target) is not None


@pytest.mark.parametrize("case", CASES)
def test_training_undisturbed_by_validation_calls(wdf, case):
    """lpf.py's loop, six Adam steps on one pair, with a validation call of each kind on a second pair at every step (the first one
    carries the optimizer updates queued by the step before in its probe launch), against a twin that never validates: the same
    parameters and training losses, bit for bit; the validation losses within the route's bound of the float64 composition."""
    tf = wdf.tf
    x, target = L.data(wdf, case)
    xv, tv_ = validation_pair(wdf, case)
    runs = {}
    for name in ("validating", "twin"):
        circ, tv, lrs = L.resident(wdf, case)
        opts = [tf.keras.optimizers.Adam(learning_rate=lr) for lr in lrs]
        train, val = [], []
        for step in range(6):
            if name == "validating":
                with serving(True):
                    v2 = circ.mse_esr(xv, tv_, SKIP, grad=False)
                    y2 = circ.last_output.clone()
                    v1 = circ.mse(xv, tv_, grad=False)
                    y1 = circ.last_output.clone()
                with torch.no_grad():
                    yf = circ(xv)
                for kind, v, y in (("mse", v1, y1), ("mse+esr", v2, y2)):
                    l0, own = float(composition(yf, tv_, kind)), float(composition(y, tv_, kind))
                    val.append((kind, float(v), l0, own))
            with tf.GradientTape() as tape:
                loss = circ.mse_esr(x, target, SKIP)
            grads = tape.gradient(loss, tv)
            for o, g, v in zip(opts, grads, tv):
                o.apply_gradients([(g, v)])
            train.append(loss)                                    # (read after the loop: the queued updates stay queued for the next probe)
        runs[name] = ([bits(v) for v in train], [bits(v) for v in tv], val)
    assert runs["validating"][0] == runs["twin"][0] and runs["validating"][1] == runs["twin"][1]
    assert len(set(runs["validating"][0])) == 6
    val = runs["validating"][2]
    first = {kind: v for kind, v, _, _ in val[:2]}
    for i, (kind, v, l0, own) in enumerate(val):
        fallen = first[kind] >= 10.0 * v
        bound = max(L.LOSS_BOUND, 2.0 * L.LOSS_MEASURED.get((case, "adam"), 0.0)) if fallen else L.LOSS_BOUND
        print(f"FIG {case} step {i // 2} {kind}: validation loss {v:.7e} forward {abs(v - l0) / l0:.2e} (bound {bound:.1e}) own y {abs(v - own) / own:.2e}")
        assert abs(v - l0) <= bound * l0 and abs(v - own) <= L.LOSS_OWN_BOUND * own, (i, kind, v, l0, own)


@pytest.mark.parametrize("case", CASES)
def test_validation_on_the_training_pair(wdf, case):
    """a validation call on the pair that is being trained on leaves the training entry's workspace, ring turn and y untouched"""
    tf = wdf.tf
    x, target = L.data(wdf, case)
    circ, tv, _ = L.resident(wdf, case)
    twin, tw, _ = L.resident(wdf, case)
    for c in (circ, twin):
        c.mse(x, target)
    ent = circ._lin.cache.get((x, target), None)
    assert ent is not None and ent["y"] is not None
    before = (ent["ws"].clone(), ent["turn"], ent["y"].clone(), ent["y"].data_ptr(), ent["ring"].clone(), ent["ring"].data_ptr())
    with serving(True):
        for kind in KINDS:
            loss_of(circ, kind, x, target, grad=False)
            assert circ.last_output.data_ptr() != ent["y"].data_ptr()
    assert circ._lin.cache.get((x, target), None) is ent
    assert torch.equal(ent["ws"], before[0]) and ent["turn"] == before[1] and torch.equal(ent["y"].view(torch.int32), before[2].view(torch.int32))
    assert ent["y"].data_ptr() == before[3] and torch.equal(ent["ring"], before[4]) and ent["ring"].data_ptr() == before[5]
    with tf.GradientTape() as t1:
        a = circ.mse(x, target)
    with tf.GradientTape() as t2:
        b = twin.mse(x, target)
    assert bits(a) == bits(b) and [bits(g) for g in t1.gradient(a, tv)] == [bits(g) for g in t2.gradient(b, tw)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES)
def test_flag_off_the_old_route_gives_the_same_bits(wdf, case, kind):
    from wdf_hip import lowering
    x, target = L.data(wdf, case)
    on, _, _ = L.resident(wdf, case)
    off, _, _ = L.resident(wdf, case)
    with serving(True):
        a = loss_of(on, kind, x, target, grad=False)
    with serving(False):
        b = loss_of(off, kind, x, target, grad=False)
    assert not hasattr(b, "_wdf_fused") and not b.requires_grad
    assert bits(a) == bits(b) and torch.equal(on.last_output.view(torch.int32), off.last_output.view(torch.int32))
    assert eval_entry_of(off, x, target) is None and eval_entry_of(on, x, target) is not None
    assert isinstance(lowering.LIN_EVAL_PASS_SERVES, bool)
