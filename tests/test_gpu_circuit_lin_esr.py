"""GPU: Circuit.mse_esr on a resident LINEAR tree through the one-pass MSE + ESR step (csrc/wdf_ss_step.h: wdf_ss_lin_step_esr) --
Circuit._mse_esr_lin_step, and Circuit.mse_esr with lowering.LIN_ESR_STEP_SERVES patched on -- on three circuits, each to_device(),
at (B, T) = (70, 300), skip 50: the RC low-pass of lpf.py, the divider of voltage_divider.py (no state) and a two-capacitor
two-source ladder.  The targets come from a teacher with moved component values (theta (1 + 0.12 (-1)^k)).

Reference: the SAME circuit's forward y = circ(x) followed by the torch composition of mse + esr in float64 and tape.gradient (the
path Circuit.mse_esr takes with the flag off, in float64 behind y).
  loss                  2e-6 relative against that composition, in every test, with two stated exceptions:
                        - the RC low-pass's five Adam steps: Adam at lpf.py's learning rates takes the loss from 7.8e-5 to 7.3e-6 in
                          five steps, and the 1.5e-7 by which the two fp32 forward kernels differ in y weighs the more the smaller
                          the error y - target is.  Measured on one MI355X, step 0..4: 1.18e-6, 6.8e-7, 4.4e-7, 3.25e-6, 1.25e-5;
                          the bound there is 2 x the worst, 2.5e-5 (LOSS_MEASURED).  Divider and ladder: at most 1.1e-7, bound 2e-6.
                        - skip = T - 1, one row of 70 samples: 2e-6 + 2 d sqrt(n / S) + d sqrt(n / E), d = 3e-6 max(1, max |y|) --
                          what S and E (the reference's own, n = 70) move by when every y moves by the y bound.
                          Measured: 4.4e-6 (low-pass), 1.7e-8, 4.9e-7.
                        Wherever one of the two applies, and in the carry_state epochs, the loss is ALSO held to the float64
                        composition of the step's own y within 32 x 2^-24 + 2^-23 (the kernel's 32-addend fp32 sums, the result).
  last_output          3e-6 max(1, max |y|): two fp32 kernels on the same recursion
  component gradients   tests/test_gpu_circuit_loss.py's bound for its RC low-pass, 2 x max(measured there, 2^-23) = 2.4e-7 relative,
                        or 2 x what was measured HERE on one MI355X where that is larger (GRAD_MEASURED below: the step carries the
                        gradient forward in time with fp32 tangents, the reference sweeps backwards over a stash: two different
                        fp32 algorithms, not one kernel fed two roundings of dL/dy), never above 1e-4.
"""
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FS = 48000
B, T, SKIP = 70, 300, 50
EPS = float(np.finfo(float).eps)
ULP32 = 2.0 ** -23
# worst relative difference of a component gradient between the step and the composition, per circuit, measured on one MI355X over
# every test of this module that compares gradients (printed by each: run with -s)
GRAD_MEASURED = {"lpf": 2.09e-7, "divider": 8.0e-8, "ladder": 2.67e-6}     # (ladder: dLoss/dC_a in the second carry_state epoch)
GRAD_BOUND = {k: 2.0 * max(v, ULP32) for k, v in GRAD_MEASURED.items()}
assert all(v <= 1e-4 for v in GRAD_BOUND.values())
LOSS_BOUND, Y_BOUND = 2e-6, 3e-6
LOSS_OWN_BOUND = 32 * 2.0 ** -24 + 2.0 ** -23      # the kernel's 32-addend fp32 sums of positive terms, the float result
# worst relative difference of the loss from the forward's composition where it exceeds 2e-6 (see the docstring): bound 2 x that
LOSS_MEASURED = {("lpf", "adam"): 1.25e-5}


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


@pytest.fixture(scope="module")
def wdf():
    import tf_wdf
    from wdf_hip import binding
    binding.require_gpu()
    return tf_wdf


def build(wdf, case):
    """-> circuit (host-resident), its trainable Variables, the learning rate of each one's Adam (lpf.py:79-80)"""
    if case == "lpf":
        R1, C1 = wdf.Resistor(1000, True), wdf.Capacitor(1.0e-6, FS, True)
        return wdf.Circuit(wdf.Inverter(wdf.Series(R1, C1)), wdf.IdealVoltageSource(), C1), [R1.R, C1.C], [25.0, 1.0e-8]
    if case == "divider":
        R1, R2 = wdf.Resistor(2.0e3, True), wdf.Resistor(500.0, True)      # (voltage_divider.py's tree; R2 inside the [180, 1e6] the
        return wdf.Circuit(wdf.Inverter(wdf.Series(R1, R2)), wdf.IdealVoltageSource(), R1), [R1.R, R2.R], [25.0, 5.0]   # optimizer clips to)
    Ra = wdf.Resistor(1.0e3, True)
    Vr = wdf.ResistiveVoltageSource(2.2e3, trainable=True)
    Ca, Cb = wdf.Capacitor(1.0e-7, FS, True), wdf.Capacitor(2.2e-7, FS, True)
    top = wdf.Inverter(wdf.Series(Ra, wdf.Parallel(Ca, wdf.Series(Vr, Cb))))
    return wdf.Circuit(top, wdf.IdealVoltageSource(), Cb), [Ra.R, Vr.R, Ca.C, Cb.C], [25.0, 25.0, 1.0e-9, 1.0e-9]


CASES = ["lpf", "divider", "ladder"]
_DATA = {}


def data(wdf, case):
    """x [B,T] ([B,T,2] for the ladder) and the teacher's output [T,B], made once per case"""
    if case not in _DATA:
        rng = np.random.default_rng(CASES.index(case))
        x = cuda(rng.standard_normal((B, T, 2) if case == "ladder" else (B, T)) * 1.2)
        teacher, tv, _ = build(wdf, case)
        for k, v in enumerate(tv):
            v.assign(float(v) * (1.0 + 0.12 * (-1.0) ** k))
        with torch.no_grad():
            _DATA[case] = (x, teacher(x).as_subclass(torch.Tensor).detach().clone())
    return _DATA[case]


def resident(wdf, case):
    circ, tv, lrs = build(wdf, case)
    circ.to_device()
    assert circ._lin is not None and (circ.ns, circ.ni) == {"lpf": (1, 1), "divider": (0, 1), "ladder": (2, 2)}[case]
    return circ, tv, lrs


def composition(y, target, skip):
    o = y.as_subclass(torch.Tensor)[skip:].double()
    t = target[skip:].double()
    S, E = ((o - t) ** 2).sum(), (o * o).sum() + EPS
    n = float(o.numel())
    return S / n + torch.sqrt(S / E / n)


def composed(wdf, circ, tv, x, target, skip, **state):
    """loss (float64), gradients and y of the composed path on this circuit at its present component values"""
    with wdf.tf.GradientTape() as tape:
        if state:
            y, zT = circ(x, return_state=True, **state)
        else:
            y, zT = circ(x), None
        loss = composition(y, target, skip)
    grads = np.array([float(g) for g in tape.gradient(loss, tv)])
    return float(loss), grads, y.as_subclass(torch.Tensor).detach(), zT


@contextlib.contextmanager
def serving(on):
    from wdf_hip import lowering
    old = lowering.LIN_ESR_STEP_SERVES
    lowering.LIN_ESR_STEP_SERVES = on
    try:
        yield
    finally:
        lowering.LIN_ESR_STEP_SERVES = old


def one_row_bound(y0, target, skip):
    """the derived bound of the docstring for a loss of few samples, from the reference's own S, E, n"""
    o, t = y0[skip:].double(), target[skip:].double()
    S, E, n = float(((o - t) ** 2).sum()), float((o * o).sum()) + EPS, float(o.numel())
    d = Y_BOUND * max(1.0, float(y0.abs().max()))
    return LOSS_BOUND + 2.0 * d * np.sqrt(n / S) + d * np.sqrt(n / E)


def compare(case, label, loss, grads, y, ref, own=None, loss_bound=LOSS_BOUND):
    """The step's loss, y and gradients against the composed path `ref`; the loss within loss_bound of the forward's composition
    (2e-6 unless the caller states another: see the docstring) and, with own = (target, skip), ALSO within LOSS_OWN_BOUND of the
    float64 composition of the step's own y."""
    l0, g0, y0, _ = ref
    rel = np.abs(grads - g0) / np.abs(g0)
    e_y = float((y - y0).abs().max()) / max(1.0, float(y0.abs().max()))
    e_l = abs(float(loss) - l0) / l0
    e_own = 0.0
    if own is not None:
        lo = float(composition(y, own[0], own[1]))
        e_own = abs(float(loss) - lo) / lo
    print(f"FIG {case} {label}: loss {float(loss):.7e} / {l0:.7e} rel {e_l:.2e} (bound {loss_bound:.2e}), against its own y {e_own:.2e}; "
          f"y {e_y:.2e}; grads {grads} / {g0} rel {rel} worst {rel.max():.3e}")
    assert np.all(np.isfinite(grads)) and np.all(g0 != 0.0)
    assert e_l <= loss_bound and e_own <= LOSS_OWN_BOUND, (e_l, loss_bound, e_own)
    assert e_y <= Y_BOUND and rel.max() <= GRAD_BOUND[case], (e_y, rel, GRAD_BOUND[case])


@pytest.mark.parametrize("via", ["method", "routed"])
@pytest.mark.parametrize("case", CASES)
def test_step_against_the_forward_and_the_float64_composition(wdf, case, via):
    tf = wdf.tf
    x, target = data(wdf, case)
    circ, tv, _ = resident(wdf, case)
    with tf.GradientTape() as tape:
        if via == "method":
            loss = circ._mse_esr_lin_step(x, target, SKIP)
        else:
            with serving(True):
                loss = circ.mse_esr(x, target, SKIP)
    assert hasattr(loss, "_wdf_fused")                            # (fails without the feature: the composed path has no such gradient)
    grads = np.array([float(g) for g in tape.gradient(loss, tv)])
    y = circ.last_output.clone()
    assert tuple(y.shape) == (T, B)
    compare(case, via, loss, grads, y, composed(wdf, circ, tv, x, target, SKIP))
    # the call's own result row: {0, g[n], mse, esr, mse + esr, S, E, gP[n], gQ[n]}
    n = len(tv)
    row = circ._lin.entry(x, target, "mse+esr", SKIP)["row"].cpu().numpy().astype(np.float64)
    o, t = y[SKIP:].double(), target[SKIP:].double()
    S, E_ = float(((o - t) ** 2).sum()), float((o * o).sum())
    assert row.size == 6 + 3 * n and row[0] == 0.0 and np.array_equal(np.sort(row[1:1 + n].astype(np.float32)), np.sort(grads.astype(np.float32)))       # (tree order)
    assert row[3 + n] == float(loss) and abs(row[4 + n] - S) <= LOSS_OWN_BOUND * S and abs(row[5 + n] - E_) <= LOSS_OWN_BOUND * E_
    assert abs(row[1 + n] - S / o.numel()) <= LOSS_OWN_BOUND * S / o.numel()


@pytest.mark.parametrize("case", CASES)
def test_five_adam_steps_follow_the_composed_path_at_each_steps_parameters(wdf, case):
    """lpf.py:86-99's loop with one optimizer per component: the step's loss and gradients (the queued updates of the step before
    ride in its probe launch), then the composed path on the same circuit at the same values, then Adam on the step's gradients"""
    tf = wdf.tf
    x, target = data(wdf, case)
    circ, tv, lrs = resident(wdf, case)
    opts = [tf.keras.optimizers.Adam(learning_rate=lr) for lr in lrs]
    start = [float(v) for v in tv]
    losses = []
    for step in range(5):
        with tf.GradientTape() as tape:
            with serving(True):
                loss = circ.mse_esr(x, target, SKIP)
        grads = tape.gradient(loss, tv)
        assert hasattr(loss, "_wdf_fused")
        y = circ.last_output.clone()
        print(f"FIG {case} step {step}: component values {[float(v) for v in tv]}")
        compare(case, f"step {step}", loss, np.array([float(g) for g in grads]), y, composed(wdf, circ, tv, x, target, SKIP), own=(target, SKIP),
                loss_bound=max(LOSS_BOUND, 2.0 * LOSS_MEASURED.get((case, "adam"), 0.0)))
        for o, g, v in zip(opts, grads, tv):
            o.apply_gradients([(g, v)])
        losses.append(float(loss))
    assert all(float(v) != s for v, s in zip(tv, start)) and losses[-1] < losses[0]


@pytest.mark.parametrize("case", ["lpf", "ladder"])
def test_three_carry_state_epochs_against_the_composed_path_handing_last_state_on(wdf, case):
    x, target = data(wdf, case)
    circ, tv, _ = resident(wdf, case)
    ref_circ, ref_tv, _ = resident(wdf, case)
    z = None
    first = None
    for epoch in range(3):
        with wdf.tf.GradientTape() as tape:
            with serving(True):
                loss = circ.mse_esr(x, target, SKIP, carry_state=True)
        grads = np.array([float(g) for g in tape.gradient(loss, tv)])
        assert hasattr(loss, "_wdf_fused") and tuple(circ.last_state.shape) == (circ.ns, B)
        ref = composed(wdf, ref_circ, ref_tv, x, target, SKIP, z0=z)
        compare(case, f"epoch {epoch}", loss, grads, circ.last_output.clone(), ref, own=(target, SKIP))
        zT = ref[3].as_subclass(torch.Tensor).detach()
        e_z = float((circ.last_state - zT).abs().max()) / max(1.0, float(zT.abs().max()))
        print(f"FIG {case} epoch {epoch}: last_state {e_z:.2e}")
        assert e_z <= Y_BOUND
        z = zT
        first = (float(loss), circ.last_state.clone()) if first is None else first
    # an explicit z0 is the same hand-over as carry_state; reset_state() forgets it
    with serving(True):
        assert float(loss) != first[0]
        again = circ.mse_esr(x, target, SKIP, z0=first[1])
        second = circ.last_output.clone()
        circ.reset_state()
        fresh = circ.mse_esr(x, target, SKIP, carry_state=True)
    assert float(fresh) == first[0] and torch.equal(circ.last_state, first[1]) and hasattr(again, "_wdf_fused")
    ref2 = composed(wdf, ref_circ, ref_tv, x, target, SKIP, z0=first[1])
    assert float((second - ref2[2]).abs().max()) <= Y_BOUND * max(1.0, float(ref2[2].abs().max()))


@pytest.mark.parametrize("case", CASES)
def test_skip_at_the_last_row_and_past_it(wdf, case):
    """skip = T - 1: one row of loss, through the step.  skip = T: no row at all -- the branch does not take it, and mse_esr does
    with the flag on exactly what it does with the flag off (the composed path on an empty slice)"""
    tf = wdf.tf
    x, target = data(wdf, case)
    circ, tv, _ = resident(wdf, case)
    with tf.GradientTape() as tape:
        with serving(True):
            loss = circ.mse_esr(x, target, T - 1)
    assert hasattr(loss, "_wdf_fused")
    grads = np.array([float(g) for g in tape.gradient(loss, tv)])
    ref = composed(wdf, circ, tv, x, target, T - 1)
    compare(case, "skip = T - 1", loss, grads, circ.last_output.clone(), ref, own=(target, T - 1), loss_bound=one_row_bound(ref[2], target, T - 1))

    def past(on):
        with serving(on):
            try:
                out = circ.mse_esr(x, target, T)
                return ("value", hasattr(out, "_wdf_fused"), np.float32(float(out)).tobytes())
            except Exception as exc:                              # noqa: BLE001  (whatever the composed path does, both must do)
                return ("raises", type(exc).__name__)

    on, off = past(True), past(False)
    assert on == off and (on[0] == "raises" or on[1] is False), (on, off)
    with pytest.raises(Exception):
        circ._mse_esr_lin_step(x, target, T)


@pytest.mark.parametrize("case", CASES)
def test_with_the_flag_off_mse_esr_is_the_composed_path(wdf, case):
    from wdf_hip import lowering
    x, target = data(wdf, case)
    circ, tv, _ = resident(wdf, case)
    with serving(False):
        with wdf.tf.GradientTape() as tape:
            loss = circ.mse_esr(x, target, SKIP)
        grads = np.array([float(g) for g in tape.gradient(loss, tv)])
    assert not hasattr(loss, "_wdf_fused")
    l0, g0, _, _ = composed(wdf, circ, tv, x, target, SKIP)
    assert abs(float(loss) - l0) <= 2e-5 * l0 and np.max(np.abs(grads - g0) / np.abs(g0)) <= 1e-4       # (tests/test_gpu_ss_step.py's bound for this path's fp32 sums)
    assert isinstance(lowering.LIN_ESR_STEP_SERVES, bool)
