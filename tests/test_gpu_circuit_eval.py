"""GPU: Circuit.mse / Circuit.mse_esr with grad=False ("I will not differentiate this loss") on resident circuits.

  the diode-pair clipper (to_device()), B = 128, T = 512 in two chunks (tests/test_gpu_circuit_no_y.py's circuit and data): the
  loss-only evaluation pass on an entry of its own
      - the loss within 2e-5 relative of the default call on a twin, last_output within Y_TOL, detached, no gradient attached
      - store_output=False: last_output None and an entry without a y buffer
      - the training entry's gradient buffer, sentinel-filled beforehand, unchanged
      - six epochs of train step + Adam with a grad=False validation call on a second pair: the trained values bit for bit those of
        a twin that never validates
  the MLP-root clipper (clipper_pot.py's model, B = 48, T = 512): forward and loss sums only
      - the loss within 2e-5 of the full step's at the same weights; st.gw (sentinel-filled) and the weights unchanged
      - a training loop with interleaved validation ends at the weights, bit for bit, of one without
  a resident linear tree and a resident diode-root tree: the default's value bit for bit, detached
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_circuit_lin_esr as CL     # noqa: E402  (linear circuits and data)
import test_gpu_circuit_no_y as NY        # noqa: E402  (the resident clipper, its data)
import test_gpu_mlp_step as MS            # noqa: E402  (_clipper_pot_model)
import test_gpu_ss_step as SS             # noqa: E402  (_hpf)
from test_gpu_circuit_no_y import wdf     # noqa: E402,F401  (fixture)

FS, SKIP = 48000.0, 50
Y_TOL, L_RTOL = 2.0e-6, 2.0e-5
cuda = NY.cuda


def call(circ, kind, x, target, **kw):
    return circ.mse(x, target, **kw) if kind == "mse" else circ.mse_esr(x, target, SKIP, **kw)


def detached(loss):
    assert isinstance(loss, torch.Tensor) and not loss.requires_grad and loss.grad_fn is None
    assert not hasattr(loss, "_wdf_fused")


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def eval_entries(circ):
    return [e for e in circ._res_cache.values() if len(e) == 4]


def train_entries(circ):
    return [e for e in circ._res_cache.values() if len(e) != 4]


@pytest.mark.parametrize("kind", ["mse", "mse_esr"])
def test_resident_clipper_grad_false(wdf, kind):
    from wdf_hip import binding as wb, engine, workload
    x, target = NY.clipper_data(wdf, 31)
    circ, tv = NY.clipper(wdf, workload.clipper_theta())
    twin, _ = NY.clipper(wdf, workload.clipper_theta())
    # a training entry on the same pair first; its gradient buffer gets a sentinel
    NY.loss_and_grads(wdf, circ, tv, x, target, kind)
    (tr,) = train_entries(circ)
    tr[0].out.fill_(-3.0)
    calls_before = tr[0].warm.info()["n_calls"]
    loss = call(circ, kind, x, target, grad=False)
    detached(loss)
    assert wb.tp_status(engine.LAST_TP_STATUS["status"])["n_bad"] == 0
    with wdf.tf.GradientTape():
        ref = call(twin, kind, x, target)
    e_l, e_y = rel(loss, ref), float((circ.last_output - twin.last_output).abs().max())
    print(f"FIG clipper {kind} grad=False: loss {float(loss):.7e} / {float(ref):.7e} rel {e_l:.2e}; |y - y'| {e_y:.2e}")
    assert e_l <= L_RTOL and e_y <= Y_TOL and tuple(circ.last_output.shape) == (512, 128)
    # its own entry; the training entry was never touched
    (ev,) = eval_entries(circ)
    assert len(train_entries(circ)) == 1 and ev[0] is not tr[0] and ev[0].warm is not tr[0].warm
    assert bool((tr[0].out == -3.0).all()) and tr[0].warm.info()["n_calls"] == calls_before
    # without the output: nothing left behind, and on a fresh circuit no y buffer at all
    loss2 = call(circ, kind, x, target, grad=False, store_output=False)
    detached(loss2)
    assert circ.last_output is None and rel(loss2, ref) <= L_RTOL
    fresh, _ = NY.clipper(wdf, workload.clipper_theta())
    loss3 = call(fresh, kind, x, target, grad=False, store_output=False)
    (ev3,) = eval_entries(fresh)
    assert fresh.last_output is None and ev3[0].y is None and not train_entries(fresh)
    assert rel(loss3, ref) <= L_RTOL
    # torch.no_grad() routes nothing: the default call inside it is the training step's code
    with torch.no_grad():
        call(fresh, kind, x, target)
    assert len(train_entries(fresh)) == 1


def test_resident_clipper_training_with_grad_false_validation(wdf):
    """clipper_pot.py:245-269: six epochs of train step + Adam, a grad=False validation call on a second pair each epoch; the twin
    does the same without the validation call."""
    from wdf_hip import workload
    tf = wdf.tf
    xt, tt = NY.clipper_data(wdf, 31)
    xv, tv_ = NY.clipper_data(wdf, 32)
    theta = workload.clipper_theta()
    ends, vals = [], []
    for validate in (True, False):
        circ, tv = NY.clipper(wdf, theta)
        opts = [tf.keras.optimizers.Adam(learning_rate=1.0e-3 * float(t)) for t in theta]
        for epoch in range(6):
            with tf.GradientTape() as tape:
                loss = circ.mse_esr(xt, tt, SKIP, store_output=False)
            grads = tape.gradient(loss, tv)
            for o, g, v in zip(opts, grads, tv):
                o.apply_gradients([(g, v)])
            if validate:
                val = circ.mse_esr(xv, tv_, SKIP, grad=False)
                detached(val)
                probe, _ = NY.clipper(wdf, [float(v) for v in tv])          # a default call at the same parameters
                want = probe.mse_esr(xv, tv_, SKIP)
                vals.append((float(val), float(want)))
                assert rel(val, want) <= L_RTOL, (epoch, vals[-1])
                assert float((circ.last_output - probe.last_output).abs().max()) <= Y_TOL
        ends.append([np.float32(float(v)).tobytes() for v in tv])
    print(f"FIG validation losses (grad=False / default): {vals}")
    assert ends[0] == ends[1]
    assert ends[0] != [np.float32(t).tobytes() for t in theta]


def _mlp_setup():
    from wdf_hip import workload, binding as wb
    B, T = 48, 512
    out = []
    for seed in (4, 5):
        x = workload.sweep_batch(B, T, seed=seed) * 0.6
        r = workload.dataset_resistance_batch(B, T)
        target, _, _ = wb.clipper_fwd(cuda(x), cuda(workload.clipper_theta()), FS, r=cuda(r), want_stash=False)
        out.append((cuda(np.stack([x, r], axis=-1)), target))
    return out


def weights(tv):
    return torch.cat([v.as_subclass(torch.Tensor).detach().reshape(-1) for v in tv]).clone()


def test_resident_mlp_clipper_grad_false():
    (xin, target), _ = _mlp_setup()
    wdf_, circ, model = MS._clipper_pot_model()
    circ.to_device()
    tv = model.trainable_variables
    w0 = weights(tv)
    loss = circ.mse_esr(xin, target, SKIP, grad=False)
    detached(loss)
    ent = next(iter(circ._mlp.cache.values()))
    st = ent["st"]
    assert ent["calls"] == 0 and circ.last_output is st.y
    st.gw.fill_(-3.0)
    loss = circ.mse_esr(xin, target, SKIP, grad=False)
    assert bool((st.gw == -3.0).all()) and torch.equal(weights(tv), w0) and ent["calls"] == 0
    # the full step at the same weights
    with wdf_.tf.GradientTape():
        full = circ.mse_esr(xin, target, SKIP)
    e = rel(loss, st.loss3[2])
    print(f"FIG mlp grad=False: {float(loss):.7e} against the full step's {float(st.loss3[2]):.7e}: rel {e:.2e}")
    assert e <= L_RTOL and rel(loss, full) <= L_RTOL and ent["calls"] == 1
    assert not bool((st.gw == -3.0).all())


def test_resident_mlp_clipper_training_with_grad_false_validation():
    (xt, tt), (xv, tv_) = _mlp_setup()
    ends = []
    for validate in (True, False):
        wdf_, circ, model = MS._clipper_pot_model()
        circ.to_device()
        tf = wdf_.tf
        opt = tf.keras.optimizers.Adam(learning_rate=1.0e-4, beta_1=0.5)
        tv = model.trainable_variables
        w_init = weights(tv)
        for _ in range(5):
            with tf.GradientTape() as tape:
                loss = circ.mse_esr(xt, tt, SKIP)
            opt.apply_gradients(zip(tape.gradient(loss, tv), tv))
            if validate:
                detached(circ.mse_esr(xv, tv_, SKIP, grad=False))
        ends.append(weights(tv))
        assert not torch.equal(ends[-1], w_init)
    assert torch.equal(ends[0], ends[1])


@pytest.mark.parametrize("kind", ["mse", "mse_esr"])
def test_other_resident_circuits_compute_as_with_the_default(wdf, kind):
    """A resident linear tree and a resident diode-root tree have no evaluation pass: the default's value, bit for bit, detached."""
    x, target = CL.data(wdf, "lpf")
    a, _, _ = CL.resident(wdf, "lpf")
    b, _, _ = CL.resident(wdf, "lpf")
    la = call(a, kind, x, target, grad=False)
    with wdf.tf.GradientTape():
        lb = call(b, kind, x, target)
    detached(la)
    assert hasattr(lb, "_wdf_fused")
    assert np.float32(float(la)).tobytes() == np.float32(float(lb)).tobytes()
    assert torch.equal(a.last_output, b.last_output)
    rng = np.random.default_rng(12)
    xh = cuda(rng.standard_normal((70, 300)) * 1.2)
    teacher, tvh = SS._hpf(wdf)
    for k, v in enumerate(tvh[:3]):
        v.assign(float(v) * (1.0 + 0.12 * (-1.0) ** k))
    with torch.no_grad():
        th = teacher(xh).as_subclass(torch.Tensor).detach().clone()
    out = []
    for grad in (False, True):
        circ, _ = SS._hpf(wdf)
        circ.to_device()
        with wdf.tf.GradientTape():
            loss = call(circ, kind, xh, th, grad=grad)
        if not grad:
            detached(loss)
        out.append(np.float32(float(loss)).tobytes())
    assert out[0] == out[1]
