"""GPU: Circuit.mse_esr(..., grad=False) on a resident MLP-root clipper through the loss-only evaluation pass
(lowering.MLP_EVAL_PASS_SERVES = True for the duration of each test; mlp_root.MlpEvalPass, csrc/wdf_mlp_eval.h).  The model and
the B = 48, T = 512 sets are tests/test_gpu_circuit_eval.py's.

  - the loss within that file's L_RTOL of the full step's at the same weights and within 2e-4 of tests/mlp_step_ref.py (float64);
    last_output is the entry's y buffer, or None with store_output=False; the training side of the entry is not advanced
  - six validation calls between training steps: the pass has committed six calls and starts its chunks from its own snapshots
  - training with a validation call per epoch -- on a second pair, and on the TRAINED pair itself -- ends at the weights, bit for
    bit, of training without it
  - with the flag off no pass is made"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mlp_step_ref as M
import test_gpu_circuit_eval as CE        # noqa: E402  (_mlp_setup, weights, detached, rel, L_RTOL)
import test_gpu_mlp_step as MS            # noqa: E402  (_clipper_pot_model)
import test_gpu_mlp_step_edges as ED      # noqa: E402  (warm_starts)

SKIP, FS = CE.SKIP, CE.FS


@pytest.fixture
def serves():
    from wdf_hip import lowering
    was = lowering.MLP_EVAL_PASS_SERVES
    lowering.MLP_EVAL_PASS_SERVES = True
    yield lowering
    lowering.MLP_EVAL_PASS_SERVES = was


def entry(circ, n=0):
    return list(circ._mlp.cache.values())[n]


def test_loss_and_buffers(serves):
    from wdf_hip import workload
    (xin, target), _ = CE._mlp_setup()
    wdf_, circ, model = MS._clipper_pot_model()
    circ.to_device()
    tv = model.trainable_variables
    w0 = CE.weights(tv)
    loss = circ.mse_esr(xin, target, SKIP, grad=False)
    CE.detached(loss)
    ent = entry(circ)
    st, ev = ent["st"], ent["eval"]
    assert ent["calls"] == 0 and ent["eval_calls"] == 1 and circ.last_output is st.y and ev.y is st.y
    assert st.read()[0]["calls"] == 0 and ev.read()[0]["calls"] == 1
    # the float64 reference at these weights
    x = xin.cpu().numpy()
    ref = M.run(x[:, :, 0], x[:, :, 1], circ._mlp.w.cpu().numpy(), st.hidden, st.n_layers, "tanh", target.cpu().numpy().reshape(512, 48), SKIP,
                C=float(np.float32(workload.C_CLIPPER)), fs=FS, grad=False)
    e_ref = abs(float(loss) - ref.loss) / ref.loss
    e_y = float(np.max(np.abs(st.y.cpu().numpy().astype(np.float64) - ref.y)))
    st.gw.fill_(-3.0)
    st.y.fill_(-7.25)
    loss2 = circ.mse_esr(xin, target, SKIP, grad=False, store_output=False)
    CE.detached(loss2)
    assert circ.last_output is None and bool((st.y == -7.25).all())
    assert bool((st.gw == -3.0).all()) and torch.equal(CE.weights(tv), w0) and ent["calls"] == 0 and ent["eval_calls"] == 2
    # the full step at the same weights
    with wdf_.tf.GradientTape():
        full = circ.mse_esr(xin, target, SKIP)
    e = CE.rel(loss, st.loss3[2])
    print(f"DIGEST circuit grad=False through the pass: {float(loss):.7e} against the full step's {float(st.loss3[2]):.7e}: rel {e:.2e} "
          f"(bound {CE.L_RTOL:.0e}); against float64 rel {e_ref:.2e} (bound 2e-04); y {e_y:.2e} (bound 1e-05); without y rel "
          f"{CE.rel(loss2, full):.2e}")
    assert e <= CE.L_RTOL and CE.rel(loss, full) <= CE.L_RTOL and CE.rel(loss2, full) <= CE.L_RTOL and ent["calls"] == 1
    assert e_ref <= 2e-4 and e_y <= 1e-5
    assert not bool((st.gw == -3.0).all())


def _train(validate_on, epochs=6):
    """clipper_pot.py:245-269: `epochs` of train step + Adam on the first pair; validate_on: None, 0 (the trained pair) or 1"""
    pairs = CE._mlp_setup()
    (xt, tt) = pairs[0]
    wdf_, circ, model = MS._clipper_pot_model()
    circ.to_device()
    tf = wdf_.tf
    opt = tf.keras.optimizers.Adam(learning_rate=1.0e-4, beta_1=0.5)
    tv = model.trainable_variables
    w_init = CE.weights(tv)
    for _ in range(epochs):
        with tf.GradientTape() as tape:
            loss = circ.mse_esr(xt, tt, SKIP)
        opt.apply_gradients(zip(tape.gradient(loss, tv), tv))
        if validate_on is not None:
            CE.detached(circ.mse_esr(*pairs[validate_on], SKIP, grad=False))
    end = CE.weights(tv)
    assert not torch.equal(end, w_init)
    return circ, end


def test_six_validation_calls_between_training_steps(serves):
    circ, _ = _train(1)
    ents = list(circ._mlp.cache.values())
    assert len(ents) == 2
    (tr,), (va,) = [e for e in ents if "eval" not in e], [e for e in ents if "eval" in e]
    assert tr["calls"] == 6 and va["calls"] == 0 and va["eval_calls"] == 6
    ev = va["eval"]
    info, wc = ev.read()
    assert info["calls"] == 6 and info["have_snap"] == 1 and va["st"].read()[0]["calls"] == 0
    starts = ED.warm_starts(ev, wc)
    print(f"DIGEST circuit six validation calls: {info} W {wc.tolist()} warm starts {starts}")
    assert any(t > 0 for t in starts)


@pytest.mark.parametrize("validate_on", [1, 0], ids=["different-pair", "same-pair"])
def test_training_is_bit_for_bit_what_it_is_without_the_validation_call(serves, validate_on):
    _, with_val = _train(validate_on)
    _, without = _train(None)
    assert torch.equal(with_val, without)


def test_flag_off_makes_no_pass():
    from wdf_hip import lowering
    was = lowering.MLP_EVAL_PASS_SERVES
    lowering.MLP_EVAL_PASS_SERVES = False
    try:
        (xin, target), _ = CE._mlp_setup()
        _, circ, _ = MS._clipper_pot_model()
        circ.to_device()
        CE.detached(circ.mse_esr(xin, target, SKIP, grad=False))
        ent = entry(circ)
        assert "eval" not in ent and "eval_out" in ent and circ.last_output is ent["st"].y
    finally:
        lowering.MLP_EVAL_PASS_SERVES = was
