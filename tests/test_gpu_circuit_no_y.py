"""GPU: Circuit.mse / Circuit.mse_esr with store_output=False ("I will not read y") on resident circuits.

  the diode-pair clipper (to_device()), B = 128, T = 512 in two chunks: the one-pass step without the y store
      - loss and tape.gradient of a twin circuit called with the default: G_RTOL = 1e-4 per component, loss 1e-5 relative
        (tests/test_gpu_fused_step.py's bounds for the step against its references)
      - last_output is None after the call, also directly after a storing call
      - a storing call on the same (x, target) afterwards leaves a y within Y_TOL = 2e-6 of circ(x): the pair's entry is shared
        and its y buffer made when first wanted, not handed over from anything else
      - a no-y training pair alternating with a storing validation pair: two entries, each warm after its first call
  the RC low-pass and the voltage divider (tests/test_gpu_circuit_lin_esr.py's circuits and data, B = 70, T = 300)
      - the same against the twin; carry_state=True over two epochs against the twin, and -- MSE + ESR on the low-pass -- against
        the composed path at that module's bounds (loss 2e-6, gradients GRAD_BOUND, last_state 3e-6)
  a circuit without a no-y kernel (the HPF diode-root tree): the storing call's loss and gradients bit for bit, last_output None
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_circuit_lin_esr as CL     # noqa: E402  (circuits, data, the composed path and its bounds)
import test_gpu_ss_step as SS             # noqa: E402  (_hpf)

FS = 48000.0
Y_TOL, G_RTOL, L_RTOL = 2.0e-6, 1.0e-4, 1.0e-5
SKIP = 50


@pytest.fixture(scope="module")
def wdf():
    import tf_wdf
    from wdf_hip import binding
    binding.require_gpu()
    return tf_wdf


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def loss_and_grads(wdf, circ, tv, x, target, kind, **kw):
    with wdf.tf.GradientTape() as tape:
        loss = circ.mse(x, target, **kw) if kind == "mse" else circ.mse_esr(x, target, SKIP, **kw)
    grads = tape.gradient(loss, tv)
    assert hasattr(loss, "_wdf_fused")
    return loss, np.array([float(g) for g in grads])


def agree(label, a, b, g_rtol=G_RTOL, l_rtol=L_RTOL):
    (la, ga), (lb, gb) = a, b
    e_l, e_g = abs(float(la) - float(lb)) / abs(float(lb)), np.abs(ga - gb) / np.abs(gb)
    print(f"FIG {label}: loss {float(la):.7e} / {float(lb):.7e} rel {e_l:.2e}; gradients rel {e_g}; bits equal: "
          f"{float(la) == float(lb) and np.array_equal(ga, gb)}")
    assert np.all(np.isfinite(ga)) and np.all(gb != 0.0)
    assert e_l <= l_rtol and e_g.max() <= g_rtol, (label, e_l, e_g)


# ---- the resident diode-pair clipper -----------------------------------------------------------------------------------------
def clipper(wdf, theta):
    from wdf_hip import engine
    Vs = wdf.ResistiveVoltageSource(float(theta[2]), trainable=True)
    Cap = wdf.Capacitor(float(theta[3]), int(FS), trainable=True)
    P1 = wdf.Parallel(Vs, Cap)
    dp = wdf.DiodePair(P1, float(theta[0]), Vt=float(theta[1]), trainable=True)
    circ = wdf.Circuit(P1, dp, Cap, time_parallel=engine.TpPlan(2, 128, 1.0e-6, 2))
    circ.to_device()
    return circ, [dp.Is, dp.nVt, Vs.R, Cap.C]


_CLIP = {}


def clipper_data(wdf, seed):
    from wdf_hip import workload
    if seed not in _CLIP:
        B, T = 128, 512
        x = cuda(workload.sweep_batch(B, T, seed=seed))
        teacher, _ = clipper(wdf, workload.target_theta())
        with torch.no_grad():
            _CLIP[seed] = (x, teacher(x).as_subclass(torch.Tensor).detach().clone())
    return _CLIP[seed]


def entries(circ):
    return list(circ._res_cache.values())


@pytest.mark.parametrize("kind", ["mse", "mse_esr"])
def test_resident_clipper_without_output(wdf, kind):
    from wdf_hip import binding as wb, engine, workload
    x, target = clipper_data(wdf, 31)
    noy, tv_n = clipper(wdf, workload.clipper_theta())
    twin, tv_t = clipper(wdf, workload.clipper_theta())
    a = loss_and_grads(wdf, noy, tv_n, x, target, kind, store_output=False)
    assert noy.last_output is None
    assert wb.tp_status(engine.LAST_TP_STATUS["status"])["n_bad"] == 0
    (st,) = [e[0] for e in entries(noy)]
    assert st.y is None                                          # no y buffer exists for the entry
    b = loss_and_grads(wdf, twin, tv_t, x, target, kind)
    assert twin.last_output is not None and tuple(twin.last_output.shape) == (512, 128)
    agree(f"clipper {kind}", a, b)
    # a storing call on the same pair afterwards: the same entry, its y made now, and right
    c = loss_and_grads(wdf, noy, tv_n, x, target, kind)
    assert len(entries(noy)) == 1 and entries(noy)[0][0] is st and st.y is not None
    y = noy.last_output.clone()
    with torch.no_grad():
        y_ref = noy(x).as_subclass(torch.Tensor)
    e_y = float((y - y_ref).abs().max())
    print(f"FIG clipper {kind}: y of the storing call behind a no-y call against circ(x): {e_y:.2e}")
    assert e_y <= Y_TOL
    agree(f"clipper {kind} storing behind no-y", c, b)
    # ... and directly after that storing call, a no-y call leaves no output behind
    d = loss_and_grads(wdf, noy, tv_n, x, target, kind, store_output=False)
    assert noy.last_output is None
    agree(f"clipper {kind} no-y behind storing", d, b)


def test_resident_clipper_training_without_and_validation_with_output(wdf):
    """clipper_pot.py:245-262's alternation: the training pair never asks for y, the validation pair does.  Two entries, each
    with its own warm-start state; no call after an entry's first runs cold (last_warm_tiles = -1), none misses a boundary."""
    from wdf_hip import binding as wb, engine, workload
    xt, tt = clipper_data(wdf, 31)
    xv, tv_ = clipper_data(wdf, 32)
    circ, tv = clipper(wdf, workload.clipper_theta())
    for epoch in range(4):
        loss_and_grads(wdf, circ, tv, xt, tt, "mse_esr", store_output=False)
        assert circ.last_output is None and wb.tp_status(engine.LAST_TP_STATUS["status"])["n_bad"] == 0
        with torch.no_grad():
            circ.mse_esr(xv, tv_, SKIP)
        assert circ.last_output is not None and wb.tp_status(engine.LAST_TP_STATUS["status"])["n_bad"] == 0
        ents = entries(circ)
        assert len(ents) == 2
        for e in ents:
            info = e[0].warm.info()
            assert info["n_calls"] == epoch + 1, info
            if epoch:
                assert info["last_warm_tiles"] >= 0 and info["valid"] >= 1, (epoch, info)
    train, val = entries(circ)
    assert train[0].y is None and val[0].y is not None
    with torch.no_grad():
        y_ref = circ(xv).as_subclass(torch.Tensor)
    assert float((circ.last_output - y_ref).abs().max()) <= Y_TOL


# ---- resident linear trees ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mse", "mse_esr"])
@pytest.mark.parametrize("case", ["lpf", "divider"])
def test_resident_linear_tree_without_output(wdf, case, kind):
    x, target = CL.data(wdf, case)
    noy, tv_n, _ = CL.resident(wdf, case)
    twin, tv_t, _ = CL.resident(wdf, case)
    a = loss_and_grads(wdf, noy, tv_n, x, target, kind, store_output=False)
    assert noy.last_output is None
    extra = (x, target) if kind == "mse" else (x, target, "mse+esr", SKIP)
    ent = noy._lin.entry(*extra, store_output=False)
    assert ent["y"] is None                                      # no y buffer exists for the entry
    b = loss_and_grads(wdf, twin, tv_t, x, target, kind)
    assert twin.last_output is not None
    agree(f"{case} {kind}", a, b)
    c = loss_and_grads(wdf, noy, tv_n, x, target, kind)          # the same entry, its y made now
    assert noy._lin.entry(*extra) is ent and ent["y"] is not None
    y = noy.last_output.clone()
    with torch.no_grad():
        y_ref = noy(x).as_subclass(torch.Tensor)
    e_y = float((y - y_ref).abs().max()) / max(1.0, float(y_ref.abs().max()))
    print(f"FIG {case} {kind}: y of the storing call behind a no-y call against circ(x): {e_y:.2e}")
    assert e_y <= CL.Y_BOUND
    agree(f"{case} {kind} storing behind no-y", c, b)
    d = loss_and_grads(wdf, noy, tv_n, x, target, kind, store_output=False)
    assert noy.last_output is None
    agree(f"{case} {kind} no-y behind storing", d, b)


@pytest.mark.parametrize("kind", ["mse", "mse_esr"])
def test_resident_low_pass_carries_its_state_without_output(wdf, kind):
    """carry_state=True over two epochs: against the twin called with the default and, for MSE + ESR, against the composed path
    handing last_state on, at tests/test_gpu_circuit_lin_esr.py's bounds for exactly that comparison."""
    case = "lpf"
    x, target = CL.data(wdf, case)
    noy, tv_n, _ = CL.resident(wdf, case)
    twin, tv_t, _ = CL.resident(wdf, case)
    ref_circ, ref_tv, _ = CL.resident(wdf, case)
    z = None
    for epoch in range(2):
        a = loss_and_grads(wdf, noy, tv_n, x, target, kind, carry_state=True, store_output=False)
        assert noy.last_output is None and tuple(noy.last_state.shape) == (noy.ns, CL.B)
        b = loss_and_grads(wdf, twin, tv_t, x, target, kind, carry_state=True)
        agree(f"lpf {kind} carry_state epoch {epoch}", a, b)
        e_z = float((noy.last_state - twin.last_state).abs().max()) / max(1.0, float(twin.last_state.abs().max()))
        assert e_z <= CL.Y_BOUND
        if kind == "mse_esr":
            l0, g0, _, zT = CL.composed(wdf, ref_circ, ref_tv, x, target, SKIP, z0=z)
            agree(f"lpf {kind} carry_state epoch {epoch} against the composed path", a, (l0, g0), g_rtol=CL.GRAD_BOUND[case], l_rtol=CL.LOSS_BOUND)
            z = zT.as_subclass(torch.Tensor).detach()
            assert float((noy.last_state - z).abs().max()) / max(1.0, float(z.abs().max())) <= CL.Y_BOUND
    assert noy._lin.entry(*((x, target) if kind == "mse" else (x, target, "mse+esr", SKIP)), store_output=False)["y"] is None


# ---- a circuit without a no-y kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mse", "mse_esr"])
def test_diode_root_tree_computes_as_with_the_default(wdf, kind):
    rng = np.random.default_rng(12)
    B, T = 70, 300
    x = cuda(rng.standard_normal((B, T)) * 1.2)
    teacher, tv = SS._hpf(wdf)
    for k, v in enumerate(tv[:3]):
        v.assign(float(v) * (1.0 + 0.12 * (-1.0) ** k))
    with torch.no_grad():
        target = teacher(x).as_subclass(torch.Tensor).detach().clone()
    out = {}
    for store in (True, False):
        circ, params = SS._hpf(wdf)
        circ.to_device()
        with wdf.tf.GradientTape() as tape:
            loss = circ.mse(x, target, store_output=store) if kind == "mse" else circ.mse_esr(x, target, SKIP, store_output=store)
        grads = tape.gradient(loss, params)
        if not store:
            assert circ.last_output is None
        elif kind == "mse":                                      # (the diode-root one-pass step: its y; mse_esr composes from circ(x))
            assert circ.last_output is not None
        out[store] = (np.float32(float(loss)).tobytes(), [np.float32(float(g)).tobytes() for g in grads])
    assert out[False] == out[True]
