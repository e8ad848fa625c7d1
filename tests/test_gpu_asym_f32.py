"""GPU: the exact two-different-diode root solved in fp32 (WDF_ASYM_NEWTON_F32), kernel to tf_wdf.Circuit.

Reference everywhere: the oracle's exact fp64 solve at the fp32-rounded parameters (as tests/test_gpu_asym.py).  The
bounds are the ones the project holds the fp64 Newton mode to -- roots 2e-6 V (dominated by Rp being formed in fp32), y
3e-6 V, gradient 2e-4 relative against fp64 central differences -- because the point of the mode is fp64-mode accuracy at
fp32 cost.  An emulation with every operation rounded to fp32 gives 3.4e-7 V at the roots and 2.1e-7 V on y.

Parameter sets {Is_up, nVt_up, Is_down, nVt_down, R, C}: the 1N4148 / germanium-like pair of tests/test_gpu_asym.py, the
same swapped, a leaky diode on a small resistance (the closed-form start value is 353 mV off: 8 Newton iterations) and a
Schottky-like diode against a nearly ideal one on a large resistance (188 mV, 6 iterations)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FS = 48000.0
VT = 25.85e-3
THETA6 = np.array([4.352e-9, VT * 1.906, 2.0e-6, VT * 1.4, 45.0e3, 4.7e-9])
SETS = {
    "theta6": THETA6,
    "swapped": THETA6[[2, 3, 0, 1, 4, 5]],
    "leaky_low_R": np.array([1.0e-4, VT * 1.0, 4.352e-9, VT * 1.906, 10.0e3, 4.7e-9]),
    "schottky_big_R": np.array([1.0e-5, VT * 1.05, 1.0e-12, VT * 1.2, 99.1e3, 1.0e-9]),
}
NAMES = list(SETS)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def r32(theta):
    return np.asarray(theta).astype(np.float32).astype(np.float64)


def status(st):
    from wdf_hip import binding as wb
    return wb.mlp_tp_status(st)


def fd_grad(oracle, theta, x, gy):
    """fp64 central differences (relative step 1e-6) of L = sum(y gy) through the oracle's exact forward"""
    t32 = r32(theta)
    x64, g64 = x.astype(np.float64), gy.astype(np.float64)
    ref = np.zeros(6)
    for i in range(6):
        h = 1e-6 * t32[i]
        tp, tm = t32.copy(), t32.copy()
        tp[i] += h
        tm[i] -= h
        ref[i] = (np.sum(oracle.clipper_asym_fwd(tp, FS, x64) * g64) - np.sum(oracle.clipper_asym_fwd(tm, FS, x64) * g64)) / (2 * h)
    return ref


@pytest.mark.parametrize("name", NAMES)
def test_roots_vs_oracle(oracle, name):
    from wdf_hip import binding as wb
    theta = SETS[name]
    t32 = r32(theta)
    Rp = 1.0 / (1.0 / t32[4] + 2.0 * t32[5] * FS)
    a = np.concatenate([np.linspace(-6, 6, 2001), np.linspace(-0.05, 0.05, 501)]).astype(np.float32)
    ref = oracle.asym_root(a.astype(np.float64), Rp, t32[0], t32[1], t32[2], t32[3])
    b = wb.asym_root(dev(a), dev(theta), FS, wb.ASYM_NEWTON_F32, tol=1e-12, max_iter=50).cpu().numpy()
    err = float(np.max(np.abs(b - ref)))
    print(f"roots {name}: max |b - oracle| = {err:.3e} V")
    assert err < 2e-6, err


@pytest.mark.parametrize("B,T", [(70, 600), (256, 2048)])
@pytest.mark.parametrize("name", NAMES)
def test_forward_vs_oracle(oracle, name, B, T):
    """Sequential kernel at the API's default tolerance 1e-12, which fp32 cannot meet: the floor 4 FLT_EPSILON is what
    keeps the mean iteration count per step at 3..8 instead of max_iter = 50."""
    from wdf_hip import binding as wb, workload
    theta = SETS[name]
    x = workload.sweep_batch(B, T, seed=B)
    ref = oracle.clipper_asym_fwd(r32(theta), FS, x.astype(np.float64))
    y, zT, it = wb.clipper_asym_fwd(dev(x), dev(theta), FS, wb.ASYM_NEWTON_F32, tol=1e-12, max_iter=50, want_zT=True, want_iters=True)
    err = float(np.max(np.abs(y.cpu().numpy() - ref)))
    mean_iters = float(it.sum()) / (it.numel() * T)
    print(f"forward {name} {B}x{T}: max |y - oracle| = {err:.3e} V, mean Newton iterations per step = {mean_iters:.2f}")
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(zT).all())
    assert err < 3e-6, err
    assert 1.0 <= mean_iters <= 12.0, mean_iters


def test_identical_diodes_vs_oracle(oracle):
    """down = up: still the exact pair (eqn 39, the symmetric kernel's root, differs from it by about Rp Is)"""
    from wdf_hip import binding as wb, workload
    th = THETA6.copy()
    th[2:4] = th[0:2]
    x = workload.sweep_batch(70, 600, seed=70)
    ref = oracle.clipper_asym_fwd(r32(th), FS, x.astype(np.float64))
    y, _, _ = wb.clipper_asym_fwd(dev(x), dev(th), FS, wb.ASYM_NEWTON_F32, tol=1e-12, max_iter=50)
    err = float(np.max(np.abs(y.cpu().numpy() - ref)))
    print(f"identical diodes: max |y - oracle| = {err:.3e} V")
    assert err < 3e-6, err


@pytest.mark.parametrize("B,T,K,W", [(70, 1000, 4, 192), (256, 2048, 8, 192), (64, 4096, 16, 192), (5, 130, 2, 64)])
def test_time_parallel_forward_equals_sequential(B, T, K, W):
    from wdf_hip import binding as wb, workload
    mode = wb.ASYM_NEWTON_F32
    x = dev(workload.sweep_batch(B, T, seed=B + T))
    th = dev(THETA6)
    z0 = dev(np.random.default_rng(B).uniform(-0.2, 0.2, B))
    y, zT, _, zs = wb.clipper_asym_fwd(x, th, FS, mode, tol=1e-12, max_iter=50, z0=z0, want_zT=True, want_stash=True)
    y2, zT2, zs2, st = wb.clipper_asym_fwd_tp(x, th, FS, mode, K, W, tol=1e-12, max_iter=50, z0=z0, want_zT=True, want_stash=True)
    s = status(st)
    ey, es, ez = float((y2 - y).abs().max()), float((zs2 - zs).abs().max()), float((zT2 - zT).abs().max())
    print(f"chunks {B}x{T} K={K} W={W}: status {s}, |dy| = {ey:.3e}, |dstash| = {es:.3e}, |dzT| = {ez:.3e}")
    assert s["n_bad"] == 0 and s["gated_waves"] == 0, s
    assert ey <= 1e-6 and es <= 2e-6 and ez <= 2e-6


def test_time_parallel_forward_repairs_a_short_warmup():
    """A warm-up of 8 steps cannot work: every wave is gated and the gated sequential launch restores the sequential result,
    bit for bit."""
    from wdf_hip import binding as wb, workload
    B, T = 130, 2048
    x = dev(workload.sweep_batch(B, T, seed=3))
    th = dev(THETA6)
    y, _, _, zs = wb.clipper_asym_fwd(x, th, FS, wb.ASYM_NEWTON_F32, want_stash=True)
    y2, _, zs2, st = wb.clipper_asym_fwd_tp(x, th, FS, wb.ASYM_NEWTON_F32, 8, 8, want_stash=True)
    s = status(st)
    print(f"repair: status {s}")
    assert s["n_bad"] > 0 and s["gated_waves"] == 3, s
    assert torch.equal(y2, y) and torch.equal(zs2, zs)


@pytest.mark.parametrize("name", ["theta6", "leaky_low_R"])
def test_gradient_vs_oracle_finite_differences(oracle, name):
    """dL/dtheta6 of L = sum(y gy) through engine.clipper_asym(mode = ASYM_NEWTON_F32): the exact pair differentiated
    implicitly at the root the fp32 forward stored, against fp64 central differences of the oracle's forward."""
    from wdf_hip import binding as wb, engine, workload
    theta = SETS[name]
    B, T = 70, 600
    x = workload.sweep_batch(B, T, seed=3)
    gy = (np.random.default_rng(0).standard_normal((T, B)) / (B * T)).astype(np.float32)
    ref = fd_grad(oracle, theta, x, gy)
    th = dev(theta).requires_grad_(True)
    y = engine.clipper_asym(th, dev(x), FS, mode=wb.ASYM_NEWTON_F32)
    (y * dev(gy)).sum().backward()
    got = th.grad.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref) / np.abs(ref)
    print(f"gradient {name}: relative error per component vs finite differences = {err}")
    assert np.max(err) < 2e-4, (got, ref, err)
    y1, _, _ = wb.clipper_asym_fwd(dev(x), dev(theta), FS, wb.ASYM_NEWTON_F32, tol=1e-12)
    assert torch.equal(y.detach(), y1)
    # forward in verified time chunks, reverse sweep in one
    th2 = dev(theta).requires_grad_(True)
    y2 = engine.clipper_asym(th2, dev(x), FS, tp=engine.TpPlan(3, 192, 1e-6, 1), mode=wb.ASYM_NEWTON_F32)
    (y2 * dev(gy)).sum().backward()
    s = status(engine.LAST_TP_STATUS["status"])
    err2 = np.abs(th2.grad.cpu().numpy() - got) / np.abs(got)
    print(f"gradient {name}, 3 forward chunks: status {s}, relative to the sequential forward's = {err2}")
    assert s["n_bad"] == 0 and s["gated_waves"] == 0, s
    assert float((y2.detach() - y1).abs().max()) <= 1e-6
    assert np.max(err2) < 2e-5
    # k_bwd = 0 asks for the sequential sweep, which is fp64-only: this mode runs the exact sweep as one chunk
    th3 = dev(theta).requires_grad_(True)
    y3 = engine.clipper_asym(th3, dev(x), FS, tp=engine.TpPlan(1, 192, 1e-6, 0), mode=wb.ASYM_NEWTON_F32)
    (y3 * dev(gy)).sum().backward()
    assert np.max(np.abs(th3.grad.cpu().numpy() - got) / np.abs(got)) < 2e-5


def test_reverse_sweep_chunk_counts_agree():
    from wdf_hip import binding as wb, workload
    B, T = 256, 2048
    x = dev(workload.sweep_batch(B, T, seed=B + T))
    th = dev(THETA6)
    gy = dev(np.random.default_rng(1).standard_normal((T, B)) / (B * T))
    y, zT, _, zs = wb.clipper_asym_fwd(x, th, FS, wb.ASYM_NEWTON_F32, tol=1e-12, want_zT=True, want_stash=True)
    g = {K: wb.clipper_asym_bwd_tp(x, th, FS, wb.ASYM_NEWTON_F32, zs, zT, gy, K).cpu().numpy().astype(np.float64) for K in (1, 5, 16)}
    for K in (5, 16):
        err = np.max(np.abs(g[K] - g[1]) / np.abs(g[1]))
        print(f"reverse sweep K={K} vs K=1: {err:.3e}")
        assert err < 2e-5, (K, g[K], g[1])


def test_state_in_and_out(oracle):
    from wdf_hip import binding as wb, engine, workload
    B, T = 70, 600
    x = dev(workload.sweep_batch(B, T, seed=9))
    th = dev(THETA6)
    y = engine.clipper_asym(th, x, FS, mode=wb.ASYM_NEWTON_F32)
    h = T // 2
    ya, z = engine.clipper_asym(th, x[:, :h].contiguous(), FS, mode=wb.ASYM_NEWTON_F32, return_state=True)
    yb, zT = engine.clipper_asym(th, x[:, h:].contiguous(), FS, mode=wb.ASYM_NEWTON_F32, z0=z, return_state=True)
    assert z.shape == (B,) and not z.requires_grad and not zT.requires_grad
    ea, eb = float((ya - y[:h]).abs().max()), float((yb - y[h:]).abs().max())
    print(f"state in/out: first half {ea:.3e}, second half {eb:.3e}")
    assert ea <= 1e-6 and eb <= 1e-6
    # z0 is a constant of the call: the gradient reaches theta6 and nothing flows into z0
    thg = dev(THETA6).requires_grad_(True)
    zg = z.clone().requires_grad_(True)
    yc = engine.clipper_asym(thg, x[:, h:].contiguous(), FS, mode=wb.ASYM_NEWTON_F32, z0=zg)
    yc.sum().backward()
    assert zg.grad is None and bool(torch.isfinite(thg.grad).all())
    # the default mode took the same two arguments
    yd, zd = engine.clipper_asym(th, x[:, h:].contiguous(), FS, z0=z, return_state=True)
    assert float((yd - y[h:]).abs().max()) <= 3e-6 and float((zd - zT).abs().max()) <= 3e-6


def build_circuit(theta, solver="newton_f32", trainable=True, **kw):
    import tf_wdf as W
    Is1, V1, Is2, V2, R, Cv = [float(t) for t in theta]
    Vs = W.ResistiveVoltageSource(R, trainable=trainable)
    Cap = W.Capacitor(Cv, FS, trainable=trainable)
    P1 = W.Parallel(Vs, Cap)
    dp = W.AsymDiodePair(P1, Is1, Is2, Vt=1.0, nDiodes_up=V1, nDiodes_down=V2, trainable=trainable, solver=solver)
    return W, W.Circuit(P1, dp, Cap, **kw), [dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down, Vs.R, Cap.C]


def test_element_and_circuit(oracle):
    from wdf_hip import binding as wb, engine, workload
    B, T = 70, 600
    x = workload.sweep_batch(B, T, seed=5)
    xd = dev(x)
    W, circ, variables = build_circuit(THETA6, time_parallel=None)
    tf = W.tf
    th = torch.tensor([float(v) for v in variables], dtype=torch.float32, device="cuda")
    y_eng = engine.clipper_asym(th, xd, FS, mode=wb.ASYM_NEWTON_F32)
    gy = (np.random.default_rng(4).standard_normal((T, B)) / (B * T)).astype(np.float32)
    with tf.GradientTape() as tape:
        y = circ(xd)
        loss = tf.reduce_sum(y * dev(gy))
    grads = tape.gradient(loss, variables)
    assert torch.equal(y.as_subclass(torch.Tensor).detach(), y_eng)
    got = np.array([float(g) for g in grads])
    ref = fd_grad(oracle, th.cpu().numpy(), x, gy)
    err = np.abs(got - ref) / np.abs(ref)
    print(f"Circuit gradient: relative error per variable vs finite differences = {err}")
    assert np.max(err) < 2e-4, (got, ref, err)
    # the planned time chunks
    Bp, Tp = 256, 2048
    xp = dev(workload.sweep_batch(Bp, Tp, seed=6))
    _, circ_auto, _ = build_circuit(THETA6, time_parallel="auto")
    assert engine.plan_asym_time_parallel(Bp, Tp, THETA6[4], THETA6[5], FS).k_fwd > 1
    ya = circ_auto(xp)
    s = status(engine.LAST_TP_STATUS["status"])
    ys = circ(xp)
    ea = float((ya - ys).abs().max())
    print(f"Circuit auto plan: status {s}, |y - sequential| = {ea:.3e}")
    assert s["n_bad"] == 0 and s["gated_waves"] == 0, s
    assert ea <= 1e-6
    # an explicit plan is used as given
    _, circ_plan, _ = build_circuit(THETA6, time_parallel=engine.TpPlan(4, 192, 1e-6, 2))
    assert float((circ_plan(xp) - ys).abs().max()) <= 1e-6
    # mse(): the forward plus the torch loss
    target = dev(np.random.default_rng(7).standard_normal((T, B)) * 0.1)
    m = float(circ.mse(xd, target))
    m_ref = float(torch.mean((y_eng - target) ** 2))
    assert abs(m - m_ref) <= 1e-6 * m_ref, (m, m_ref)
    e = float(circ.mse_esr(xd, target))
    S, E = float(torch.sum((y_eng - target) ** 2)), float(torch.sum(y_eng ** 2))
    e_ref = S / (B * T) + np.sqrt(S / E / (B * T))
    assert abs(e - e_ref) <= 1e-5 * e_ref, (e, e_ref)
    # carry_state: two calls on the halves in time equal one call on the whole
    h = T // 2
    circ.reset_state()
    circ.mse(xd[:, :h].contiguous(), target[:h], carry_state=True)
    y_first = circ.last_output.clone()
    circ.mse(xd[:, h:].contiguous(), target[h:], carry_state=True)
    y_second = circ.last_output.clone()
    ec = max(float((y_first - y_eng[:h]).abs().max()), float((y_second - y_eng[h:]).abs().max()))
    print(f"carry_state: {ec:.3e}")
    assert tuple(circ.last_state.shape) == (1, B) and ec <= 1e-6
    # the other solvers
    _, c64, _ = build_circuit(THETA6, solver="newton_f64", time_parallel=None)
    _, cw, _ = build_circuit(THETA6, solver="omega_f32", time_parallel=None)
    e64, ew = float((c64(xd) - y_eng).abs().max()), float((cw(xd) - y_eng).abs().max())
    print(f"solvers: newton_f64 {e64:.3e} V, omega_f32 {ew:.3e} V from newton_f32")
    assert e64 <= 3e-6 and ew > 1e-3
    with pytest.raises(wb.WdfHipError):
        circ.to_device()


def test_ragged_shapes(oracle):
    from wdf_hip import binding as wb, workload
    B, T = 5, 131
    mode = wb.ASYM_NEWTON_F32
    x = workload.sweep_batch(B, T, seed=2)
    xd, th = dev(x), dev(THETA6)
    ref = oracle.clipper_asym_fwd(r32(THETA6), FS, x.astype(np.float64))
    y, zT, _, zs = wb.clipper_asym_fwd(xd, th, FS, mode, want_zT=True, want_stash=True)
    assert bool(torch.isfinite(y).all()) and float(np.max(np.abs(y.cpu().numpy() - ref))) < 3e-6
    y2, zT2, zs2, st = wb.clipper_asym_fwd_tp(xd, th, FS, mode, 2, 64, want_zT=True, want_stash=True)
    s = status(st)
    assert s["n_bad"] == 0 and s["gated_waves"] == 0, s
    assert float((y2 - y).abs().max()) <= 1e-6 and float((zs2 - zs).abs().max()) <= 2e-6 and float((zT2 - zT).abs().max()) <= 2e-6
    gy = dev(np.random.default_rng(5).standard_normal((T, B)) / (B * T))
    g1 = wb.clipper_asym_bwd_tp(xd, th, FS, mode, zs, zT, gy, 1).cpu().numpy().astype(np.float64)
    g3 = wb.clipper_asym_bwd_tp(xd, th, FS, mode, zs, zT, gy, 3).cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(g1)) and np.max(np.abs(g3 - g1) / np.abs(g1)) < 2e-5, (g1, g3)
    ref_g = fd_grad(oracle, THETA6, x, gy.cpu().numpy())
    assert np.max(np.abs(g1 - ref_g) / np.abs(ref_g)) < 2e-4, (g1, ref_g)
