"""GPU: tf_wdf.Circuit.mse_gn (loss, gradient and Gauss-Newton matrix of the two-different-diode clipper in one pass,
wdf_clipper_asym_step_gn) and wdf_hip.lm.LevenbergMarquardt on it.

mse_gn's loss against Circuit.mse's: one fp32 ulp (the same sums, one division in fp64 instead of fp32).  Its gradient against
tape.gradient(circ.mse(...)) in the order of circ.gn_variables: 2e-5 relative (the project's step-against-composed bound; the
same kernel expressions, so it is far inside).  A circuit with fewer trainable values returns the sub-block of the full H.

The fit, 70 x 600, from theta towards the teacher at 1.25 theta, theta6 and leaky_low_R: the budget is twice the number of
evaluations the float64 reference loop of tests/asym_gn_ref.py (finite-difference Jacobian of the oracle) needs on the same data
to bring the loss to 1e-6 of its start, computed here; the factor 2 covers the fp32 forward's different accept / reject path.
Within it the device fit reaches 1e-6 of its own starting loss.  schottky_big_R is left out: its reference stalls near 1e-4 of
the start for more than ten iterations, so a budget there would test luck.  The six-parameter clipper has an exact gauge, so
the fit is judged by its loss, never by the values.

Measured on one MI355X (newton_f32), loss after each accepted step (evaluations so far):
    theta6       reference 4.074e-3 (1), 1.593e-4 (2), 3.262e-5 (3), 1.761e-8 (4), 2.032e-14 (5): 5 evaluations, budget 10
                 device    4.074e-3 (1), 1.593e-4 (2), 3.262e-5 (3), 1.762e-8 (4), 2.103e-14 (5)
    leaky_low_R  reference 6.326e-3 (1), 6.273e-3 (3), 1.019e-4 (4), 4.997e-5 (5), 6.779e-6 (7), ... 8.416e-8 (16), 3.707e-10 (17):
                           17 evaluations, budget 34
                 device    6.326e-3 (1), 6.273e-3 (3), 1.019e-4 (4), 4.997e-5 (7), 6.779e-6 (9), ... 8.416e-8 (18), 3.710e-10 (19)
(the same accepted losses; the device path took two more rejected trials).  The fitted values sat 2.8-2.9 % (theta6) and 4.4-5.2 %
(leaky_low_R) from the teacher's on the gauge components at those losses.  mse_gn's loss within 0.14-0.55 ulp of mse's, g equal to
the tape's gradient bit for bit, H within 3.6e-7 of H_ref.
"""
import numpy as np
import pytest

import asym_gn_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FS = R.FS


def dev(a):
    return torch.tensor(np.array(a, dtype=np.float32), device="cuda")


def build_circuit(theta, solver="newton_f32", trainable=(True,) * 6, root_kw=None, **kw):
    """trainable: per value of [Is_up, nVt_up, Is_down, nVt_down, R, C]"""
    import tf_wdf as W
    Is1, V1, Is2, V2, Rv, Cv = [float(t) for t in theta]
    Vs = W.ResistiveVoltageSource(Rv, trainable=trainable[4])
    Cap = W.Capacitor(Cv, FS, trainable=trainable[5])
    P1 = W.Parallel(Vs, Cap)
    dp = W.AsymDiodePair(P1, Is1, Is2, Vt=1.0, nDiodes_up=V1, nDiodes_down=V2, trainable=True, solver=solver, **(root_kw or {}))
    for v, t in zip((dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down), trainable[:4]):
        v.trainable = bool(t)
        v.requires_grad_(bool(t))
    return W, W.Circuit(P1, dp, Cap, **kw), [dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down, Vs.R, Cap.C]


@pytest.mark.parametrize("solver", ["newton_f32", "newton_f64"])
@pytest.mark.parametrize("name", ["theta6", "leaky_low_R"])
def test_mse_gn_against_mse_and_the_tape(oracle, name, solver):
    x, tg = R.workload_case(oracle, name, 70, 600, 3)
    xd, tgd = dev(x), dev(tg)
    W, circ, variables = build_circuit(R.SETS[name], solver=solver, time_parallel=None)
    tf = W.tf
    assert all(a is b for a, b in zip(circ.gn_variables, variables))
    loss, g, H = circ.mse_gn(xd, tgd)
    y_gn = circ.last_output.clone()
    with tf.GradientTape() as tape:
        loss_m = circ.mse(xd, tgd)
    grads = tape.gradient(loss_m, variables)
    assert loss.dim() == 0 and tuple(g.shape) == (6,) and tuple(H.shape) == (6, 6)
    assert loss.dtype == g.dtype == H.dtype == torch.float64 and loss.is_cuda and g.is_cuda and H.is_cuda
    assert not (loss.requires_grad or g.requires_grad or H.requires_grad)
    assert torch.equal(H, H.t())
    lm_, lg = float(loss_m), float(loss)
    ulp = float(np.spacing(np.float32(lm_)))
    got, ref = g.cpu().numpy(), np.array([float(v) for v in grads])
    rel = np.abs(got - ref) / np.abs(ref)
    _, _, H_ref = R.gn_reference(oracle, name, 70, 600, 3)
    eh = float(np.max(np.abs(H.cpu().numpy() - H_ref) / R.scale(H_ref)))
    print(f"Circuit.mse_gn {name} {solver}: loss {lg:.9e} vs mse {lm_:.9e} ({abs(lg - lm_) / ulp:.2f} ulp), g vs tape {rel}, "
          f"H vs H_ref {eh:.3e}")
    assert abs(lg - lm_) <= ulp
    assert np.max(rel) <= 2e-5
    assert eh <= 4e-4
    assert circ.last_output is not None and tuple(y_gn.shape) == (600, 70)
    y_ref = oracle.clipper_asym_fwd(R.r32(R.SETS[name]), FS, x.astype(np.float64))
    assert float(np.max(np.abs(y_gn.cpu().numpy() - y_ref))) < 3e-6


def test_sub_block_of_the_trainable_values(oracle):
    x, tg = R.workload_case(oracle, "theta6", 70, 600, 3)
    xd, tgd = dev(x), dev(tg)
    _, full, _ = build_circuit(R.THETA6, time_parallel=None)
    _, g6, H6 = full.mse_gn(xd, tgd)
    _, part, variables = build_circuit(R.THETA6, trainable=(False, True, False, False, False, True), time_parallel=None)
    assert [v is w for v, w in zip(part.gn_variables, (variables[1], variables[5]))] == [True, True]
    loss, g2, H2 = part.mse_gn(xd, tgd)
    assert tuple(g2.shape) == (2,) and tuple(H2.shape) == (2, 2)
    idx = torch.tensor([1, 5], device="cuda")
    assert torch.equal(g2, g6[idx]) and torch.equal(H2, H6[idx][:, idx])


def test_planned_chunks_agree_with_one_chunk(oracle):
    """time_parallel="auto": the MSE step's plan (plan_asym_time_parallel) through the same step"""
    from wdf_hip import binding as wb, engine
    B, T = 256, 2048
    x, tg = R.workload_case(oracle, "theta6", B, T, 6)
    xd, tgd = dev(x), dev(tg)
    assert engine.plan_asym_time_parallel(B, T, R.THETA6[4], R.THETA6[5], FS).k_fwd > 1
    _, auto, _ = build_circuit(R.THETA6, time_parallel="auto")
    la, ga, Ha = auto.mse_gn(xd, tgd)
    s = wb.mlp_tp_status(engine.LAST_TP_STATUS["status"])
    _, seq, _ = build_circuit(R.THETA6, time_parallel=None)
    ls, gs, Hs = seq.mse_gn(xd, tgd)
    eh = float(((Ha - Hs).abs() / torch.sqrt(torch.outer(torch.diag(Hs), torch.diag(Hs)))).max())
    eg = float(((ga - gs).abs() / gs.abs()).max())
    print(f"Circuit.mse_gn auto plan: status {s}, loss {float(la):.6e} vs one chunk {float(ls):.6e}, g {eg:.3e}, H {eh:.3e}")
    assert s["n_bad"] == 0 and s["gated_waves"] == 0, s
    assert abs(float(la) - float(ls)) <= 1e-6 * float(ls) and eg <= 2e-5 and eh <= 2e-5


def test_refusals_raise_by_name(oracle):
    import tf_wdf as W
    from wdf_hip import binding as wb
    xd, tgd = torch.zeros((4, 64), device="cuda"), torch.zeros((64, 4), device="cuda")
    _, circ, _ = build_circuit(R.THETA6, solver="omega_f32")
    with pytest.raises(wb.WdfHipError, match="omega_f32"):
        circ.mse_gn(xd, tgd)
    _, circ, _ = build_circuit(R.THETA6, root_kw=dict(streamed=True))
    with pytest.raises(wb.WdfHipError, match="streamed"):
        circ.mse_gn(xd, tgd)
    _, circ, _ = build_circuit(R.THETA6, root_kw=dict(any_tree=True), force_generic=True)
    with pytest.raises(wb.WdfHipError, match="any_tree"):
        circ.mse_gn(xd, tgd)
    _, circ, _ = build_circuit(R.THETA6)
    with pytest.raises(wb.WdfHipError, match="z0 / carry_state"):
        circ.mse_gn(xd, tgd, carry_state=True)
    with pytest.raises(wb.WdfHipError, match="z0 / carry_state"):
        circ.mse_gn(xd, tgd, z0=torch.zeros((1, 4), device="cuda"))
    vs = W.ResistiveVoltageSource(45.0e3, trainable=True)
    cap = W.Capacitor(4.7e-9, FS, trainable=True)
    P1 = W.Parallel(vs, cap)
    dp = W.AsymDiodePair(P1, 4.352e-9, 2.0e-6, trainable=True)
    with pytest.raises(wb.WdfHipError, match="per_sequence_R"):
        W.Circuit(P1, dp, cap, per_sequence_R=vs).mse_gn(torch.zeros((4, 64, 2), device="cuda"), tgd)
    with pytest.raises(wb.WdfHipError, match="DiodePair root"):
        W.Circuit(P1, W.DiodePair(P1, 4.352e-9, trainable=True), cap).mse_gn(xd, tgd)


@pytest.mark.parametrize("name", ["theta6", "leaky_low_R"])
def test_lm_fit_within_twice_the_reference_budget(oracle, name):
    from wdf_hip import lm
    B, T, ratio = 70, 600, 1e-6
    x, tg = R.workload_case(oracle, name, B, T, 3)
    t0 = R.r32(R.SETS[name])
    _, path = R.lm_reference(lambda th: R.gn_at(oracle, th, x, tg), t0, 40)
    n_ref = R.evaluations_to_reach(path, ratio)
    assert n_ref is not None, path
    budget = 2 * n_ref
    xd, tgd = dev(x), dev(tg)
    _, circ, _ = build_circuit(R.SETS[name], time_parallel=None)
    opt = lm.LevenbergMarquardt(lambda: circ.mse_gn(xd, tgd), circ.gn_variables)
    traj = []
    while opt.evaluations < budget:
        loss = opt.step()
        first = opt.start_loss                     # (the first step's first evaluation: the loss at the start)
        traj.append((opt.evaluations, loss))
        if loss <= ratio * first:
            break
    print(f"LM fit {name}: reference (evaluations, loss) {[(n, '%.3e' % v) for n, v in path]} -> {n_ref} evaluations to {ratio:g} of "
          f"its start, budget {budget}; device start {first:.3e}, (evaluations, loss) {[(n, '%.3e' % v) for n, v in traj]}, "
          f"lambda {opt.lam:.2e}; values / teacher {[float(v) / (t * R.TEACHER) for v, t in zip(circ.gn_variables, t0)]}")
    assert opt.evaluations <= budget
    assert traj[-1][1] <= ratio * first, (traj, first)
