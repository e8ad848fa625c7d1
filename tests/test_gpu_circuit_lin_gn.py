"""GPU: Circuit.mse_gn / Circuit.gn_variables on resident linear trees (csrc/wdf_ss_lin_gn.h through lowering._LinResident.gn_entry /
gn_step) and wdf_hip.lm.LevenbergMarquardt on them.

Circuits: lpf.py's tree (Inverter(Series(R1, C1)), ideal-source root; ns = 1) at B = 4, T = 1280, and the voltage divider (ns = 0)
at B = 4, T = 256.  Targets are made by the float64 reference at other component values (ss_lin_gn_ref.fit_data), so the loss
floor is far below the fits' goal.

Reference: tests/ss_lin_gn_ref.py composed with probe_tape's host evaluation of the circuit's own tape (the float64 coefficients and
Jacobian at the block's float32 values), the coefficients rounded to float32 once, as the device probe hands them to the step.
Bounds: the kernel module's -- y 3e-6, loss 1e-5, g (4e-6 mag) |J|, H sum B_H magH |J| |J| -- with 1e-9 of the same magnitudes on
top for the device probe's float64 Jacobian against the host's (tests/test_gpu_ss_lin_step_kernel.py section F bounds it far below).

The fits: LevenbergMarquardt(lambda: circ.mse_gn(x, t), circ.gn_variables) reaches 1e-6 of its starting loss within 2 N_ref
evaluations, N_ref the float64 reference's count (tests/test_ss_lin_gn_cpu.py: 6 and 4); the margin of 2 allows for fp32 trial
rejections near the end.  H is singular here too (y depends on R C, respectively on R1 / R2, only): fits are judged by loss.

Every check prints `FIG | <case> | ...` (error / bound) before it asserts.  Measured on an MI355X (10 tests, under 1 s): y 0.040, loss
0.002, g 0.004, H below 0.0005 of their bounds on every circuit; lpf.py's tree 9.340e-3 -> 7.085e-12 in 6 evaluations (the reference:
7.086e-12 in 6, budget 12), the voltage divider 3.203e-1 -> 2.252e-8 in 4 (the reference the same, budget 8).
"""
import gc

import numpy as np
import pytest

import ss_lin_gn_ref as G
import ss_lin_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B_Y, B_SSE, B_G = 3e-6, 1e-5, 4e-6


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture
def W():
    import tf_wdf
    return tf_wdf


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def pair(which):
    """the fit's data as the Circuit takes it: x [B,T] and target [T,B] on the device, and x_tm for the reference"""
    x_tm, target = G.fit_data(which)
    return cuda(x_tm[:, 0, :].T), cuda(target), x_tm, target


def reference(circ, x_tm, target, z0=None):
    """the reference at the block's float32 values: (loss, g [n], H [n,n], g's bound, H's bound, y) over ALL n values of the block"""
    lin = circ._lin
    values = lin.pb.block.cpu().numpy().astype(np.float64)[:lin.n_tree]
    coef64, jac = lin.host_tape.evaluate(values, lin.host_outs)
    coef = coef64.astype(np.float32)
    assert np.array_equal(coef, lin.coef.cpu().numpy()), "the device probe's float32 coefficients are the host evaluation's, rounded"
    ns, ni = circ.ns, circ.ni
    T, _, B = x_tm.shape
    gscale = 2.0 / (B * T)
    r = G.run(ns, ni, coef, x_tm, target, gscale, z0=z0)
    mag = R.run(ns, ni, coef, x_tm, target, gscale, z0=z0).mag
    rows = R.rows(ns, ni)
    g = r.g @ jac[rows]
    gb = ((B_G + 1e-9) * mag) @ np.abs(jac[rows])
    H, Hb = G.chain(ns, ni, r.Hc, jac, gscale), G.chain_bound(ns, ni, r.magH, jac, G.B_H + 1e-9, gscale)
    return r.sse / (B * T), g, H, gb, Hb, r.y


def ratio(err, bound):
    return float(np.max(np.asarray(err) / np.asarray(bound)))


def check(label, circ, got, x_tm, target, keep=None, z0=None):
    loss, g, H = got
    assert all(t.is_cuda and t.dtype == torch.float64 and not t.requires_grad for t in got) and loss.dim() == 0
    rl, rg, rH, gb, Hb, ry = reference(circ, x_tm, target, z0)
    if keep is not None:
        rg, gb, rH, Hb = rg[keep], gb[keep], rH[np.ix_(keep, keep)], Hb[np.ix_(keep, keep)]
    n = len(rg)
    assert tuple(g.shape) == (n,) and tuple(H.shape) == (n, n)
    Hn = H.cpu().numpy()
    y = circ.last_output.cpu().numpy().astype(np.float64)
    f = {"y": ratio(np.max(np.abs(y - ry)), B_Y * max(1.0, np.max(np.abs(ry)))), "loss": ratio(abs(float(loss) - rl), B_SSE * rl),
         "g": ratio(np.abs(g.cpu().numpy() - rg), gb), "H": ratio(np.abs(Hn - rH), Hb)}
    print(f"FIG | {label} | " + " ".join(f"{k}={v:.3f}" for k, v in f.items()) + f" | loss {float(loss):.4e}")
    assert all(v <= 1.0 for v in f.values()), (label, f)
    assert np.array_equal(Hn, Hn.T)


@pytest.mark.parametrize("which", ["lpf", "divider"])
def test_mse_gn_against_the_reference(W, which):
    spec, build = G.FITS[which]
    circ, pvars = build(W)
    circ.to_device()
    x, t, x_tm, target = pair(which)
    assert len(circ.gn_variables) == 2 and all(a is b for a, b in zip(circ.gn_variables, pvars))
    check(which, circ, circ.mse_gn(x, t), x_tm, target)
    # the matrix is singular: y depends on R C (R1 / R2) only
    H = circ.mse_gn(x, t)[2].cpu().numpy()
    d = np.sqrt(np.diag(H))
    assert np.min(np.linalg.eigvalsh(H / np.outer(d, d))) < 1e-4


def test_a_value_that_is_not_trainable_loses_its_row_and_column(W):
    circ, pvars = G.build_lpf(W, trainable=(True, False))
    circ.to_device()
    x, t, x_tm, target = pair("lpf")
    assert len(circ.gn_variables) == 1 and circ.gn_variables[0] is pvars[0]
    check("lpf, C fixed", circ, circ.mse_gn(x, t), x_tm, target, keep=[0])
    circ2, pvars2 = G.build_lpf(W, trainable=(False, True))
    circ2.to_device()
    assert len(circ2.gn_variables) == 1 and circ2.gn_variables[0] is pvars2[1]
    check("lpf, R fixed", circ2, circ2.mse_gn(x, t), x_tm, target, keep=[1])
    from wdf_hip import binding as wb
    circ3, _ = G.build_lpf(W, trainable=(False, False))
    circ3.to_device()
    with pytest.raises(wb.WdfHipError, match="no trainable"):
        circ3.mse_gn(x, t)


def test_initial_state_is_served_and_carry_state_and_a_host_tree_raise(W):
    from wdf_hip import binding as wb
    circ, _ = G.build_lpf(W)
    x, t, x_tm, target = pair("lpf")
    with pytest.raises(wb.WdfHipError, match=r"to_device\(\)"):
        circ.mse_gn(x, t)
    circ.to_device()
    z0 = np.random.default_rng(5).standard_normal((1, x_tm.shape[2])).astype(np.float32)
    got = circ.mse_gn(x, t, z0=cuda(z0))
    check("lpf from z0", circ, got, x_tm, target, z0=z0)
    assert abs(float(got[0]) - float(circ.mse_gn(x, t)[0])) > 1e-3 * float(got[0])          # (the state mattered)
    with pytest.raises(wb.WdfHipError, match="carry_state"):
        circ.mse_gn(x, t, carry_state=True)
    # no capacitor: nothing to start from
    div, _ = G.build_divider(W)
    div.to_device()
    xd, td, xd_tm, targetd = pair("divider")
    check("divider with a z0", div, div.mse_gn(xd, td, z0=cuda(np.ones((1, xd_tm.shape[2])))), xd_tm, targetd)


def test_mse_on_the_same_pair_is_not_touched(W):
    """circ.mse after circ.mse_gn on the same (x, target): the bits it gives on a circuit that never ran mse_gn"""
    tf = W.tf
    x, t, _, _ = pair("lpf")

    def mse_bits(circ, pvars):
        with tf.GradientTape() as tape:
            loss = circ.mse(x, t)
        grads = tape.gradient(loss, pvars)
        return [loss.detach().clone(), circ.last_output.detach().clone()] + [g.detach().clone() for g in grads]

    a, pa = G.build_lpf(W)
    a.to_device()
    want = mse_bits(a, pa)
    b, pb = G.build_lpf(W)
    b.to_device()
    b.mse_gn(x, t)
    got = mse_bits(b, pb)
    b.mse_gn(x, t)
    again = mse_bits(b, pb)
    for u, v, w in zip(want, got, again):
        u, v, w = (q.as_subclass(torch.Tensor).float().contiguous().view(torch.int32) for q in (u, v, w))
        assert torch.equal(u, v) and torch.equal(u, w)


@pytest.mark.parametrize("which", ["lpf", "divider"])
def test_lm_fit_within_twice_the_reference_budget(W, which):
    from wdf_hip import lm
    ratio_goal = 1e-6
    path, start = G.reference_fit(which)
    n_ref = G.evaluations_to_reach(path, start, ratio_goal)
    assert n_ref is not None, path
    budget = 2 * n_ref
    circ, _ = G.FITS[which][1](W)
    circ.to_device()
    x, t, _, _ = pair(which)
    opt = lm.LevenbergMarquardt(lambda: circ.mse_gn(x, t), circ.gn_variables)
    traj = []
    while opt.evaluations < budget:
        loss = opt.step()
        traj.append((opt.evaluations, loss))
        if loss <= ratio_goal * opt.start_loss:
            break
    print(f"LM fit {which}: reference start {start:.3e}, (evaluations, loss) {[(n, '%.3e' % v) for n, v in path]} -> {n_ref} evaluations to "
          f"{ratio_goal:g} of its start, budget {budget}; device start {opt.start_loss:.3e}, (evaluations, loss) "
          f"{[(n, '%.3e' % v) for n, v in traj]}, lambda {opt.lam:.2e}; values {[float(v) for v in circ.gn_variables]}")
    assert opt.evaluations <= budget
    assert traj[-1][1] <= ratio_goal * opt.start_loss, (traj, opt.start_loss)
