"""GPU: the two-different-diode root (exact Shockley pair, fp32 Newton) on generic trees -- root kind WDF_ROOT_ASYM_PAIR of the
state-space kernels (csrc/wdf_statespace.h), through tf_wdf.AsymDiodePair(..., any_tree=True) and tf_wdf.Circuit.

Reference: the fp64 NumPy tree of tests/asym_tree_ref.py under oracle.asym_root (pinned to the oracle in
tests/test_ss_asym_cpu.py), evaluated at the float32-rounded parameter values; gradients by central differences through it.
Bounds are the project's own for the same kernels under the symmetric root: y within 3e-6 V, every gradient component within
3e-4 relative (tests/test_gpu_circuit.py), chunked against sequential y 2e-6 and gradients 2e-5.  Circuits, shapes and seeds:
tests/ss_asym_cases.py (every reference gradient component keeps |sum of terms| >= 0.03 sum |terms|: asserted below).
"""
import numpy as np
import pytest

import ss_asym_cases as cases

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FS = cases.FS


@pytest.fixture(scope="module")
def wdf():
    import tf_wdf
    from wdf_hip import binding
    binding.require_gpu()
    return tf_wdf


@pytest.fixture(scope="module")
def reference(oracle):
    """case -> its reference (computed once per case, shared, never written to)."""
    memo = {}

    def get(case):
        if case not in memo:
            r = cases.reference(oracle, case)
            for v in r.values():
                v.setflags(write=False)
            memo[case] = r
        return memo[case]
    return get


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b) / np.abs(b)


def grads_of(wdf, y, gy, params):
    g = wdf.tf.GradientTape().gradient(wdf.tf.reduce_sum(y * gy), params)
    return np.array([float(v) for v in g])


def check_against_reference(wdf, circ, params, r, what):
    y = circ(cuda(r["x"]))
    got = grads_of(wdf, y, cuda(r["gy"]), params)
    dy = float(np.max(np.abs(y.numpy() - r["y"])))
    dg = rel(got, r["grad"])
    print(f"{what}: max |y - ref| = {dy:.3g}; gradient relative errors = {np.array2string(dg, precision=3)}; "
          f"balance = {np.array2string(r['balance'], precision=3)}")
    assert np.all(r["balance"] >= cases.BALANCE), r["balance"]
    assert dy <= 3e-6
    assert np.all(np.isfinite(got)) and np.all(dg <= 3e-4), (got, r["grad"])
    return y


# 1 ---------------------------------------------------------------------------------------------------------------------
def test_hpf_tree_sequential_vs_reference(wdf, reference):
    """Parallel(R, Series(Vs, C)) probed at R (33 kOhm, 1 kOhm, 22 nF): ns 1, ni 1; 70 sequences (one full and one ragged wave)
    of 300 samples (37 blocks of 8 and a tail of 4), sequential kernels; y and the seven gradients."""
    circ, params = cases.hpf(wdf, None)
    assert (circ.ns, circ.ni) == (1, 1)
    check_against_reference(wdf, circ, params, reference("hpf"), "hpf")


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_two_state_two_source_tree_vs_reference(wdf, reference):
    circ, params = cases.two_state(wdf, None)
    assert (circ.ns, circ.ni) == (2, 2)
    check_against_reference(wdf, circ, params, reference("two_state"), "two_state")


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_three_state_tree_vs_reference_and_four_states_are_refused(wdf, reference):
    """Four states are refused under this root (the chunked reverse sweep does not fit a wave's registers there): the
    four-state tone-shaping tree of tests/test_gpu_circuit.py raises, the same network less one section (ns = 3) runs."""
    from wdf_hip.binding import WdfHipError
    top, probe = cases.four_state_top(wdf)
    with pytest.raises(WdfHipError, match="at most three capacitors"):
        wdf.Circuit(top, wdf.AsymDiodePair(top, 4.352e-9, 2.0e-6, any_tree=True), probe)
    circ, params = cases.three_state(wdf, None)
    assert (circ.ns, circ.ni) == (3, 1)
    check_against_reference(wdf, circ, params, reference("three_state"), "three_state")


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_clipper_tree_forced_through_the_generic_kernels(wdf, reference):
    """force_generic=True: y against oracle.clipper_asym_fwd, the six gradients against its finite differences, and y against
    the clipper's own kernels (any_tree=False, the same values)."""
    r = reference("clipper")
    circ, params = cases.clipper(wdf, None, force_generic=True)
    assert circ._asym_generic
    y = check_against_reference(wdf, circ, params, r, "clipper through the generic kernels")
    own, _ = cases.clipper(wdf, None, any_tree=False)
    assert not own._asym_generic
    d = float((own(cuda(r["x"])) - y).abs().max())
    print("max |generic - dedicated| =", d)
    assert d <= 2e-6


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,B,T", [("hpf", 200, 2048), ("two_state", 130, 1536)])
def test_chunked_kernels_equal_sequential(wdf, case, B, T):
    """The planner's own plan (time_parallel="auto"): the HPF tree speculates (k_fwd >= 2: chunks warmed up from z = 0, verified
    on the device, a clean verdict), the two-state tree does not (its Jacobian reaches |eigenvalue| >= 1 at the conducting end
    of the root's slope) and takes the exact chunked reverse sweep only."""
    from wdf_hip import lowering, binding as wb
    build = getattr(cases, case)
    x, gy = cases.data(case, seed=B + T, shape=(B, T, cases.SHAPES[case][2]))
    x, gy = cuda(x), cuda(gy)

    def run(tp):
        circ, params = build(wdf, tp)
        y = circ(x)
        return circ, y, grads_of(wdf, y, gy, params)

    _, y_seq, g_seq = run(None)
    lowering.LAST_SS_TP_STATUS["status"] = None
    circ, y_tp, g_tp = run("auto")
    plan = lowering.plan_ss_time_parallel(circ.matrices()[0], circ.ns, circ.ni, wb.ROOT_ASYM_PAIR, B, T)
    assert plan is not None and plan.k_bwd >= 2, plan
    if case == "hpf":
        assert plan.k_fwd >= 2, plan
        st = wb.ss_tp_status(lowering.LAST_SS_TP_STATUS["status"])
        assert st["n_bad"] == 0 and st["gated_waves"] == 0 and st["max_miss"] <= 1e-6, (st, plan)
    else:
        assert plan.k_fwd == 1 and lowering.LAST_SS_TP_STATUS["status"] is None, plan
    dy, dg = float((y_tp - y_seq).abs().max()), rel(g_tp, g_seq)
    print(f"{case} {B} x {T}: plan {plan}; max |y_tp - y_seq| = {dy:.3g}; gradients {np.array2string(dg, precision=3)}")
    assert dy <= 2e-6
    assert np.all(dg <= 2e-5), (g_tp, g_seq)


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_time_parallel_forward_reruns_what_missed(wdf):
    """A warm-up far too short: every wave is gated and the sequential kernel behind the verification restores it -- the solve is
    deterministic, so the result IS the sequential kernel's."""
    from wdf_hip import lowering, binding as wb
    x = cuda(cases.data("hpf", seed=3, shape=(200, 2048, 1))[0])
    y_seq = cases.hpf(wdf, None)[0](x)
    lowering.LAST_SS_TP_STATUS["status"] = None
    y_tp = cases.hpf(wdf, lowering.SsTpPlan(8, 8, 1.0e-6, 8))[0](x)
    st = wb.ss_tp_status(lowering.LAST_SS_TP_STATUS["status"])
    assert st["n_bad"] > 0 and st["gated_waves"] == 4, st
    assert torch.equal(y_tp.as_subclass(torch.Tensor), y_seq.as_subclass(torch.Tensor))


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_forward_warm_starts_when_a_batch_is_visited_again(wdf):
    """The same batch object three times, the parameters nudged by 1e-3 relative in between: the third call's chunks start from
    the earlier calls' states with a warm-up below the cold plan's, the verdict is clean and y is the sequential kernel's
    within 2e-6."""
    from wdf_hip import lowering, binding as wb
    B, T = 200, 2048
    x = cuda(cases.data("hpf", seed=11, shape=(B, T, 1))[0])
    gy = cuda(np.full((T, B), 1.0 / (B * T)))
    circ, params = cases.hpf(wdf, "auto")
    seq, seq_params = cases.hpf(wdf, None)
    cold = lowering.plan_ss_time_parallel(circ.matrices()[0], 1, 1, wb.ROOT_ASYM_PAIR, B, T)
    used = []
    for call in range(3):
        y = circ(x)
        grads_of(wdf, y, gy, params)
        used.append((lowering.LAST_SS_TP_STATUS["warmup_used"], wb.ss_tp_status(lowering.LAST_SS_TP_STATUS["status"])))
        if call < 2:
            for p, q in zip(params, seq_params):
                p.assign(float(p) * (1.0 + 1.0e-3))
                q.assign(float(p))
    print("warm-ups and verdicts:", used, "cold plan:", cold)
    assert used[0][0] == cold.warmup
    assert used[2][0] < cold.warmup, used
    assert used[2][1]["n_bad"] == 0 and used[2][1]["gated_waves"] == 0 and used[2][1]["max_miss"] <= 1e-6, used
    assert float((y - seq(x)).abs().max()) <= 2e-6


# 8 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_kind", ["mse", "mse_esr"])
def test_losses_compose_from_the_forward_on_a_generic_tree(wdf, reference, loss_kind):
    tf = wdf.tf
    r = reference("hpf")
    x = cuda(r["x"])
    tgt = cuda(0.8 * r["y"])
    circ, params = cases.hpf(wdf, None)
    with tf.GradientTape() as tape:
        loss = circ.mse(x, tgt) if loss_kind == "mse" else circ.mse_esr(x, tgt, skip=50)
    got = np.array([float(v) for v in tape.gradient(loss, params)])
    circ2, params2 = cases.hpf(wdf, None)
    with tf.GradientTape() as tape2:
        y = circ2(x)
        if loss_kind == "mse":
            want = tf.reduce_mean(tf.square(y - tgt))
        else:
            o, t = y[50:], tgt[50:]
            S, E = tf.reduce_sum(tf.square(o - t)), tf.reduce_sum(tf.square(o)) + float(np.finfo(float).eps)
            want = S / float(o.numel()) + tf.sqrt(S / E / float(o.numel()))
    ref_g = np.array([float(v) for v in tape2.gradient(want, params2)])
    print(loss_kind, float(loss), float(want), got, ref_g)
    assert abs(float(loss) - float(want)) <= 1e-6 * abs(float(want))
    assert got.shape == (7,) and np.all(np.isfinite(got))
    assert np.all(rel(got, ref_g) <= 1e-5), (got, ref_g)
    # state in and out, composed from the forward as for any other generic circuit
    z0 = cuda(np.random.default_rng(1).uniform(-0.2, 0.2, (1, x.shape[0])))
    l2 = circ.mse(x, tgt, z0=z0) if loss_kind == "mse" else circ.mse_esr(x, tgt, skip=50, z0=z0)
    y2, zT = circ2(x, z0=z0, return_state=True)
    assert torch.equal(circ.last_state.as_subclass(torch.Tensor), zT.as_subclass(torch.Tensor)) and np.isfinite(float(l2))
    assert torch.equal(circ.last_output.as_subclass(torch.Tensor), y2.as_subclass(torch.Tensor).detach())


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_c_abi_through_binding(wdf):
    from wdf_hip import binding as wb
    B, T = 70, 300
    x, gy = cases.data("hpf")
    xs, gy = cuda(x).unsqueeze(-1).contiguous(), cuda(gy)
    circ, _ = cases.hpf(wdf, None)
    coef64, r_port = circ.matrices()
    coef = coef64.detach().float().cuda()
    rootp = torch.tensor(list(cases.f32(cases.DIODES)) + [float(r_port)], dtype=torch.float32, device="cuda")
    with pytest.raises(wb.WdfHipError, match="Is_up, nVt_up, Is_down, nVt_down, R_port"):
        wb.ss_fwd(xs, coef, 1, 1, wb.ROOT_ASYM_PAIR, rootp=None)
    y, zs, _ = wb.ss_fwd(xs, coef, 1, 1, wb.ROOT_ASYM_PAIR, rootp)
    gcoef, groot, _ = wb.ss_bwd(xs, coef, 1, 1, zs, gy, wb.ROOT_ASYM_PAIR, rootp)
    assert tuple(groot.shape) == (5,) and bool(torch.isfinite(groot).all()) and bool(torch.isfinite(gcoef).all())
    gcoef2, groot2, _ = wb.ss_bwd_tp(xs, coef, 1, 1, zs, gy, 4, wb.ROOT_ASYM_PAIR, rootp)
    assert tuple(groot2.shape) == (5,)
    assert float(((groot2 - groot).abs() / groot.abs()).max()) <= 2e-5 and float(((gcoef2 - gcoef).abs()).max()) <= 2e-5 * float(gcoef.abs().max())
    # the chunked forward with the root kind named: a warm-up far too short, so the gated re-run makes it the sequential result
    y2, _, _, st = wb.ss_fwd_tp(xs, coef, 1, 1, rootp, 4, 8, 1e-6, root_kind=wb.ROOT_ASYM_PAIR)
    assert wb.ss_tp_status(st)["n_bad"] > 0 and torch.equal(y2, y)
    # ... and the default keyword still runs the symmetric pair
    rp3 = torch.tensor([4.352e-9, 0.0493, float(r_port)], dtype=torch.float32, device="cuda")
    y_sym, _, _ = wb.ss_fwd(xs, coef, 1, 1, wb.ROOT_DIODE_PAIR, rp3, 2, 3)
    y3, _, _, st3 = wb.ss_fwd_tp(xs, coef, 1, 1, rp3, 4, 8, 1e-6, 2, 3)
    assert wb.ss_tp_status(st3)["n_bad"] > 0 and torch.equal(y3, y_sym) and not torch.equal(y3, y)
    groot3 = wb.ss_bwd(xs, coef, 1, 1, zs, gy, wb.ROOT_DIODE_PAIR, rp3, 2, 3)[1]
    assert tuple(groot3.shape) == (3,)
