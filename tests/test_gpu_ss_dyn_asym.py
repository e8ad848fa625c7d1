"""GPU: the two-different-diode root (exact Shockley pair, fp32 Newton) on the streamed-coefficient kernels -- root kind
WDF_ROOT_ASYM_PAIR of csrc/wdf_ss_dyn.h, through tf_wdf.AsymDiodePair(..., streamed=True) and tf_wdf.Circuit: a resistance
that moves per sample (per_sample_R on any Resistor / ResistiveVoltageSource), one that is constant along every sequence, and
a fourth capacitor.

Reference: the fp64 NumPy tree of tests/asym_pot_tree_ref.py (impedances propagated again at every step, the oracle's exact
root per element), evaluated at the float32-rounded parameter values; gradients by central differences through it over every
parameter but the pot's.  Bounds are the project's own for these kernels: y within 3e-6 V, every live gradient component
within 3e-4 relative; path against path y within 2e-6 V, gradients within 2e-5 (chunked against sequential) and 1e-4
(per-sequence rows against per-sample rows, streamed against the static-coefficient kernels).  Circuits, shapes, pots and
seeds: tests/ss_dyn_asym_cases.py (every reference gradient component keeps |sum of terms| >= 0.03 sum |terms|: asserted).

Measured on an MI355X (the worst over this module): y within 2.9e-7 V of the reference, gradient components within 2.1e-6
relative (the four-capacitor tree at 70 x 300); path against path y within 2.4e-7 V, gradients within 7.8e-7.
"""
import numpy as np
import pytest

import ss_asym_cases as base
import ss_dyn_asym_cases as cases

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

    def get(name):
        if name not in memo:
            r = cases.reference(oracle, name)
            for v in r.values():
                v.setflags(write=False)
            memo[name] = r
        return memo[name]
    return get


def cuda(a):
    return torch.as_tensor(np.array(a, dtype=np.float32, order="C"), device="cuda")          # (a copy: the references are read-only)


def rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b) / np.abs(b)


def grads_of(wdf, y, gy, params):
    g = wdf.tf.GradientTape().gradient(wdf.tf.reduce_sum(y * gy), params)
    return np.array([float(v) for v in g])


def run(wdf, circ, params, xin, gy):
    y = circ(xin)
    return y.as_subclass(torch.Tensor).detach().clone(), grads_of(wdf, y, gy, params)


def check_against_reference(wdf, circ, params, r, what):
    xin = cuda(cases.with_pot(r["x"], r.get("r")))
    y = circ(xin)
    pot = circ.per_sample_R
    g = wdf.tf.GradientTape().gradient(wdf.tf.reduce_sum(y * cuda(r["gy"])), params + ([pot.R] if pot is not None else []))
    got = np.array([float(v) for v in g[:len(params)]])
    dy = float(np.max(np.abs(y.numpy() - r["y"])))
    dg = rel(got, r["grad"])
    print(f"{what}: max |y - ref| = {dy:.3g}; gradient relative errors = {np.array2string(dg, precision=3)}; "
          f"balance = {np.array2string(r['balance'], precision=3)}")
    assert np.all(r["balance"] >= cases.BALANCE), r["balance"]
    assert dy <= 3e-6
    assert got.shape == r["grad"].shape and np.all(np.isfinite(got)) and np.all(dg <= 3e-4), (got, r["grad"])
    if pot is not None:
        assert g[-1] is None or float(g[-1]) == 0.0               # the pot is data: its own value has no gradient
    return xin, y, got


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hpf_vs", "hpf_r"])
def test_hpf_tree_with_a_pot_per_sample_vs_reference(wdf, reference, name):
    """Parallel(R, Series(Vs, C)) probed at R with the pot on Vs (300 .. 5 kOhm) or on R (5 .. 80 kOhm), a row per sample: 70
    sequences (one full and one ragged wave) of 300 samples, sequential kernels; y and the six live gradients."""
    circ, params = cases.build(wdf, name)
    assert (circ.ns, circ.ni) == (1, 1) and len(params) == 6
    xin, _, _ = check_against_reference(wdf, circ, params, reference(name), name)
    assert list(circ._dyn_chan_const.values()) == [False]


@pytest.mark.parametrize("B,T", [(1, 1), (3, 7), (65, 9)])
def test_hpf_tree_with_a_pot_at_edge_shapes(wdf, oracle, B, T):
    """One sequence of one sample; fewer samples than a chunk unit; a second wave with ONE live lane -- its 63 dead lanes are
    clamped to the last sequence and vote in the solve's ballot with it.  y only."""
    x, _ = base.data("hpf", 2, (B, T, 1))
    r = cases.pot_channel(B, T, 300.0, 5.0e3, 1)
    f, theta = cases.forward_of(oracle, "hpf_vs", x.astype(np.float64), r)
    circ, _ = cases.build(wdf, "hpf_vs")
    y = circ(cuda(cases.with_pot(x, r)))
    d = float(np.max(np.abs(y.numpy() - f(theta))))
    print(f"{B} x {T}: max |y - ref| = {d:.3g}")
    assert tuple(y.shape) == (T, B) and d <= 3e-6


# 2 ---------------------------------------------------------------------------------------------------------------------
def test_two_state_two_source_tree_with_a_pot_vs_reference(wdf, reference):
    circ, params = cases.build(wdf, "two_state_vs2")
    assert (circ.ns, circ.ni) == (2, 2) and len(params) == 8
    check_against_reference(wdf, circ, params, reference("two_state_vs2"), "two_state, pot on Vs2")


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_a_pot_constant_along_each_sequence_runs_one_row_per_sequence(wdf, reference):
    r = reference("hpf_vs_seq")
    circ, params = cases.build(wdf, "hpf_vs_seq")
    xin, y, g = check_against_reference(wdf, circ, params, r, "hpf, one pot value per sequence")
    assert list(circ._dyn_chan_const.values()) == [True]
    per_sample, params2 = cases.build(wdf, "hpf_vs_seq")
    per_sample.per_sequence_rows = False
    y2, g2 = run(wdf, per_sample, params2, xin, cuda(r["gy"]))
    assert "_dyn_chan_const" not in per_sample.__dict__
    dy, dg = float((y.as_subclass(torch.Tensor).detach() - y2).abs().max()), rel(g, g2)
    print(f"rows per sequence against rows per sample: max |dy| = {dy:.3g}; gradients {np.array2string(dg, precision=3)}")
    assert dy <= 2e-6 and np.all(dg <= 1e-4), (g, g2)


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", ["hpf", "two_state"])
def test_without_a_pot_the_streamed_kernels_give_what_the_static_ones_give(wdf, tree):
    """streamed=True with one static row against any_tree=True (csrc/wdf_statespace.h) at the same values and data."""
    x, gy = base.data(tree)
    x, gy = cuda(x), cuda(gy)
    dyn, p_dyn = cases.BUILD[tree](wdf)
    assert dyn._dyn and dyn.per_sample_R is None
    ss, p_ss = getattr(base, tree)(wdf, None)
    assert not ss._dyn
    y1, g1 = run(wdf, dyn, p_dyn, x, gy)
    y2, g2 = run(wdf, ss, p_ss, x, gy)
    dy, dg = float((y1 - y2).abs().max()), rel(g1, g2)
    print(f"{tree}: streamed against static: max |dy| = {dy:.3g}; gradients {np.array2string(dg, precision=3)}")
    assert dy <= 2e-6 and g1.shape == g2.shape and np.all(dg <= 1e-4), (g1, g2)


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["four_state_small", "four_state"])
def test_four_capacitor_tree_vs_reference(wdf, reference, name):
    """What any_tree=True refuses: the tone-shaping tree of four capacitors, one static row; y and the twelve gradients."""
    circ, params = cases.build(wdf, name)
    assert (circ.ns, circ.ni) == (4, 1) and len(params) == 12
    check_against_reference(wdf, circ, params, reference(name), name)


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pot", ["per_sample", "per_sequence"])
def test_streamed_kernels_in_time_chunks_equal_the_sequential_ones(wdf, pot):
    """The planner's own plan on the HPF tree at 200 x 2048 with the pot on Vs: the forward in verified chunks (where the plan
    speculates) with a clean verdict, the exact chunked reverse sweep; against the sequential kernels."""
    from wdf_hip import binding as wb, lowering
    B, T = 200, 2048
    x, gy = base.data("hpf", B + T, (B, T, 1))
    r = cases.pot_channel(B, T, 300.0, 5.0e3, 1) if pot == "per_sample" else cases.pot_grid(B, T)
    xin, gy = cuda(cases.with_pot(x, r)), cuda(gy)

    def one(tp):
        circ, params = cases.build(wdf, "hpf_vs", tp)
        lowering.LAST_SS_TP_STATUS["status"] = None
        y, g = run(wdf, circ, params, xin, gy)
        st = lowering.LAST_SS_TP_STATUS["status"]
        return circ, y, g, (None if st is None else wb.ss_tp_status(st))

    _, y_seq, g_seq, st_seq = one(None)
    circ, y_tp, g_tp, st_tp = one("auto")
    plan = next(iter(circ._dyn_plans.values()))[0]
    assert st_seq is None and plan.k_bwd >= 2, plan
    assert list(circ._dyn_chan_const.values()) == [pot == "per_sequence"]
    if st_tp is not None:
        assert st_tp["n_bad"] == 0, (st_tp, plan)
    dy, dg = float((y_tp - y_seq).abs().max()), rel(g_tp, g_seq)
    print(f"{pot}: plan {plan}; verdict {st_tp}; max |y_tp - y_seq| = {dy:.3g}; gradients {np.array2string(dg, precision=3)}")
    assert dy <= 2e-6
    assert np.all(dg <= 2e-5), (g_tp, g_seq)


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_time_parallel_forward_reruns_what_missed(wdf):
    """A warm-up far too short (eight chunks, eight steps): whatever the device's verdict, the result is the sequential
    kernel's within 2e-6 V -- the waves that missed were re-run sequentially."""
    from wdf_hip import lowering, binding as wb
    B, T = 200, 2048
    x = base.data("hpf", 3, (B, T, 1))[0]
    xin = cuda(cases.with_pot(x, cases.pot_channel(B, T, 300.0, 5.0e3, 1)))
    y_seq = cases.build(wdf, "hpf_vs", None)[0](xin)
    lowering.LAST_SS_TP_STATUS["status"] = None
    y_tp = cases.build(wdf, "hpf_vs", lowering.SsTpPlan(8, 8, 1.0e-6, 8))[0](xin)
    st = wb.ss_tp_status(lowering.LAST_SS_TP_STATUS["status"])
    d = float((y_tp - y_seq).abs().max())
    print("verdict:", st, "max |y_tp - y_seq| =", d)
    assert d <= 2e-6


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_forward_warm_starts_when_a_batch_is_visited_again(wdf):
    """The same batch object three times, the parameters nudged by 1e-3 relative in between: the third call's chunks start from
    the previous call's states, the verdict is clean and y is a cold sequential run's within 2e-6 V."""
    from wdf_hip import lowering, binding as wb
    B, T = 200, 2048
    x = base.data("hpf", 11, (B, T, 1))[0]
    xin = cuda(cases.with_pot(x, cases.pot_channel(B, T, 300.0, 5.0e3, 1)))
    gy = cuda(np.full((T, B), 1.0 / (B * T)))
    circ, params = cases.build(wdf, "hpf_vs", "auto")
    seq, seq_params = cases.build(wdf, "hpf_vs", None)
    started = []
    for call in range(3):
        if call == 2:                                             # what the third call starts from: (chunks, warm-up, states) or None
            warm = next(iter(circ._dyn_warm.values()))
            start = warm.start
            warm.start = lambda: (started.append(start()), started[-1])[1]
        lowering.LAST_SS_TP_STATUS["status"] = None
        y = circ(xin)
        grads_of(wdf, y, gy, params)
        if call < 2:
            for p, q in zip(params, seq_params):
                p.assign(float(p) * (1.0 + 1.0e-3))
                q.assign(float(p))
    print("third call: started from (chunks, warm-up)", None if started[0] is None else started[0][:2])
    assert len(started) == 1 and started[0] is not None and started[0][0] >= 2 and tuple(started[0][2].shape) == (started[0][0], 1, B)
    st = wb.ss_tp_status(lowering.LAST_SS_TP_STATUS["status"])
    print("verdict", st)
    assert st["n_bad"] == 0 and st["gated_waves"] == 0, st
    d = float((y - seq(xin)).abs().max())
    print("max |warm - cold sequential| =", d)
    assert d <= 2e-6


# 9 ---------------------------------------------------------------------------------------------------------------------
def test_c_abi_through_binding(wdf):
    """wdf_ss_dyn_fwd / _bwd / _bwd_tp with ONE static row against wdf_ss_fwd / _bwd under the same root on the same
    coefficients: the row is the coefficient vector with R_port appended, rootp the four diode values."""
    from wdf_hip import binding as wb
    x, gy = base.data("hpf")
    B, T = x.shape
    xs, gy = cuda(x).unsqueeze(-1).contiguous(), cuda(gy)
    circ, _ = base.hpf(wdf, None)
    coef64, r_port = circ.matrices()
    coef = coef64.detach().float().cuda()
    rootp5 = torch.tensor(list(base.f32(base.DIODES)) + [float(r_port)], dtype=torch.float32, device="cuda")
    row = torch.cat([coef, rootp5[4:]]).contiguous()
    rootp4 = rootp5[:4].contiguous()
    assert row.numel() == wb.lib().wdf_ss_dyn_row_len(1, 1)
    with pytest.raises(wb.WdfHipError, match="Is_up, nVt_up, Is_down, nVt_down"):
        wb.ss_dyn_fwd(xs, row, 1, 1, wb.ROOT_ASYM_PAIR, rootp=None)
    y_ss, zs_ss, _ = wb.ss_fwd(xs, coef, 1, 1, wb.ROOT_ASYM_PAIR, rootp5)
    gcoef, groot5, _ = wb.ss_bwd(xs, coef, 1, 1, zs_ss, gy, wb.ROOT_ASYM_PAIR, rootp5)
    y, zs, _ = wb.ss_dyn_fwd(xs, row, 1, 1, wb.ROOT_ASYM_PAIR, rootp=rootp4)
    assert float((y - y_ss).abs().max()) <= 2e-6
    grows, groot, _ = wb.ss_dyn_bwd(xs, row, 1, 1, zs, gy, wb.ROOT_ASYM_PAIR, rootp=rootp4)
    assert tuple(groot.shape) == (4,) and groot.dtype == torch.float64 and tuple(grows.shape) == (1, row.numel(), B)
    grow = grows.sum(dim=(0, 2), dtype=torch.float64)
    want = torch.cat([groot5[:4].double(), groot5[4:].double()])
    got = torch.cat([groot, grow[-1:]])
    d_root = ((got - want).abs() / want.abs()).cpu().numpy()
    d_coef = float((grow[:-1] - gcoef.double()).abs().max() / gcoef.double().abs().max())
    print("streamed against static: root gradients and R_port", d_root, "coefficients (to the largest)", d_coef)
    assert np.all(d_root <= 2e-5) and d_coef <= 2e-5
    # the exact chunked sweep: four chunks
    grows2, groot2, _ = wb.ss_dyn_bwd_tp(xs, row, 1, 1, zs, gy, 4, wb.ROOT_ASYM_PAIR, rootp=rootp4)
    assert tuple(groot2.shape) == (4,) and groot2.dtype == torch.float64 and tuple(grows2.shape) == (1, row.numel(), B)
    grow2 = grows2.sum(dim=(0, 2), dtype=torch.float64)
    d2 = torch.cat([(groot2 - groot).abs() / groot.abs(), (grow2[-1:] - grow[-1:]).abs() / grow[-1:].abs()]).cpu().numpy()
    print("chunked against sequential:", d2)
    assert np.all(d2 <= 2e-5) and float((grow2 - grow).abs().max() / grow.abs().max()) <= 2e-5
    # five capacitors under this root: refused before any launch
    with pytest.raises(wb.WdfHipError, match="scratch"):
        wb.ss_dyn_fwd(xs, torch.zeros((wb.lib().wdf_ss_dyn_row_len(5, 1),), device="cuda"), 5, 1, wb.ROOT_ASYM_PAIR, rootp=rootp4)


# 10 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_kind", ["mse_esr", "loss"])
def test_losses_compose_from_the_forward_under_a_pot(wdf, reference, loss_kind):
    tf = wdf.tf
    r = reference("hpf_vs")
    xin = cuda(cases.with_pot(r["x"], r["r"]))
    tgt = cuda(0.8 * r["y"])
    circ, params = cases.build(wdf, "hpf_vs")
    with tf.GradientTape() as tape:
        loss = circ.mse_esr(xin, tgt, skip=50) if loss_kind == "mse_esr" else circ.loss(xin, tgt, skip=50, mse=1.0, esr=1.0)
    got = np.array([float(v) for v in tape.gradient(loss, params)])
    circ2, params2 = cases.build(wdf, "hpf_vs")
    with tf.GradientTape() as tape2:
        y = circ2(xin)
        o, t = y[50:], tgt[50:]
        S, E = tf.reduce_sum(tf.square(o - t)), tf.reduce_sum(tf.square(o)) + float(np.finfo(float).eps)
        want = S / float(o.numel()) + tf.sqrt(S / E / float(o.numel()))
    ref_g = np.array([float(v) for v in tape2.gradient(want, params2)])
    dl, dg = abs(float(loss) - float(want)) / abs(float(want)), rel(got, ref_g)
    print(loss_kind, float(loss), float(want), "relative", dl, "gradients", np.array2string(dg, precision=3))
    assert dl <= 1e-6
    assert got.shape == (6,) and np.all(np.isfinite(got))
    assert np.all(dg <= 1e-5), (got, ref_g)
