"""GPU: the one-pass MSE and MSE + ESR step of small trees under the two-different-diode root (csrc/wdf_ss_asym_step.h;
wdf_ss_asym_step_mse / _esr) through binding.ss_asym_step_* and Circuit._asym_tree_step / mse / mse_esr.

Reference: the fp64 NumPy tree of tests/asym_tree_ref.py under oracle.asym_root at the float32-rounded parameters; gradients
are central differences (h = 1e-5 relative) of the loss itself (tests/ss_asym_step_cases.py).  Bounds are the project's own
rows for these kernels' siblings (DESIGN.md "Edges", tests/test_gpu_ss_asym.py): y 3e-6 V; loss, S, E 1e-5 relative; gradients
3e-4 relative with one capacitor, 5e-4 on larger trees; chunked against K = 1: y 2e-6, gradients 2e-5 relative.
Three states are not built (the chunk kernel spills): that tree keeps the composed path, asserted in test 1."""
import numpy as np
import pytest

import ss_asym_step_cases as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

Y_TOL, SUM_TOL, CHUNK_Y, CHUNK_G = 3e-6, 1e-5, 2e-6, 2e-5


def g_tol(case):
    return 3e-4 if sc.NS_NI[case][0] == 1 else 5e-4


@pytest.fixture(scope="module")
def wdf():
    import tf_wdf
    from wdf_hip import binding
    binding.require_gpu()
    return tf_wdf


@pytest.fixture(scope="module")
def refs(oracle):
    """(case, shape) -> its reference (computed once, shared, never written to)."""
    memo = {}

    def get(case, shape=None):
        key = (case, shape)
        if key not in memo:
            memo[key] = sc.Reference(oracle, case, shape)
        return memo[key]
    return get


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b) / np.abs(b)


def grads(wdf, loss, params):
    return np.array([float(v) for v in wdf.tf.GradientTape().gradient(loss, params)])


def status():
    from wdf_hip import lowering, binding
    return binding.ss_tp_status(lowering.LAST_SS_TP_STATUS["status"])


def run_step(wdf, case, x, tgt, kind, skip=0, plan=None, **kw):
    """-> loss (float), y [T,B] (numpy), gradients (numpy), the circuit."""
    circ, params = sc.BUILD[case](wdf, plan)
    assert circ._asym_step_tree(x, tgt, kind, skip)
    loss = circ._asym_tree_step(x, tgt, kind, skip, **kw)
    g = grads(wdf, loss, params)
    return float(loss), circ.last_output.cpu().numpy(), g, circ


def composed(wdf, circ, params, x, tgt, kind, skip=0):
    """The loss built by hand from circ(x) in torch -> loss (float), y, gradients."""
    y = circ(x)
    o, t = y[skip:], tgt[skip:]
    S = wdf.tf.reduce_sum(wdf.tf.square(o - t))
    n = float(o.numel())
    if kind == "mse":
        loss = S / n
    else:
        loss = S / n + wdf.tf.sqrt(S / (wdf.tf.reduce_sum(wdf.tf.square(o)) + sc.EPS) / n)
    return float(loss), y.detach().cpu().numpy(), grads(wdf, loss, params)


def check_reference(r, kind, skip, loss, y, g, what):
    gref, bal = r.grad_and_balance(kind, skip)
    S, E = r.sums(skip)
    dy, dl, dg = float(np.max(np.abs(y - r.y))), abs(loss - r.loss(kind, skip)) / r.loss(kind, skip), rel(g, gref)
    print(f"{what}: max |y - ref| = {dy:.3g}; loss rel = {dl:.3g}; worst gradient rel = {dg.max():.3g} "
          f"({np.array2string(dg, precision=2)}); min balance = {bal.min():.3g}")
    assert S > 0.0 and E > 0.0
    if (kind, skip) in (("mse", 0), ("mse_esr", 50)):             # (where the cases were chosen for it)
        assert np.all(bal >= sc.BALANCE), bal
    assert dy <= Y_TOL and dl <= SUM_TOL
    assert np.all(np.isfinite(g)) and np.all(dg <= g_tol(r.case)), (g, gref)


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.ALL)
def test_sequential_mse_vs_reference(wdf, refs, case):
    """K = 1, MSE, every case at (70, 300) -- one full wave, one ragged wave, a tail of 4 after 37 blocks -- and (5, 131) for
    three_state: y, the loss and every gradient through tape.gradient.  three_state (not built): the composed fallback -- the
    step refuses, circ.mse is the composed loss bit for bit, y and the reverse sweep meet their rows, and the composed loss and
    gradient stay within what y's row allows their weight y - target (figures in the body)."""
    r = refs(case)
    x, tgt = cuda(r.x), cuda(r.target)
    if case == "three_state":
        # not built: Circuit keeps the composed path.  Asserted: the step refuses, circ.mse IS the loss composed by hand from
        # circ(x), y meets its row, and the reverse sweep meets the gradients' row (5e-4) where that row applies: given the
        # reference's own weight 2 e / n, as in tests/test_gpu_ss_asym.py.  The composed loss and gradient also carry the forward's
        # own error dy in their weight e = y - target, which the sweep's row does not cover; they are bounded by what y's row
        # (|dy| <= 3e-6) allows, from reference quantities alone: |d loss| / loss <= 2 rms(dy) / rms(e), and per component
        # |dg_k| <= 5e-4 |g_k| + (2 / n) 3e-6 sum |dy/dtheta_k|.  On this tree the residual is small (rms e = 5e-3 V) and the
        # terms of Vs.R and R0 cancel over time to 0.063 of their sum, so that room is 1.3e-2 of those two components.  Measured
        # on an MI355X: max |dy| = 6.7e-7 (mean -1.2e-7), loss 2.5e-5, sweep alone 6.3e-5, composed gradient 1.16e-3 on R0 and
        # 1.05e-3 on Vs.R, of which (2 / n) sum dy dy/dtheta accounts for 1.2e-3; every other component <= 3.1e-4.
        from wdf_hip import binding
        circ, params = sc.BUILD[case](wdf, None)
        assert not circ._asym_step_tree(x, tgt, "mse") and not binding.ss_asym_step_built(3, 1, "mse")
        assert not circ._asym_step_tree(x, tgt, "mse_esr", 50) and not binding.ss_asym_step_built(3, 1, "mse_esr")
        loss = circ.mse(x, tgt)
        g = grads(wdf, loss, params)
        lc, yc, gc = composed(wdf, circ, params, x, tgt, "mse")
        assert float(loss) == lc and np.array_equal(g, gc)
        gref, bal = r.grad_and_balance("mse", 0)
        S, _ = r.sums(0)
        n = r.n()
        sweep, sweep_params = sc.BUILD[case](wdf, None)
        gs = grads(wdf, wdf.tf.reduce_sum(sweep(x) * cuda(2.0 * r.residual() / n)), sweep_params)
        room = g_tol(case) * np.abs(gref) + (2.0 / n) * Y_TOL * r.abs_sensitivity()
        dy, dl, dg, dgs = float(np.max(np.abs(yc - r.y))), abs(lc - r.loss("mse")) / r.loss("mse"), rel(g, gref), rel(gs, gref)
        print(f"three_state, composed: max |y - ref| = {dy:.3g}; loss rel = {dl:.3g}; sweep with the reference's weight: worst "
              f"gradient rel = {dgs.max():.3g}; composed gradient rel = {np.array2string(dg, precision=2)} of the allowed "
              f"{np.array2string(room / np.abs(gref), precision=2)}; min balance = {bal.min():.3g}")
        assert np.all(bal >= sc.BALANCE) and dy <= Y_TOL
        assert np.all(np.isfinite(gs)) and np.all(dgs <= g_tol(case)), (gs, gref)
        assert np.all(np.isfinite(g)) and np.all(np.abs(g - gref) <= room), (g, gref, room)
        assert dl <= 2.0 * Y_TOL / np.sqrt(S / n)
        return
    loss, y, g, _ = run_step(wdf, case, x, tgt, "mse")
    check_reference(r, "mse", 0, loss, y, g, f"{case} mse K=1")


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hpf", "hpf2", "a", "b"])
@pytest.mark.parametrize("skip", [50, 0, 299])
def test_sequential_mse_esr_vs_reference(wdf, refs, case, skip):
    """MSE + ESR at K = 1, skip inside a block, 0 and T - 1: loss3, S and E, the gradients; g against ga gP + gb gQ from sums."""
    from wdf_hip import binding
    r = refs(case)
    x, tgt = cuda(r.x), cuda(r.target)
    loss, y, g, circ = run_step(wdf, case, x, tgt, "mse_esr", skip)
    check_reference(r, "mse_esr", skip, loss, y, g, f"{case} mse+esr skip {skip} K=1")
    # the binding: sums, g, loss3 of the same step
    coef64, r_port = circ.matrices()
    dp = circ.root
    rootp = torch.tensor([float(v) for v in (dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down)] + [float(r_port)], device="cuda")
    xs = x if x.dim() == 3 else x.unsqueeze(-1)
    n = r.n(skip)
    y2, _, sums, gv, loss3, _ = binding.ss_asym_step_esr(xs.contiguous(), coef64.float().cuda(), rootp, circ.ns, circ.ni, tgt, n, sc.EPS, skip)
    s64 = sums.cpu().numpy().astype(np.float64)
    S, E = r.sums(skip)
    ng = coef64.numel() + 5
    esr = np.sqrt(s64[0] / (s64[1] + sc.EPS) / n)
    ga, gb = 2.0 / n + 1.0 / (esr * (s64[1] + sc.EPS) * n), -esr / (s64[1] + sc.EPS)
    want = ga * s64[2:2 + ng] + gb * s64[2 + ng:]
    l3 = loss3.cpu().numpy()
    dS, dE = abs(s64[0] - S) / S, abs(s64[1] - E) / E
    # (sums holds float32 roundings of the doubles g was formed from: 2^-24 relative per term, and g's own rounding)
    room = 2.0 ** -23 * (np.abs(ga * s64[2:2 + ng]) + np.abs(gb * s64[2 + ng:])) + 1e-30
    dgq = np.max(np.abs(gv.cpu().numpy() - want) / room)
    print(f"{case} skip {skip}: S rel {dS:.3g}, E rel {dE:.3g}, g vs ga gP + gb gQ: {dgq:.3g} of the float32 rounding room")
    assert dS <= SUM_TOL and dE <= SUM_TOL
    assert abs(l3[0] - S / n) <= SUM_TOL * S / n and abs(l3[2] - r.loss("mse_esr", skip)) <= SUM_TOL * r.loss("mse_esr", skip)
    assert abs(l3[0] + l3[1] - l3[2]) <= 1e-6 * l3[2]
    assert dgq <= 1.0
    assert torch.equal(y2, circ.last_output)


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,B,T,plan", [("hpf", 200, 2048, "auto"), ("a", 130, 1536, "auto"), ("hpf", 130, 3072, "four")])
@pytest.mark.parametrize("kind", ["mse", "mse_esr"])
def test_chunked_equals_sequential(wdf, case, B, T, plan, kind):
    """The planner's plan (and an explicit four-chunk plan): a clean verdict, y within 2e-6 and gradients within 2e-5 of K = 1.
    LOSS = 1: skip = chunk length + 3 (a later chunk, mid-block)."""
    from wdf_hip import lowering, binding
    ni = sc.NS_NI[case][1]
    x = cuda(sc.data_x(case, (B, T, ni)))
    tgt = cuda(np.random.default_rng(1).standard_normal((T, B)) * 0.1)
    circ, _ = sc.BUILD[case](wdf, "auto")
    p = lowering.plan_ss_time_parallel(circ.matrices()[0], circ.ns, circ.ni, binding.ROOT_ASYM_PAIR, B, T)
    assert p is not None and p.k_fwd >= 2, p
    if plan == "four":
        assert p.warmup <= T // 4
        plan, K = lowering.SsTpPlan(4, p.warmup, p.tol, 1), 4
    else:
        K = binding.lib().wdf_ss_tp_chunks(T, p.k_fwd)
    L = -(-(-(-T // K)) // 8) * 8
    skip = L + 3 if kind == "mse_esr" else 0
    l1, y1, g1, _ = run_step(wdf, case, x, tgt, kind, skip, None)
    lk, yk, gk, _ = run_step(wdf, case, x, tgt, kind, skip, plan)
    st = status()
    from wdf_hip import lowering as lw
    assert lw.LAST_SS_TP_STATUS["chunks_used"] == K and st["n_bad"] == 0 and st["gated_waves"] == 0, (st, lw.LAST_SS_TP_STATUS)
    dy, dl, dg = float(np.max(np.abs(yk - y1))), abs(lk - l1) / abs(l1), rel(gk, g1)
    print(f"{case} {kind} K={K} (B={B}, T={T}): max miss {st['max_miss']:.3g}; max |y - y(K=1)| = {dy:.3g}; loss rel {dl:.3g}; "
          f"worst gradient rel {dg.max():.3g}")
    assert dy <= CHUNK_Y and dl <= SUM_TOL and np.all(dg <= CHUNK_G), (dg, gk, g1)


# 4 ---------------------------------------------------------------------------------------------------------------------
def test_chunked_vs_reference(wdf, refs):
    """hpf at (70, 1536), K = 2, against the reference directly, both losses."""
    from wdf_hip import lowering
    r = refs("hpf", (70, 1536, 1))
    x, tgt = cuda(r.x), cuda(r.target)
    plan = lowering.SsTpPlan(2, 712, 1.0e-6, 1)
    for kind, skip in [("mse", 0), ("mse_esr", 50)]:
        loss, y, g, _ = run_step(wdf, "hpf", x, tgt, kind, skip, plan)
        st = status()
        assert lowering.LAST_SS_TP_STATUS["chunks_used"] == 2 and st["n_bad"] == 0, st
        check_reference(r, kind, skip, loss, y, g, f"hpf {kind} K=2 (70, 1536)")


# 5 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,B,T", [("hpf", 130, 2048), ("two_state", 130, 1536)])
@pytest.mark.parametrize("kind", ["mse", "mse_esr"])
def test_repair_is_the_sequential_recursion(wdf, case, B, T, kind):
    """An explicit plan with a warm-up far too short (K = 4, W = 8: ordinary inputs, the boundaries miss): every wave is
    gated and re-run as one chunk, and everything equals K = 1 bit for bit.  Mixed: the first 64 sequences get x = 0 (y exactly 0,
    their boundaries never miss) -- the status counts the other waves only and the results equal K = 1."""
    from wdf_hip import lowering
    ni = sc.NS_NI[case][1]
    xn = sc.data_x(case, (B, T, ni))
    tgt = cuda(np.random.default_rng(1).standard_normal((T, B)) * 0.1)
    plan = lowering.SsTpPlan(4, 8, 1.0e-6, 1)
    skip = T // 4 + 3 if kind == "mse_esr" else 0
    waves = -(-B // 64)
    for mixed in (False, True):
        if mixed:
            xn = xn.copy()
            xn[:64] = 0.0
        x = cuda(xn)
        l1, y1, g1, _ = run_step(wdf, case, x, tgt, kind, skip, None)
        lk, yk, gk, _ = run_step(wdf, case, x, tgt, kind, skip, plan)
        st = status()
        print(f"{case} {kind} mixed={mixed}: {st}")
        assert st["gated_waves"] == (waves - 1 if mixed else waves) and st["n_bad"] > 0, st
        if mixed:
            assert np.all(yk[:, :64] == 0.0)
            assert np.max(np.abs(yk - y1)) <= CHUNK_Y and abs(lk - l1) <= SUM_TOL * abs(l1) and np.all(rel(gk, g1) <= CHUNK_G)
            assert np.array_equal(yk[:, 64:], y1[:, 64:])
        else:
            assert np.array_equal(yk, y1) and lk == l1 and np.array_equal(gk, g1), (lk, l1, gk, g1)


# 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hpf", "b"])
def test_state_in_and_out(wdf, case):
    """z0 != 0: zT and y match circ(x, z0, return_state=True); two carry_state calls equal one call over the concatenated input."""
    B, T = 70, 304
    ns, ni = sc.NS_NI[case]
    xn = sc.data_x(case, (B, 2 * T, ni))
    x = cuda(xn)
    tgt = cuda(np.random.default_rng(1).standard_normal((2 * T, B)) * 0.1)
    z0 = cuda(np.random.default_rng(2).standard_normal((ns, B)) * 0.2)
    circ, _ = sc.BUILD[case](wdf, None)
    yr, zr = circ(x[:, :T].contiguous(), z0=z0, return_state=True)
    circ._asym_tree_step(x[:, :T].contiguous(), tgt[:T].contiguous(), "mse", 0, z0=z0, stateful=True)
    dy, dz = float((circ.last_output - yr).abs().max()), float((circ.last_state - zr).abs().max())
    print(f"{case}: z0 != 0: max |y - circ(x, z0)| = {dy:.3g}, max |zT - state| = {dz:.3g}")
    assert dy <= CHUNK_Y and dz <= CHUNK_Y
    # two halves, the state carried, against one call
    whole, _ = sc.BUILD[case](wdf, None)
    whole._asym_tree_step(x, tgt, "mse_esr", 5, stateful=True)
    halves, _ = sc.BUILD[case](wdf, None)
    halves._asym_tree_step(x[:, :T].contiguous(), tgt[:T].contiguous(), "mse_esr", 5, z0=None, stateful=True)
    y_a = halves.last_output.clone()
    halves._asym_tree_step(x[:, T:].contiguous(), tgt[T:].contiguous(), "mse_esr", 5, z0=halves.last_state, stateful=True)
    dy = float((torch.cat([y_a, halves.last_output]) - whole.last_output).abs().max())
    dz = float((halves.last_state - whole.last_state).abs().max())
    print(f"{case}: two carried calls against one: max |y| diff = {dy:.3g}, final state diff = {dz:.3g}")
    assert dy <= 2e-6 and dz <= 2e-6


# 7 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hpf", "a"])
def test_through_circuit(wdf, case):
    """circ.mse / circ.mse_esr (public, whichever path they route to) and _asym_tree_step (private) each agree with the composed
    path built by hand from circ(x); two identical calls are bit-identical; carry_state works through the public methods."""
    B, T, skip = 130, 1536, 50
    ni = sc.NS_NI[case][1]
    x = cuda(sc.data_x(case, (B, T, ni)))
    tgt = cuda(np.random.default_rng(1).standard_normal((T, B)) * 0.1)
    for kind in ("mse", "mse_esr"):
        sk = skip if kind == "mse_esr" else 0
        circ, params = sc.BUILD[case](wdf, "auto")
        lc, yc, gc = composed(wdf, circ, params, x, tgt, kind, sk)
        pub, pp = sc.BUILD[case](wdf, "auto")
        lp_t = pub.mse(x, tgt) if kind == "mse" else pub.mse_esr(x, tgt, skip=sk)
        lp, gp = float(lp_t), grads(wdf, lp_t, pp)
        ls, ys, gs, _ = run_step(wdf, case, x, tgt, kind, sk, "auto")
        ls2, ys2, gs2, _ = run_step(wdf, case, x, tgt, kind, sk, "auto")
        dpub = (abs(lp - lc) / lc, rel(gp, gc).max())
        dprv = (abs(ls - lc) / lc, rel(gs, gc).max(), float(np.max(np.abs(ys - yc))))
        print(f"{case} {kind}: public vs composed: loss rel {dpub[0]:.3g}, gradient rel {dpub[1]:.3g}; "
              f"step vs composed: loss rel {dprv[0]:.3g}, gradient rel {dprv[1]:.3g}, max |y| diff {dprv[2]:.3g}")
        assert dpub[0] <= SUM_TOL and dpub[1] <= g_tol(case)
        assert dprv[0] <= SUM_TOL and dprv[1] <= g_tol(case) and dprv[2] <= CHUNK_Y
        assert ls == ls2 and np.array_equal(gs, gs2) and np.array_equal(ys, ys2)


def test_refusals_stay(wdf):
    from wdf_hip.binding import WdfHipError
    top, probe = sc.cases.four_state_top(wdf)
    with pytest.raises(WdfHipError, match="at most three capacitors"):
        wdf.Circuit(top, wdf.AsymDiodePair(top, 4.352e-9, 2.0e-6, any_tree=True), probe)
    circ, _ = sc.BUILD["hpf"](wdf, None)
    with pytest.raises(WdfHipError, match="no resident training step"):
        circ.to_device()
