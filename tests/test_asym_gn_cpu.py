"""CPU: the Gauss-Newton step of the two-different-diode clipper (wdf_clipper_asym_step_gn, csrc/wdf_asym_gn.h) and the
Levenberg-Marquardt optimizer on it (wdf_hip/lm.py) as far as they can be checked without a GPU -- the symbols in the header,
the export list and the library; the C ABI's argument validation (through ctypes: no pointer is dereferenced, validation fails
first; the cases of tests/test_asym_step_cpu.py); the workspace size; the record algebra of the kernels on random data; the
finite-difference reference's own accuracy and the gauge it must show; the optimizer driven by the oracle; the circuits
tf_wdf.Circuit.mse_gn refuses.

Bounds.  Record algebra: 1e-12 of sqrt(H_qq H_rr) (fp64 sums of a few hundred terms, reordered).  The reference against itself
at four times the step: 1e-8 of sqrt(H_qq H_rr) (measured 2.5e-10 at 70 x 600 on the four sets).  The gauge: v^T H v <= 1e-8 x
sum |v_q v_r| sqrt(H_qq H_rr) for v = theta o (1, 0, 1, 0, -1, 1) (|J v| / |J| = 2..5e-10, squared, leaves six decades).  The
fit at 16 x 600 from theta towards 1.25 theta: loss ratio <= 1e-12 within 8 evaluations on theta6, <= 1e-9 within 24 on
leaky_low_R (measured within those budgets: 1.5e-14 and 6e-15, where both stop at the floor the fp32-rounded target sets, a
loss of 6e-17 and 4e-17)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import asym_gn_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = R.FS
NAMES = ("wdf_clipper_asym_step_gn_ws_bytes", "wdf_clipper_asym_step_gn")


@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


def test_symbols_declared_exported_and_listed(lib):
    from wdf_hip import binding
    hdr = open(os.path.join(REPO, "include", "wdf_hip.h")).read()
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH], text=True)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, dyn, re.M), name
        assert name in binding.EXPORTED_SYMBOLS and name in binding.SIGNATURES, name
    assert "#define WDF_HIP_ABI_VERSION 6" in hdr and lib.wdf_abi_version() == 6
    # the MSE step's arguments without the Adam tail
    mse, gn = binding.SIGNATURES["wdf_clipper_asym_step_mse"][1], binding.SIGNATURES["wdf_clipper_asym_step_gn"][1]
    assert len(gn) == len(mse) - 9 and gn[:-1] == mse[:len(gn) - 1] and gn[-1] == mse[-1]


def _call(lib, **kw):
    one = C.c_void_p(16)   # never dereferenced
    a = dict(x=one, theta6=one, mode=2, tol=1e-12, max_iter=50, target=one, y=one, z0=None, zT=None, B=4, T=64, K=2, W=8,
             ws=one, status=one, out28=one)
    a.update(kw)
    rc = lib.wdf_clipper_asym_step_gn(a["x"], a["theta6"], FS, a["mode"], a["tol"], a["max_iter"], a["target"], 1.0, a["y"],
                                      a["z0"], a["zT"], a["B"], a["T"], a["K"], a["W"], 1e-6, a["ws"], a["status"], a["out28"], None)
    return rc, lib.wdf_last_error()


@pytest.mark.parametrize("arg", ["x", "theta6", "target", "y", "ws", "status", "out28"])
def test_null_pointers_are_rejected(lib, arg):
    rc, err = _call(lib, **{arg: None})
    assert rc == -1 and b"null" in err, (rc, err)


def test_sizes_modes_and_chunking_are_rejected(lib):
    for kw, word in [(dict(B=0), b"B, T"), (dict(B=-3), b"B, T"), (dict(T=0), b"B, T"), (dict(T=-1), b"B, T"),
                     (dict(mode=3), b"unknown mode 3"), (dict(mode=-1), b"unknown mode"), (dict(mode=0), b"mode 0"),
                     (dict(K=0), b"n_chunks"), (dict(K=-2), b"n_chunks"), (dict(K=70000), b"n_chunks"),
                     (dict(K=5, T=64), b"does not tile"), (dict(W=-1), b"warmup"), (dict(tol=0.0), b"tol"),
                     (dict(max_iter=0), b"max_iter"), (dict(ws=C.c_void_p(20)), b"aligned"),
                     (dict(z0=C.c_void_p(32), zT=C.c_void_p(32)), b"alias")]:
        rc, err = _call(lib, **kw)
        assert rc == -1 and word in err, (kw, rc, err)


def test_the_words_are_the_mse_steps(lib):
    """one mistake, one set of words in wdf_last_error(), whichever step meets it"""
    one = C.c_void_p(16)
    for kw in (dict(B=0), dict(mode=0), dict(mode=7), dict(K=70000), dict(K=5), dict(tol=0.0), dict(ws=C.c_void_p(20)),
               dict(z0=C.c_void_p(32), zT=C.c_void_p(32))):
        a = dict(mode=2, tol=1e-12, z0=None, zT=None, B=4, K=2, ws=one)
        a.update(kw)
        rc = lib.wdf_clipper_asym_step_mse(one, one, FS, a["mode"], a["tol"], 50, one, 1.0, one, a["z0"], a["zT"], a["B"], 64, a["K"], 8,
                                           1e-6, a["ws"], one, one, None, None, None, None, 0.0, 0.0, 0.0, None, None, None)
        words = lib.wdf_last_error()
        rc_gn, words_gn = _call(lib, **kw)
        assert rc == rc_gn == -1 and words == words_gn, (kw, words, words_gn)


def test_workspace_size(lib):
    f = lib.wdf_clipper_asym_step_gn_ws_bytes
    assert f(0, 4) == 0 and f(64, 0) == 0 and f(-1, 4) == 0
    assert 0 < f(64, 4) < f(128, 4) < f(128, 8)
    # the records alone: K x 43 doubles per sequence
    assert f(8192, 16) >= 16 * 43 * 8192 * 8
    assert f(8192, 16) > lib.wdf_clipper_asym_step_mse_ws_bytes(8192, 16)


@pytest.mark.parametrize("n_chunks", [1, 3, 7])
def test_record_algebra_on_random_data(n_chunks):
    """kappa in (-1, 1), c and e random: the chunks' records walked first to last give the unsplit sums"""
    rng = np.random.default_rng(20 + n_chunks)
    T = 331
    kappa, c, e = rng.uniform(-1.0, 1.0, T), rng.standard_normal((T, 6)) * 10.0 ** rng.uniform(-3, 3, 6), rng.standard_normal(T)
    G0, H0 = R.unsplit(kappa, c, e)
    G, H = R.chunked(kappa, c, e, n_chunks)
    s = R.scale(H0)
    eh = float(np.max(np.abs(H - H0) / s))
    eg = float(np.max(np.abs(G - G0) / np.sqrt(np.diag(H0) * float(e @ e))))
    print(f"record algebra, {n_chunks} chunks: H {eh:.3e} of sqrt(H_qq H_rr), G {eg:.3e} of sqrt(H_qq S)")
    assert eh <= 1e-12 and eg <= 1e-12


def test_tri_order_is_row_major_upper():
    from wdf_hip import binding
    assert list(binding.GN_TRI) == R.TRI and len(R.TRI) == 21 and R.TRI[6] == (1, 1) and R.TRI[20] == (5, 5)
    torch = pytest.importorskip("torch")
    H = binding.gn_matrix(torch.arange(21, dtype=torch.float32)).numpy()
    assert H.dtype == np.float64 and np.array_equal(H, H.T)
    assert [H[q, r] for q, r in R.TRI] == list(range(21))


@pytest.mark.parametrize("name", R.NAMES)
def test_reference_accuracy_and_gauge(oracle, name):
    B, T = 70, 600
    _, _, H = R.gn_reference(oracle, name, B, T, 3)
    _, _, H4 = R.gn_reference(oracle, name, B, T, 3, step=4e-6)
    err = float(np.max(np.abs(H - H4) / R.scale(H)))
    vHv, bound = R.gauge_residual(H, R.r32(R.SETS[name]))
    print(f"reference {name}: step 1e-6 vs 4e-6 {err:.3e} of sqrt(H_qq H_rr); gauge v^T H v = {vHv:.3e}, {vHv / bound:.3e} of its scale")
    assert err <= 1e-8
    assert abs(vHv) <= 1e-8 * bound


def _oracle_fit(oracle, name, dtype="float64"):
    """LevenbergMarquardt on Variables, evaluate() through the oracle at the Variables' values -> the optimizer, the losses"""
    import tf_wdf as W
    from wdf_hip import lm
    tf = W.tf
    x, tg = R.workload_case(oracle, name, 16, 600, 3)
    variables = [tf.Variable(v, dtype=getattr(tf, dtype), trainable=True) for v in R.r32(R.SETS[name])]
    opt = lm.LevenbergMarquardt(lambda: R.gn_at(oracle, np.array([float(v) for v in variables]), x, tg), variables)
    return opt, variables


@pytest.mark.parametrize("name,ratio,budget", [("theta6", 1e-12, 8), ("leaky_low_R", 1e-9, 24)])
def test_lm_fits_the_teacher(oracle, name, ratio, budget):
    opt, variables = _oracle_fit(oracle, name)
    losses = []
    while opt.evaluations < budget:
        losses.append(opt.step())
        if len(losses) == 1:
            start = opt.evaluations        # (the first step evaluates at the start, then at its trials)
    first = R.gn_at(oracle, R.r32(R.SETS[name]), *R.workload_case(oracle, name, 16, 600, 3))[0]
    best = min(losses)
    print(f"LM {name}: start {first:.3e}, losses {['%.2e' % v for v in losses]}, {opt.evaluations} evaluations, lambda {opt.lam:.2e}; "
          f"values / teacher {[float(v) / (t * R.TEACHER) for v, t in zip(variables, R.r32(R.SETS[name]))]}")
    assert start >= 2 and opt.evaluations <= budget
    assert best <= ratio * first, (best, first)
    assert all(b <= a for a, b in zip(losses, losses[1:]))           # a step never returns a larger loss


def test_lm_rejected_trial_restores_every_value_bit_for_bit():
    import tf_wdf as W
    from wdf_hip import lm
    tf = W.tf
    start = [4.352e-9, 0.0492701, 45.0e3]
    variables = [tf.Variable(v, dtype=tf.float32, trainable=True) for v in start]
    before = [v.detach().clone() for v in variables]
    calls = []

    def evaluate():                                    # every trial is worse than the start
        calls.append([float(v) for v in variables])
        H = np.diag([1e16, 4.0, 1e-10])
        return (1.0 if len(calls) == 1 else 2.0), np.array([1e7, -1.0, 1e-6]), H

    opt = lm.LevenbergMarquardt(evaluate, variables, max_trials=3)
    loss = opt.step()
    assert loss == 1.0 and opt.evaluations == 4 and len(calls) == 4
    assert all(c != calls[0] for c in calls[1:])       # the trials did move the values
    for v, b in zip(variables, before):
        assert v.dtype == b.dtype and v.detach().numpy().tobytes() == b.numpy().tobytes()
    assert opt.lam == pytest.approx(1e-3 * 4.0 ** 3)


def test_lm_honours_a_clip_constraint_and_rejects_non_positive_values():
    import tf_wdf as W
    from wdf_hip import lm
    tf = W.tf
    clipped = tf.Variable(1.0, dtype=tf.float64, trainable=True, constraint=lambda z: tf.clip_by_value(z, 0.5, 1.5))
    free = tf.Variable(1.0, dtype=tf.float64, trainable=True)
    seen = []

    def evaluate():                                    # loss = (a - 3)^2 + (b - 3)^2: the unconstrained step goes to (3, 3)
        a, b = float(clipped), float(free)
        seen.append((a, b))
        return (a - 3) ** 2 + (b - 3) ** 2, np.array([2 * (a - 3), 2 * (b - 3)]), 2.0 * np.eye(2)

    opt = lm.LevenbergMarquardt(evaluate, [clipped, free], lam=1e-6)
    opt.step()
    assert float(clipped) == 1.5 and abs(float(free) - 3.0) < 1e-4, seen
    # a step into the negative is rejected without an evaluation: lambda grows until the trial is positive
    v = tf.Variable(1.0, dtype=tf.float64, trainable=True)
    n = []

    def evaluate2():
        n.append(float(v))
        return (float(v) + 1.0) ** 2, np.array([2 * (float(v) + 1.0)]), np.array([[2.0]])

    opt2 = lm.LevenbergMarquardt(evaluate2, [v], lam=1e-6)
    opt2.step()
    assert all(t > 0.0 for t in n) and 0.0 < float(v) < 1.0 and opt2.lam > 1e-6, (n, opt2.lam)


def _clipper(W, root_kw=None, circ_kw=None, solver="newton_f32", trainable=True):
    vs = W.ResistiveVoltageSource(45.0e3, trainable=trainable)
    cap = W.Capacitor(4.7e-9, FS, trainable=trainable)
    P1 = W.Parallel(vs, cap)
    dp = W.AsymDiodePair(P1, 4.352e-9, 2.0e-6, nDiodes_up=1.906, nDiodes_down=1.4, trainable=trainable, solver=solver, **(root_kw or {}))
    kw = dict(circ_kw or {})
    if kw.pop("pot", False):
        kw["per_sequence_R"] = vs
    return W.Circuit(P1, dp, cap, **kw), dp, vs, cap


def test_circuit_refusals_need_no_device():
    import tf_wdf as W
    from wdf_hip import binding as wb
    x = np.zeros((2, 16), dtype=np.float32)
    tg = np.zeros((16, 2), dtype=np.float32)
    for kw, word in [(dict(circ_kw=dict(pot=True)), "per_sequence_R"), (dict(solver="omega_f32"), "omega_f32"),
                     (dict(root_kw=dict(streamed=True)), "streamed"),
                     (dict(root_kw=dict(any_tree=True), circ_kw=dict(force_generic=True)), "any_tree")]:
        circ = _clipper(W, **kw)[0]
        with pytest.raises(wb.WdfHipError, match=word):
            circ.mse_gn(x, tg)
        with pytest.raises(wb.WdfHipError, match=word):
            circ.gn_variables
    circ = _clipper(W)[0]
    with pytest.raises(wb.WdfHipError, match="z0 / carry_state"):
        circ.mse_gn(x, tg, z0=np.zeros((1, 2), dtype=np.float32))
    with pytest.raises(wb.WdfHipError, match="z0 / carry_state"):
        circ.mse_gn(x, tg, carry_state=True)
    # every other root kind
    vs = W.ResistiveVoltageSource(45.0e3)
    cap = W.Capacitor(4.7e-9, FS)
    P1 = W.Parallel(vs, cap)
    sym = W.Circuit(P1, W.DiodePair(P1, 4.352e-9), cap)
    with pytest.raises(wb.WdfHipError, match="DiodePair root"):
        sym.mse_gn(x, tg)


def test_gn_variables_order_and_selection():
    import tf_wdf as W
    circ, dp, vs, cap = _clipper(W)
    got = circ.gn_variables
    want = [dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down, vs.R, cap.C]
    assert len(got) == 6 and all(a is b for a, b in zip(got, want))
    circ2, dp2, vs2, cap2 = _clipper(W, trainable=False)
    assert circ2.gn_variables == []
    from wdf_hip import binding as wb
    with pytest.raises(wb.WdfHipError, match="no trainable"):
        circ2.mse_gn(np.zeros((2, 16), dtype=np.float32), np.zeros((16, 2), dtype=np.float32))
