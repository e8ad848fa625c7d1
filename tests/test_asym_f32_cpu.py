"""CPU: the fp32 Newton mode of the two-different-diode clipper (WDF_ASYM_NEWTON_F32 = 2) as far as it can be checked
without a GPU -- the C ABI's argument validation (through ctypes; no pointer is dereferenced, validation fails first), the
tf_wdf.AsymDiodePair element and the trees tf_wdf.Circuit accepts it on."""
import ctypes as C
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 48000.0


@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


def test_mode_constants():
    from wdf_hip import binding as wb
    assert (wb.ASYM_OMEGA_F32, wb.ASYM_NEWTON_F64, wb.ASYM_NEWTON_F32) == (0, 1, 2)
    hdr = open(os.path.join(REPO, "include", "wdf_hip.h")).read()
    assert "#define WDF_ASYM_NEWTON_F32 2" in hdr


def test_asym_root_validates_mode_2(lib):
    one = C.c_void_p(16)   # never dereferenced
    f = lib.wdf_asym_root
    assert f(one, one, FS, 2, 0.0, 50, one, 8, None) == -1
    err = lib.wdf_last_error()
    assert b"tol" in err and b"unknown mode" not in err, err
    assert f(one, one, FS, 2, 1e-12, 0, one, 8, None) == -1
    assert b"max_iter" in lib.wdf_last_error()
    assert f(one, one, FS, 3, 1e-12, 50, one, 8, None) == -1
    assert b"unknown mode 3" in lib.wdf_last_error()
    assert f(one, one, FS, -1, 1e-12, 50, one, 8, None) == -1
    assert b"unknown mode" in lib.wdf_last_error()


def test_clipper_asym_fwd_validates_mode_2(lib):
    one = C.c_void_p(16)
    f = lib.wdf_clipper_asym_fwd
    assert f(one, one, FS, 2, 0.0, 50, one, None, None, None, None, 4, 8, None) == -1
    err = lib.wdf_last_error()
    assert b"tol" in err and b"unknown mode" not in err, err
    assert f(one, one, FS, 3, 1e-12, 50, one, None, None, None, None, 4, 8, None) == -1
    assert b"unknown mode 3" in lib.wdf_last_error()


def test_time_parallel_entry_points_validate_mode_2(lib):
    one = C.c_void_p(16)
    f = lib.wdf_clipper_asym_fwd_tp
    assert f(one, one, FS, 2, 0.0, 50, one, None, None, None, 4, 64, 2, 8, 1e-6, one, one, None) == -1
    err = lib.wdf_last_error()
    assert b"tol" in err and b"unknown mode" not in err, err
    assert f(one, one, FS, 3, 1e-12, 50, one, None, None, None, 4, 64, 2, 8, 1e-6, one, one, None) == -1
    assert b"unknown mode 3" in lib.wdf_last_error()
    # mode 2 is known to the reverse sweep: the call gets past the mode check and fails on the chunk count
    g = lib.wdf_clipper_asym_bwd_tp
    assert g(one, one, FS, 2, one, one, one, None, one, one, None, 4, 64, 0, None) == -1
    assert b"n_chunks" in lib.wdf_last_error()
    assert g(one, one, FS, 3, one, one, one, None, one, one, None, 4, 64, 1, None) == -1
    assert b"unknown mode 3" in lib.wdf_last_error()


def _tree(R=45.0e3, Cv=4.7e-9, trainable=False):
    import tf_wdf as W
    vs = W.ResistiveVoltageSource(R, trainable=trainable)
    cap = W.Capacitor(Cv, FS, trainable=trainable)
    return W, vs, cap


def test_asym_diode_pair_variables_and_constraints():
    import tf_wdf as W
    _, vs, cap = _tree()
    P1 = W.Parallel(vs, cap)
    dp = W.AsymDiodePair(P1, 4.352e-9, 2.0e-6, nDiodes_up=1.906, nDiodes_down=1.4)
    assert dp.solver == "newton_f32" and dp.mode == 2
    assert float(dp.Is_up) == pytest.approx(4.352e-9, rel=1e-6) and float(dp.Is_down) == pytest.approx(2.0e-6, rel=1e-6)
    assert float(dp.nVt_up) == pytest.approx(25.85e-3 * 1.906, rel=1e-6)
    assert float(dp.nVt_down) == pytest.approx(25.85e-3 * 1.4, rel=1e-6)
    assert len(dp.variables) >= 4 and len(dp.trainable_variables) == 0
    # DiodePair's constraints: Is in [1e-15, 1e-3], nVt in [1e-3, 1]
    for v, lo, hi in ((dp.Is_up, 1e-15, 1e-3), (dp.Is_down, 1e-15, 1e-3), (dp.nVt_up, 1e-3, 1.0), (dp.nVt_down, 1e-3, 1.0)):
        assert float(v.constraint(W.tf.constant(10.0))) == pytest.approx(hi)
        assert float(v.constraint(W.tf.constant(0.0))) == pytest.approx(lo)
    dt = W.AsymDiodePair(P1, 1e-9, 1e-8, trainable=True, solver="newton_f64")
    assert {id(v) for v in dt.trainable_variables} == {id(dt.Is_up), id(dt.nVt_up), id(dt.Is_down), id(dt.nVt_down)}
    assert dt.mode == 1 and W.AsymDiodePair(P1, 1e-9, 1e-8, solver="omega_f32").mode == 0
    with pytest.raises(ValueError):
        W.AsymDiodePair(P1, 1e-9, 1e-8, solver="newton")
    P1.calc_impedance()
    dp.calc_impedance()
    assert float(dp.R) == pytest.approx(float(P1.R))
    from wdf_hip.binding import WdfHipError
    with pytest.raises(WdfHipError, match="Circuit"):
        dp.reflected()


def test_circuit_accepts_the_clipper_tree_only():
    from wdf_hip.binding import WdfHipError
    W, vs, cap = _tree()
    P1 = W.Parallel(vs, cap)
    circ = W.Circuit(P1, W.AsymDiodePair(P1, 4.352e-9, 2.0e-6), cap)
    assert circ.root_kind == "AsymDiodePair" and circ.ns == 1 and circ.ni == 1
    with pytest.raises(WdfHipError, match="resident"):
        circ.to_device()
    # an RC low-pass under this root: not the clipper tree
    W, vs, cap = _tree()
    S1 = W.Series(vs, cap)
    with pytest.raises(WdfHipError, match="clipper"):
        W.Circuit(S1, W.AsymDiodePair(S1, 4.352e-9, 2.0e-6), cap)
    # the clipper tree probed at the source instead of the capacitor
    W, vs, cap = _tree()
    P1 = W.Parallel(vs, cap)
    with pytest.raises(WdfHipError, match="clipper"):
        W.Circuit(P1, W.AsymDiodePair(P1, 4.352e-9, 2.0e-6), vs)
    W, vs, cap = _tree()
    P1 = W.Parallel(vs, cap)
    with pytest.raises(WdfHipError, match="per_sample_R"):
        W.Circuit(P1, W.AsymDiodePair(P1, 4.352e-9, 2.0e-6), cap, per_sample_R=vs)
    W, vs, cap = _tree()
    P1 = W.Parallel(vs, cap)
    with pytest.raises(WdfHipError, match="force_generic"):
        W.Circuit(P1, W.AsymDiodePair(P1, 4.352e-9, 2.0e-6), cap, force_generic=True)


def test_planner_reproduces_the_best_recorded_plan():
    """8192 x 4096 at 45 kOhm / 4.7 nF: 16 forward chunks, 32 reverse chunks, and a warm-up that outlasts the diode-off
    forgetting rate 1 - 2p (p = Rc / (R + Rc), Rc = 1 / (2 C fs)) down to 1e-8."""
    import math
    from wdf_hip import engine
    plan = engine.plan_asym_time_parallel(8192, 4096, 45.0e3, 4.7e-9, FS)
    assert (plan.k_fwd, plan.k_bwd) == (16, 32) and plan.tol == 1e-6
    Rc = 1.0 / (2.0 * 4.7e-9 * FS)
    rho = 1.0 - 2.0 * Rc / (45.0e3 + Rc)
    assert rho ** plan.warmup <= 1e-8 and plan.warmup % 8 == 0 and plan.warmup <= 2 * math.log(1e-8) / math.log(rho)
    short = engine.plan_asym_time_parallel(5, 131, 45.0e3, 4.7e-9, FS)
    assert short.k_fwd == 1 and short.k_bwd >= 1
