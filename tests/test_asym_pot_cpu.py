"""CPU-side checks of the per-sequence pot of the two-different-diode clipper: the five wdf_clipper_asym_*_rseq entry points
are declared and exported, their wrappers refuse a missing or wrong-shaped rseq and the closed form before anything is
launched, the channel helper, Circuit(per_sequence_R=...) and the plan from the largest pot.  No GPU needed."""
import fnmatch
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FS = 48000.0
SYMBOLS = ["wdf_clipper_asym_fwd_rseq", "wdf_clipper_asym_fwd_tp_rseq", "wdf_clipper_asym_bwd_tp_rseq",
           "wdf_clipper_asym_step_mse_rseq", "wdf_clipper_asym_step_esr_rseq"]


def test_the_five_symbols_are_declared_and_exported():
    from wdf_hip import binding
    header = open(os.path.join(ROOT, "include", "wdf_hip.h")).read()
    exports = open(os.path.join(ROOT, "differentiable-wdfs_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    for sym in SYMBOLS:
        m = re.search(r"^int " + sym + r"\(const float\* x, const float\* rseq,", header, re.M)
        assert m, f"{sym}: not declared with rseq behind x"
        assert any(fnmatch.fnmatch(sym, p.strip()) for p in patterns), f"{sym}: no global pattern of exports.map matches"
        assert sym in binding.EXPORTED_SYMBOLS
    assert "#define WDF_HIP_ABI_VERSION 6" in header


def _args(B=5, T=16):
    x = torch.zeros((B, T), dtype=torch.float32)
    theta6 = torch.tensor([4.352e-9, 0.0493, 2.0e-6, 0.0362, 45.0e3, 4.7e-9], dtype=torch.float32)
    return x, theta6, torch.zeros((T, B), dtype=torch.float32)


def _calls(rseq, mode):
    """the five wrappers, each called with this rseq and mode"""
    from wdf_hip import binding as wb
    x, th, tg = _args()
    return [
        lambda: wb.clipper_asym_fwd_rseq(x, rseq, th, FS, mode),
        lambda: wb.clipper_asym_fwd_tp_rseq(x, rseq, th, FS, mode, 2, 8),
        lambda: wb.clipper_asym_bwd_tp_rseq(x, rseq, th, FS, mode, tg, torch.zeros(5), tg, 2),
        lambda: wb.clipper_asym_step_mse_rseq(x, rseq, th, FS, mode, tg, 1.0, 2, 8),
        lambda: wb.clipper_asym_step_esr_rseq(x, rseq, th, FS, mode, tg, 80.0, 1e-16, 0, 2, 8),
    ]


@pytest.mark.parametrize("rseq", [None, torch.ones(4), torch.ones((5, 1)), torch.ones(5, dtype=torch.float64), [1.0] * 5],
                         ids=["missing", "short", "two_dims", "float64", "list"])
def test_wrappers_reject_a_bad_rseq_before_any_launch(rseq):
    from wdf_hip import binding as wb
    for call in _calls(rseq, wb.ASYM_NEWTON_F32):
        with pytest.raises(wb.WdfHipError, match="rseq"):
            call()


def test_wrappers_reject_the_closed_form_before_any_launch():
    from wdf_hip import binding as wb
    for call in _calls(torch.full((5,), 45.0e3), wb.ASYM_OMEGA_F32):
        with pytest.raises(wb.WdfHipError, match="mode 0"):
            call()


def test_channel_helper_on_cpu_tensors():
    from wdf_hip import binding as wb
    vals = torch.tensor([10.0e3, 45.0e3, 75.0e3])
    r = vals[torch.arange(7) % 3].reshape(7, 1).repeat(1, 33).contiguous()
    v = wb.r_per_sequence(r)
    assert tuple(v.shape) == (7,) and v.dtype == torch.float32 and v.is_contiguous()
    assert torch.equal(v, vals[torch.arange(7) % 3])
    assert wb.r_per_sequence(r) is v                        # one comparison per tensor: the answer is cached with it
    moving = r.clone()
    moving[3, 20] = 46.0e3
    with pytest.raises(wb.WdfHipError, match="one resistance per sequence"):
        wb.r_per_sequence(moving)
    r[2, 5] = 1.0                                           # in-place change: a new version of the same object is looked at again
    with pytest.raises(wb.WdfHipError, match="one resistance per sequence"):
        wb.r_per_sequence(r)
    with pytest.raises(wb.WdfHipError):
        wb.r_per_sequence(torch.ones(7))


def _tree(R=45.0e3, Cv=4.7e-9):
    import tf_wdf as W
    vs = W.ResistiveVoltageSource(R)
    cap = W.Capacitor(Cv, FS)
    return W, vs, cap, W.Parallel(vs, cap)


def test_circuit_takes_per_sequence_R_for_the_source_under_a_newton_solver():
    from wdf_hip.binding import WdfHipError
    for solver in ("newton_f32", "newton_f64"):
        W, vs, cap, P1 = _tree()
        circ = W.Circuit(P1, W.AsymDiodePair(P1, 4.352e-9, 2.0e-6, solver=solver), cap, per_sequence_R=vs)
        assert circ.per_sequence_R is vs and circ.per_sample_R is None and circ.root_kind == "AsymDiodePair"
        with pytest.raises(WdfHipError, match="resident"):
            circ.to_device()
    W, vs, cap, P1 = _tree()
    with pytest.raises(WdfHipError, match="top.P1"):        # the capacitor is no pot
        W.Circuit(P1, W.AsymDiodePair(P1, 4.352e-9, 2.0e-6), cap, per_sequence_R=cap)
    W, vs, cap, _ = _tree()
    S1 = W.Series(vs, cap)
    with pytest.raises(WdfHipError, match="clipper"):       # another tree
        W.Circuit(S1, W.AsymDiodePair(S1, 4.352e-9, 2.0e-6), cap, per_sequence_R=vs)
    W, vs, cap, P1 = _tree()
    with pytest.raises(WdfHipError, match="Newton"):
        W.Circuit(P1, W.AsymDiodePair(P1, 4.352e-9, 2.0e-6, solver="omega_f32"), cap, per_sequence_R=vs)
    W, vs, cap, P1 = _tree()
    with pytest.raises(WdfHipError, match="force_generic"):
        W.Circuit(P1, W.AsymDiodePair(P1, 4.352e-9, 2.0e-6), cap, per_sequence_R=vs, force_generic=True)
    W, vs, cap, P1 = _tree()
    with pytest.raises(WdfHipError, match="AsymDiodePair"):  # the symmetric pair streams its pot per sample
        W.Circuit(P1, W.DiodePair(P1, 4.352e-9), cap, per_sequence_R=vs)
    W, vs, cap, P1 = _tree()
    with pytest.raises(WdfHipError, match="per_sample_R.*per_sequence_R"):
        W.Circuit(P1, W.AsymDiodePair(P1, 4.352e-9, 2.0e-6), cap, per_sample_R=vs)


def test_the_plan_comes_from_the_largest_pot(monkeypatch):
    """Circuit._asym_inputs on CPU tensors: the [B] vector, a placeholder for theta6[4] that carries no gradient to vs.R, and
    the planner called with the largest pot of the batch (it forgets slowest: 1 - 2p, p = Rc / (R + Rc))."""
    from wdf_hip import engine
    from wdf_hip.binding import WdfHipError
    W, vs, cap, P1 = _tree()
    circ = W.Circuit(P1, W.AsymDiodePair(P1, 4.352e-9, 2.0e-6), cap, per_sequence_R=vs)
    B, T = 9, 64
    vals = torch.tensor([10.0e3, 45.0e3, 75.0e3])
    x = torch.zeros((B, T, 2), dtype=torch.float32)
    x[:, :, 1] = vals[torch.arange(B) % 3].reshape(B, 1)
    seen = []
    real = engine.plan_asym_time_parallel

    def spy(Bq, Tq, R, C, fs, **kw):
        seen.append((Bq, Tq, R, C, fs))
        return real(Bq, Tq, R, C, fs, **kw)
    monkeypatch.setattr(engine, "plan_asym_time_parallel", spy)
    theta6, xv, rseq, tp = circ._asym_inputs(x, x)
    assert seen == [(B, T, 75.0e3, pytest.approx(4.7e-9), FS)]
    assert tuple(xv.shape) == (B, T) and torch.equal(rseq, vals[torch.arange(B) % 3]) and isinstance(tp, engine.TpPlan)
    assert tuple(theta6.shape) == (6,) and float(theta6[4]) == 1.0
    Rc = 1.0 / (2.0 * 4.7e-9 * FS)
    assert (1.0 - 2.0 * Rc / (75.0e3 + Rc)) ** tp.warmup <= 1e-8 < (1.0 - 2.0 * Rc / (75.0e3 + Rc)) ** (tp.warmup // 4)
    x[4, 7, 1] = 1.0                                        # the channel now moves inside sequence 4
    with pytest.raises(WdfHipError, match="one resistance per sequence"):
        circ._asym_inputs(x, x)
    with pytest.raises(WdfHipError, match=r"\[B,T,2\]"):
        circ._asym_inputs(torch.zeros((B, T, 1)), None)


def test_steppers_key_on_the_pot():
    from wdf_hip import engine
    import inspect
    assert "pot" in inspect.signature(engine._ClipperAsymEsrFn.stepper).parameters
    for fn in (engine.clipper_asym, engine.clipper_asym_mse, engine.clipper_asym_mse_esr, engine.AsymMseStep.step_fused,
               engine.AsymEsrStep.step_fused):
        assert inspect.signature(fn).parameters["r"].default is None
    with pytest.raises(engine.binding.WdfHipError, match="one resistance per sequence"):
        engine._rseq_of(torch.ones(3), torch.zeros((4, 8)))
    assert np.array_equal(engine._rseq_of(torch.full((4, 8), 7.0), torch.zeros((4, 8))).numpy(), np.full(4, 7.0, np.float32))
