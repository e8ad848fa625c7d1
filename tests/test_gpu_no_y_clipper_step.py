"""GPU: the one-pass clipper step WITHOUT the y store (WDF_NO_Y_STORE; binding.clipper_step_mse_tp / _esr_tp with store_y=False).

Nothing but the two stores of y is compiled out, so everything the step hands back -- gradient, sums, loss values, zT, status,
the warm-start state, the Adam update -- is held against the references the storing step is held against, at the same bounds
(tests/test_gpu_fused_step.py: the fp64 oracle, the two-kernel step, torch autograd through the kernel pair for MSE + ESR), and
against the storing step on the same inputs.  Bit equality with the storing step is NOT asserted: dropping a use of y may change
how the compiler contracts a multiply-add.  (On one MI355X every case of this module gave the storing step's gradient, sums, loss
values and zT bit for bit: the `bits` entry of each printed line, run with -s.)  The no-y call repeated on the same inputs and
workspace must give the same bits.

Both lane widths run every test.  T = 40 cannot carry skip = 50 (skip <= T is an argument check): that shape masks 8 steps.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_fused_step as ref      # noqa: E402  (its helpers and bounds: two_kernel_step, _esr_reference, problem, dev, close_grad)

FS, Y_TOL, G_RTOL = ref.FS, ref.Y_TOL, ref.G_RTOL
dev, close_grad = ref.dev, ref.close_grad
EPS = float(np.finfo(float).eps)


@pytest.fixture(scope="module")
def wb():
    from wdf_hip import binding
    binding.require_gpu()
    return binding


@pytest.fixture(autouse=True, params=["two sequences per lane", "one sequence per lane"])
def lanes(request, wb):
    wb.ONE_SEQUENCE_PER_LANE = request.param.startswith("one")
    yield request.param
    wb.ONE_SEQUENCE_PER_LANE = False


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def clean(wb, st):
    s = wb.tp_status(st)
    assert s["n_bad"] == 0 and not s["fallback_ran"], s


_REFS = {}


def references(wb, oracle, B, T, K, W, n_up, n_down):
    """Computed once per case, shared by both lane widths, never written again."""
    key = (B, T, K, W, n_up, n_down)
    if key not in _REFS:
        lanes_now, wb.ONE_SEQUENCE_PER_LANE = wb.ONE_SEQUENCE_PER_LANE, False
        try:
            x, th, ths = ref.problem(B, T, seed=B + T)
            xd, thd = dev(x), dev(th)
            tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, n_up=n_up, n_down=n_down, want_stash=False)
            skip = 50 if T > 50 else 8
            _, g2, sse2 = ref.two_kernel_step(wb, xd, thd, tgt, 2.0 / (B * T), n_up=n_up, n_down=n_down)
            th64 = th.astype(np.float32).astype(np.float64)
            loss64, g64, _ = oracle.clipper_mse_step(th64, FS, x.astype(np.float64), tgt.cpu().numpy().astype(np.float64), n_up=n_up,
                                                     n_down=n_down, dtype=np.float64)
            _, ge, mse, esr, S, E = ref._esr_reference(wb, xd, thd, tgt, skip, n_up=n_up, n_down=n_down)
            _REFS[key] = dict(xd=xd, xt=xd.t().contiguous(), thd=thd, tgt=tgt, skip=skip, g2=g2.clone(), sse2=sse2, loss64=float(loss64),
                              g64=torch.as_tensor(np.asarray(g64)), ge=ge.clone(), mse=mse, esr=esr, S=S, E=E)
        finally:
            wb.ONE_SEQUENCE_PER_LANE = lanes_now
    return _REFS[key]


@pytest.mark.parametrize("B,T,K,W", [(3, 40, 1, 0), (2, 64, 2, 32), (70, 1001, 3, 248), (258, 1000, 2, 256), (64, 2048, 4, 256)])
@pytest.mark.parametrize("n_up,n_down", [(1, 1), (2, 3)])
def test_no_y_step_every_arm_of_the_dispatch(wb, oracle, B, T, K, W, n_up, n_down):
    r = references(wb, oracle, B, T, K, W, n_up, n_down)
    tgt, thd, skip = r["tgt"], r["thd"], r["skip"]
    gscale, n = 2.0 / (B * T), float(B * (T - skip))
    for time_major in (False, True):
        x = r["xt"] if time_major else r["xd"]
        kw = dict(n_up=n_up, n_down=n_down, time_major=time_major, want_zT=True)
        # ---- MSE
        y, zT, g, sse, st = wb.clipper_step_mse_tp(x, thd, FS, tgt, gscale, K, W, store_y=False, **kw)
        assert y is None
        clean(wb, st)
        ys, zTs, gs, sses, _ = wb.clipper_step_mse_tp(x, thd, FS, tgt, gscale, K, W, **kw)
        e = dict(oracle_g=float((g.double().cpu() - r["g64"]).abs().div(r["g64"].abs()).max()), oracle_loss=rel(float(sse) / (B * T), r["loss64"]),
                 pair_g=float((g - r["g2"]).abs().div(r["g2"].abs()).max()), pair_sse=rel(sse, r["sse2"]),
                 storing_g=float((g - gs).abs().div(gs.abs()).max()), storing_zT=float((zT - zTs).abs().max()),
                 bits=bool(torch.equal(g, gs) and torch.equal(sse, sses) and torch.equal(zT, zTs)))
        print(f"mse B={B} T={T} K={K} tm={time_major} ({n_up},{n_down}): {e}")
        ok, info = close_grad(g.cpu(), r["g64"])
        assert ok, info
        assert e["oracle_loss"] <= 1e-5
        ok, info = close_grad(g, r["g2"])
        assert ok, info
        assert e["pair_sse"] <= 2e-5
        ok, info = close_grad(g, gs, rtol=2e-5)
        assert ok, info
        assert e["storing_zT"] <= Y_TOL
        _, zT2, g2, sse2, st2 = wb.clipper_step_mse_tp(x, thd, FS, tgt, gscale, K, W, store_y=False, **kw)
        assert torch.equal(g2, g) and torch.equal(sse2, sse) and torch.equal(zT2, zT) and torch.equal(st2, st)
        # ---- MSE + ESR past skip
        y, zT, s10, g, l3, st = wb.clipper_step_esr_tp(x, thd, FS, tgt, n, EPS, skip, K, W, store_y=False, **kw)
        assert y is None
        clean(wb, st)
        _, zTs, s10s, gs, l3s, _ = wb.clipper_step_esr_tp(x, thd, FS, tgt, n, EPS, skip, K, W, **kw)
        l, s = l3.cpu().numpy(), s10.cpu().numpy()
        e = dict(autograd_g=float((g - r["ge"]).abs().div(r["ge"].abs()).max()), mse=rel(l[0], r["mse"]), esr=rel(l[1], r["esr"]),
                 S=rel(s[0], r["S"]), E=rel(s[1], r["E"]), storing_g=float((g - gs).abs().div(gs.abs()).max()),
                 storing_zT=float((zT - zTs).abs().max()), bits=bool(torch.equal(g, gs) and torch.equal(s10, s10s) and torch.equal(l3, l3s)))
        print(f"esr B={B} T={T} K={K} tm={time_major} ({n_up},{n_down}): {e}")
        ok, info = close_grad(g, r["ge"])
        assert ok, info
        assert e["mse"] <= 2e-5 and e["esr"] <= 2e-5 and rel(l[2], r["mse"] + r["esr"]) <= 2e-5
        assert e["S"] <= 2e-5 and e["E"] <= 2e-5
        ok, info = close_grad(g, gs, rtol=2e-5)
        assert ok, info
        assert e["storing_zT"] <= Y_TOL
        r2 = wb.clipper_step_esr_tp(x, thd, FS, tgt, n, EPS, skip, K, W, store_y=False, **kw)
        assert torch.equal(r2[2], s10) and torch.equal(r2[3], g) and torch.equal(r2[4], l3) and torch.equal(r2[1], zT)


def test_no_y_per_sample_resistance_and_skip(wb):
    """test_fused_per_sample_resistance_and_skip's shape: the streamed resistance channel (DYN_R = 1), both layouts, both losses."""
    B, T, K, W, skip = 71, 1024, 2, 256, 50
    x, th, ths = ref.problem(B, T, seed=3)
    xd, thd = dev(x), dev(th)
    r = dev(45.0e3 * np.exp(0.8 * np.sin(np.arange(T)[None, :] * 0.01 * (1 + np.arange(B)[:, None] % 5))))
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, r=r, want_stash=False)
    gscale, n = 2.0 / (B * (T - skip)), float(B * (T - skip))
    _, g_ref, sse_ref = ref.two_kernel_step(wb, xd, thd, tgt, gscale, r=r, skip=skip)
    _, ge_ref, mse, esr, S, E = ref._esr_reference(wb, xd, thd, tgt, skip, r=r)
    for time_major in (False, True):
        xin, rin = (xd.t().contiguous(), r.t().contiguous()) if time_major else (xd, r)
        y, zT, g, sse, st = wb.clipper_step_mse_tp(xin, thd, FS, tgt, gscale, K, W, r=rin, skip=skip, time_major=time_major, want_zT=True,
                                                   store_y=False)
        assert y is None and wb.tp_status(st)["n_bad"] == 0
        ok, info = close_grad(g[[0, 1, 3]], g_ref[[0, 1, 3]])            # dL/dR is identically 0 with a streamed resistance
        assert ok and float(g[2]) == 0.0, info
        assert rel(sse, sse_ref) <= 2e-5
        _, zTs, gs, _, _ = wb.clipper_step_mse_tp(xin, thd, FS, tgt, gscale, K, W, r=rin, skip=skip, time_major=time_major, want_zT=True)
        ok, info = close_grad(g[[0, 1, 3]], gs[[0, 1, 3]], rtol=2e-5)
        assert ok, info
        assert float((zT - zTs).abs().max()) <= Y_TOL
        y, _, s10, g, l3, st = wb.clipper_step_esr_tp(xin, thd, FS, tgt, n, EPS, skip, K, W, r=rin, time_major=time_major, store_y=False)
        assert y is None and wb.tp_status(st)["n_bad"] == 0
        ok, info = close_grad(g[[0, 1, 3]], ge_ref[[0, 1, 3]])
        assert ok and float(g[2]) == 0.0, info
        l, s = l3.cpu().numpy(), s10.cpu().numpy()
        assert rel(l[0], mse) <= 2e-5 and rel(l[1], esr) <= 2e-5 and rel(s[0], S) <= 2e-5 and rel(s[1], E) <= 2e-5


@pytest.mark.parametrize("time_major", [True, False])
@pytest.mark.parametrize("n_up,n_down", [(1, 1), (1, 2)])
def test_no_y_one_pot_value_per_sequence(wb, time_major, n_up, n_down):
    """test_fused_one_pot_value_per_sequence's shape: WDF_R_PER_SEQUENCE (DYN_R = 2), against the per-sample evaluation of the
    same data through the two-kernel step and against the storing step."""
    from wdf_hip import workload
    B, T, K, W, skip = 200, 2048, 8, 448, 50
    x, th, ths = ref.problem(B, T, seed=13)
    xd, rd, thd = dev(x), dev(workload.dataset_resistance_batch(B, T)), dev(th)
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, r=rd, n_up=n_up, n_down=n_down, want_stash=False)
    xin, rin = (xd.t().contiguous(), rd.t().contiguous()) if time_major else (xd, rd)
    assert wb.r_is_per_sequence(rin, time_major)
    gscale, n = 2.0 / (B * T), float(B * (T - skip))
    kw = dict(r=rin, n_up=n_up, n_down=n_down, time_major=time_major)
    _, g_ref, sse_ref = ref.two_kernel_step(wb, xd, thd, tgt, gscale, r=rd, n_up=n_up, n_down=n_down)
    y, zT, g, sse, st = wb.clipper_step_mse_tp(xin, thd, FS, tgt, gscale, K, W, want_zT=True, store_y=False, **kw)
    assert y is None and wb.tp_status(st)["n_bad"] == 0
    ok, info = close_grad(g[[0, 1, 3]], g_ref[[0, 1, 3]])
    assert ok and float(g[2]) == 0.0, info
    assert rel(sse, sse_ref) <= 2e-5
    _, zTs, gs, sses, _ = wb.clipper_step_mse_tp(xin, thd, FS, tgt, gscale, K, W, want_zT=True, **kw)
    ok, info = close_grad(g[[0, 1, 3]], gs[[0, 1, 3]], rtol=2e-5)
    assert ok, info
    assert float((zT - zTs).abs().max()) <= Y_TOL
    y, _, s10, ge, l3, st = wb.clipper_step_esr_tp(xin, thd, FS, tgt, n, EPS, skip, K, W, store_y=False, **kw)
    _, _, s10s, ges, l3s, _ = wb.clipper_step_esr_tp(xin, thd, FS, tgt, n, EPS, skip, K, W, **kw)
    assert y is None and wb.tp_status(st)["n_bad"] == 0
    ok, info = close_grad(ge[[0, 1, 3]], ges[[0, 1, 3]], rtol=2e-5)
    assert ok, info
    assert float((l3 - l3s).abs().max()) <= 1e-5 * float(l3s.abs().max())


def test_no_y_initial_state_general_root_and_accumulate(wb):
    B, T, K, W = 64, 1024, 4, 256
    x, th, ths = ref.problem(B, T, seed=2)
    xd, thd = dev(x), dev(th)
    z0 = dev(np.random.default_rng(0).uniform(-0.3, 0.3, B))
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, want_stash=False)
    gscale = 2.0 / (B * T)
    _, g_ref, _ = ref.two_kernel_step(wb, xd, thd, tgt, gscale, z0=z0)
    y, zT, g, _, st = wb.clipper_step_mse_tp(xd, thd, FS, tgt, gscale, K, W, z0=z0, want_zT=True, store_y=False)
    assert y is None and wb.tp_status(st)["n_bad"] == 0
    ok, info = close_grad(g, g_ref)
    assert ok, info
    _, _, zT_ref = wb.clipper_fwd(xd, thd, FS, z0=z0, want_stash=False, want_zT=True)
    assert float((zT - zT_ref).abs().max()) <= Y_TOL
    wb.GENERAL_ROOT = True
    try:
        _, zT_g, g_g, _, _ = wb.clipper_step_mse_tp(xd, thd, FS, tgt, gscale, K, W, z0=z0, want_zT=True, store_y=False)
    finally:
        wb.GENERAL_ROOT = False
    ok, info = close_grad(g_g, g, rtol=2e-5)
    assert ok, info
    assert float((zT_g - zT).abs().max()) <= 1e-6
    acc = g.clone()
    wb.clipper_step_mse_tp(xd, thd, FS, tgt, gscale, K, W, z0=z0, gtheta=acc, accumulate=True, store_y=False)
    assert torch.allclose(acc, 2.0 * g, rtol=1e-6, atol=0)


def test_no_y_repairs_when_warmup_is_too_short(wb):
    """test_fused_repairs_when_warmup_is_too_short's set-up: every boundary is missed, the finish launch's wave 0 re-runs the
    chunks from the exact state (records, snapshots, zT -- no outputs), and the step equals the sequential computation."""
    from wdf_hip import workload
    B, T, K = 70, 2048, 8
    x = workload.sweep_batch(B, T, seed=11)
    theta = workload.clipper_theta()
    theta[3] = 1.0e-6
    ths = workload.target_theta()
    ths[3] = 1.1e-6
    xd, thd = dev(x), dev(theta)
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, want_stash=False)
    gscale = 2.0 / (B * T)
    _, g_ref, sse_ref = ref.two_kernel_step(wb, xd, thd, tgt, gscale)
    _, _, zT_ref = wb.clipper_fwd(xd, thd, FS, want_stash=False, want_zT=True)
    y, zT, g, sse, st = wb.clipper_step_mse_tp(xd, thd, FS, tgt, gscale, K, 64, want_zT=True, store_y=False)
    s = wb.tp_status(st)
    assert y is None
    assert s["n_bad"] > 0 and s["repaired_tiles"] == 2 * 7, s     # 7 boundaries x (2 waves | 2 interleaved halves of one wave)
    ok, info = close_grad(g, g_ref, rtol=5e-5)
    assert ok, info
    assert rel(sse, sse_ref) <= 2e-5
    assert float((zT - zT_ref).abs().max()) <= Y_TOL
    # MSE + ESR through the same repair
    n = float(B * (T - 50))
    _, ge_ref, mse, esr, S, E = ref._esr_reference(wb, xd, thd, tgt, 50)
    _, _, s10, ge, l3, st = wb.clipper_step_esr_tp(xd, thd, FS, tgt, n, EPS, 50, K, 64, store_y=False)
    assert wb.tp_status(st)["repaired_tiles"] == 2 * 7
    ok, info = close_grad(ge, ge_ref)
    assert ok, info
    assert rel(l3[0], mse) <= 2e-5 and rel(l3[1], esr) <= 2e-5 and rel(s10[0], S) <= 2e-5 and rel(s10[1], E) <= 2e-5
    # the tickets were left clean: the same workspace serves good calls afterwards, with and without y
    ws = wb.step_mse_workspace(B, K, xd.device)
    for W, store in ((64, False), (64, True), (4096, False)):
        _, _, g2, _, _ = wb.clipper_step_mse_tp(xd, thd, FS, tgt, gscale, K, W, ws=ws, store_y=store)
        ok, info = close_grad(g2, g_ref, rtol=5e-5)
        assert ok, info


def test_no_y_warm_started_training_loop_with_adam(wb):
    """test_fused_warm_started_training_loop_with_adam in small: the same loop with and without the y store, each with its own
    warm-start state and optimizer; theta after the loop agrees at that test's bound for theta (1e-6 relative)."""
    B, T, K, W, steps = 128, 2048, 8, 256, 6
    x, th0, ths = ref.problem(B, T, seed=5)
    xd = dev(x)
    xt = xd.t().contiguous()
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, want_stash=False)
    gscale = 2.0 / (B * T)
    lr = [1e-3 * float(v) for v in th0]
    lo, hi = [1e-15, 1e-3, 180.0, 1e-13], [1e-3, 1.0, 1.0e6, 1.0]
    thetas, losses = {}, {}
    for store in (True, False):
        theta = dev(th0)
        state = wb.TpWarmState(B, T, K, 256 // wb.warm_unit(), xd.device)
        ws = wb.step_mse_workspace(B, K, xd.device)
        opt = wb.Adam(4, lr=lr, lo=lo, hi=hi, device=xd.device)
        hist = []
        for it in range(steps):
            th_before = theta.clone()
            y, _, g, sse, st = wb.clipper_step_mse_tp(xt, theta, FS, tgt, gscale, K, W, ws=ws, state=state, opt=opt, time_major=True,
                                                      store_y=store)
            assert (y is None) == (not store)
            if not store:
                _, g_ref, _ = ref.two_kernel_step(wb, xd, th_before, tgt, gscale)
                ok, info = close_grad(g, g_ref)
                assert ok, (it, info)
            if it >= 2:
                assert wb.tp_status(st)["n_bad"] == 0, (it, wb.tp_status(st))
            hist.append(float(sse))
        info = state.info()
        assert info["valid"] == 3 and info["n_calls"] == steps
        thetas[store], losses[store] = theta.clone(), hist
    assert losses[False][-1] < losses[False][0]
    # (Adam's step is lr m / sqrt(v): gradients that agree to 2e-5 move theta by lr x 2e-5 = 2e-8 of itself per step at most)
    assert torch.allclose(thetas[False], thetas[True], rtol=1e-6, atol=0), (thetas, losses)


def test_no_y_two_stage_esr_finish(wb):
    B, T, K, W, skip = 130, 2048, 8, 256, 50
    x, th, ths = ref.problem(B, T, seed=B + T + 1)
    xd, thd = dev(x), dev(th)
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, want_stash=False)
    n = float(B * (T - skip))
    _, _, s10, g, l3, _ = wb.clipper_step_esr_tp(xd, thd, FS, tgt, n, EPS, skip, K, W, store_y=False)
    y, _, s10b, g_none, l_none, _ = wb.clipper_step_esr_tp(xd, thd, FS, tgt, n, EPS, skip, K, W, finish=False, store_y=False)
    assert y is None and g_none is None and l_none is None and torch.equal(s10b, s10)
    g2, l2 = wb.esr_finish(s10b, n, EPS)
    assert torch.allclose(g2, g, rtol=1e-6, atol=0) and torch.allclose(l2, l3, rtol=1e-6, atol=0)


def _no_y_bits(one_per_lane):
    """A no-y MSE and MSE + ESR call at a shape the group form would take (time-major x, 8 chunks): every result, as hex."""
    from wdf_hip import binding as wb
    old, wb.ONE_SEQUENCE_PER_LANE = wb.ONE_SEQUENCE_PER_LANE, bool(one_per_lane)
    try:
        B, T, K, W = 130, 2048, 8, 256
        x, th, ths = ref.problem(B, T, seed=7)
        xt = dev(x).t().contiguous()
        tgt, _, _ = wb.clipper_fwd(dev(x), dev(ths), FS, want_stash=False)
        _, zT, g, sse, st = wb.clipper_step_mse_tp(xt, dev(th), FS, tgt, 2.0 / (B * T), K, W, time_major=True, want_zT=True, store_y=False)
        _, _, s10, ge, l3, _ = wb.clipper_step_esr_tp(xt, dev(th), FS, tgt, float(B * (T - 50)), EPS, 50, K, W, time_major=True, store_y=False)
        torch.cuda.synchronize()
        return torch.cat((g, sse, zT, s10, ge, l3)).cpu().numpy().tobytes().hex() + " " + str(st.cpu().tolist())
    finally:
        wb.ONE_SEQUENCE_PER_LANE = old


_CHILD = """
import sys
sys.path[:0] = {paths!r}
import test_gpu_no_y_clipper_step as m
print("BITS", m._no_y_bits({one!r}))
"""


def test_no_y_ignores_the_finish_form_switch(wb, lanes, monkeypatch):
    """WDF_FUSED_FINISH=group in the environment of a fresh process: a no-y call takes the finish launch whatever the switch
    says, so the child's results are this process's (no switch set), bit for bit.  (The storing step WOULD take the group form at
    this shape: tests/test_gpu_fused_group_finish.py.)"""
    from wdf_hip import binding
    monkeypatch.delenv("WDF_FUSED_FINISH", raising=False)
    here = _no_y_bits(lanes.startswith("one"))
    paths = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(binding.__file__)))]
    code = _CHILD.format(paths=paths, one=lanes.startswith("one"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, WDF_FUSED_FINISH="group"), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    bits = [ln[5:] for ln in out.stdout.splitlines() if ln.startswith("BITS ")]
    assert bits == [here]


def test_engine_mse_step_without_output(wb):
    from wdf_hip import engine
    B, T, skip = 128, 2048, 50
    x, th, ths = ref.problem(B, T, seed=9)
    xd = dev(x)
    xt = xd.t().contiguous()
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, want_stash=False)
    plan = engine.TpPlan(8, 192, 1e-6, 8)
    for loss, kw in (("mse", {}), ("mse+esr", dict(skip=skip))):
        noy = engine.MseStep(B, T, FS, plan, xd.device, time_major=True, loss=loss, warm=True, store_output=False, **kw)
        sto = engine.MseStep(B, T, FS, plan, xd.device, time_major=True, loss=loss, warm=True, **kw)
        theta = dev(th)
        for _ in range(3):
            sse, g = noy.step_fused(theta, xt, tgt)
            sse_s, g_s = sto.step_fused(theta, xt, tgt)
        assert noy.y is None and sto.y is not None
        assert wb.tp_status(noy.status)["n_bad"] == 0
        ok, info = close_grad(g, g_s, rtol=2e-5)
        assert ok, info
        assert rel(sse, sse_s) <= 2e-5
        if loss == "mse+esr":
            assert torch.allclose(noy.loss, sto.loss, rtol=2e-5, atol=0)
        for call in (lambda: noy.forward(theta, xt), lambda: noy.backward(theta, xt, tgt), lambda: noy.step(theta, xt, tgt)):
            with pytest.raises(wb.WdfHipError, match="store_output=False"):
                call()
    # the sharded form: the ten sums go through the all-reduce hook between the pass and its finish
    seen = []
    shard = engine.MseStep(B, T, FS, plan, xd.device, time_major=True, loss="mse+esr", skip=skip, store_output=False,
                           sums_allreduce=lambda s: seen.append(s.clone()))
    one = engine.MseStep(B, T, FS, plan, xd.device, time_major=True, loss="mse+esr", skip=skip, store_output=False)
    shard.step_fused(dev(th), xt, tgt)
    one.step_fused(dev(th), xt, tgt)
    assert shard.y is None and len(seen) == 1 and seen[0].numel() == 10
    assert torch.allclose(shard.gtheta, one.gtheta, rtol=1e-6, atol=0) and torch.allclose(shard.loss, one.loss, rtol=1e-6, atol=0)
