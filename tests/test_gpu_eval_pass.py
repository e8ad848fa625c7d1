"""GPU: the clipper's loss-only evaluation pass at kernel level (binding.clipper_eval_tp -> wdf_clipper_eval_tp,
csrc/wdf_clipper_eval.h), both lane widths.

References and bounds are the project's own for the same quantities: y and zT within Y_TOL of the sequential clipper_fwd;
S, E, mse and esr within 2e-5 relative of the fp64 sums over that y and of the storing one-pass step's sums10[0:2] / loss3; the
MSE within 1e-5 relative of the fp64 oracle's loss; a repeated call on the same workspace gives the same bits, the status word
included.  Clean cases assert n_bad == 0 and no re-run: a result the repair produced does not count as the chunked path's.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_fused_step as ref      # noqa: E402  (its helpers and bounds: problem, dev, Y_TOL)
from test_gpu_fused_step import lanes  # noqa: E402,F401  (autouse: every test runs with two sequences per lane and with one)

FS, Y_TOL = ref.FS, ref.Y_TOL
dev = ref.dev
EPS = float(np.finfo(float).eps)
SUM_RTOL = 2e-5


@pytest.fixture(scope="module")
def wb():
    from wdf_hip import binding
    binding.require_gpu()
    return binding


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def clean(wb, st):
    s = wb.tp_status(st)
    assert s["n_bad"] == 0 and not s["fallback_ran"], s


def sums64(y, tgt, skip):
    o, t = y[skip:].double(), tgt[skip:].double()
    S, E = float(((o - t) ** 2).sum()), float((o ** 2).sum())
    n = float(o.numel())
    return S, E, S / n, float(np.sqrt(S / (E + EPS) / n))


def check_sums(sums, l3, S, E, mse, esr, what=""):
    s, l = sums.cpu().numpy(), l3.cpu().numpy()
    e = dict(S=rel(s[0], S), E=rel(s[1], E), mse=rel(l[0], mse), esr=rel(l[1], esr), sum=rel(l[2], mse + esr))
    print(f"{what}: {e}")
    assert max(e.values()) <= SUM_RTOL, (what, e)
    return e


_REFS = {}


def references(wb, oracle, B, T, n_up, n_down):
    """Computed once per case, shared by both lane widths and every chunking, never written again."""
    key = (B, T, n_up, n_down)
    if key not in _REFS:
        lanes_now, wb.ONE_SEQUENCE_PER_LANE = wb.ONE_SEQUENCE_PER_LANE, False
        try:
            x, th, ths = ref.problem(B, T, seed=B + T)
            xd, thd = dev(x), dev(th)
            tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, n_up=n_up, n_down=n_down, want_stash=False)
            y, _, zT = wb.clipper_fwd(xd, thd, FS, n_up=n_up, n_down=n_down, want_stash=False, want_zT=True)
            skip = 50 if T > 50 else 8
            th64 = th.astype(np.float32).astype(np.float64)
            loss64, _, _ = oracle.clipper_mse_step(th64, FS, x.astype(np.float64), tgt.cpu().numpy().astype(np.float64), n_up=n_up,
                                                   n_down=n_down, dtype=np.float64)
            _REFS[key] = dict(xd=xd, xt=xd.t().contiguous(), thd=thd, tgt=tgt, y=y, zT=zT, skip=skip, loss64=float(loss64),
                              past=sums64(y, tgt, skip), all=sums64(y, tgt, 0))
        finally:
            wb.ONE_SEQUENCE_PER_LANE = lanes_now
    return _REFS[key]


@pytest.mark.parametrize("B,T,K,W", [(3, 40, 1, 0), (2, 64, 2, 32), (70, 1001, 3, 248), (258, 1000, 2, 256), (64, 2048, 4, 256)])
@pytest.mark.parametrize("n_up,n_down", [(1, 1), (2, 3)])
def test_eval_pass_every_arm_of_the_dispatch(wb, oracle, B, T, K, W, n_up, n_down):
    r = references(wb, oracle, B, T, n_up, n_down)
    tgt, thd, skip = r["tgt"], r["thd"], r["skip"]
    n = float(B * (T - skip))
    th_before = thd.clone()
    for time_major in (False, True):
        x = r["xt"] if time_major else r["xd"]
        kw = dict(n_up=n_up, n_down=n_down, time_major=time_major, want_zT=True)
        # the storing one-pass step on the same inputs: its sums10[0:2] and loss3
        _, _, s10, _, l3s, _ = wb.clipper_step_esr_tp(x, thd, FS, tgt, n, EPS, skip, K, W, **kw)
        for store in (True, False):
            what = f"B={B} T={T} K={K} tm={time_major} ({n_up},{n_down}) store_y={store}"
            ws = wb.eval_workspace(B, wb.lib().wdf_clipper_tp_chunks(T, K), x.device)
            y, zT, sums, l3, st = wb.clipper_eval_tp(x, thd, FS, tgt, n, EPS, skip, K, W, store_y=store, ws=ws, **kw)
            clean(wb, st)
            assert (y is None) == (not store) and sums.dtype == torch.float64
            if store:
                assert float((y - r["y"]).abs().max()) <= Y_TOL
            assert float((zT - r["zT"]).abs().max()) <= Y_TOL
            check_sums(sums, l3, *r["past"], what=what)
            assert rel(sums[0], s10[0]) <= SUM_RTOL and rel(sums[1], s10[1]) <= SUM_RTOL
            assert float((l3 - l3s).abs().div(l3s.abs()).max()) <= SUM_RTOL
            # the same call on the same workspace: the same bits, the status word included
            y2, zT2, sums2, l32, st2 = wb.clipper_eval_tp(x, thd, FS, tgt, n, EPS, skip, K, W, store_y=store, ws=ws, **kw)
            assert torch.equal(sums2, sums) and torch.equal(l32, l3) and torch.equal(zT2, zT) and torch.equal(st2, st)
            assert not store or torch.equal(y2, y)
            # the plain MSE (skip = 0, n = B T) against the fp64 oracle's loss
            _, _, sums0, l30, st0 = wb.clipper_eval_tp(x, thd, FS, tgt, float(B * T), EPS, 0, K, W, store_y=store, ws=ws, **kw)
            clean(wb, st0)
            assert rel(l30[0], r["loss64"]) <= 1e-5
            check_sums(sums0, l30, *r["all"], what=what + " skip=0")
    assert torch.equal(thd, th_before)                              # theta is const


def test_eval_pass_streamed_resistance(wb):
    """A per-sample resistance channel (DYN_R = 1), both layouts."""
    B, T, K, W, skip = 71, 1024, 2, 256, 50
    x, th, ths = ref.problem(B, T, seed=3)
    xd, thd = dev(x), dev(th)
    r = dev(45.0e3 * np.exp(0.8 * np.sin(np.arange(T)[None, :] * 0.01 * (1 + np.arange(B)[:, None] % 5))))
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, r=r, want_stash=False)
    y_ref, _, zT_ref = wb.clipper_fwd(xd, thd, FS, r=r, want_stash=False, want_zT=True)
    n = float(B * (T - skip))
    want = sums64(y_ref, tgt, skip)
    for time_major in (False, True):
        xin, rin = (xd.t().contiguous(), r.t().contiguous()) if time_major else (xd, r)
        assert not wb.r_is_per_sequence(rin, time_major)
        for store in (True, False):
            y, zT, sums, l3, st = wb.clipper_eval_tp(xin, thd, FS, tgt, n, EPS, skip, K, W, r=rin, time_major=time_major, want_zT=True,
                                                     store_y=store)
            clean(wb, st)
            assert y is None or float((y - y_ref).abs().max()) <= Y_TOL
            assert float((zT - zT_ref).abs().max()) <= Y_TOL
            check_sums(sums, l3, *want, what=f"streamed r tm={time_major} store_y={store}")


@pytest.mark.parametrize("time_major", [True, False])
@pytest.mark.parametrize("n_up,n_down", [(1, 1), (1, 2)])
def test_eval_pass_one_pot_value_per_sequence(wb, time_major, n_up, n_down):
    """WDF_R_PER_SEQUENCE (DYN_R = 2; the binding observes it on the channel) against the sequential per-sample evaluation."""
    from wdf_hip import workload
    B, T, K, W, skip = 200, 2048, 8, 448, 50
    x, th, ths = ref.problem(B, T, seed=13)
    xd, rd, thd = dev(x), dev(workload.dataset_resistance_batch(B, T)), dev(th)
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, r=rd, n_up=n_up, n_down=n_down, want_stash=False)
    y_ref, _, zT_ref = wb.clipper_fwd(xd, thd, FS, r=rd, n_up=n_up, n_down=n_down, want_stash=False, want_zT=True)
    xin, rin = (xd.t().contiguous(), rd.t().contiguous()) if time_major else (xd, rd)
    assert wb.r_is_per_sequence(rin, time_major)
    n = float(B * (T - skip))
    want = sums64(y_ref, tgt, skip)
    for store in (True, False):
        y, zT, sums, l3, st = wb.clipper_eval_tp(xin, thd, FS, tgt, n, EPS, skip, K, W, r=rin, n_up=n_up, n_down=n_down,
                                                 time_major=time_major, want_zT=True, store_y=store)
        clean(wb, st)
        assert y is None or float((y - y_ref).abs().max()) <= Y_TOL
        assert float((zT - zT_ref).abs().max()) <= Y_TOL
        check_sums(sums, l3, *want, what=f"r per sequence tm={time_major} ({n_up},{n_down}) store_y={store}")


def test_eval_pass_initial_state_and_general_root(wb):
    B, T, K, W, skip = 64, 1024, 4, 256, 50
    x, th, ths = ref.problem(B, T, seed=2)
    xd, thd = dev(x), dev(th)
    z0 = dev(np.random.default_rng(0).uniform(-0.3, 0.3, B))
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, want_stash=False)
    y_ref, _, zT_ref = wb.clipper_fwd(xd, thd, FS, z0=z0, want_stash=False, want_zT=True)
    n = float(B * (T - skip))
    want = sums64(y_ref, tgt, skip)
    y, zT, sums, l3, st = wb.clipper_eval_tp(xd, thd, FS, tgt, n, EPS, skip, K, W, z0=z0, want_zT=True)
    clean(wb, st)
    assert float((y - y_ref).abs().max()) <= Y_TOL and float((zT - zT_ref).abs().max()) <= Y_TOL
    check_sums(sums, l3, *want, what="z0")
    wb.GENERAL_ROOT = True
    try:
        yg, zTg, sumsg, l3g, stg = wb.clipper_eval_tp(xd, thd, FS, tgt, n, EPS, skip, K, W, z0=z0, want_zT=True)
        _, _, sumsn, l3n, _ = wb.clipper_eval_tp(xd, thd, FS, tgt, n, EPS, skip, K, W, z0=z0, store_y=False)
    finally:
        wb.GENERAL_ROOT = False
    clean(wb, stg)
    assert float((yg - y_ref).abs().max()) <= Y_TOL and float((zTg - zT_ref).abs().max()) <= Y_TOL
    check_sums(sumsg, l3g, *want, what="z0, general root")
    check_sums(sumsn, l3n, *want, what="z0, general root, no y")


@pytest.mark.parametrize("is_scale,tier", [(1.0, "lean"), (2.9, "lean"), (3.05, "fast"), (1.0e-3, "lean"), (40.0, "fast")])
def test_eval_pass_across_the_tier_boundary(wb, oracle, is_scale, tier):
    """test_root_tiers_against_the_oracle_across_the_tier_boundary's circuits: y against the fp64 oracle, the MSE against its loss."""
    B, T, K, W = 96, 2048, 8, 256
    x, th, ths = ref.problem(B, T, seed=23)
    th, ths = th.copy(), ths.copy()
    th[0] *= is_scale
    ths[0] *= is_scale
    th32 = th.astype(np.float32).astype(np.float64)
    Rp = 1.0 / (1.0 / th32[2] + 2.0 * th32[3] * FS)
    assert (np.log(Rp * th32[0] / th32[1]) <= -7.5) == (tier == "lean")
    tgt64 = oracle.clipper_fwd(ths.astype(np.float64), FS, x.astype(np.float64))
    loss_ref, _, y_ref = oracle.clipper_mse_step(th32, FS, x.astype(np.float64), tgt64.astype(np.float32).astype(np.float64), dtype=np.float64)
    tgt = dev(tgt64)
    for store in (True, False):
        y, _, sums, l3, st = wb.clipper_eval_tp(dev(x), dev(th), FS, tgt, float(B * T), EPS, 0, K, W, store_y=store)
        clean(wb, st)
        assert y is None or float(np.max(np.abs(y.cpu().numpy() - y_ref))) <= Y_TOL
        assert rel(l3[0], loss_ref) <= 1e-5
    ys, _, _ = wb.clipper_fwd(dev(x), dev(th), FS, want_stash=False)
    check_sums(sums, l3, *sums64(ys, tgt, 0), what=f"Is x {is_scale} ({tier})")


def test_eval_pass_repairs_when_warmup_is_too_short(wb):
    """test_fused_repairs_when_warmup_is_too_short's inputs: every boundary is missed (the forward arithmetic is the step's, so
    the same boundaries miss), the finish launch re-runs the chunks from the exact state, and the results are the sequential ones."""
    from wdf_hip import workload
    B, T, K, skip = 70, 2048, 8, 50
    x = workload.sweep_batch(B, T, seed=11)
    theta = workload.clipper_theta()
    theta[3] = 1.0e-6
    ths = workload.target_theta()
    ths[3] = 1.1e-6
    xd, thd = dev(x), dev(theta)
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, want_stash=False)
    y_ref, _, zT_ref = wb.clipper_fwd(xd, thd, FS, want_stash=False, want_zT=True)
    n = float(B * (T - skip))
    want = sums64(y_ref, tgt, skip)
    ws = wb.eval_workspace(B, K, xd.device)
    for store in (True, False):
        y, zT, sums, l3, st = wb.clipper_eval_tp(xd, thd, FS, tgt, n, EPS, skip, K, 64, want_zT=True, store_y=store, ws=ws)
        s = wb.tp_status(st)
        assert s["n_bad"] > 0 and s["repaired_tiles"] == 2 * 7, s     # 7 boundaries x (2 waves | 2 interleaved halves of one wave)
        assert y is None or float((y - y_ref).abs().max()) <= Y_TOL
        assert float((zT - zT_ref).abs().max()) <= Y_TOL
        check_sums(sums, l3, *want, what=f"repaired, store_y={store}")
    # the tickets were left clean: the same workspace serves clean calls afterwards
    for W, store in ((4096, True), (4096, False)):
        y, _, sums, l3, st = wb.clipper_eval_tp(xd, thd, FS, tgt, n, EPS, skip, K, W, store_y=store, ws=ws)
        clean(wb, st)
        check_sums(sums, l3, *want, what=f"after the repair, store_y={store}")


def test_eval_pass_warm_started_sequence(wb):
    """A TpWarmState over a sequence of calls, time-major: theta moves by small steps, then jumps as in
    test_fused_warm_started_training_loop_with_adam (repaired), then stands still (no miss).  Every call against the sequential
    forward at the same theta."""
    B, T, K, W, skip = 128, 4096, 16, 256, 50
    x, th0, ths = ref.problem(B, T, seed=5)
    xd = dev(x)
    xt = xd.t().contiguous()
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, want_stash=False)
    n = float(B * (T - skip))
    theta = dev(th0)
    state = wb.TpWarmState(B, T, K, 256 // wb.warm_unit(), xd.device)
    ws = wb.eval_workspace(B, K, xd.device)
    small = torch.tensor([1.0 - 1e-3, 1.0 + 5e-4, 1.0 - 1e-3, 1.0 + 1e-3], device="cuda")
    calls = 0
    for it in range(12):
        if it == 8:                                                  # a jump the snapshots cannot follow
            theta = theta * torch.tensor([1.5, 1.1, 0.6, 1.6], device="cuda")
        elif it > 0:
            theta = theta * small
        store = it % 2 == 0
        y, zT, sums, l3, st = wb.clipper_eval_tp(xt, theta, FS, tgt, n, EPS, skip, K, W, ws=ws, state=state, time_major=True, want_zT=True,
                                                 store_y=store)
        calls += 1
        s = wb.tp_status(st)
        y_ref, _, zT_ref = wb.clipper_fwd(xd, theta, FS, want_stash=False, want_zT=True)
        assert y is None or float((y - y_ref).abs().max()) <= Y_TOL, (it, s)
        assert float((zT - zT_ref).abs().max()) <= Y_TOL, (it, s)
        check_sums(sums, l3, *sums64(y_ref, tgt, skip), what=f"warm call {it} {s}")
        if it == 8:
            assert s["n_bad"] > 0 and s["repaired_tiles"] > 0, s
        elif it >= 2:
            assert s["n_bad"] == 0, (it, s)
    # theta stands still: plain warm start from the snapshots, no miss
    y_ref, _, _ = wb.clipper_fwd(xd, theta, FS, want_stash=False)
    for _ in range(3):
        y, _, sums, l3, st = wb.clipper_eval_tp(xt, theta, FS, tgt, n, EPS, skip, K, W, ws=ws, state=state, time_major=True)
        calls += 1
        clean(wb, st)
        assert float((y - y_ref).abs().max()) <= Y_TOL
        check_sums(sums, l3, *sums64(y_ref, tgt, skip), what="theta stands still")
    info = state.info()
    assert info["valid"] == 3 and info["n_calls"] == calls


def test_engine_eval_fused(wb):
    """engine.MseStep.eval_fused, both loss kinds: the loss of step_fused at the same theta, self.gtheta / self.sse untouched,
    store_output and sums_allreduce honoured."""
    from wdf_hip import engine
    B, T, skip = 128, 2048, 50
    x, th, ths = ref.problem(B, T, seed=9)
    xd = dev(x)
    xt = xd.t().contiguous()
    tgt, _, _ = wb.clipper_fwd(xd, dev(ths), FS, want_stash=False)
    plan = engine.TpPlan(8, 192, 1e-6, 8)
    theta = dev(th)
    for loss, kw in (("mse", {}), ("mse+esr", dict(skip=skip))):
        st = engine.MseStep(B, T, FS, plan, xd.device, time_major=True, loss=loss, warm=True, **kw)
        sse, _ = st.step_fused(theta, xt, tgt)
        want = float(sse) / (B * T) if loss == "mse" else float(st.loss[2])
        ev = engine.MseStep(B, T, FS, plan, xd.device, time_major=True, loss=loss, warm=True, store_output=False, **kw)
        ev.out.fill_(-7.0)
        for _ in range(3):
            l3 = ev.eval_fused(theta, xt, tgt)
        assert l3 is ev.loss_eval and ev.y is None
        clean(wb, ev.status)
        assert rel(l3[0 if loss == "mse" else 2], want) <= SUM_RTOL
        assert bool((ev.out == -7.0).all())                        # gtheta and sse are not this call's
        ev.store_output = True
        ev.eval_fused(theta, xt, tgt)
        assert float((ev.y - st.y).abs().max()) <= Y_TOL
    seen = []
    shard = engine.MseStep(B, T, FS, plan, xd.device, time_major=True, loss="mse+esr", skip=skip, store_output=False,
                           sums_allreduce=lambda s: seen.append(s.clone()))
    l3 = shard.eval_fused(theta, xt, tgt)
    assert len(seen) == 1 and seen[0].dtype == torch.float64 and seen[0].numel() == 2
    assert torch.allclose(l3, ev.loss_eval, rtol=1e-6, atol=0)
