"""GPU: the one-pass step's finish launch (clipper_fused_finish_kernel, csrc/wdf_clipper_fused.h) at every wave geometry
the host can pick, against the fp64 CPU oracle.

The host starts one finishing wave per tile for every 4 chunks, 8 at the most, and a wave holds up to 8 chunk records in
registers, loaded in halves of 4.  The chunk counts below are where that code changes its path:
    K = 2   one wave, half a batch            K = 5   two waves, 3 + 2 chunks (ragged last wave)
    K = 8   two waves of exactly 4            K = 9   three waves of 3 (one past two full halves)
    K = 32  eight waves of 4 (the bench plan's geometry)
B = 130: two tiles of 128 sequences with two per lane (the second tile: 2 live sequences, 63 dead lanes), three tiles of 64
with one per lane.  T is the shortest length at which the planner (chunks are multiples of 32 steps) gives that K.

Tolerances are those of tests/test_gpu_fused_step.py for the same quantities.  theta after the folded Adam step: the first
Adam step moves a component by lr * g / (|g| + eps / sqrt(1 - beta2)) ~ lr = 1e-3 theta, whatever the gradient's size, so the
gradient's 1e-4 tolerance reaches theta as < 1e-7 relative; what is left is fp32 rounding of the update (a few ulp of a
term 1e-3 of theta) and of theta itself (6e-8): rtol 1e-6, as the existing loop test uses for the same comparison.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FS = 48000.0
Y_TOL = 2.0e-6        # volts (tests/test_gpu_fused_step.py)
G_RTOL = 1.0e-4       # per gradient component (same)
LOSS_RTOL = 1.0e-5    # MSE loss against the oracle (same: test_fused_vs_oracle_f64)
ESR_RTOL = 2.0e-5     # the MSE + ESR loss values (same: test_fused_esr_step_matches_autograd)
TH_RTOL = 1.0e-6      # theta after Adam (same: test_fused_warm_started_training_loop_with_adam; module docstring)
B = 130
W = 256
SKIP = 50
EPS = float(np.finfo(float).eps)
T_FOR_K = {2: 512, 5: 640, 8: 512, 9: 576, 32: 1024}
LO, HI = [1e-15, 1e-3, 180.0, 1e-13], [1e-3, 1.0, 1.0e6, 1.0]
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-7


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def adam_first_step(th32, g, lr):
    """wdf_adam_step's rule (csrc/wdf_optim.h) for step 1 from zero moments, in fp64"""
    th, g, lr = th32.astype(np.float64), np.asarray(g, dtype=np.float64), np.asarray(lr, dtype=np.float64)
    m, v = (1.0 - BETA1) * g, (1.0 - BETA2) * g * g
    c1, c2 = 1.0 - BETA1, 1.0 - BETA2
    return np.clip(th - lr * np.sqrt(c2) / c1 * m / (np.sqrt(v) + ADAM_EPS), LO, HI)


def make_problem(T, seed):
    from wdf_hip import workload
    x = workload.sweep_batch(B, T, seed=seed)
    th = workload.clipper_theta().astype(np.float32)
    return x, th, workload.target_theta()


def oracle_refs(oracle, x, th, tgt32, T):
    """fp64 references of both losses at theta (float32 values) against the float32 target"""
    th64, x64, t64 = th.astype(np.float64), x.astype(np.float64), tgt32.astype(np.float64)
    loss, g, y = oracle.clipper_mse_step(th64, FS, x64, t64, dtype=np.float64)
    # MSE + ESR past SKIP, evaluated on the oracle's own y (clipper_pot.py:146-156,177), its reverse sweep for the gradient
    n = B * (T - SKIP)
    o, t = y[SKIP:], t64[SKIP:]
    S, E = float(np.sum((o - t) ** 2)), float(np.sum(o ** 2)) + EPS
    mse, esr = S / n, float(np.sqrt(S / E / n))
    gy = np.zeros_like(y)
    gy[SKIP:] = (2.0 / n + 1.0 / (esr * E * n)) * (o - t) - (esr / E) * o
    _, g_esr = oracle.clipper_fwd_bwd(th64, FS, x64, gy)
    return {"y": y, "loss": loss, "g": g, "n": n, "mse": mse, "esr": esr, "g_esr": g_esr}


_CACHE = {}


@pytest.fixture(scope="module")
def wb():
    from wdf_hip import binding
    binding.require_gpu()
    yield binding
    binding.ONE_SEQUENCE_PER_LANE = False


@pytest.fixture
def case(oracle):
    """(x, theta, target, references) of a chunk count: computed once, shared by the tests, never written to"""
    def get(K, T=None, theta_scale=None):
        T = T_FOR_K[K] if T is None else T
        key = (T, None if theta_scale is None else tuple(theta_scale))
        if key not in _CACHE:
            x, th, ths = make_problem(T, seed=B + T)
            if theta_scale is not None:
                th = (th * np.asarray(theta_scale, dtype=np.float32)).astype(np.float32)
            tgt32 = oracle.clipper_fwd(ths.astype(np.float64), FS, x.astype(np.float64)).astype(np.float32)
            _CACHE[key] = (x, th, tgt32, oracle_refs(oracle, x, th, tgt32, T))
        return (T,) + _CACHE[key]
    return get


def check_mse(wb, y, g, sse, st, ref, T, want_repair=False):
    s = wb.tp_status(st)
    if want_repair:
        assert s["n_bad"] > 0 and s["fallback_ran"], s
    else:
        assert s["n_bad"] == 0 and not s["fallback_ran"], s
    ey = float(np.max(np.abs(y.cpu().numpy() - ref["y"])))
    got = g.cpu().numpy().astype(np.float64)
    eg = np.abs(got - ref["g"]) / np.abs(ref["g"])
    el = abs(float(sse) / (B * T) - ref["loss"]) / ref["loss"]
    print(f"mse: max|y - oracle| {ey:.2e}  rel grad err {eg}  rel loss err {el:.2e}")
    assert ey <= Y_TOL
    assert np.all(eg <= G_RTOL), (got, ref["g"])
    assert el <= LOSS_RTOL


def check_esr(wb, y, g, loss3, st, ref):
    s = wb.tp_status(st)
    assert s["n_bad"] == 0 and not s["fallback_ran"], s
    ey = float(np.max(np.abs(y.cpu().numpy() - ref["y"])))
    got = g.cpu().numpy().astype(np.float64)
    eg = np.abs(got - ref["g_esr"]) / np.abs(ref["g_esr"])
    l = loss3.cpu().numpy().astype(np.float64)
    el = [abs(l[0] - ref["mse"]) / ref["mse"], abs(l[1] - ref["esr"]) / ref["esr"],
          abs(l[2] - (ref["mse"] + ref["esr"])) / (ref["mse"] + ref["esr"])]
    print(f"mse+esr: max|y - oracle| {ey:.2e}  rel grad err {eg}  rel loss errs {el}")
    assert ey <= Y_TOL
    assert np.all(eg <= G_RTOL), (got, ref["g_esr"])
    assert max(el) <= ESR_RTOL


def check_theta(theta, th_before, g_ref, lr):
    want = adam_first_step(th_before, g_ref, lr)
    got = theta.cpu().numpy().astype(np.float64)
    err = np.abs(got - want) / np.abs(want)
    print(f"theta after Adam: rel err {err}")
    assert np.all(err <= TH_RTOL), (got, want)


@pytest.mark.parametrize("lanes", ["two sequences per lane", "one sequence per lane"])
@pytest.mark.parametrize("K", [2, 5, 8, 9, 32])
def test_finish_wave_geometries_against_the_oracle(wb, case, K, lanes):
    T, x, th, tgt32, ref = case(K)
    assert wb.lib().wdf_clipper_tp_chunks(T, K) == K
    wb.ONE_SEQUENCE_PER_LANE = lanes.startswith("one")
    try:
        xd, tgt = dev(x), dev(tgt32)
        lr = [1e-3 * float(v) for v in th]
        # MSE, Adam folded into the launch
        theta = dev(th)
        opt = wb.Adam(4, lr=lr, lo=LO, hi=HI, device=xd.device)
        y, _, g, sse, st = wb.clipper_step_mse_tp(xd, theta, FS, tgt, 2.0 / (B * T), K, W, opt=opt)
        check_mse(wb, y, g, sse, st, ref, T)
        check_theta(theta, th, ref["g"], lr)
        # MSE + ESR past SKIP, Adam folded into the launch
        theta = dev(th)
        opt = wb.Adam(4, lr=lr, lo=LO, hi=HI, device=xd.device)
        y, _, _, g, loss3, st = wb.clipper_step_esr_tp(xd, theta, FS, tgt, ref["n"], EPS, SKIP, K, W, opt=opt)
        check_esr(wb, y, g, loss3, st, ref)
        check_theta(theta, th, ref["g_esr"], lr)
    finally:
        wb.ONE_SEQUENCE_PER_LANE = False


@pytest.mark.parametrize("K", [9, 32])
def test_finish_is_bit_reproducible(wb, case, K):
    T, x, th, tgt32, _ = case(K)
    xd, tgt = dev(x), dev(tgt32)
    lr = [1e-3 * float(v) for v in th]
    runs = []
    for _ in range(2):
        theta = dev(th)
        opt = wb.Adam(4, lr=lr, lo=LO, hi=HI, device=xd.device)
        _, _, g, sse, _ = wb.clipper_step_mse_tp(xd, theta, FS, tgt, 2.0 / (B * T), K, W, opt=opt)
        runs.append((sse.clone(), g.clone(), theta.clone()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), (a, b)


def _run_both_losses(wb, x, th, tgt32, T, K):
    xd, tgt = dev(x), dev(tgt32)
    y1, _, g1, sse, st1 = wb.clipper_step_mse_tp(xd, dev(th), FS, tgt, 2.0 / (B * T), K, W)
    y2, _, _, g2, loss3, st2 = wb.clipper_step_esr_tp(xd, dev(th), FS, tgt, B * (T - SKIP), EPS, SKIP, K, W)
    return (y1, g1, sse, st1), (y2, g2, loss3, st2)


def test_default_and_inkernel_forms_agree(wb, case, tmp_path):
    """WDF_FUSED_FINISH=inkernel (the chunk kernel's last wave finishes the tile) is read once per process: a fresh child
    runs it, this process the default form; both are held against the oracle and against each other."""
    K = 8
    T, x, th, tgt32, ref = case(K)
    (y1, g1, sse, st1), (y2, g2, loss3, st2) = _run_both_losses(wb, x, th, tgt32, T, K)
    check_mse(wb, y1, g1, sse, st1, ref, T)
    check_esr(wb, y2, g2, loss3, st2, ref)
    src, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, x=x, th=th, tgt=tgt32, T=T, K=K)
    env = dict(os.environ, WDF_FUSED_FINISH="inkernel")
    subprocess.run([sys.executable, os.path.abspath(__file__), src, out], check=True, env=env, timeout=300)
    c = np.load(out)
    assert int(c["n_bad"]) == 0
    # each within the oracle's tolerance of the oracle (above for this process, here for the child) ...
    assert float(np.max(np.abs(c["y1"] - ref["y"]))) <= Y_TOL and float(np.max(np.abs(c["y2"] - ref["y"]))) <= Y_TOL
    assert np.all(np.abs(c["g1"] - ref["g"]) <= G_RTOL * np.abs(ref["g"]))
    assert np.all(np.abs(c["g2"] - ref["g_esr"]) <= G_RTOL * np.abs(ref["g_esr"]))
    assert abs(float(c["sse"]) / (B * T) - ref["loss"]) <= LOSS_RTOL * ref["loss"]
    assert abs(float(c["loss3"][2]) - (ref["mse"] + ref["esr"])) <= ESR_RTOL * (ref["mse"] + ref["esr"])
    # ... and of each other
    assert float(np.max(np.abs(c["y1"] - y1.cpu().numpy()))) <= Y_TOL
    assert np.all(np.abs(c["g1"] - g1.cpu().numpy()) <= G_RTOL * np.abs(ref["g"]))
    assert np.all(np.abs(c["g2"] - g2.cpu().numpy()) <= G_RTOL * np.abs(ref["g_esr"]))
    assert abs(float(c["sse"]) - float(sse)) <= LOSS_RTOL * float(sse)


def test_missed_tile_is_repaired_by_the_finish_launch(wb, case):
    """Warm-started calls at theta0 fill the snapshot ring; then theta jumps (the factors of the loop test in
    tests/test_gpu_fused_step.py) and the warm start misses: the finish launch's wave 0 re-runs the chunks while the other
    waves wait, and the step must still be the oracle's at the new theta."""
    K, T = 8, 2048
    jump = [1.5, 1.1, 0.6, 1.6]
    _, x, th0, tgt32, _ = case(K, T=T)
    _, _, th1, _, ref1 = case(K, T=T, theta_scale=jump)
    xd, tgt = dev(x), dev(tgt32)
    xt = xd.t().contiguous()
    state = wb.TpWarmState(B, T, K, 192 // wb.warm_unit(), xd.device)
    ws = wb.step_mse_workspace(B, K, xd.device)
    theta = dev(th0)
    for it in range(4):
        _, _, _, _, st = wb.clipper_step_mse_tp(xt, theta, FS, tgt, 2.0 / (B * T), K, W, ws=ws, state=state, time_major=True)
    assert wb.tp_status(st)["n_bad"] == 0
    theta = dev(th1)
    y, _, g, sse, st = wb.clipper_step_mse_tp(xt, theta, FS, tgt, 2.0 / (B * T), K, W, ws=ws, state=state, time_major=True)
    check_mse(wb, y, g, sse, st, ref1, T, want_repair=True)


if __name__ == "__main__":          # the child of test_default_and_inkernel_forms_agree
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, "differentiable-wdfs_amd", "lib"))
    from wdf_hip import binding
    d = np.load(sys.argv[1])
    (y1, g1, sse, st1), (y2, g2, loss3, st2) = _run_both_losses(binding, d["x"], d["th"], d["tgt"], int(d["T"]), int(d["K"]))
    np.savez(sys.argv[2], y1=y1.cpu().numpy(), g1=g1.cpu().numpy().astype(np.float64), sse=float(sse), y2=y2.cpu().numpy(),
             g2=g2.cpu().numpy().astype(np.float64), loss3=loss3.cpu().numpy(),
             n_bad=binding.tp_status(st1)["n_bad"] + binding.tp_status(st2)["n_bad"])
