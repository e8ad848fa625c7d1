"""GPU: the one-pass step's group form (csrc/wdf_clipper_fused.h: G = min(8, K) chunk waves to a workgroup, combined in LDS by
fused_group_compose; clipper_fused_group_finish_kernel walks ceil(K / G) group records per tile) against the fp64 CPU oracle.

The group form is opt-in: WDF_FUSED_FINISH=group, read at every call, asks for it, and every test here sets it.  x is TIME-MAJOR in
every call: with batch-major x in 16-byte rows the chunk kernel keeps a window of x in LDS per workgroup and the host stays
with one chunk wave per workgroup (the finish launch of tests/test_gpu_fused_finish_waves.py).

Chunk counts, by what the workgroups and the finish launch then do:
    K = 2   one group of 2 waves (below one full group)      K = 5   one group of 5
    K = 8   exactly one full group                           K = 9   one full group + a group of ONE wave
    K = 16  two full groups                                  K = 17  two full groups + a group of one
    K = 32  four full groups (the bench plan's geometry)
B = 258: with two sequences per lane three tiles of 128 (the last one: 2 live sequences, 63 dead lanes), with one per lane
five tiles of 64 -- the step's ticket has more than one arriver in both.  T is the shortest length at which the planner
(chunks are multiples of 32 steps) gives that K.

Tolerances: those of tests/test_gpu_fused_finish_waves.py for the same quantities (its module docstring has the reasoning for
theta after the folded Adam step).  A group record rounds the composed map {P, q[3], GA} to fp32 once more than the walk over
the per-chunk records does: 6e-8 relative on a tangent, three orders below the gradient's tolerance.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FS = 48000.0
Y_TOL = 2.0e-6        # volts
G_RTOL = 1.0e-4       # per gradient component
LOSS_RTOL = 1.0e-5    # MSE loss against the oracle
ESR_RTOL = 2.0e-5     # the MSE + ESR loss values
TH_RTOL = 1.0e-6      # theta after Adam
TOL = 1.0e-6          # the boundary check's tolerance (the binding's default)
B = 258
W = 256
SKIP = 50
EPS = float(np.finfo(float).eps)
T_FOR_K = {2: 512, 5: 640, 8: 512, 9: 576, 16: 512, 17: 544, 32: 1024}
LO, HI = [1e-15, 1e-3, 180.0, 1e-13], [1e-3, 1.0, 1.0e6, 1.0]
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-7
JUMP = [1.5, 1.1, 0.6, 1.6]     # the theta jump of tests/test_gpu_fused_step.py's loop test


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def adam_first_step(th32, g, lr):
    """wdf_adam_step's rule (csrc/wdf_optim.h) for step 1 from zero moments, in fp64"""
    th, g, lr = th32.astype(np.float64), np.asarray(g, dtype=np.float64), np.asarray(lr, dtype=np.float64)
    m, v = (1.0 - BETA1) * g, (1.0 - BETA2) * g * g
    c1, c2 = 1.0 - BETA1, 1.0 - BETA2
    return np.clip(th - lr * np.sqrt(c2) / c1 * m / (np.sqrt(v) + ADAM_EPS), LO, HI)


def oracle_refs(oracle, x, th, tgt32, T):
    """fp64 references of both losses at theta (float32 values) against the float32 target"""
    th64, x64, t64 = th.astype(np.float64), x.astype(np.float64), tgt32.astype(np.float64)
    loss, g, y = oracle.clipper_mse_step(th64, FS, x64, t64, dtype=np.float64)
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


@pytest.fixture(autouse=True)
def group_form(monkeypatch):
    monkeypatch.setenv("WDF_FUSED_FINISH", "group")


@pytest.fixture
def case(oracle):
    """(T, x, theta, target, references) of a chunk count: computed once per (T, theta), shared by the tests, never written to"""
    def get(K, T=None, theta_scale=None):
        from wdf_hip import workload
        T = T_FOR_K[K] if T is None else T
        key = (T, None if theta_scale is None else tuple(theta_scale))
        if key not in _CACHE:
            x = workload.sweep_batch(B, T, seed=B + T)
            th = workload.clipper_theta().astype(np.float32)
            if theta_scale is not None:
                th = (th * np.asarray(theta_scale, dtype=np.float32)).astype(np.float32)
            tgt32 = oracle.clipper_fwd(workload.target_theta().astype(np.float64), FS, x.astype(np.float64)).astype(np.float32)
            _CACHE[key] = (x, th, tgt32, oracle_refs(oracle, x, th, tgt32, T))
        return (T,) + _CACHE[key]
    return get


def check_status(wb, st, want_repair=False):
    s = wb.tp_status(st)
    if want_repair:
        assert s["n_bad"] > 0 and s["fallback_ran"], s
    else:
        assert s["n_bad"] == 0 and not s["fallback_ran"], s


def check_mse(wb, y, g, sse, st, ref, T, want_repair=False):
    check_status(wb, st, want_repair)
    ey = float(np.max(np.abs(y.cpu().numpy() - ref["y"])))
    got = g.cpu().numpy().astype(np.float64)
    eg = np.abs(got - ref["g"]) / np.abs(ref["g"])
    el = abs(float(sse) / (B * T) - ref["loss"]) / ref["loss"]
    print(f"mse: max|y - oracle| {ey:.2e}  rel grad err {eg}  rel loss err {el:.2e}")
    assert ey <= Y_TOL
    assert np.all(eg <= G_RTOL), (got, ref["g"])
    assert el <= LOSS_RTOL


def check_esr(wb, y, g, loss3, st, ref, want_repair=False):
    check_status(wb, st, want_repair)
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
@pytest.mark.parametrize("K", [2, 5, 8, 9, 16, 17, 32])
def test_group_geometries_against_the_oracle(wb, case, K, lanes):
    T, x, th, tgt32, ref = case(K)
    assert wb.lib().wdf_clipper_tp_chunks(T, K) == K
    wb.ONE_SEQUENCE_PER_LANE = lanes.startswith("one")
    try:
        xt, tgt = dev(x).t().contiguous(), dev(tgt32)
        lr = [1e-3 * float(v) for v in th]
        # MSE, Adam folded into the launch
        theta = dev(th)
        opt = wb.Adam(4, lr=lr, lo=LO, hi=HI, device=xt.device)
        y, _, g, sse, st = wb.clipper_step_mse_tp(xt, theta, FS, tgt, 2.0 / (B * T), K, W, opt=opt, time_major=True)
        check_mse(wb, y, g, sse, st, ref, T)
        check_theta(theta, th, ref["g"], lr)
        # MSE + ESR past SKIP, Adam folded into the launch
        theta = dev(th)
        opt = wb.Adam(4, lr=lr, lo=LO, hi=HI, device=xt.device)
        y, _, _, g, loss3, st = wb.clipper_step_esr_tp(xt, theta, FS, tgt, ref["n"], EPS, SKIP, K, W, opt=opt, time_major=True)
        check_esr(wb, y, g, loss3, st, ref)
        check_theta(theta, th, ref["g_esr"], lr)
    finally:
        wb.ONE_SEQUENCE_PER_LANE = False


@pytest.mark.parametrize("K", [9, 32])
def test_group_form_is_bit_reproducible(wb, case, K):
    T, x, th, tgt32, _ = case(K)
    xt, tgt = dev(x).t().contiguous(), dev(tgt32)
    lr = [1e-3 * float(v) for v in th]
    runs = []
    for _ in range(2):
        theta = dev(th)
        opt = wb.Adam(4, lr=lr, lo=LO, hi=HI, device=xt.device)
        _, _, g, sse, _ = wb.clipper_step_mse_tp(xt, theta, FS, tgt, 2.0 / (B * T), K, W, opt=opt, time_major=True)
        runs.append((sse.clone(), g.clone(), theta.clone()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), (a, b)


def _warm_calls_then_jump(wb, xt, tgt, th0, th1, T, K):
    """four warm-started calls at theta0, then one at theta1: that call's outputs and status"""
    state = wb.TpWarmState(B, T, K, min(192, T // K) // wb.warm_unit(), xt.device)
    ws = wb.step_mse_workspace(B, K, xt.device)
    theta = dev(th0)
    for it in range(4):
        _, _, _, _, st = wb.clipper_step_mse_tp(xt, theta, FS, tgt, 2.0 / (B * T), K, W, ws=ws, state=state, time_major=True)
    check_status(wb, st)
    theta = dev(th1)
    y, _, g, sse, st = wb.clipper_step_mse_tp(xt, theta, FS, tgt, 2.0 / (B * T), K, W, ws=ws, state=state, time_major=True)
    return y, g, sse, st, ws, state, theta


@pytest.mark.parametrize("K", [8, 16])
def test_missed_boundaries_inside_and_between_groups_are_repaired(wb, case, K, monkeypatch):
    """Warm-started calls at theta0 fill the snapshot ring; then theta jumps and the warm start misses.  K = 8: every boundary
    is inside the tile's one group (found by the workgroup in LDS).  K = 16: boundary 8 | 9 -- chunk index 8 entered from chunk
    7's end -- lies BETWEEN the two groups (found by the finish launch), the others inside one.

    The jump misses boundaries inside the groups too, and one miss anywhere sends the tile to the repair, which walks EVERY
    per-chunk boundary: the repaired step alone would not notice a finish launch that skipped the boundaries between groups.
    What pins them is the COUNT: the same five calls under WDF_FUSED_FINISH=launch, whose finish launch reads all K - 1
    boundaries of a tile from memory, must report the same n_bad and the same largest miss (the chunk bodies are the same code
    from the same start states in both forms, so the boundary states are the same bits; the group form adds the workgroups'
    counts from LDS to the finish launch's count over the boundaries between groups: a boundary left out, or read at another
    index, changes the sum).  That the boundary between the groups does miss is argued on the oracle's outputs: with the ring
    filled at one theta the extrapolated start state of a chunk is the theta0 trajectory's state, the controller has settled
    at no more than 4 warm-up units of 16 steps by the fifth call (a unit shrinks a miss ~5x, csrc/wdf_clipper.h), and the two
    trajectories' outputs one step before the boundary (y = (z' + z) / 2: the mean of the states on either side of that step)
    differ by more than 10 x 5^4 tol for some sequence.  T = 2048 as in the finish launch's repair test: the shortest length
    at which that test's recipe (192 steps of snapshots per chunk at K = 8) fits the chunks."""
    T = 2048
    _, x, th0, tgt32, ref0 = case(K, T=T)
    _, _, th1, _, ref1 = case(K, T=T, theta_scale=JUMP)
    assert wb.lib().wdf_clipper_tp_chunks(T, K) == K
    L = T // K
    for k in ([8] if K == 16 else [4]):
        gap = float(np.max(np.abs(ref1["y"][k * L - 1] - ref0["y"][k * L - 1])))
        print(f"oracle outputs one step before chunk {k}: max |y(theta1) - y(theta0)| = {gap:.3e}")
        assert gap > 10.0 * 625.0 * TOL
    xt, tgt = dev(x).t().contiguous(), dev(tgt32)
    monkeypatch.setenv("WDF_FUSED_FINISH", "launch")
    y, g, sse, st, _, _, _ = _warm_calls_then_jump(wb, xt, tgt, th0, th1, T, K)
    check_mse(wb, y, g, sse, st, ref1, T, want_repair=True)
    s_launch = wb.tp_status(st)
    monkeypatch.setenv("WDF_FUSED_FINISH", "group")
    y, g, sse, st, ws, state, theta = _warm_calls_then_jump(wb, xt, tgt, th0, th1, T, K)
    check_mse(wb, y, g, sse, st, ref1, T, want_repair=True)
    s_group = wb.tp_status(st)
    print(f"launch form {s_launch}  group form {s_group}")
    assert s_group["n_bad"] == s_launch["n_bad"] and s_group["max_miss"] == s_launch["max_miss"]
    # the workspace is left clean: the next step at the same theta (its warm start may miss again) is the oracle's too
    y, _, g, sse, st = wb.clipper_step_mse_tp(xt, theta, FS, tgt, 2.0 / (B * T), K, W, ws=ws, state=state, time_major=True)
    check_mse(wb, y, g, sse, st, ref1, T, want_repair=wb.tp_status(st)["n_bad"] > 0)


def test_more_group_records_than_one_register_batch(wb, case):
    """K = 128: 16 group records per tile, the finish launch's second batch of 8 (and two rounds of boundaries between groups:
    15 of them, 8 at a time).  T = 4096: the shortest length with 128 chunks of 32 steps."""
    K, T = 128, 4096
    _, x, th, tgt32, ref = case(K, T=T)
    assert wb.lib().wdf_clipper_tp_chunks(T, K) == K
    xt, tgt = dev(x).t().contiguous(), dev(tgt32)
    y, _, g, sse, st = wb.clipper_step_mse_tp(xt, dev(th), FS, tgt, 2.0 / (B * T), K, W, time_major=True)
    check_mse(wb, y, g, sse, st, ref, T)
    y, _, _, g, loss3, st = wb.clipper_step_esr_tp(xt, dev(th), FS, tgt, ref["n"], EPS, SKIP, K, W, time_major=True)
    check_esr(wb, y, g, loss3, st, ref)


@pytest.mark.parametrize("pot", ["one value per sample", "one value per sequence"])
def test_group_form_with_a_pot_channel(wb, oracle, pot):
    """The resistance channel under the group form: streamed per sample (DYN_R = 1 in the kernels: tiles half as long) and one
    value per sequence (DYN_R = 2: the binding notices a channel that is constant in time).  K = 9: a full group and a group of
    one wave.  MSE step against the oracle with the same channel.  Warm-up 512 steps instead of the module's 256: the channel
    reaches 99.1 kOhm, where the tree's time constant R C = 22 samples at 4.7 nF and a cold chunk's start error of ~0.1 V has
    decayed to e^-11 ~ 2e-6 V after 256 steps -- at the boundary check's 1e-6 V tolerance, not under it (45 kOhm, the static
    circuit of the other tests: 10 samples, e^-25)."""
    W_POT = 512
    from wdf_hip import workload
    K, T = 9, T_FOR_K[9]
    x = workload.sweep_batch(B, T, seed=B + T + 1)
    r = np.ascontiguousarray(workload.pot_resistance_batch(B, T), dtype=np.float32)      # one pot value per sequence
    if pot.endswith("sample"):                                                          # a pot that moves: +-25 % along the sequence
        r = np.ascontiguousarray(r * (1.0 + 0.25 * np.sin(np.arange(T) / 15.0))[None, :], dtype=np.float32)
    th = workload.clipper_theta().astype(np.float32)
    x64, r64, th64 = x.astype(np.float64), r.astype(np.float64), th.astype(np.float64)
    tgt32 = oracle.clipper_fwd(workload.target_theta().astype(np.float64), FS, x64, r=r64).astype(np.float32)
    y64 = oracle.clipper_fwd(th64, FS, x64, r=r64)
    t64 = tgt32.astype(np.float64)
    _, g64 = oracle.clipper_fwd_bwd(th64, FS, x64, 2.0 * (y64 - t64) / (B * T), r=r64)
    ref = {"y": y64, "g": g64, "loss": float(np.mean((y64 - t64) ** 2))}
    xt, rt, tgt = dev(x).t().contiguous(), dev(r).t().contiguous(), dev(tgt32)
    assert wb.r_is_per_sequence(rt, True) == pot.endswith("sequence")
    y, _, g, sse, st = wb.clipper_step_mse_tp(xt, dev(th), FS, tgt, 2.0 / (B * T), K, W_POT, r=rt, time_major=True)
    check_status(wb, st)
    ey = float(np.max(np.abs(y.cpu().numpy() - ref["y"])))
    got = g.cpu().numpy().astype(np.float64)
    el = abs(float(sse) / (B * T) - ref["loss"]) / ref["loss"]
    print(f"pot: max|y - oracle| {ey:.2e}  grad {got} oracle {ref['g']}  rel loss err {el:.2e}")
    assert ey <= Y_TOL and el <= LOSS_RTOL
    # (theta's R is replaced by the channel: components Is, nVt and C carry the gradient, as tests/test_gpu_fused_step.py checks them)
    assert all(abs(got[i] - ref["g"][i]) <= G_RTOL * abs(ref["g"][i]) for i in (0, 1, 3)), (got, ref["g"])


def _run_both_losses(wb, x, th, tgt32, T, K):
    xt, tgt = dev(x).t().contiguous(), dev(tgt32)
    y1, _, g1, sse, st1 = wb.clipper_step_mse_tp(xt, dev(th), FS, tgt, 2.0 / (B * T), K, W, time_major=True)
    y2, _, _, g2, loss3, st2 = wb.clipper_step_esr_tp(xt, dev(th), FS, tgt, B * (T - SKIP), EPS, SKIP, K, W, time_major=True)
    return (y1, g1, sse, st1), (y2, g2, loss3, st2)


def test_group_and_launch_forms_agree(wb, case, tmp_path):
    """This process runs the group form, a fresh child process WDF_FUSED_FINISH=launch (one chunk wave to a workgroup,
    clipper_fused_finish_kernel); each is held against the oracle, and the two against each other."""
    K = 17
    T, x, th, tgt32, ref = case(K)
    (y1, g1, sse, st1), (y2, g2, loss3, st2) = _run_both_losses(wb, x, th, tgt32, T, K)
    check_mse(wb, y1, g1, sse, st1, ref, T)
    check_esr(wb, y2, g2, loss3, st2, ref)
    src, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, x=x, th=th, tgt=tgt32, T=T, K=K)
    env = dict(os.environ, WDF_FUSED_FINISH="launch")
    subprocess.run([sys.executable, os.path.abspath(__file__), src, out], check=True, env=env, timeout=300)
    c = np.load(out)
    assert int(c["n_bad"]) == 0 and int(c["fallback_ran"]) == 0
    # each within the oracle's tolerance of the oracle (above for this process, here for the child) ...
    assert float(np.max(np.abs(c["y1"] - ref["y"]))) <= Y_TOL and float(np.max(np.abs(c["y2"] - ref["y"]))) <= Y_TOL
    assert np.all(np.abs(c["g1"] - ref["g"]) <= G_RTOL * np.abs(ref["g"]))
    assert np.all(np.abs(c["g2"] - ref["g_esr"]) <= G_RTOL * np.abs(ref["g_esr"]))
    assert abs(float(c["sse"]) / (B * T) - ref["loss"]) <= LOSS_RTOL * ref["loss"]
    assert abs(float(c["loss3"][2]) - (ref["mse"] + ref["esr"])) <= ESR_RTOL * (ref["mse"] + ref["esr"])
    # ... and of each other
    assert float(np.max(np.abs(c["y1"] - y1.cpu().numpy()))) <= Y_TOL and float(np.max(np.abs(c["y2"] - y2.cpu().numpy()))) <= Y_TOL
    assert np.all(np.abs(c["g1"] - g1.cpu().numpy()) <= G_RTOL * np.abs(ref["g"]))
    assert np.all(np.abs(c["g2"] - g2.cpu().numpy()) <= G_RTOL * np.abs(ref["g_esr"]))
    assert abs(float(c["sse"]) - float(sse)) <= LOSS_RTOL * float(sse)
    assert abs(float(c["loss3"][2]) - float(loss3[2])) <= ESR_RTOL * float(loss3[2])


def test_group_form_with_skewed_chunk_spans(wb, case, tmp_path):
    """Long and short spans by half groups (chunk_span's negative skew: every SIMD of a workgroup holds one of each).  The library
    applies them only to launches of about two waves per SIMD; WDF_FUSED_SKEW=force, read once per process, applies them wherever
    the geometry allows -- whole groups, here K = 16 at T = 2048: 128-step chunks become 160 and 96 steps.  A fresh child process
    runs both losses that way; held against the oracle."""
    K, T = 16, 2048
    _, x, th, tgt32, ref = case(K, T=T)
    src, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, x=x, th=th, tgt=tgt32, T=T, K=K)
    env = dict(os.environ, WDF_FUSED_FINISH="group", WDF_FUSED_SKEW="force")
    subprocess.run([sys.executable, os.path.abspath(__file__), src, out], check=True, env=env, timeout=300)
    c = np.load(out)
    assert int(c["n_bad"]) == 0 and int(c["fallback_ran"]) == 0
    assert float(np.max(np.abs(c["y1"] - ref["y"]))) <= Y_TOL and float(np.max(np.abs(c["y2"] - ref["y"]))) <= Y_TOL
    assert np.all(np.abs(c["g1"] - ref["g"]) <= G_RTOL * np.abs(ref["g"]))
    assert np.all(np.abs(c["g2"] - ref["g_esr"]) <= G_RTOL * np.abs(ref["g_esr"]))
    assert abs(float(c["sse"]) / (B * T) - ref["loss"]) <= LOSS_RTOL * ref["loss"]
    assert abs(float(c["loss3"][2]) - (ref["mse"] + ref["esr"])) <= ESR_RTOL * (ref["mse"] + ref["esr"])


if __name__ == "__main__":          # the child of test_group_and_launch_forms_agree and test_group_form_with_skewed_chunk_spans
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, "differentiable-wdfs_amd", "lib"))
    from wdf_hip import binding
    d = np.load(sys.argv[1])
    (y1, g1, sse, st1), (y2, g2, loss3, st2) = _run_both_losses(binding, d["x"], d["th"], d["tgt"], int(d["T"]), int(d["K"]))
    s1, s2 = binding.tp_status(st1), binding.tp_status(st2)
    np.savez(sys.argv[2], y1=y1.cpu().numpy(), g1=g1.cpu().numpy().astype(np.float64), sse=float(sse), y2=y2.cpu().numpy(),
             g2=g2.cpu().numpy().astype(np.float64), loss3=loss3.cpu().numpy(), n_bad=s1["n_bad"] + s2["n_bad"],
             fallback_ran=int(bool(s1["fallback_ran"])) + int(bool(s2["fallback_ran"])))
