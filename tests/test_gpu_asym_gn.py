"""GPU: the Gauss-Newton form of the two-different-diode clipper's one-pass MSE step (wdf_clipper_asym_step_gn,
csrc/wdf_asym_gn.h) at kernel level, small shapes, both Newton modes, the four parameter sets of tests/test_gpu_asym_step.py.

Reference: tests/asym_gn_ref.py -- the oracle's exact fp64 forward at the fp32-rounded parameters, its central-difference
Jacobian (relative step 1e-6), H_ref = (2/n) J^T J.  The target is the oracle's forward at 1.25 x the parameters.

Bounds.  y 3e-6 V (the project's bound for both Newton modes).  out28[0:7] against clipper_asym_step_mse's out7 at the same
plan: one fp32 ulp (the same expressions in the same order; whether it is bit for bit is printed).  H against H_ref:
|dH_qr| <= 4e-4 sqrt(H_qq H_rr) -- the project's 2e-4 gradient bound, once per factor.  K = 3 against K = 1: 2e-5 on the same
scale (the project's step-against-composed bound).  The gauge v = theta o (1, 0, 1, 0, -1, 1): |v^T H v| <= 4e-4 sum |v_q v_r|
sqrt(H_qq H_rr).  The smallest eigenvalue of D^-1 H D^-1, D = sqrt(diag H): >= -1e-5.

Measured on one MI355X, 70 x 600, largest |dH_qr| / sqrt(H_qq H_rr) against H_ref (K = 1 and K = 3, W = 192, gave the same
figures: after the rounding to fp32 the K = 3 out28 was the K = 1 out28 bit for bit in all eight runs, y included):
    theta6          newton_f32 2.36e-7   newton_f64 1.23e-7
    swapped         newton_f32 1.93e-7   newton_f64 1.89e-7
    leaky_low_R     newton_f32 3.56e-7   newton_f64 2.40e-7
    schottky_big_R  newton_f32 7.74e-8   newton_f64 1.45e-7
out28[0:7] was clipper_asym_step_mse's out7 bit for bit in all sixteen runs.  y within 2.7e-7 V (fp32) / 9.8e-8 V (fp64) of the
oracle.  Gauge |v^T H v| at most 1.6e-8 of its scale; smallest eigenvalue of D^-1 H D^-1 between -4.6e-8 and 2.7e-8, largest
2.2 .. 2.7.  70 x 131: H 2.5e-7 / 1.5e-7, g 7.5e-7 / 4.0e-8 (fp32 / fp64).  256 x 2048, K = 4, W = 320: status clean, bit for
bit K = 1.  130 x 2048, K = 8, W = 8: 3 gated waves, bit for bit K = 1.
"""
import numpy as np
import pytest

import asym_gn_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FS = R.FS
MODES = {"newton_f32": 2, "newton_f64": 1}


def dev(a):
    return torch.tensor(np.array(a, dtype=np.float32), device="cuda")


def status(st):
    from wdf_hip import binding as wb
    return wb.mlp_tp_status(st)


def ulp32(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float32))).astype(np.float64)


def unpack(out28):
    """out28 (device) -> sse, g [6], H [6,6], all float64 numpy"""
    from wdf_hip import binding as wb
    o = out28.cpu()
    return float(o[0]), o[1:7].numpy().astype(np.float64), wb.gn_matrix(o[7:28]).numpy()


def gn(theta, xd, tgd, mode, K, W, **kw):
    from wdf_hip import binding as wb
    T, B = tgd.shape
    return wb.clipper_asym_step_gn(xd, dev(theta), FS, mode, tgd, 2.0 / (B * T), K, W, **kw)


_RUNS = {}


def runs_70x600(oracle, name, solver):
    """the K = 1 and the K = 3, W = 192 run of one set and mode at 70 x 600, and the MSE step's out7 at both plans; once"""
    key = (name, solver)
    if key not in _RUNS:
        from wdf_hip import binding as wb
        x, tg = R.workload_case(oracle, name, 70, 600, 3)
        xd, tgd, mode = dev(x), dev(tg), MODES[solver]
        res = {}
        for K, W in ((1, 0), (3, 192)):
            y, _, out28, st = gn(R.SETS[name], xd, tgd, mode, K, W)
            _, _, out7, st7 = wb.clipper_asym_step_mse(xd, dev(R.SETS[name]), FS, mode, tgd, 2.0 / (70 * 600), K, W)
            res[K] = dict(y=y.cpu().numpy(), out28=out28.cpu().numpy(), H=unpack(out28)[2], st=status(st), out7=out7.cpu().numpy(),
                          st7=status(st7))
        _RUNS[key] = res
    return _RUNS[key]


@pytest.mark.parametrize("solver", list(MODES))
@pytest.mark.parametrize("name", R.NAMES)
def test_70x600_against_the_oracle_and_the_mse_step(oracle, name, solver):
    x, tg = R.workload_case(oracle, name, 70, 600, 3)
    _, _, H_ref = R.gn_reference(oracle, name, 70, 600, 3)
    y_ref = oracle.clipper_asym_fwd(R.r32(R.SETS[name]), FS, x.astype(np.float64))
    s = R.scale(H_ref)
    res = runs_70x600(oracle, name, solver)
    worst = {}
    for K in (1, 3):
        r = res[K]
        assert r["st"]["n_bad"] == 0 and r["st"]["gated_waves"] == 0 and r["st7"]["gated_waves"] == 0, (r["st"], r["st7"])
        ey = float(np.max(np.abs(r["y"].astype(np.float64) - y_ref)))
        d7 = np.abs(r["out28"][:7].astype(np.float64) - r["out7"].astype(np.float64)) / ulp32(r["out7"])
        worst[K] = float(np.max(np.abs(r["H"] - H_ref) / s))
        print(f"gn {name} {solver} 70x600 K={K}: max |y - oracle| = {ey:.3e} V; out28[0:7] vs out7: "
              f"{'bit for bit' if np.array_equal(r['out28'][:7], r['out7']) else 'max %.2f ulp' % float(np.max(d7))}; "
              f"H vs H_ref: {worst[K]:.3e} of sqrt(H_qq H_rr)")
        assert ey < 3e-6, ey
        assert np.all(d7 <= 1.0), (r["out28"][:7], r["out7"])
        assert np.all(np.isfinite(r["H"])) and np.array_equal(r["H"], r["H"].T)
        assert worst[K] <= 4e-4, (r["H"], H_ref)
    e31 = float(np.max(np.abs(res[3]["H"] - res[1]["H"]) / R.scale(res[1]["H"])))
    g1 = res[1]["out28"][1:7].astype(np.float64)
    eg = float(np.max(np.abs(res[3]["out28"][1:7] - g1) / np.abs(g1)))
    print(f"gn {name} {solver} 70x600 K=3 vs K=1: H {e31:.3e} of sqrt(H_qq H_rr), g {eg:.3e} relative, "
          f"|dy| {float(np.max(np.abs(res[3]['y'] - res[1]['y']))):.3e} V")
    assert e31 <= 2e-5 and eg <= 2e-5


@pytest.mark.parametrize("solver", list(MODES))
@pytest.mark.parametrize("name", R.NAMES)
def test_70x600_gauge_and_spectrum(oracle, name, solver):
    res = runs_70x600(oracle, name, solver)
    for K in (1, 3):
        H = res[K]["H"]
        vHv, bound = R.gauge_residual(H, R.r32(R.SETS[name]))
        d = np.sqrt(np.diag(H))
        ev = np.linalg.eigvalsh(H / np.outer(d, d))
        print(f"gn {name} {solver} K={K}: gauge v^T H v = {vHv / bound:.3e} of its scale; eigenvalues of D^-1 H D^-1 "
              f"{ev[0]:.3e} .. {ev[-1]:.3e}")
        assert np.all(d > 0.0)
        assert abs(vHv) <= 4e-4 * bound, (vHv, bound)
        assert ev[0] >= -1e-5, ev


@pytest.mark.parametrize("solver", list(MODES))
def test_ragged_block_70x131(oracle, solver):
    """T is no multiple of the 8-step block (nor of 4: the scalar loads)"""
    name = "theta6"
    x, tg = R.workload_case(oracle, name, 70, 131, 5)
    _, g_ref, H_ref = R.gn_reference(oracle, name, 70, 131, 5)
    y_ref = oracle.clipper_asym_fwd(R.r32(R.SETS[name]), FS, x.astype(np.float64))
    y, _, out28, st = gn(R.SETS[name], dev(x), dev(tg), MODES[solver], 1, 0)
    sse, g, H = unpack(out28)
    ey = float(np.max(np.abs(y.cpu().numpy().astype(np.float64) - y_ref)))
    eh, eg = float(np.max(np.abs(H - H_ref) / R.scale(H_ref))), float(np.max(np.abs(g - g_ref) / np.abs(g_ref)))
    sse_ref = float(np.sum((y_ref - tg.astype(np.float64)) ** 2))
    print(f"gn {name} {solver} 70x131: |y - oracle| {ey:.3e} V, sse {abs(sse - sse_ref) / sse_ref:.3e}, g {eg:.3e}, H {eh:.3e}")
    assert status(st)["n_bad"] == 0
    assert ey < 3e-6 and abs(sse - sse_ref) <= 1e-5 * sse_ref and eg <= 2e-4 and eh <= 4e-4


def test_short_warmup_is_repaired(oracle):
    """The forced-miss shape of tests/test_gpu_asym_step.py: a warm-up of 8 steps cannot work, the ordinary verification gates
    every wave, each is re-run as one chunk, and y, zT and out28 are the K = 1 result bit for bit.  A wrong start state being
    repaired, not a fault; it runs once."""
    from wdf_hip import binding as wb
    B, T = 130, 2048
    x, tg = R.workload_case(oracle, "theta6", B, T, 3)
    xd, tgd = dev(x), dev(tg)
    y1, zT1, o1, st1 = gn(R.THETA6, xd, tgd, wb.ASYM_NEWTON_F32, 1, 0, want_zT=True)
    y8, zT8, o8, st8 = gn(R.THETA6, xd, tgd, wb.ASYM_NEWTON_F32, 8, 8, want_zT=True)
    s = status(st8)
    print(f"repair: status {s}, out28 {o8.cpu().numpy()} vs K=1 {o1.cpu().numpy()}")
    assert s["n_bad"] > 0 and s["gated_waves"] == 3, s
    assert torch.equal(y8, y1) and torch.equal(zT8, zT1) and torch.equal(o8, o1)


@pytest.mark.parametrize("solver", list(MODES))
def test_four_chunks_256x2048_are_clean(oracle, solver):
    B, T = 256, 2048
    x, tg = R.workload_case(oracle, "theta6", B, T, 6)
    xd, tgd = dev(x), dev(tg)
    _, _, o1, st1 = gn(R.THETA6, xd, tgd, MODES[solver], 1, 0)
    y, _, o4, st4 = gn(R.THETA6, xd, tgd, MODES[solver], 4, 320)
    s = status(st4)
    (_, g1, H1), (_, g4, H4) = unpack(o1), unpack(o4)
    eh, eg = float(np.max(np.abs(H4 - H1) / R.scale(H1))), float(np.max(np.abs(g4 - g1) / np.abs(g1)))
    print(f"gn theta6 {solver} 256x2048 K=4 W=320: status {s}; vs K=1: H {eh:.3e}, g {eg:.3e}")
    assert s["n_bad"] == 0 and s["gated_waves"] == 0, s
    assert status(st1)["n_bad"] == 0
    assert eh <= 2e-5 and eg <= 2e-5


def test_binding_refuses_before_any_launch():
    from wdf_hip import binding as wb
    B, T = 8, 64
    xd, tgd, th = torch.zeros((B, T), device="cuda"), torch.zeros((T, B), device="cuda"), dev(R.THETA6)
    need = wb.lib().wdf_clipper_asym_step_gn_ws_bytes(B, 2)
    with pytest.raises(wb.WdfHipError, match="ws holds"):
        wb.clipper_asym_step_gn(xd, th, FS, wb.ASYM_NEWTON_F32, tgd, 1.0, 2, 8, ws=torch.empty((need - 8,), dtype=torch.uint8, device="cuda"))
    # (the MSE step's workspace is too short for this step)
    with pytest.raises(wb.WdfHipError, match="ws holds"):
        wb.clipper_asym_step_gn(xd, th, FS, wb.ASYM_NEWTON_F32, tgd, 1.0, 2, 8,
                                ws=torch.empty((wb.lib().wdf_clipper_asym_step_mse_ws_bytes(B, 2),), dtype=torch.uint8, device="cuda"))
    with pytest.raises(wb.WdfHipError, match="out28"):
        wb.clipper_asym_step_gn(xd, th, FS, wb.ASYM_NEWTON_F32, tgd, 1.0, 2, 8, out28=torch.empty((7,), device="cuda"))
    with pytest.raises(wb.WdfHipError, match="mode 0"):
        wb.clipper_asym_step_gn(xd, th, FS, wb.ASYM_OMEGA_F32, tgd, 1.0, 2, 8)
