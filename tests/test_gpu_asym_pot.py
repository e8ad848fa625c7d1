"""GPU: one pot resistance per sequence for the two-different-diode clipper (the wdf_clipper_asym_*_rseq entry points), kernel
to tf_wdf.Circuit(per_sequence_R=...).

Reference everywhere: the oracle's clipper_asym_fwd(theta6, fs, x) takes one scalar R, so it is called once per distinct pot
value on the rows that carry it, theta6[4] set to the fp32-rounded value; losses and sums are formed in fp64 over the
re-assembled y, gradients are fp64 central differences (relative step 1e-6) of the whole-batch loss over the five trainable
components {Is_up, nVt_up, Is_down, nVt_down, C}.  Inputs workload.sweep_batch; the target is the oracle at TEACHER = 1.25 x the
diode parameters and C with the same pots; pots r[b] = {10e3, 45e3, 75e3}[b % 3], so every wave holds all three and a
constant left wave-uniform cannot pass.  Parameter sets: theta6 and swapped of tests/test_gpu_asym_f32.py.  Both Newton modes.

Shapes: 70 x 600 (K = 1, W = 0: two waves, the second ragged, T no multiple of 8); 256 x 2048 (K = 4, W = 320: the diode-off
forgetting at 75 kOhm / 4.7 nF is 0.9426 per step, 0.9426^320 ~ 6e-9 is below the verification's 1e-6: the status must be
clean); 130 x 2048 (K = 8, W = 8: boundaries miss, waves are gated and repaired; the result equals the K = 1 result bit for bit).

Bounds (DESIGN section 5 and the existing asym test files): y 3e-6 V; S and E 1e-5 relative to the fp64 sums over the oracle's y
and 1e-6 to those over the step's own y; each trainable gradient component 2e-4 relative to finite differences; step against
the composed pot path: loss 1e-6, gradient 2e-5, y 1e-6 V.  Gradient component 4 (the pot is data) is exactly 0.

Measured on an MI355X (every test prints its figures before it asserts: run with -s), the largest over both modes and both sets:
y against the oracle 3.6e-7 V (sequential, chunked and in the steps); S 5.7e-7 and E 1.6e-7 of the oracle's sums, 4.1e-8 and
4.6e-8 of the sums over the step's own y; gradient against finite differences 3.6e-7 (reverse sweep), 3.9e-7 (MSE step),
3.6e-7 (MSE + ESR step); step against the composed pot path: loss equal in every printed digit, gradient 2.6e-7, y 6e-8 V; a
uniform pot against the static entry points: every difference 0; component 4 exactly 0.0 everywhere; 256 x 2048: status clean;
130 x 2048: 793 missed boundaries (fp64: 792), 3 of 3 waves gated, bit for bit the K = 1 result; Adam: theta6[4] bit-identical,
the other five equal to wdf_adam_step's.
"""
import functools
import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FS = 48000.0
VT = 25.85e-3
TEACHER = 1.25
EPS = float(np.finfo(float).eps)
THETA6 = np.array([4.352e-9, VT * 1.906, 2.0e-6, VT * 1.4, 45.0e3, 4.7e-9])
SETS = {"theta6": THETA6, "swapped": THETA6[[2, 3, 0, 1, 4, 5]]}
NAMES = list(SETS)
MODES = {"newton_f32": 2, "newton_f64": 1}
POTS = np.array([10.0e3, 45.0e3, 75.0e3], dtype=np.float32)
TRAIN = [0, 1, 2, 3, 5]                                   # the trainable components of theta6
SHAPES = {"ragged": (70, 600, 1, 0), "clean": (256, 2048, 4, 320), "repair": (130, 2048, 8, 8)}
_ORACLE = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def r32(theta):
    return np.asarray(theta).astype(np.float32).astype(np.float64)


def status(st):
    from wdf_hip import binding as wb
    return wb.mlp_tp_status(st)


def clean(s):
    return s["n_bad"] == 0 and s["gated_waves"] == 0


def pots(B):
    return POTS[np.arange(B) % 3]


def oracle_fwd(t64, x, r):
    """the oracle's y [T,B] with one pot per sequence: one call per distinct pot value on the rows that carry it"""
    oracle = _ORACLE["o"]
    y = np.zeros((x.shape[1], x.shape[0]))
    for v in np.unique(r):
        rows = np.nonzero(r == v)[0]
        th = t64.copy()
        th[4] = float(np.float32(v))
        y[:, rows] = oracle.clipper_asym_fwd(th, FS, np.ascontiguousarray(x[rows].astype(np.float64)))
    return y


def sums64(y, tg, skip=0):
    """(S, E, mse, mse + esr) in fp64 over the rows skip..T-1 of y, tg [T,B]"""
    o, t = np.asarray(y[skip:], dtype=np.float64), np.asarray(tg[skip:], dtype=np.float64)
    S, E, n = float(np.sum((o - t) ** 2)), float(np.sum(o ** 2)), float(o.size)
    return S, E, S / n, S / n + np.sqrt(S / (E + EPS) / n)


@functools.lru_cache(maxsize=None)
def case(name, shape, seed=3):
    """x, the pots, the teacher's target (fp32, as the device reads it), the oracle's y at the fp32-rounded parameters and its
    y at every perturbed parameter of the finite differences: computed once per input, shared by the tests, never modified."""
    from wdf_hip import workload
    B, T = SHAPES[shape][:2]
    t64 = r32(SETS[name])
    x, r = workload.sweep_batch(B, T, seed=seed), pots(B)
    teacher = t64.copy()
    teacher[TRAIN] *= TEACHER
    tg = oracle_fwd(teacher, x, r).astype(np.float32)
    ref = oracle_fwd(t64, x, r)
    pert = {}
    for i in TRAIN:
        h = 1e-6 * t64[i]
        tp, tm = t64.copy(), t64.copy()
        tp[i] += h
        tm[i] -= h
        pert[i] = (oracle_fwd(tp, x, r), oracle_fwd(tm, x, r), h)
    for a in (x, r, tg, ref):
        a.setflags(write=False)
    return x, r, tg, ref, pert


def fd_grad(pert, tg, skip=None):
    """central differences of the whole-batch MSE (skip None) or MSE + ESR past skip over the five trainable components"""
    k, s = (2, 0) if skip is None else (3, skip)
    return np.array([(sums64(pert[i][0], tg, s)[k] - sums64(pert[i][1], tg, s)[k]) / (2 * pert[i][2]) for i in TRAIN])


def rel(got, ref):
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / np.abs(ref)


@pytest.fixture(autouse=True)
def _oracle(oracle):
    _ORACLE["o"] = oracle


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """The steppers this file's calls cached and the blocks its tensors freed go back to the device when the file is done:
    tests/test_gpu_cache_identity.py relies on the caching allocator handing a freed block straight back."""
    yield
    from wdf_hip import binding, engine
    engine._ClipperAsymEsrFn._steppers.clear()
    engine._ClipperAsymMseFn._steppers.clear()
    engine.LAST_TP_STATUS["status"] = None
    binding._R_VEC_CACHE.d.clear()
    case.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def composed(theta, xd, rd, tgd, mode, tp, skip=None):
    """the composed pot path: forward with stash, the torch loss, bwd_tp_rseq -> loss, gradient (fp64 numpy), y"""
    from wdf_hip import engine
    th = dev(theta).requires_grad_(True)
    y = engine.clipper_asym(th, xd, FS, mode=mode, tp=tp, r=rd)
    if skip is None:
        loss = torch.mean((y - tgd) ** 2)
    else:
        o, t = y[skip:], tgd[skip:]
        S, E, n = torch.sum((o - t) ** 2), torch.sum(o ** 2) + EPS, float(o.numel())
        loss = S / n + torch.sqrt(S / E / n)
    loss.backward()
    return float(loss.detach()), th.grad.cpu().numpy().astype(np.float64), y.detach()


@pytest.mark.parametrize("solver", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_forward_sequential_and_chunked_vs_oracle(name, solver):
    from wdf_hip import binding as wb
    mode = MODES[solver]
    for shape in ("ragged", "clean"):
        B, T, K, W = SHAPES[shape]
        x, r, _, ref, _ = case(name, shape)
        xd, rd, th = dev(x), dev(r), dev(SETS[name])
        y, zT, _ = wb.clipper_asym_fwd_rseq(xd, rd, th, FS, mode, want_zT=True)
        e_seq = float(np.max(np.abs(y.cpu().numpy() - ref)))
        print(f"forward {name} {solver} {B}x{T}: sequential max|y - oracle| = {e_seq:.3e}")
        assert e_seq <= 3e-6
        if K > 1:
            yc, zTc, _, st = wb.clipper_asym_fwd_tp_rseq(xd, rd, th, FS, mode, K, W, want_zT=True)
            s = status(st)
            e_tp = float(np.max(np.abs(yc.cpu().numpy() - ref)))
            print(f"forward {name} {solver} {B}x{T}: K = {K}, W = {W}: max|y - oracle| = {e_tp:.3e}, status {s}, "
                  f"max|zT - sequential| = {float((zTc - zT).abs().max()):.3e}")
            assert clean(s), s
            assert e_tp <= 3e-6 and float((zTc - zT).abs().max()) <= 1e-6


@pytest.mark.parametrize("solver", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_reverse_sweep_vs_finite_differences(name, solver):
    from wdf_hip import binding as wb
    mode = MODES[solver]
    for shape, kb in (("ragged", 1), ("ragged", 3), ("clean", 4)):
        B, T, _, _ = SHAPES[shape]
        x, r, tg, _, pert = case(name, shape)
        xd, rd, tgd, th = dev(x), dev(r), dev(tg), dev(SETS[name])
        y, zT, _, zs = wb.clipper_asym_fwd_rseq(xd, rd, th, FS, mode, want_zT=True, want_stash=True)
        gy = (2.0 / y.numel()) * (y - tgd)
        g = wb.clipper_asym_bwd_tp_rseq(xd, rd, th, FS, mode, zs, zT, gy.contiguous(), kb).cpu().numpy()
        err = rel(g[TRAIN], fd_grad(pert, tg))
        print(f"bwd_tp_rseq {name} {solver} {B}x{T} in {kb} chunk(s): gradient vs finite differences {err}, dR = {g[4]!r}")
        assert g[4] == 0.0
        assert np.max(err) <= 2e-4, (g, err)


@pytest.mark.parametrize("solver", list(MODES))
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_mse_step_vs_oracle(shape, name, solver):
    from wdf_hip import binding as wb
    mode = MODES[solver]
    B, T, K, W = SHAPES[shape]
    x, r, tg, ref, pert = case(name, shape)
    xd, rd, tgd, th = dev(x), dev(r), dev(tg), dev(SETS[name])
    y, zT, out7, st = wb.clipper_asym_step_mse_rseq(xd, rd, th, FS, mode, tgd, 2.0 / (B * T), K, W, want_zT=True)
    s, o, yh = status(st), out7.cpu().numpy().astype(np.float64), y.cpu().numpy()
    S_ref, S_own = sums64(ref, tg)[0], sums64(yh, tg)[0]
    e_y, err = float(np.max(np.abs(yh - ref))), rel(o[1:][TRAIN], fd_grad(pert, tg))
    print(f"MSE step {shape} {name} {solver}: status {s}, max|y - oracle| = {e_y:.3e}, S vs oracle {abs(o[0] - S_ref) / S_ref:.3e}, "
          f"vs own y {abs(o[0] - S_own) / S_own:.3e}, gradient vs finite differences {err}, dR = {o[5]!r}")
    assert e_y <= 3e-6
    assert abs(o[0] - S_ref) <= 1e-5 * S_ref and abs(o[0] - S_own) <= 1e-6 * S_own
    assert o[5] == 0.0 and np.max(err) <= 2e-4
    if shape == "clean":
        assert clean(s), s
    if shape == "repair":          # every wave holds a 75 kOhm sequence: all boundaries miss, the gated launch repairs every wave
        assert s["n_bad"] > 0 and s["gated_waves"] == (B + 63) // 64, s
        y1, zT1, out1, _ = wb.clipper_asym_step_mse_rseq(xd, rd, th, FS, mode, tgd, 2.0 / (B * T), 1, 0, want_zT=True)
        assert torch.equal(y, y1) and torch.equal(zT, zT1) and torch.equal(out7, out1)       # the K = 1 result, bit for bit
        n = float(B * (T - 50))
        e8 = wb.clipper_asym_step_esr_rseq(xd, rd, th, FS, mode, tgd, n, EPS, 50, K, W)
        e1 = wb.clipper_asym_step_esr_rseq(xd, rd, th, FS, mode, tgd, n, EPS, 50, 1, 0)
        print(f"   MSE + ESR step: status {status(e8[5])}")
        assert status(e8[5])["gated_waves"] == (B + 63) // 64
        assert all(torch.equal(a, b) for a, b in zip(e8[:5:2] + (e8[3],), e1[:5:2] + (e1[3],)))


@pytest.mark.parametrize("solver", list(MODES))
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("skip", [0, 50, 517])
def test_esr_step_vs_oracle(skip, name, solver):
    """skip = 517 falls inside an 8-step block (512..519) of the second of four 512-step chunks"""
    from wdf_hip import binding as wb
    mode = MODES[solver]
    B, T, K, W = SHAPES["clean"]
    x, r, tg, ref, pert = case(name, "clean")
    xd, rd, tgd, th = dev(x), dev(r), dev(tg), dev(SETS[name])
    n = float(B * (T - skip))
    y, _, sums, g, loss3, st = wb.clipper_asym_step_esr_rseq(xd, rd, th, FS, mode, tgd, n, EPS, skip, K, W)
    s, sm, gh, yh = status(st), sums.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64), y.cpu().numpy()
    (S_ref, E_ref, _, L_ref), (S_own, E_own, _, _) = sums64(ref, tg, skip), sums64(yh, tg, skip)
    err = rel(gh[TRAIN], fd_grad(pert, tg, skip))
    print(f"ESR step skip {skip} {name} {solver}: status {s}, S vs oracle {abs(sm[0] - S_ref) / S_ref:.3e} / own y "
          f"{abs(sm[0] - S_own) / S_own:.3e}, E vs oracle {abs(sm[1] - E_ref) / E_ref:.3e} / own y {abs(sm[1] - E_own) / E_own:.3e}, "
          f"loss {float(loss3[2]):.6e} vs {L_ref:.6e}, gradient vs finite differences {err}, dR slots {gh[4]!r} {sm[6]!r} {sm[12]!r}")
    assert clean(s), s
    assert float(np.max(np.abs(yh - ref))) <= 3e-6
    assert abs(sm[0] - S_ref) <= 1e-5 * S_ref and abs(sm[1] - E_ref) <= 1e-5 * E_ref
    assert abs(sm[0] - S_own) <= 1e-6 * S_own and abs(sm[1] - E_own) <= 1e-6 * E_own
    assert abs(float(loss3[2]) - L_ref) <= 1e-5 * L_ref
    assert gh[4] == 0.0 and sm[6] == 0.0 and sm[12] == 0.0
    assert np.max(err) <= 2e-4, (gh, err)


@pytest.mark.parametrize("solver", list(MODES))
def test_steps_with_state_and_the_multi_rank_form(solver):
    """z0 / zT: two calls on the halves in time equal one call on the whole; n_global + wdf_asym_esr_finish: two shards of the
    batch, their sums14 added, give the single call's loss and gradient."""
    from wdf_hip import binding as wb
    mode, name, skip = MODES[solver], "theta6", 50
    B, T, K, W = SHAPES["clean"]
    x, r, tg, _, _ = case(name, "clean")
    xd, rd, tgd, th = dev(x), dev(r), dev(tg), dev(SETS[name])
    n = float(B * (T - skip))
    y, zT, sums, g, loss3, _ = wb.clipper_asym_step_esr_rseq(xd, rd, th, FS, mode, tgd, n, EPS, skip, K, W, want_zT=True)
    h = T // 2
    ya, za, sa, _, _, _ = wb.clipper_asym_step_esr_rseq(xd[:, :h].contiguous(), rd, th, FS, mode, tgd[:h].contiguous(), n, EPS, skip, 2, W,
                                                        want_zT=True, finish=False)
    yb, zb, sb, _, _, _ = wb.clipper_asym_step_esr_rseq(xd[:, h:].contiguous(), rd, th, FS, mode, tgd[h:].contiguous(), n, EPS, 0, 2, W,
                                                        z0=za, want_zT=True, finish=False)
    e_y = max(float((ya - y[:h]).abs().max()), float((yb - y[h:]).abs().max()))
    e_s = float(((sa + sb)[:2] - sums[:2]).abs().max() / sums[:2].abs().min())
    print(f"z0 / zT {solver}: y {e_y:.3e} V, zT {float((zb - zT).abs().max()):.3e}, S and E of the halves added vs whole {e_s:.3e}")
    assert e_y <= 1e-6 and float((zb - zT).abs().max()) <= 1e-6 and e_s <= 1e-6
    ym, zm, om, _ = wb.clipper_asym_step_mse_rseq(xd[:, h:].contiguous(), rd, th, FS, mode, tgd[h:].contiguous(), 1.0, 2, W, z0=za, want_zT=True)
    print(f"   MSE step from z0: y {float((ym - y[h:]).abs().max()):.3e} V")
    assert float((ym - y[h:]).abs().max()) <= 1e-6 and float((zm - zT).abs().max()) <= 1e-6
    hb = 128                                              # two ranks: the halves of the batch (pots and all)
    parts = [wb.clipper_asym_step_esr_rseq(xd[a:b].contiguous(), rd[a:b].contiguous(), th, FS, mode, tgd[:, a:b].contiguous(), n, EPS, skip,
                                           K, W, finish=False) for a, b in ((0, hb), (hb, B))]
    assert parts[0][3] is None and parts[0][4] is None
    g2, l2 = wb.asym_esr_finish(parts[0][2] + parts[1][2], n, EPS)
    e_g = rel(g2.cpu().numpy()[TRAIN], g.cpu().numpy().astype(np.float64)[TRAIN])
    print(f"   two ranks {solver}: loss {float(l2[2]):.6e} vs {float(loss3[2]):.6e}, gradient {e_g}, dR = {float(g2[4])!r}")
    assert abs(float(l2[2]) - float(loss3[2])) <= 1e-6 * float(loss3[2]) and np.max(e_g) <= 2e-5 and float(g2[4]) == 0.0


@pytest.mark.parametrize("solver", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_a_uniform_pot_reproduces_the_static_entry_points(name, solver):
    from wdf_hip import binding as wb
    mode, theta = MODES[solver], SETS[name]
    B, T, K, W = SHAPES["clean"]
    x, _, tg, _, _ = case(name, "clean")
    xd, tgd, th = dev(x), dev(tg), dev(theta)
    rd = th[4].repeat(B).contiguous()
    n, skip = float(B * (T - 50)), 50
    y0, _, o0, _ = wb.clipper_asym_step_mse(xd, th, FS, mode, tgd, 2.0 / (B * T), K, W)
    y1, _, o1, _ = wb.clipper_asym_step_mse_rseq(xd, rd, th, FS, mode, tgd, 2.0 / (B * T), K, W)
    e0, e1 = wb.clipper_asym_step_esr(xd, th, FS, mode, tgd, n, EPS, skip, K, W), wb.clipper_asym_step_esr_rseq(xd, rd, th, FS, mode, tgd, n, EPS, skip, K, W)
    yf0, yf1 = wb.clipper_asym_fwd(xd, th, FS, mode)[0], wb.clipper_asym_fwd_rseq(xd, rd, th, FS, mode)[0]
    o0, o1 = o0.cpu().numpy().astype(np.float64), o1.cpu().numpy().astype(np.float64)
    s0, s1 = e0[2].cpu().numpy().astype(np.float64), e1[2].cpu().numpy().astype(np.float64)
    g0, g1 = e0[3].cpu().numpy().astype(np.float64), e1[3].cpu().numpy().astype(np.float64)
    e_y = max(float((y1 - y0).abs().max()), float((e1[0] - e0[0]).abs().max()), float((yf1 - yf0).abs().max()))
    e_g, e_ge = rel(o1[1:][TRAIN], o0[1:][TRAIN]), rel(g1[TRAIN], g0[TRAIN])
    print(f"uniform pot {name} {solver}: y {e_y:.3e} V, S {abs(o1[0] - o0[0]) / o0[0]:.3e}, ESR S / E {rel(s1[:2], s0[:2])}, "
          f"MSE gradient {e_g}, MSE + ESR gradient {e_ge}, dR {o1[5]!r} {g1[4]!r}")
    assert e_y <= 1e-6
    assert abs(o1[0] - o0[0]) <= 1e-6 * o0[0] and np.max(rel(s1[:2], s0[:2])) <= 1e-6
    assert np.max(e_g) <= 2e-5 and np.max(e_ge) <= 2e-5
    assert o1[5] == 0.0 and g1[4] == 0.0 and s1[6] == 0.0 and s1[12] == 0.0


@pytest.mark.parametrize("loss", ["mse", "esr"])
def test_adam_in_the_finish_never_writes_the_pot_slot(loss):
    from wdf_hip import binding as wb
    B, T, K, W = SHAPES["ragged"]
    x, r, tg, _, _ = case("theta6", "ragged")
    xd, rd, tgd = dev(x), dev(r), dev(tg)
    lr = np.array([1e-10, 1e-3, 1e-8, 1e-3, 1e2, 1e-10], dtype=np.float32)
    lo, hi = np.full(6, 1e-15, dtype=np.float32), np.array([1e-3, 1.0, 1e-3, 1.0, 1.0, 1.0], dtype=np.float32)   # hi[4] = 1 < R
    th, th_ref = dev(THETA6), dev(THETA6)
    before = th.clone()
    opt, opt_ref = wb.Adam(6, lr, lo=lo, hi=hi), wb.Adam(6, lr, lo=lo, hi=hi)
    for it in range(2):
        th_ref.copy_(th)                                  # one update each, from the same values
        if loss == "mse":
            g = wb.clipper_asym_step_mse_rseq(xd, rd, th, FS, 2, tgd, 2.0 / (B * T), K, W, opt=opt)[2][1:7].clone()
        else:
            g = wb.clipper_asym_step_esr_rseq(xd, rd, th, FS, 2, tgd, float(B * T), EPS, 0, K, W, opt=opt)[3].clone()
        opt_ref.apply(th_ref, g.contiguous())            # (clips slot 4 to hi[4] = 1: the step's finish must not)
        same = torch.equal(th[4].view(torch.int32), before[4].view(torch.int32))
        err = ((th - th_ref).abs() / th_ref.abs()).cpu().numpy()
        print(f"Adam in the {loss} finish, step {it + 1}: theta6[4] bit-identical: {same}, moments of slot 4: {float(opt.m[4])!r} "
              f"{float(opt.v[4])!r}, others vs wdf_adam_step {err}")
        assert same and float(opt.m[4]) == 0.0 and float(opt.v[4]) == 0.0
        assert float(g[4]) == 0.0 and np.max(err[TRAIN]) <= 4 * 2.0 ** -24
    assert int(opt.step) == 2 and float(th_ref[4]) == 1.0


def build_circuit(theta, solver="newton_f32", **kw):
    import tf_wdf as W
    Is1, V1, Is2, V2, R, Cv = [float(t) for t in theta]
    Vs = W.ResistiveVoltageSource(R, trainable=True)
    Cap = W.Capacitor(Cv, FS, trainable=True)
    P1 = W.Parallel(Vs, Cap)
    dp = W.AsymDiodePair(P1, Is1, Is2, Vt=1.0, nDiodes_up=V1, nDiodes_down=V2, trainable=True, solver=solver)
    return W, W.Circuit(P1, dp, Cap, per_sequence_R=Vs, **kw), [dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down, Cap.C], Vs


@pytest.mark.parametrize("solver", list(MODES))
def test_circuit_with_a_pot_per_sequence(solver):
    from wdf_hip import binding as wb
    mode, name, skip = MODES[solver], "theta6", 50
    B, T, _, _ = SHAPES["ragged"]
    x, r, tg, ref, _ = case(name, "ragged")
    x2 = dev(np.stack([x, np.repeat(r[:, None], T, axis=1)], axis=2))          # [B,T,2] = (Vin, R): clipper_pot.py:68-70
    xd, rd, tgd = dev(x), dev(r), dev(tg)
    W, circ, variables, Vs = build_circuit(SETS[name], solver=solver, time_parallel=None)
    tf = W.tf
    l_mse, g_mse, y_eng = composed(r32(SETS[name]), xd, rd, tgd, mode, None)
    l_esr, g_esr, _ = composed(r32(SETS[name]), xd, rd, tgd, mode, None, skip)
    y = circ(x2)
    e_y = float((y - y_eng).abs().max())
    print(f"Circuit {solver}: circ(x) vs engine {e_y:.3e} V, vs oracle {float(np.max(np.abs(y.cpu().numpy() - ref))):.3e} V")
    assert e_y <= 1e-6 and float(np.max(np.abs(y.cpu().numpy() - ref))) <= 3e-6
    for what, call, l_ref, g_ref in (("circ(x) + tf loss", lambda: tf.reduce_mean(tf.square(circ(x2) - tgd)), l_mse, g_mse),
                                     ("mse", lambda: circ.mse(x2, tgd), l_mse, g_mse),
                                     ("mse_esr", lambda: circ.mse_esr(x2, tgd, skip=skip), l_esr, g_esr)):
        with tf.GradientTape() as tape:
            loss = call()
        grads = tape.gradient(loss, variables + [Vs.R])
        got = np.array([float(g) for g in grads[:5]])
        err = rel(got, g_ref[TRAIN])
        print(f"Circuit.{what} {solver}: loss {float(loss):.6e} vs composed {l_ref:.6e}, gradient vs composed {err}, "
              f"vs.R gradient: {grads[5]!r}")
        assert abs(float(loss) - l_ref) <= 1e-6 * l_ref and np.max(err) <= 2e-5
        assert grads[5] is None or float(grads[5]) == 0.0
    assert float((circ.last_output - y_eng).abs().max()) <= 1e-6
    # carry_state: two calls on the halves in time equal one call on the whole
    h = T // 2
    for fn in (lambda xs, ts: circ.mse(xs, ts, carry_state=True), lambda xs, ts: circ.mse_esr(xs, ts, carry_state=True)):
        circ.reset_state()
        fn(x2[:, :h].contiguous(), tgd[:h])
        y_first = circ.last_output.clone()
        fn(x2[:, h:].contiguous(), tgd[h:])
        ec = max(float((y_first - y_eng[:h]).abs().max()), float((circ.last_output - y_eng[h:]).abs().max()))
        print(f"   carry_state: {ec:.3e} V")
        assert tuple(circ.last_state.shape) == (1, B) and ec <= 1e-6
    # z0 / return_state through __call__
    ya, za = circ(x2[:, :h].contiguous(), return_state=True)
    yb = circ(x2[:, h:].contiguous(), z0=za)
    assert max(float((ya - y_eng[:h]).abs().max()), float((yb - y_eng[h:]).abs().max())) <= 1e-6
    moving = x2.clone()
    moving[3, 100, 1] = 46.0e3
    for call in (lambda: circ(moving), lambda: circ.mse(moving, tgd), lambda: circ.mse_esr(moving, tgd, skip=skip)):
        with pytest.raises(wb.WdfHipError, match="one resistance per sequence"):
            call()


@pytest.mark.parametrize("solver", list(MODES))
def test_steps_vs_the_composed_pot_path_with_the_planned_chunks(solver):
    from wdf_hip import engine
    mode, name, skip = MODES[solver], "theta6", 50
    B, T, _, _ = SHAPES["clean"]
    x, r, tg, _, _ = case(name, "clean")
    xd, rd, tgd = dev(x), dev(r), dev(tg)
    tp = engine.plan_asym_time_parallel(B, T, float(POTS.max()), THETA6[5], FS)
    assert tp.k_fwd > 1
    for what, sk in (("mse", None), ("mse_esr", skip)):
        l_c, g_c, y_c = composed(r32(SETS[name]), xd, rd, tgd, mode, tp, sk)
        th = dev(SETS[name]).requires_grad_(True)
        if sk is None:
            loss, y, _ = engine.clipper_asym_mse(th, xd, tgd, FS, tp=tp, mode=mode, return_state=True, r=rd)
        else:
            loss, y, _ = engine.clipper_asym_mse_esr(th, xd, tgd, FS, skip=sk, tp=tp, mode=mode, return_state=True, r=rd)
        s = status(engine.LAST_TP_STATUS["status"])
        loss.backward()
        g = th.grad.cpu().numpy().astype(np.float64)
        err = rel(g[TRAIN], g_c[TRAIN])
        print(f"engine {what} {solver}, plan {tuple(tp)}: status {s}, loss {float(loss):.6e} vs composed {l_c:.6e}, gradient {err}, "
              f"y {float((y - y_c).abs().max()):.3e} V")
        assert clean(s), s
        assert abs(float(loss) - l_c) <= 1e-6 * l_c and np.max(err) <= 2e-5 and g[4] == 0.0 and g_c[4] == 0.0
        assert float((y - y_c).abs().max()) <= 1e-6
