"""GPU: the linear one-pass MSE + ESR step (csrc/wdf_ss_step.h: wdf_ss_lin_step_esr, wdf_ss_lin_esr_finish) at kernel level, through
binding.ss_lin_step_esr / ss_lin_esr_finish, against the float64 restatement of tests/ss_lin_esr_ref.py (pinned on the CPU by
tests/test_ss_lin_esr_ref_cpu.py, which also asserts the caps and the absence of cancelled gradients over exactly these cases).

  A  every instantiation: ns in {0,1,2} x ni in {1,2} x {one, two sequences per lane} at (B, T, k) = (1, 40, 1), (65, 100, 4),
     (130, 257, 3): dead lanes, last chunks of 4 and 65 steps (of one step: section C's (33, 2) and (65, 3)), B = 130 dropping to
     one per lane when x, target and y sit at 4 mod 8;
  B  skip in {0, 1, 7, 32, inside chunk 2 and no multiple of 8, T - 1} on trees (1,1) and (2,2): y is right on the rows before skip too;
  C  chunk geometry (T, k) in {(33, 2), (65, 3), (1000, 5), (2048, 64)} on (2,1), both lane widths;
  D  z0 / zT handed across two calls on (2,2), against the references of the halves and one call of double length;
  E  the finish: 1 and 15 parameters, an n_global larger than the call's own n, esr = 0, g == NULL, two half-batch calls + finish,
     the same bits on a reused workspace and the ticket left 0, the MSE step's SSE and gcoef at skip = 0, the wrapper's refusals,
     the three families' finish exports giving the same bits on the same sums (one kernel) within one fp32 ulp of dist.py.

Bounds (none relative to a gradient entry, none taken from what the kernel gives):
  y, zT        3e-6 max(1, max |ref|)            tests/test_gpu_ss_lin_step_kernel.py's row for this arithmetic
  S, E         1e-5 relative                      that module's SSE bound
  GP[i], GQ[i] 4e-6 mag_i                         that module's derivation: 8 x the fp32 restatement's cap (2e-7; 2.2e-7 for the Q family,
                                                  see the CPU file) + the kernel's 32-addend fp32 sums, 32 x 2^-24: 3.5e-6 / 3.7e-6, rounded up
  sums gP, gQ  sum_i 4e-6 mag_i |jac[row_i, p]| + one fp32 ulp of the value            (the contraction is in fp64)
  g[p] against the device's own sums   2 fp32 ulp of |ga gP| + |gb gQ|, ga and gb recomputed in fp64 from the device's float S and E
  g[p] end to end   4e-6 (|ga| magP_p + |gb| magQ_p) + what S and E within 1e-5 move ga and gb by: 1e-5 |gP_p / (esr (E + eps) n)|
                    + 2e-5 |gb gQ_p| (d ln ga_2 = -(d ln S + d ln E) / 2, d ln gb = d ln S / 2 - 3 d ln E / 2) + one fp32 ulp
  loss3        mse 1e-5, esr 1e-5 (a square root of S / E), each + one fp32 ulp

Every check prints `FIG <section> | <case> | ...` with each error divided by its bound before it asserts (run with -s).

Also in E: NaN and Inf in the rows of target before skip leave every output bit for bit what a clean target gives.

Measured on an MI355X (worst figure of each section, error / bound; 74 tests, all passing, 3.1 s in all; the figures below are
the same on the build with two pass-2 kernels and on the one with ss_lin_step_kernel<NS, NI, V, LOSS> alone: the outputs are the
same bytes; the three finish exports against dist.py, of one fp32 ulp: g 0.41, loss3 0.46):
  A  y 0.049  S 0.012  E 0.011  GP 0.109  GQ 0.136 (B = 1, T = 40)  gP 0.015  gQ 0.016  g 0.009  g_own 0.428  loss3 0.010  zT 0.025
  B  y 0.049  S 0.006  E 0.005  GP 0.017  GQ 0.020  g 0.006  g_own 0.522 ((2,2) B = 65 skip = 1)  loss3 0.006  zT 0.025
  C  y 0.043  S 0.009  E 0.005  GP 0.051  GQ 0.047  gP 0.031  g 0.016  g_own 0.398  loss3 0.009
  D  y 0.034  S 0.003  E 0.003  GP 0.004  GQ 0.007  g 0.001  g_own 0.400  zT 0.038
  E  y 0.049  GP 0.006  GQ 0.003  g 0.007  g_own 0.447  halves + finish 0.345; the same bits on a reused workspace, the ticket 0;
     at skip = 0, S, GP and y equal the MSE step's SSE, gcoef_out (gscale = 1) and y BIT FOR BIT
"""
import gc

import numpy as np
import pytest

import ss_lin_esr_ref as E
import ss_lin_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B_Y, B_SUM, B_G = 3e-6, 1e-5, E.B_G


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def cuda(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def one_float_in(a):
    """The array on the device as a dense view that starts one float into its storage: 4 mod 8 bytes."""
    a = np.asarray(a, dtype=np.float32)
    base = torch.empty((a.size + 1,), dtype=torch.float32, device="cuda")
    v = base[1:].view(*a.shape)
    v.copy_(torch.as_tensor(a))
    assert v.is_contiguous() and v.data_ptr() % 8 == 4
    return v


def call(c, n_chunks, want_zT=False, z0="case", finish=True, misaligned=False, ws=None, x=None, target=None, n_global="case"):
    from wdf_hip import binding as wb
    z0 = (None if c.z0 is None else cuda(c.z0)) if isinstance(z0, str) else z0
    xs = (one_float_in(c.x) if misaligned else cuda(c.x)) if x is None else x
    tg = (one_float_in(c.target) if misaligned else cuda(c.target)) if target is None else target
    y = one_float_in(np.zeros((c.T, c.B))) if misaligned else None
    return wb.ss_lin_step_esr(xs, cuda(c.coef), cuda(c.jac, np.float64), tg, c.skip, n_chunks,
                              n_global=c.n_global if isinstance(n_global, str) else n_global, z0=z0, want_zT=want_zT, want_gcoef=True,
                              ws=ws, y=y, finish=finish)


def ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def g_from_sums(sums, n_params, n, eps=E.EPS):
    """ga, gb, |ga gP| + |gb gQ| and g in fp64 from float sums {S, E, gP, gQ}"""
    s = np.asarray(sums, dtype=np.float64)
    r = E.Result()
    r.S, r.E, r.n = s[0], s[1], float(n)
    E.finish(r, eps)
    gP, gQ = s[2:2 + n_params], s[2 + n_params:]
    return r, np.abs(r.ga * gP) + np.abs(r.gb * gQ), r.ga * gP + r.gb * gQ


def check(section, label, c, res, ref=None):
    """every output of one call against the reference; prints the figures (error / bound), then asserts"""
    ref = c.ref() if ref is None else ref
    P, kG = c.n_params, R.kg(c.ns, c.ni)
    y = res["y"].cpu().numpy().astype(np.float64)
    sums = res["sums"].cpu().numpy().astype(np.float64)
    gc_ = res["gcoef"].cpu().numpy().astype(np.float64)
    f = {"y": ratio(np.max(np.abs(y - ref.y)), B_Y * max(1.0, np.max(np.abs(ref.y)))),
         "S": ratio(abs(sums[0] - ref.S), B_SUM * ref.S), "E": ratio(abs(sums[1] - ref.E), B_SUM * ref.E),
         "GP": ratio(np.abs(gc_[:kG] - ref.GP), B_G * ref.magP), "GQ": ratio(np.abs(gc_[kG:] - ref.GQ), B_G * ref.magQ),
         "gP": ratio(np.abs(sums[2:2 + P] - ref.gP), B_G * ref.magPp + ulp32(ref.gP)),
         "gQ": ratio(np.abs(sums[2 + P:] - ref.gQ), B_G * ref.magQp + ulp32(ref.gQ))}
    fin = [y, sums, gc_]
    if res["g"] is not None:
        g = res["g"].cpu().numpy().astype(np.float64)
        l3 = res["loss3"].cpu().numpy().astype(np.float64)
        fin += [g, l3]
        dev, dev_mag, dev_g = g_from_sums(sums, P, ref.n)
        f["g_own"] = ratio(np.abs(g - dev_g), 2 * ulp32(dev_mag))
        a2 = 1.0 / (ref.esr * (ref.E + E.EPS) * ref.n)
        f["g"] = ratio(np.abs(g - ref.gp), B_G * ref.gpmag + B_SUM * np.abs(a2 * ref.gP) + 2 * B_SUM * np.abs(ref.gb * ref.gQ) + ulp32(ref.gp))
        f["mse"] = ratio(abs(l3[0] - ref.mse), B_SUM * ref.mse + ulp32(ref.mse))
        f["esr"] = ratio(abs(l3[1] - ref.esr), B_SUM * ref.esr + ulp32(ref.esr))
        f["loss"] = ratio(abs(l3[2] - ref.loss), B_SUM * ref.loss + ulp32(ref.loss))
    if res["zT"] is not None:
        f["zT"] = ratio(np.max(np.abs(res["zT"].cpu().numpy().astype(np.float64) - ref.zT)), B_Y * max(1.0, np.max(np.abs(ref.zT))))
    print(f"FIG {section} | {label} {c} | " + " ".join(f"{k}={v:.3f}" for k, v in f.items()))
    assert all(np.all(np.isfinite(a)) for a in fin)
    assert all(v <= 1.0 for v in f.values()), (section, label, repr(c), f)
    return f


# ---- A: every instantiation --------------------------------------------------------------------------------------------------
CASES_A = [(B, T, k, False) for B, T, k in E.SHAPES_A] + [(130, 257, 3, True)]


@pytest.mark.parametrize("B,T,k,mis", CASES_A, ids=[f"B{B}-T{T}-k{k}-" + ("one-4mod8" if m else ("two" if B % 2 == 0 else "one")) for B, T, k, m in CASES_A])
@pytest.mark.parametrize("ns,ni", R.TREES, ids=[f"ns{a}-ni{b}" for a, b in R.TREES])
def test_a_every_instantiation(ns, ni, B, T, k, mis):
    c = E.case(ns, ni, B, T, E.SKIP_A)
    res = call(c, k, want_zT=True, misaligned=mis)
    assert (res["zT"] is None) == (ns == 0) and (res["y"].data_ptr() % 8 == 4) == mis
    check("A", ("4 mod 8 " if mis else "") + f"k={k}", c, res)


# ---- B: skip positions -------------------------------------------------------------------------------------------------------
CASES_B = [(ns, ni, B, T, k, s) for ns, ni in E.TREES_B for B, T, k in E.SHAPES_B for s in E.skips_b(T)]


@pytest.mark.parametrize("ns,ni,B,T,k,skip", CASES_B, ids=[f"ns{a}-ni{b}-B{B}-T{T}-skip{s}" for a, b, B, T, k, s in CASES_B])
def test_b_skip_positions(ns, ni, B, T, k, skip):
    check("B", f"k={k}", E.case(ns, ni, B, T, skip), call(E.case(ns, ni, B, T, skip), k, want_zT=True))


# ---- C: chunk geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,k", E.GEOM_C, ids=[f"T{T}-k{k}" for T, k in E.GEOM_C])
@pytest.mark.parametrize("B", E.BATCHES_C, ids=["one-B65", "two-B130"])
def test_c_chunk_geometry(B, T, k):
    from wdf_hip import binding as wb
    c = E.case(2, 1, B, T, E.skip_c(T))
    res = call(c, k)
    L, K = wb.chunk_geom(T, k, 32)
    assert res["ws"].numel() == wb.lib().wdf_ss_lin_step_esr_ws_bytes(2, 1, B, T, K)
    check("C", f"L={L} K={K} (asked {k})", c, res)


# ---- D: the state handed over ------------------------------------------------------------------------------------------------
def test_d_two_calls_with_the_state_handed_over():
    """the first half from a random z0, the second from the first's zT: each against its own reference (the hand-over is a constant
    of the second call: its tangents start at 0); and against ONE call over all 514 steps with skip = 257 + the second call's skip:
    the same y rows, final states, S and E (its gradient carries the tangents across the hand-over, so that one is not compared)"""
    long, first, second = E.carried()
    z0 = cuda(first.z0)
    before = z0.clone()
    r1 = call(first, 3, want_zT=True, z0=z0)
    check("D", "first half", first, r1)
    assert torch.equal(z0.view(torch.int32), before.view(torch.int32)) and r1["zT"].data_ptr() != z0.data_ptr()
    r2 = call(second, 3, want_zT=True, z0=r1["zT"])
    check("D", "second half from the first's zT", second, r2)
    rl = call(long, 6, want_zT=True)
    check("D", "one call of double length", long, rl)
    both = torch.cat([r1["y"], r2["y"]]).cpu().numpy().astype(np.float64)
    yl, wref = rl["y"].cpu().numpy().astype(np.float64), long.ref()
    assert np.max(np.abs(both - yl)) <= 2 * B_Y * max(1.0, np.max(np.abs(wref.y)))
    assert np.max(np.abs((r2["zT"] - rl["zT"]).cpu().numpy())) <= 2 * B_Y * max(1.0, np.max(np.abs(wref.zT)))
    s2, sl = r2["sums"].cpu().numpy().astype(np.float64), rl["sums"].cpu().numpy().astype(np.float64)
    assert abs(s2[0] - sl[0]) <= 2 * B_SUM * wref.S and abs(s2[1] - sl[1]) <= 2 * B_SUM * wref.E


# ---- E: counts and finish ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_params", E.PARAMS_E)
def test_e_parameter_counts_and_a_reused_workspace(n_params):
    """1 and 15 parameters; two more calls on the workspace of the first give the same bits, the ticket (its first word) 0 after each"""
    c = E.case(2, 2, 130, 257, E.SKIP_E, n_params=n_params)
    res = call(c, 3, want_zT=True)
    check("E", f"n_params={n_params} call 1", c, res)
    ws = res["ws"]
    assert int(ws[:4].view(torch.int32)[0]) == 0
    keep = {k: res[k].clone() for k in ("y", "sums", "g", "loss3", "gcoef", "zT")}
    for n in (2, 3):
        res = call(c, 3, want_zT=True, ws=ws)
        assert res["ws"].data_ptr() == ws.data_ptr() and int(ws[:4].view(torch.int32)[0]) == 0
        for k, v in keep.items():
            assert torch.equal(res[k].view(torch.int32), v.view(torch.int32)), (k, n)
    check("E", f"n_params={n_params} call 3", c, res)


def test_e_n_global_larger_than_the_calls_own_n():
    c = E.case(2, 2, 130, 257, E.SKIP_E, n_global=E.N_GLOBAL_E)
    assert c.ref().n == 4 * 130 * (257 - E.SKIP_E)
    check("E", "n_global = 4 n", c, call(c, 3))


def test_e_esr_zero_gives_the_mse_part():
    """target = the y of a first call: e = 0 on every row, S = 0, esr = 0 -- no division by it: g is finite and equals ga gP with
    ga = 2 / n (the MSE part; gP is exactly 0 here), loss3 = 0"""
    c = E.case(2, 2, 130, 257, E.SKIP_E)
    first = call(c, 3)
    res = call(c, 3, target=first["y"])
    sums, g, l3 = (res[k].cpu().numpy() for k in ("sums", "g", "loss3"))
    assert torch.equal(res["y"].view(torch.int32), first["y"].view(torch.int32))
    assert sums[0] == 0.0 and sums[1] > 0 and np.all(np.isfinite(g)) and np.all(np.isfinite(l3))
    P = c.n_params
    assert np.all(sums[2:2 + P] == 0) and np.array_equal(g, (2.0 / c.ref().n * sums[2:2 + P].astype(np.float64)).astype(np.float32))
    assert np.all(l3 == 0) and np.any(sums[2 + P:] != 0)


@pytest.mark.parametrize("B", [65, 130], ids=["one-B65", "two-B130"])
def test_e_skipped_rows_of_the_target_count_for_nothing_whatever_they_hold(B):
    """NaN and Inf in the rows of target before skip (padding): the composed path slices those rows away, and the step gives the
    bits it gives on a clean target -- skip = 203 sits inside an 8-step block, inside a 32-step window, inside the last chunk"""
    c = E.case(2, 2, 130, 257, 203) if B == 130 else E.case(2, 2, 65, 100, 75)
    k = 3 if B == 130 else 4
    clean = call(c, k, want_zT=True)
    bad = c.target.copy()
    bad[:c.skip:2], bad[1:c.skip:2] = np.nan, np.inf
    res = call(c, k, want_zT=True, target=cuda(bad))
    for key in ("y", "sums", "g", "loss3", "gcoef", "zT"):
        assert torch.equal(res[key].view(torch.int32), clean[key].view(torch.int32)), key
    assert np.all(np.isfinite(res["sums"].cpu().numpy()))


def test_e_without_g_only_sums_is_written():
    c = E.case(2, 2, 130, 257, E.SKIP_E)
    res = call(c, 3, finish=False)
    assert res["g"] is None and res["loss3"] is None
    check("E", "g == NULL", c, res)
    full = call(c, 3)
    assert torch.equal(res["sums"].view(torch.int32), full["sums"].view(torch.int32))


def test_e_two_half_batches_and_the_finish_launch():
    """B = 130 as 65 + 65 (one sequence per lane each; the whole batch runs two per lane), each with n_global of the whole: the sums
    added in float and handed to ss_lin_esr_finish against the whole batch's own g and loss3.  Rounding of the float sums (2^-24
    each: two halves and their sum) through the fp64 formulas: |ga| 2^-24 (|gP_1| + |gP_2| + |gP|) and the same for gQ, ga's second
    term and gb moved by S and E (3 x 2^-24 each: d ln ga_2 <= 3 x 2^-24, d ln gb <= 6 x 2^-24), one rounding of each g."""
    from wdf_hip import binding as wb
    c = E.case(2, 2, 130, 257, E.SKIP_E)
    whole = call(c, 3)
    n, P, u = c.ref().n, c.n_params, 2.0 ** -24
    halves = []
    for lo in (0, 65):
        h = object.__new__(E.Case)
        h.__dict__.update(c.__dict__)
        h.B, h.x, h.target, h.z0 = 65, c.x[:, :, lo:lo + 65], c.target[:, lo:lo + 65], None
        halves.append(call(h, 3, finish=False, n_global=n)["sums"])
    total = halves[0] + halves[1]
    g, l3 = wb.ss_lin_esr_finish(total, n)
    h1, h2, tt = (t.cpu().numpy().astype(np.float64) for t in (halves[0], halves[1], total))
    r, _, _ = g_from_sums(tt, P, n)
    a2 = 1.0 / (r.esr * (r.E + E.EPS) * r.n)
    gw = whole["g"].cpu().numpy().astype(np.float64)
    absP, absQ = (np.abs(h1[s]) + np.abs(h2[s]) + np.abs(tt[s]) for s in (slice(2, 2 + P), slice(2 + P, None)))
    bound = u * (abs(r.ga) * absP + abs(r.gb) * absQ + 3 * np.abs(a2 * tt[2:2 + P]) + 6 * np.abs(r.gb * tt[2 + P:]) + 2 * np.abs(gw))
    fg = ratio(np.abs(g.cpu().numpy().astype(np.float64) - gw), bound)
    lw = whole["loss3"].cpu().numpy().astype(np.float64)
    fl = ratio(np.abs(l3.cpu().numpy().astype(np.float64) - lw), 5 * u * np.abs(lw))      # (S: 3 roundings; esr: S and E halved; the result's own two)
    print(f"FIG E | halves + finish | g={fg:.3f} loss3={fl:.3f}")
    assert fg <= 1.0 and fl <= 1.0
    assert np.abs(tt[:2] - whole["sums"].cpu().numpy()[:2].astype(np.float64)).max() <= 3 * u * tt[:2].max()


FINISH_GP = [0.5, -1.25, 2.0, 0.03125, -3.0, 0.75]
FINISH_GQ = [1.5, -0.75, 0.25, 0.5, 0.125, -2.5]


@pytest.mark.parametrize("S", [3.5, 0.0], ids=["S3.5", "S0"])
@pytest.mark.parametrize("P", [4, 6], ids=["clipper-4", "asym-6"])
def test_e_the_three_finish_exports_are_one_kernel(P, S):
    """{S, E, gP[P], gQ[P]} through the family's own finish export (wdf_esr_finish: 4 entries, wdf_asym_esr_finish: 6) and through
    wdf_ss_lin_esr_finish with n_params = P: g and loss3 BIT FOR BIT (one kernel, csrc/wdf_esr.h), and both within one fp32 ulp of
    dist.esr_coefficients in float64 (the device rounds an fp64 result once; no term of g cancels here: |gb gQ| < |ga gP| / 3).
    S = 0: esr = 0 contributes 0 to ga -- g = 2/n gP exactly, loss3 = 0, nothing NaN."""
    from wdf_hip import binding as wb, dist
    n, eps = 1000.0, wb.ESR_EPS
    sums = np.array([S, 120.25] + FINISH_GP[:P] + FINISH_GQ[:P], dtype=np.float32)
    own = wb.esr_finish if P == 4 else wb.asym_esr_finish
    g1, l1 = own(cuda(sums), n, eps)
    g2, l2 = wb.ss_lin_esr_finish(cuda(sums), n, eps)
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)) and torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    s64 = sums.astype(np.float64)
    ga, gb, mse, esr = dist.esr_coefficients(s64[0], s64[1], n, eps)
    g_ref, l_ref = ga * s64[2:2 + P] + gb * s64[2 + P:], np.array([mse, esr, mse + esr])
    g, l3 = g2.cpu().numpy().astype(np.float64), l2.cpu().numpy().astype(np.float64)
    fg, fl = ratio(np.abs(g - g_ref), ulp32(g_ref)), ratio(np.abs(l3 - l_ref), ulp32(l_ref))
    print(f"FIG E | one finish kernel P={P} S={S} | g={fg:.3f} loss3={fl:.3f}")
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(l3)) and fg <= 1.0 and fl <= 1.0
    if S == 0.0:
        assert np.all(l3 == 0) and np.array_equal(g2.cpu().numpy(), (2.0 / n * s64[2:2 + P]).astype(np.float32))


@pytest.mark.parametrize("B,T,k", E.SHAPES_B, ids=["one-B65", "two-B130"])
@pytest.mark.parametrize("ns,ni", E.TREES_B, ids=[f"ns{a}-ni{b}" for a, b in E.TREES_B])
def test_e_the_mse_steps_sums_at_skip_zero(ns, ni, B, T, k):
    """S and GP at skip = 0 are ss_lin_step_mse's SSE and gcoef at gscale = 1 BIT FOR BIT: the same weights (e x 1), the same
    fused multiply-adds in the same order, the same chunks, partial sums and wave order"""
    from wdf_hip import binding as wb
    c = E.case(ns, ni, B, T, 0)
    res = call(c, k)
    mse = wb.ss_lin_step_mse(cuda(c.x), cuda(c.coef), cuda(c.jac, np.float64), cuda(c.target), 1.0, k, want_gcoef=True)
    kG = R.kg(ns, ni)
    assert torch.equal(res["sums"][:1].view(torch.int32), mse["out"][:1].view(torch.int32))
    assert torch.equal(res["gcoef"][:kG].view(torch.int32), mse["gcoef"].view(torch.int32))
    assert torch.equal(res["y"].view(torch.int32), mse["y"].view(torch.int32))


def test_e_wrapper_refuses_what_does_not_fit():
    from wdf_hip import binding as wb
    c = E.case(1, 1, 65, 100, 7)
    x, coef, tgt, jac = cuda(c.x), cuda(c.coef), cuda(c.target), cuda(c.jac, np.float64)
    good = dict(x_tm=x, coef=coef, jac=jac, target=tgt, skip=7, n_chunks=4)
    for over in (dict(skip=-1), dict(skip=100), dict(n_global=0.0), dict(eps=-1.0), dict(coef=coef[:7]), dict(jac=jac.float()),
                 dict(target=tgt[:99]), dict(z0=cuda(np.zeros((2, 65)))), dict(y=cuda(np.zeros((100, 64)))), dict(n_chunks=0),
                 dict(ws=torch.zeros(16, dtype=torch.uint8, device="cuda")),
                 dict(ws=torch.zeros(wb.lib().wdf_ss_lin_step_ws_bytes(1, 1, 65, 100, 4), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(wb.WdfHipError):
            wb.ss_lin_step_esr(**{**good, **over})
    res = wb.ss_lin_step_esr(**good)
    assert tuple(res["y"].shape) == (100, 65) and res["gcoef"] is None and res["zT"] is None and res["sums"].numel() == 2 + 2 * 3
    for bad in (torch.zeros(5, device="cuda"), torch.zeros(34, device="cuda")):
        with pytest.raises(wb.WdfHipError):
            wb.ss_lin_esr_finish(bad, 10.0)
    with pytest.raises(wb.WdfHipError):
        wb.ss_lin_esr_finish(res["sums"], 0.0)
