"""GPU: the linear one-pass step (csrc/wdf_ss_step.h: wdf_ss_lin_step_mse) and its device probe (ss_probe_kernel) at kernel level,
through binding.ss_lin_step_mse and binding.ss_probe -- where tests/test_gpu_ss_step.py, which reaches them through
Circuit.to_device() + Circuit.mse(), does not take them:

  A  every instantiation: ns in {0,1,2} x ni in {1,2} x {one, two sequences per lane}, single chunk, dead lanes, a last chunk of
     four steps / of one step, a second wave with one live lane; even B dropping to one per lane when a pointer is 4 mod 8;
  B  chunk geometry that is not the planner's: one chunk, a last chunk of one step, K different from the count asked for, five
     chunks of 224, 64 chunks (the longest walk; 128 partials for the finishing wave);
  C  the carried state z0 / zT with one and two capacitors, both lane widths: from a random z0, a second call from the first's
     zT, zT without z0, ns = 0;
  D  poles the planner's trees never show: 0.9995, negative, complex, fast -- `slow` over 2048 steps in 1, 8 and 64 chunks;
  E  the finishing wave: 1, 2 and 15 parameters, the same bits from two calls on one workspace, the ticket left 0, gscale = 0;
  F  the probe: tapes of 1, 128 (exactly the prefetch), 129 and 384 operations, 1 and 15 tangent lanes, outputs past lane 64, and
     up to 8 folded Adam jobs of 1, 9 and 20 parameters with clipping.

Reference, everywhere: tests/ss_lin_ref.py -- the recursion restated directly in float64 (run), the tape evaluated in float64 with
a magnitude pass (evaluate_mag); pinned on the CPU by tests/test_ss_lin_ref_cpu.py.  No other path of this library is compared with.

Bounds (none taken from what the kernel gives):
  y            3e-6 max(1, max |y_ref|)       tests/test_gpu_ss_step.py's row for this arithmetic; 8 x the fp32 restatement's cap
  SSE, loss    1e-5 relative                  the same file
  zT           3e-6 max(1, max |z_ref|)       the same file
  gcoef[i]     4e-6 mag_i                     mag_i = sum |g| |addend|.  The fp32 restatement stays within 2e-7 mag_i of the fp64 one
                                              (asserted on the CPU over these very cases); 8 x that = 1.6e-6 allows for fused against
                                              separate roundings and one affine map per chunk boundary; the kernel adds 32 addends in
                                              fp32 before it goes to double, at most 32 x 2^-24 = 1.9e-6; together 3.5e-6, rounded up
  out[1 + p]   sum_i 4e-6 mag_i |jac[row_i, p]| + one fp32 ulp of the value     (the contraction is in fp64)
  probe        64 n_ops 2^-53 (vmag, tmag)    a few roundings of the magnitudes per operation; the fp64 host evaluation stays within
                                              a quarter of it of the extended-precision one (CPU file)
  Adam state   2e-5                           tests/test_gpu_pretraining.py's bound for wdf_adam_step
A relative bound on a gradient entry would mean nothing (|g_i| / mag_i goes down to 0.001): entries are judged against mag_i only.

Every check prints `FIG <section> | <case> | y=... sse=... g=...` before it asserts, each error divided by its bound (run with -s).

Measured on an MI355X (worst figure of each section, error / bound; 164 tests, 226 FIG lines, all passing, 5 s in all):
  A  y 0.049  sse 0.017  loss 0.020  out 0.047  g 0.098 ((2,2) B = 1, T = 40: 40 addends, nothing averages out)  zT 0.049
  B  y 0.043  sse 0.008  loss 0.006  out 0.010  g 0.047 ((2,1) B = 65, T = 2048 in 64 chunks)
  C  y 0.049  sse 0.004  loss 0.004  out 0.003  g 0.006  zT 0.042 (the second call, from the first's zT)
  D  y 0.072 ((1,1) slow B = 130, one chunk)  sse 0.005  loss 0.005  out 0.045  g 0.050 ((1,1) slow in 8 chunks; 64 chunks: less)
  E  y 0.049  sse 0.004  loss 0.003  out 0.002  g 0.003; the same bits on a reused workspace, the ticket 0, gscale = 0 exactly 0
  F  coef64 < 1e-4  jac 1e-4 (384 operations, 15 lanes, 100 outputs)  Adam theta 0.007  m 0.006  v 0.001 of 2e-5; the fused launch
     bit for bit what adam_step_multi followed by ss_probe gives
No case came near its bound and no wrong number was found: nothing under csrc/ changed.  That the module is not blind at these
margins: against two deliberately wrong builds of the library it fails 83 of its 164 tests (lin_walk_to without the G_c z term:
every case of more than one chunk with a state) and 128 (dead lanes counted in the sums: every case with a dead lane).
"""
import gc

import numpy as np
import pytest

import ss_lin_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B_Y, B_SSE, B_G = 3e-6, 1e-5, 4e-6


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """(as tests/test_gpu_ss_nl_step_edges.py does: tests/test_gpu_cache_identity.py relies on the caching allocator handing a freed
    block straight back)"""
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


def jac_of(c, n_params):
    ns, ni, B, T = c.key[0], c.key[1], c.B, c.T
    return np.random.default_rng([ns, ni, B, T, n_params]).standard_normal((R.ncoef(ns, ni) + 1, n_params))


def call(c, n_chunks, n_params=3, want_gcoef=True, want_zT=False, z0="case", gscale=None, x=None, target=None, y=None, ws=None):
    """one launch of the step on case c -> the binding's dict and the jac it ran with (numpy)"""
    from wdf_hip import binding as wb
    jac = jac_of(c, n_params)
    z0 = (None if c.z0 is None else cuda(c.z0)) if isinstance(z0, str) else z0
    res = wb.ss_lin_step_mse(cuda(c.x) if x is None else x, cuda(c.coef), cuda(jac, np.float64), cuda(c.target) if target is None else target,
                             c.gscale if gscale is None else gscale, n_chunks, z0=z0, want_zT=want_zT, want_gcoef=want_gcoef, ws=ws, y=y)
    return res, jac


def ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0


def check(section, label, c, res, jac, ref=None, gscale=None):
    """every output of one call against the reference; prints the figures (error / bound), then asserts"""
    ref = c.ref() if ref is None else ref
    ns, ni = c.ns, c.ni
    gs = float(np.float32(c.gscale if gscale is None else gscale))
    y = res["y"].cpu().numpy().astype(np.float64)
    out = res["out"].cpu().numpy()
    f = {"y": ratio(np.max(np.abs(y - ref.y)), B_Y * max(1.0, np.max(np.abs(ref.y)))),
         "sse": ratio(abs(float(out[0]) - ref.sse), B_SSE * ref.sse),
         "loss": ratio(abs(float(res["loss"].cpu()) - 0.5 * gs * ref.sse), B_SSE * 0.5 * gs * ref.sse if gs else 0.0)}
    rows = R.rows(ns, ni)
    want = ref.g @ jac[rows]
    bound = (B_G * ref.mag) @ np.abs(jac[rows]) + np.where(want != 0, np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), 0.0)
    f["out"] = ratio(np.abs(out[1:].astype(np.float64) - want), bound)
    if res["gcoef"] is not None:
        f["g"] = ratio(np.abs(res["gcoef"].cpu().numpy().astype(np.float64) - ref.g), B_G * ref.mag)
    if res["zT"] is not None:
        f["zT"] = ratio(np.max(np.abs(res["zT"].cpu().numpy().astype(np.float64) - ref.zT)), B_Y * max(1.0, np.max(np.abs(ref.zT))))
    print(f"FIG {section} | {label} {c} | " + " ".join(f"{k}={v:.3f}" for k, v in f.items()))
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(out))
    assert all(v <= 1.0 for v in f.values()), (section, label, repr(c), f)
    return f


def lanes(B):
    return "two" if B % 2 == 0 else "one"


# ---- A: every instantiation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,k", R.SHAPES_A, ids=[f"{lanes(B)}-B{B}-T{T}-k{k}" for B, T, k in R.SHAPES_A])
@pytest.mark.parametrize("ns,ni", R.TREES, ids=[f"ns{a}-ni{b}" for a, b in R.TREES])
def test_a_every_instantiation(ns, ni, B, T, k):
    c = R.case(ns, ni, "plain", B, T)
    res, jac = call(c, k, want_zT=True)
    assert (res["zT"] is None) == (ns == 0)
    check("A", f"{lanes(B)} per lane k={k}", c, res, jac)


@pytest.mark.parametrize("what", ["x_target_y", "z0"])
@pytest.mark.parametrize("ns,ni", R.MISALIGNED_A, ids=[f"ns{a}-ni{b}" for a, b in R.MISALIGNED_A])
def test_a_even_batch_drops_to_one_per_lane_when_a_pointer_is_4_mod_8(ns, ni, what):
    """B = 64, aligned, runs two per lane (one wave of 32 live lanes); with x, target and y one float into their storage -- or
    with only z0 there -- 8-byte loads would be misaligned: the host has to pick the one-per-lane kernels"""
    if what == "z0":
        c = R.case(ns, ni, "plain", 64, 100, True)
        res, jac = call(c, 4, want_zT=True, z0=one_float_in(c.z0))
    else:
        c = R.case(ns, ni, "plain", 64, 100)
        y = one_float_in(np.zeros((c.T, c.B)))
        res, jac = call(c, 4, want_zT=True, x=one_float_in(c.x), target=one_float_in(c.target), y=y)
        assert res["y"].data_ptr() == y.data_ptr()
    check("A", f"4 mod 8: {what}", c, res, jac)


# ---- B: chunk geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,k", R.GEOM_B, ids=[f"T{T}-k{k}" for T, k in R.GEOM_B])
@pytest.mark.parametrize("B", R.BATCHES, ids=["one-B65", "two-B130"])
@pytest.mark.parametrize("ns,ni", R.TREES_B, ids=[f"ns{a}-ni{b}" for a, b in R.TREES_B])
def test_b_chunk_geometry(ns, ni, B, T, k):
    from wdf_hip import binding as wb
    c = R.case(ns, ni, "plain", B, T)
    res, jac = call(c, k)
    L, K = wb.chunk_geom(T, k, 32)
    assert res["ws"].numel() == wb.lib().wdf_ss_lin_step_ws_bytes(ns, ni, B, T, K)        # (sized by the chunks it runs with)
    check("B", f"L={L} K={K} (asked {k})", c, res, jac)


# ---- C: carried state --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", R.BATCHES, ids=["one-B65", "two-B130"])
@pytest.mark.parametrize("ns,ni", R.TREES_C, ids=[f"ns{a}-ni{b}" for a, b in R.TREES_C])
def test_c_two_calls_with_the_state_handed_over(ns, ni, B):
    """from a random z0 (|z0| ~ 1): y, gradients and zT of the first call; z0 untouched; a second call from the first's zT is the
    second half of the reference's run over the 2 T inputs -- y, zT, and the second half's gradient with the hand-over a constant"""
    whole, first, second = R.carried(ns, ni, B)
    z0 = cuda(first.z0)
    before = z0.clone()
    res1, jac1 = call(first, 3, want_zT=True, z0=z0)
    check("C", "first half", first, res1, jac1)
    assert torch.equal(z0.view(torch.int32), before.view(torch.int32))
    assert res1["zT"].data_ptr() != z0.data_ptr()
    res2, jac2 = call(second, 3, want_zT=True, z0=res1["zT"])
    check("C", "second half from the first's zT", second, res2, jac2)
    both = np.concatenate([res1["y"].cpu().numpy(), res2["y"].cpu().numpy()]).astype(np.float64)
    wref = whole.ref()
    assert np.max(np.abs(both - wref.y)) <= B_Y * max(1.0, np.max(np.abs(wref.y)))
    assert np.max(np.abs(res2["zT"].cpu().numpy() - wref.zT)) <= B_Y * max(1.0, np.max(np.abs(wref.zT)))


@pytest.mark.parametrize("B", R.BATCHES, ids=["one-B65", "two-B130"])
@pytest.mark.parametrize("ns,ni", R.TREES_C, ids=[f"ns{a}-ni{b}" for a, b in R.TREES_C])
def test_c_final_state_without_an_initial_one(ns, ni, B):
    c = R.case(ns, ni, "plain", B, 257)
    res, jac = call(c, 3, want_zT=True)
    assert res["zT"] is not None and tuple(res["zT"].shape) == (ns, B)
    check("C", "zT without z0", c, res, jac)


def test_c_no_state_ignores_z0_and_zT():
    c = R.case(0, 1, "plain", 65, 257)
    res, jac = call(c, 3, want_zT=True, z0=cuda(np.ones((1, 65))))
    assert res["zT"] is None
    check("C", "ns = 0 with z0", c, res, jac)


# ---- D: poles ----------------------------------------------------------------------------------------------------------------
CASES_D = [(ns, ni, fam) for ns, ni in R.TREES_D for fam in R.families(ns)]


@pytest.mark.parametrize("B", R.BATCHES, ids=["one-B65", "two-B130"])
@pytest.mark.parametrize("ns,ni,fam", CASES_D, ids=[f"ns{a}-ni{b}-{f}" for a, b, f in CASES_D])
def test_d_poles(ns, ni, fam, B):
    """`slow` (0.9995: the memory outlasts every chunk, Phi = {A^L, G_c} carries all of it) over 2048 steps in 1, 8 and 64 chunks:
    the walk's fp32 A^L and G_c from L = 2048 / 256 / 32 repeated steps"""
    if fam == "slow":
        c = R.case(ns, ni, fam, B, 2048)
        for k in R.SLOW_CHUNKS:
            res, jac = call(c, k)
            check("D", f"k={k}", c, res, jac)
    else:
        c = R.case(ns, ni, fam, B, 200)
        res, jac = call(c, 4)
        check("D", "k=4", c, res, jac)


# ---- E: reduction and chain rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_params", R.PARAMS_E)
def test_e_parameter_counts_and_a_reused_workspace(n_params):
    """two calls on one workspace give the same bits; the ticket (the workspace's first word) is 0 after each; a third call on the
    workspace, zeroed only once, still matches the reference"""
    c = R.case(2, 2, "plain", 130, 257)
    res, jac = call(c, 3, n_params=n_params)
    check("E", f"n_params={n_params} call 1", c, res, jac)
    ws = res["ws"]
    assert int(ws[:4].view(torch.int32)[0]) == 0
    keep = {k: res[k].clone() for k in ("y", "out", "loss", "gcoef")}
    for n in (2, 3):
        res, _ = call(c, 3, n_params=n_params, ws=ws)
        assert res["ws"].data_ptr() == ws.data_ptr() and int(ws[:4].view(torch.int32)[0]) == 0
        for k, v in keep.items():
            assert torch.equal(res[k].view(torch.int32), v.view(torch.int32)), (k, n)
    check("E", f"n_params={n_params} call 3", c, res, jac)


@pytest.mark.parametrize("B", [129, 130], ids=["one-B129", "two-B130"])
def test_e_gscale_zero(B):
    """gradients exactly 0 (every bound is 0 x mag), the SSE still right"""
    c = R.case(2, 2, "plain", B, 257)
    ref = R.run(2, 2, c.coef, c.x, c.target, 0.0)
    assert np.all(ref.g == 0) and np.all(ref.mag == 0) and ref.sse == c.ref().sse
    res, jac = call(c, 3, gscale=0.0)
    check("E", "gscale=0", c, res, jac, ref=ref, gscale=0.0)
    assert np.all(res["out"].cpu().numpy()[1:] == 0) and np.all(res["gcoef"].cpu().numpy() == 0) and float(res["loss"].cpu()) == 0.0


def test_e_wrapper_refuses_shapes_that_do_not_fit():
    from wdf_hip import binding as wb
    c = R.case(1, 1, "plain", 65, 100)
    x, coef, tgt = cuda(c.x), cuda(c.coef), cuda(c.target)
    jac = cuda(jac_of(c, 3), np.float64)
    good = dict(x_tm=x, coef=coef, jac=jac, target=tgt, gscale=c.gscale, n_chunks=4)
    for over in (dict(coef=coef[:7]), dict(coef=cuda(np.zeros(10))), dict(jac=jac[:5].contiguous()), dict(jac=cuda(np.zeros((9, 16)), np.float64)),
                 dict(jac=jac.float()), dict(target=tgt[:99]), dict(target=cuda(np.zeros((65, 100)))), dict(z0=cuda(np.zeros((2, 65)))),
                 dict(z0=cuda(np.zeros((1, 64)))), dict(y=cuda(np.zeros((100, 64)))), dict(x_tm=x[:, 0]), dict(x_tm=cuda(np.zeros((100, 3, 65)))),
                 dict(ws=torch.zeros(16, dtype=torch.uint8, device="cuda")), dict(n_chunks=0)):
        with pytest.raises(wb.WdfHipError):
            wb.ss_lin_step_mse(**{**good, **over})
    res = wb.ss_lin_step_mse(**good)                              # (... and the arguments they were derived from are fine)
    assert tuple(res["y"].shape) == (100, 65) and res["gcoef"] is None and res["zT"] is None


# ---- F: the probe ------------------------------------------------------------------------------------------------------------
def probe_bound(n_ops):
    return 64 * n_ops * 2.0 ** -53


def check_probe(label, ops, consts, params64, outs, got):
    coef, coef64, jac = (t.cpu().numpy() for t in got)
    val, tan, vm, tm = R.evaluate_mag(ops, consts, params64, outs)
    f_v, f_j = ratio(np.abs(coef64 - val), probe_bound(len(ops)) * vm), ratio(np.abs(jac - tan), probe_bound(len(ops)) * tm)
    print(f"FIG F | {label} | coef64={f_v:.4f} jac={f_j:.4f}")
    assert coef.dtype == np.float32 and np.array_equal(coef.view(np.int32), coef64.astype(np.float32).view(np.int32))
    assert f_v <= 1.0 and f_j <= 1.0, (label, f_v, f_j)
    assert np.any(tan != 0) or len(ops) == 1 or len(params64) == 1


CASES_F = [(n, P, o) for n in (1, 128, 129, 384) for P in (1, 15) for o in ((1,) if n == 1 else (1, 64, 65, 100))]


@pytest.mark.parametrize("n_ops,P,n_out", CASES_F, ids=[f"ops{n}-P{P}-out{o}" for n, P, o in CASES_F])
def test_f_probe_tapes(n_ops, P, n_out):
    """128 operations are exactly what the prefetch holds in registers (6 words x 64 lanes), 129 take `the rest the plain way`;
    outputs past lane 64 are read from memory by the lane that writes them; outputs may repeat"""
    from wdf_hip import binding as wb
    ops, consts, params = R.random_tape(n_ops, P, seed=0)
    outs = np.random.default_rng([n_ops, P, n_out]).integers(0, n_ops, n_out)
    if n_out > 1:
        outs[-1] = n_ops - 1
    got = wb.ss_probe(ops, consts, cuda(params), outs)
    assert tuple(got[2].shape) == (n_out, P)
    check_probe(f"ops={n_ops} P={P} n_out={n_out}", ops, consts, params.astype(np.float64), outs, got)


JOBS_F = [("1x1", [1]), ("1x9", [9]), ("1x20", [20]), ("8", [1, 9, 20, 1, 20, 1, 20, 1])]


class AdamRef:
    """the fp64 restatement of the Adam rule tests/test_gpu_pretraining.py uses for wdf_adam_step, from fp32 inputs"""

    def __init__(self, theta, lr, lo, hi, b1, b2, eps):
        self.th = np.asarray(theta, np.float32).astype(np.float64)
        self.lr, self.lo, self.hi = np.asarray(lr, np.float32).astype(np.float64), lo, hi
        self.b1, self.b2, self.eps = float(np.float32(b1)), float(np.float32(b2)), float(np.float32(eps))
        self.m, self.v, self.t = np.zeros_like(self.th), np.zeros_like(self.th), 0

    def step(self, g):
        g = np.asarray(g, np.float32).astype(np.float64)
        self.t += 1
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        th = self.th - self.lr * np.sqrt(1 - self.b2 ** self.t) / (1 - self.b1 ** self.t) * self.m / (np.sqrt(self.v) + self.eps)
        self.th = np.clip(th, -np.inf if self.lo is None else self.lo, np.inf if self.hi is None else self.hi)


@pytest.mark.parametrize("name,sizes", JOBS_F, ids=[j[0] for j in JOBS_F])
def test_f_probe_behind_adam_jobs(name, sizes):
    """three consecutive launches of wdf_ss_probe_adam: jobs of 1, 9 and 20 parameters (the 8-lane loop runs 1, 2 and 3 times), those
    of at most 15 on slices of the parameter block itself, the 20s on arrays of their own; every other job clipped to +-0.005 around
    its start (less than one step: the learning rates are 0.01 and up), so that lo / hi bind.  After each launch: theta, m, v against the fp64 rule, every step counter up by one, the probe's
    outputs those of the tape at the UPDATED block, and everything bit for bit what adam_step_multi followed by ss_probe gives on
    copies."""
    from wdf_hip import binding as wb
    P, n_ops, n_out = 15, 129, 65
    ops, consts, p0 = R.random_tape(n_ops, P, seed=1)
    outs = np.random.default_rng(len(sizes)).integers(0, n_ops, n_out)
    rng = np.random.default_rng([7, len(sizes), sizes[0]])

    def build():
        """the block, the jobs [(Adam, theta, grad buffer)] on it and their references -- the same every time it is called"""
        r = np.random.default_rng([11, len(sizes), sizes[0]])
        block = cuda(p0)
        jobs, refs, off = [], [], 0
        for j, n in enumerate(sizes):
            if n <= P:
                theta, off = block[off:off + n], off + n
            else:
                theta = cuda(r.uniform(0.7, 1.3, n))
            start = theta.cpu().numpy()
            lr = r.uniform(0.01, 0.05, n).astype(np.float32)
            lo, hi = ((start - 0.005).astype(np.float32), (start + 0.005).astype(np.float32)) if j % 2 == 0 else (None, None)
            b1, b2, eps = (0.5, 0.999, 1e-7) if j % 3 == 0 else (0.9, 0.99, 1e-6)
            opt = wb.Adam(n, lr, beta_1=b1, beta_2=b2, epsilon=eps, lo=lo, hi=hi)
            jobs.append((opt, theta, torch.zeros(n, dtype=torch.float32, device="cuda")))
            refs.append(AdamRef(start, lr, lo, hi, b1, b2, eps))
        assert off <= P
        return block, jobs, refs

    block, jobs, refs = build()
    block2, jobs2, _ = build()
    clipped = False
    for launch in range(3):
        grads = [rng.standard_normal(n).astype(np.float32) * (1.0 + launch) for n in sizes]
        for (_, _, gbuf), (_, _, gbuf2), g in zip(jobs, jobs2, grads):
            gbuf.copy_(torch.as_tensor(g))
            gbuf2.copy_(torch.as_tensor(g))
        got = wb.ss_probe(ops, consts, block, outs, jobs=jobs)
        wb.adam_step_multi(jobs2)
        want = wb.ss_probe(ops, consts, block2, outs)
        for (opt, theta, _), ref, g in zip(jobs, refs, grads):
            ref.step(g)
            assert int(opt.step.cpu()[0]) == launch + 1
            e = [float(np.max(np.abs(t.cpu().numpy() - r))) for t, r in ((theta, ref.th), (opt.m, ref.m), (opt.v, ref.v))]
            print(f"FIG F | jobs {name} launch {launch} n={opt.n} | theta={e[0] / 2e-5:.4f} m={e[1] / 2e-5:.4f} v={e[2] / 2e-5:.4f}")
            assert max(e) < 2e-5, (name, launch, opt.n, e)
            if ref.lo is not None:
                clipped |= bool(np.any(ref.th == ref.lo) or np.any(ref.th == ref.hi))
        check_probe(f"jobs {name} launch {launch}", ops, consts, block.cpu().numpy().astype(np.float64), outs, got)
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(block.view(torch.int32), block2.view(torch.int32))
        for (opt, theta, _), (opt2, theta2, _) in zip(jobs, jobs2):
            for a, b in ((theta, theta2), (opt.m, opt2.m), (opt.v, opt2.v), (opt.step, opt2.step)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, launch, opt.n)
    assert clipped
    assert min(sizes) > P or not np.array_equal(block.cpu().numpy(), p0)      # (the jobs on the block moved it)


def test_f_wrapper_refuses_before_any_launch():
    from wdf_hip import binding as wb
    params = cuda(np.ones(2))
    with pytest.raises(wb.WdfHipError):
        wb.ss_probe([[R.OP_PARAM, 0, 0], [R.OP_NEG, 2, 0], [R.OP_PARAM, 1, 0]], [], params, [1])      # names a later operation
    with pytest.raises(wb.WdfHipError):
        wb.ss_probe([[R.OP_PARAM, 2, 0]], [], params, [0])                                            # a parameter outside the block
    with pytest.raises(wb.WdfHipError):
        wb.ss_probe([[R.OP_PARAM, 0, 0]], [], params, [1])                                            # an output outside the tape
    with pytest.raises(wb.WdfHipError):
        wb.ss_probe([[R.OP_PARAM, 0, 0]], [], params.double(), [0])
    coef, coef64, jac = wb.ss_probe([[R.OP_PARAM, 1, 0]], [], params, [0])
    assert float(coef64.cpu()[0]) == 1.0 and jac.cpu().numpy().tolist() == [[0.0, 1.0]]
