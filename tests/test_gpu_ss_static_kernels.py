"""GPU: the static state-space kernels (csrc/wdf_statespace.h) at kernel level, through wdf_hip.binding only -- ss_fwd / ss_bwd,
ss_fwd_lin_tp, ss_fwd_tp, ss_bwd_tp on RAW coefficient vectors, every size they are built for -- where the rest of the suite reaches
them through Circuit (physical trees, gradients seen only after the chain rule) or at ns = ni = 1:

  A  every sequential instantiation: ns 0..4 x ni 1,2 x root {none, pair 1U-1D, pair 2U-3D, two different diodes (ns <= 3)}, from a
     random z0, at (B,T) = (65,43) ragged second wave, no 16-byte loads; (65,44) 16-byte loads; (1,1); (1,7) no full block; (130,8)
     exactly one block; (64,44) with x one float into its storage (no 16-byte loads through alignment).  y, stash, zT, gcoef, groot, gz0.
  B  ss_fwd_lin_tp: ns 1..4 x ni 1,2 at (B,T,K) = (65,131,3), (130,128,4), (1,40,1), (65,257,8) and every pole family (0.9995,
     negative, fast, a complex pair) at the last; z0 in, zT out; against the reference and within the path bound of ss_fwd.
  C  ss_bwd_tp on the stash of a sequential forward: ns 1..4 x ni 1,2 x the four roots at (65,131,3) chunks of 48, 48, 35 (the
     every-fourth-block flush, a tail of 3), (130,128,4), (65,44,2) chunks of 24 and 20, (1,9,2) a last chunk of one step,
     (65,131,16) which the binding cuts to 9 chunks of 16, and one chunk.  gcoef, groot, gz0.
  D  ss_fwd_tp under the three nonlinear roots at C's geometries: poles <= 0.5 with a warm-up of 64 (nothing gated: the speculating
     kernel's own output is judged), poles 0.9 .. 0.98 with a warm-up of 8 (every wave gated: bit for bit ss_fwd), zinit from the
     sequential stash with no warm-up (nothing gated, bit for bit ss_fwd), a zinit of the wrong shape.
  E  the carried state at ns 2..4: a run split at step 57 through zT -> z0 is bit for bit the unsplit one, ss_fwd under each root
     and ss_fwd_lin_tp.
  F  what is refused by WdfHipError before any launch.

Reference, everywhere: tests/ss_static_ref.py -- the recursion and its analytic adjoint restated directly in float64, pinned on the
CPU by tests/test_ss_static_ref_cpu.py.  Path against path only where the text above says so.

Bounds (none taken from what the kernels give; R = ss_static_ref):
  y, stash, zT       3e-6 max(1, max |ref|)         the project's row for this arithmetic (tests/test_gpu_ss_step.py, Y_REF of
                                                    tests/test_gpu_ss_dyn_chunks_state.py); the float32 mode of the reference stays
                                                    within an eighth of it on every case (CPU file)
  gcoef, groot, gz0  (8 CAP32 + n 2^-24) mag_i      linear trees.  CAP32 = 4e-7: what the float32 mode is asserted under on the CPU over
                                                    these very cases (it reaches 3.3e-7); n the float32 addends the kernel sums before
                                                    it goes to double: 8 in ss_bwd (3.7e-6), max(32, L) in the chunked sweep
  gcoef, groot, gz0  9e-6 mag_i                     nonlinear roots: the project's 3e-4 relative bound at its 0.03 balance floor; the
                                                    float32 mode stays within an eighth of it (CPU file)
  path against path  2e-6 max(1, max |ref|)         y, stash, zT where nothing was gated (Y_PATH); bit equality where stated
mag_i = sum |addend| over steps and sequences; gz0 is judged per state row against the row's largest sum |addend|.  A relative bound
on an entry would mean nothing (|g_i| / mag_i goes down to 1e-4).

Every check prints `FIG <section> | <case> | ...` before it asserts, each error divided by its bound (run with -s).

Measured on an MI355X (worst figure of each section, error / bound; 903 tests, 652 FIG lines and 396 status lines, all passing,
17 s in all, the references included):
  A  y 0.144  stash 0.114  zT 0.111 ((4,1) pair 2U-3D, B = 64, T = 44, x one float in)  linear: g 0.058  gz0 0.058
     under a root: g 0.367 ((3,1) two different diodes, B = 1, T = 1: one addend, nothing averages out)  groot 0.168  gz0 0.129
  B  y 0.066  stash 0.065  zT 0.018; against ss_fwd (of 2e-6): y 0.104  stash 0.145  zT 0.149 ((3,1) slow, five chunks)
  C  linear: g 0.058  gz0 0.033; under a root: g 0.233 ((4,1) pair 2U-3D, B = 1, T = 9, chunks of 8 and 1)  groot 0.035  gz0 0.069
  D  speculation that holds: nothing gated, no miss above tol; y 0.152 ((4,1) pair 2U-3D fast, B = 65, T = 44)  stash 0.086  zT 0.047
     speculation that misses: every wave gated, every output ss_fwd's bit for bit; zinit: max_miss exactly 0, bit for bit
  E  bit for bit under every root and in the one-chunk scan; the scan in two calls of two chunks: y 0.034  stash 0.049  zT 0.014
No case came near its bound and no wrong number was found: nothing under csrc/ changed (profiles/ss_static_kernels_digest.txt).
That the module is not blind at these margins: against five deliberately wrong builds of the library (scratch builds, never
committed) it fails
  (a) s and s2 swapped in A's index in ss_bwd_linear's adjoint update      132 tests (C: every case with two states or more)
  (b) Phi written transposed by ss_bwd_tp_kernel                            110 tests (C: two states or more, more than one chunk)
  (c) dead lanes counted in ss_bwd_tp_combine_kernel's wave sum             180 tests (C, all of it: no B there is a multiple of 64)
  (d) Bx indexed [i][s] in ss_fwd_step                                      223 tests (A .. E: two states or more with two inputs)
  (e) zwarm not stored for a last chunk shorter than a block                110 tests (D: (65,131,16) and (1,9,2), all three tests)
(a), (b) and (d) are the identity at one state: no one-state test can see them (tests/test_gpu_circuit.py's trees of two to four
capacitors fail on them: 8, 4 and 3 tests of that file and tests/test_gpu_ss_asym.py).  (e) leaves both files green.
"""
import functools
import gc

import numpy as np
import pytest

import ss_static_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """(as tests/test_gpu_ss_lin_step_kernel.py does: tests/test_gpu_cache_identity.py relies on the caching allocator handing a freed
    block straight back)"""
    yield
    dev.cache_clear()
    seq.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def one_float_in(a):
    """The array on the device as a dense view that starts one float into its storage: no 16-byte alignment."""
    a = np.asarray(a, dtype=np.float32)
    base = torch.empty((a.size + 1,), dtype=torch.float32, device="cuda")
    v = base[1:].view(*a.shape)
    v.copy_(torch.as_tensor(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return (a is None and b is None) or (a.shape == b.shape and bool(torch.equal(bits(a), bits(b))))


@functools.lru_cache(maxsize=None)
def dev(key):
    """the case's inputs on the device: x, coef, rootp | None, z0 | None, gy"""
    c = R.case(*key)
    return (cuda(c.x), cuda(c.coef), None if c.root.p is None else cuda(c.root.p), None if c.z0 is None else cuda(c.z0), cuda(c.gy))


def root_kw(c):
    return dict(root_kind=c.root.kind, n_up=c.root.n_up, n_down=c.root.n_down)


def run_seq(c, x, coef, rootp, z0):
    from wdf_hip import binding as wb
    return wb.ss_fwd(x, coef, c.ns, c.ni, rootp=rootp, want_stash=True, z0=z0, want_zT=True, **root_kw(c))


@functools.lru_cache(maxsize=None)
def seq(key):
    """ss_fwd on the case: y, stash | None, zT"""
    c = R.case(*key)
    x, coef, rootp, z0, _ = dev(key)
    return run_seq(c, x, coef, rootp, z0)


def np64(t):
    return t.cpu().numpy().astype(np.float64)


def fig_fwd(c, y, zs, zT, ref=None, bound=R.Y_REF):
    ref = c.fwd() if ref is None else ref
    f = {"y": R.ratio(np.max(np.abs(np64(y) - ref.y)), bound * max(1.0, np.max(np.abs(ref.y))))}
    assert np.all(np.isfinite(np64(y)))
    if c.ns:
        f["stash"] = R.ratio(np.max(np.abs(np64(zs) - ref.zs)), bound * max(1.0, np.max(np.abs(ref.zs))))
        f["zT"] = R.ratio(np.max(np.abs(np64(zT) - ref.zT)), bound * max(1.0, np.max(np.abs(ref.zT))))
    return f


def fig_grad(c, gcoef, groot, gz0, n):
    """n: the float32 addends the kernel sums before it goes to double (linear trees' bound)"""
    ref = c.ref()
    k = R.g_lin(n) if c.linear else R.G_NL
    f = {"g": R.ratio(np.abs(np64(gcoef) - ref.g), k * ref.mag)}
    assert (groot is None) == c.linear and (gz0 is None) == (c.ns == 0)
    if groot is not None:
        assert tuple(groot.shape) == (c.root.nr,)
        f["groot"] = R.ratio(np.abs(np64(groot) - ref.groot), k * ref.groot_mag)
    if gz0 is not None:
        assert tuple(gz0.shape) == (c.ns, c.B)
        f["gz0"] = R.ratio(np.abs(np64(gz0) - ref.gz0), k * ref.gz0_row_mag[:, None])
    return f


def judge(section, label, c, f):
    print(f"FIG {section} | {label} {c} | " + " ".join(f"{k}={v:.3f}" for k, v in f.items()))
    assert all(v <= 1.0 for v in f.values()), (section, label, repr(c), f)


def tree_id(t):
    return f"ns{t[0]}-ni{t[1]}"


# ---- A: every sequential instantiation ---------------------------------------------------------------------------------------
CASES_A = [(ns, ni, root, B, T) for ns, ni in R.TREES for root in R.ROOTS if R.built(ns, root) for B, T in R.SHAPES_A]


@pytest.mark.parametrize("ns,ni,root,B,T", CASES_A, ids=[f"ns{a}-ni{b}-{r}-B{B}-T{T}" for a, b, r, B, T in CASES_A])
def test_a_every_sequential_instantiation(ns, ni, root, B, T):
    from wdf_hip import binding as wb
    key = (ns, ni, root, "plain", B, T)
    c = R.case(*key)
    x, coef, rootp, z0, gy = dev(key)
    label = "x 16-byte aligned"
    if (B, T) == (64, 44):
        x, label = one_float_in(c.x), "x one float in"
        assert (T * ni) % 4 == 0
    y, zs, zT = run_seq(c, x, coef, rootp, z0)
    assert (zs is None) == (ns == 0) and tuple(y.shape) == (T, B) and tuple(zT.shape) == (ns, B)
    gcoef, groot, gz0 = wb.ss_bwd(x, coef, ns, ni, zs, gy, rootp=rootp, want_gz0=True, **root_kw(c))
    f = fig_fwd(c, y, zs, zT)
    f.update(fig_grad(c, gcoef, groot, gz0, 8))
    judge("A", label, c, f)


# ---- B: the exact linear scan ------------------------------------------------------------------------------------------------
CASES_B = ([(ns, ni, "plain", B, T, K) for ns, ni in R.TREES1 for B, T, K in R.GEOM_B]
           + [(ns, ni, fam, 65, 257, 8) for ns, ni in R.TREES1 for fam in R.families(ns) if fam != "plain"])


@pytest.mark.parametrize("ns,ni,fam,B,T,K", CASES_B, ids=[f"ns{a}-ni{b}-{f}-B{B}-T{T}-k{K}" for a, b, f, B, T, K in CASES_B])
def test_b_linear_scan(ns, ni, fam, B, T, K):
    from wdf_hip import binding as wb
    key = (ns, ni, "none", fam, B, T)
    c = R.case(*key)
    x, coef, _, z0, _ = dev(key)
    y, zs, zT = wb.ss_fwd_lin_tp(x, coef, ns, ni, K, want_stash=True, z0=z0, want_zT=True)
    f = fig_fwd(c, y, zs, zT)
    ys, zss, zTs = seq(key)
    path = R.Result()
    path.y, path.zs, path.zT = np64(ys), np64(zss), np64(zTs)
    f.update({f"{k} path": v for k, v in fig_fwd(c, y, zs, zT, ref=path, bound=R.Y_PATH).items()})
    L, Kc = wb.chunk_geom(T, K, 32)
    judge("B", f"L={L} K={Kc}", c, f)


# ---- C: the exact chunked sweep ----------------------------------------------------------------------------------------------
CASES_C = [(ns, ni, root, B, T, K) for ns, ni in R.TREES1 for root in R.ROOTS if R.built(ns, root) for B, T, K in R.GEOM_C]


@pytest.mark.parametrize("ns,ni,root,B,T,K", CASES_C, ids=[f"ns{a}-ni{b}-{r}-B{B}-T{T}-k{K}" for a, b, r, B, T, K in CASES_C])
def test_c_chunked_sweep(ns, ni, root, B, T, K):
    from wdf_hip import binding as wb
    key = (ns, ni, root, "plain", B, T)
    c = R.case(*key)
    x, coef, rootp, _, gy = dev(key)
    _, zs, _ = seq(key)
    gcoef, groot, gz0 = wb.ss_bwd_tp(x, coef, ns, ni, zs, gy, K, rootp=rootp, want_gz0=True, **root_kw(c))
    L, Kc = wb.chunk_geom(T, K, 8)
    assert Kc == wb.lib().wdf_ss_tp_chunks(T, K)
    judge("C", f"L={L} K={Kc} (asked {K})", c, fig_grad(c, gcoef, groot, gz0, max(32, min(L, T))))


# ---- D: the speculating forward ----------------------------------------------------------------------------------------------
CASES_D = [(ns, ni, root, B, T, K) for ns, ni in R.TREES1 for root in R.NL_ROOTS if R.built(ns, root) for B, T, K in R.GEOM_C]
IDS_D = [f"ns{a}-ni{b}-{r}-B{B}-T{T}-k{K}" for a, b, r, B, T, K in CASES_D]


def run_tp(c, key, K, warmup, zinit=None):
    from wdf_hip import binding as wb
    x, coef, rootp, z0, _ = dev(key)
    y, zs, zT, st = wb.ss_fwd_tp(x, coef, c.ns, c.ni, rootp, K, warmup, want_stash=True, z0=z0, want_zT=True, zinit=zinit, **root_kw(c))
    return y, zs, zT, wb.ss_tp_status(st)


@pytest.mark.parametrize("ns,ni,root,B,T,K", CASES_D, ids=IDS_D)
def test_d_speculation_that_holds_is_judged_on_its_own_output(ns, ni, root, B, T, K):
    """poles <= 0.5 and a warm-up of 64 steps: every chunk arrives where its predecessor ended, nothing is re-run"""
    key = (ns, ni, root, "fast", B, T)
    c = R.case(*key)
    y, zs, zT, st = run_tp(c, key, K, 64)
    print(f"FIG D | fast W=64 {c} k={K} | status {st}")
    assert st["gated_waves"] == 0 and st["n_bad"] == 0, st
    judge("D", f"fast W=64 k={K}", c, fig_fwd(c, y, zs, zT))


@pytest.mark.parametrize("ns,ni,root,B,T,K", CASES_D, ids=IDS_D)
def test_d_speculation_that_misses_is_rerun_sequentially(ns, ni, root, B, T, K):
    """poles 0.9 .. 0.98 and a warm-up of 8 steps: a chunk that starts after step 8 misses on every sequence, every wave is gated
    and the outputs are ss_fwd's bit for bit.  Where no chunk starts after step 8 (one chunk; two chunks of 8 and 1) nothing is
    speculated: nothing gated, and the output answers to the reference and to ss_fwd within the path bound."""
    from wdf_hip import binding as wb
    key = (ns, ni, root, "plain", B, T)
    c = R.case(*key)
    y, zs, zT, st = run_tp(c, key, K, 8)
    ys, zss, zTs = seq(key)
    speculated = any(s > 0 for s in wb.ss_tp_starts(T, K, 8)[1:])
    print(f"FIG D | plain W=8 {c} k={K} | status {st} speculated {speculated}")
    if speculated:
        assert st["gated_waves"] == (B + 63) // 64 and st["n_bad"] > 0, st
        assert same_bits(y, ys) and same_bits(zs, zss) and same_bits(zT, zTs)
    else:
        assert st["gated_waves"] == 0 and st["n_bad"] == 0, st
        path = R.Result()
        path.y, path.zs, path.zT = np64(ys), np64(zss), np64(zTs)
        f = fig_fwd(c, y, zs, zT)
        f.update({f"{k} path": v for k, v in fig_fwd(c, y, zs, zT, ref=path, bound=R.Y_PATH).items()})
        judge("D", f"plain W=8 k={K}", c, f)


@pytest.mark.parametrize("ns,ni,root,B,T,K", CASES_D, ids=IDS_D)
def test_d_zinit_from_the_sequential_stash(ns, ni, root, B, T, K):
    """no warm-up, every chunk started from the sequential state of its first sample: nothing gated, y bit for bit ss_fwd's"""
    from wdf_hip import binding as wb
    key = (ns, ni, root, "plain", B, T)
    c = R.case(*key)
    ys, zss, zTs = seq(key)
    starts = wb.ss_tp_starts(T, K, 0)
    L, Kc = wb.chunk_geom(T, K, 8)
    assert starts == [k * L for k in range(Kc)]
    zinit = zss[torch.as_tensor(starts, device="cuda")].contiguous()
    assert tuple(zinit.shape) == (Kc, ns, B)
    y, zs, zT, st = run_tp(c, key, K, 0, zinit=zinit)
    print(f"FIG D | zinit {c} k={K} | status {st}")
    assert st["gated_waves"] == 0 and st["n_bad"] == 0 and st["max_miss"] == 0.0, st
    assert same_bits(y, ys) and same_bits(zs, zss) and same_bits(zT, zTs)


def test_d_zinit_of_the_wrong_shape_is_refused():
    from wdf_hip import binding as wb
    key = (2, 1, "pair11", "plain", 65, 131)
    c = R.case(*key)
    x, coef, rootp, z0, _ = dev(key)
    for shape in [(3, 2, 64), (2, 2, 65), (3, 1, 65), (3, 65, 2), (3 * 2 * 65,)]:
        with pytest.raises(wb.WdfHipError, match="zinit"):
            wb.ss_fwd_tp(x, coef, 2, 1, rootp, 3, 0, z0=z0, zinit=torch.zeros(shape, device="cuda"), **root_kw(c))


# ---- E: the carried state ----------------------------------------------------------------------------------------------------
TREES_E = [(ns, ni) for ns, ni in R.TREES if ns >= 2]
CASES_E = [(ns, ni, root) for ns, ni in TREES_E for root in R.ROOTS if R.built(ns, root)]


@pytest.mark.parametrize("ns,ni,root", CASES_E, ids=[f"ns{a}-ni{b}-{r}" for a, b, r in CASES_E])
def test_e_sequential_run_split_at_step_57(ns, ni, root):
    key = (ns, ni, root, "plain", 65, 131)
    c = R.case(*key)
    x, coef, rootp, z0, _ = dev(key)
    y, zs, zT = seq(key)
    y1, zs1, zT1 = run_seq(c, x[:, :R.SPLIT].contiguous(), coef, rootp, z0)
    y2, zs2, zT2 = run_seq(c, x[:, R.SPLIT:].contiguous(), coef, rootp, zT1)
    assert same_bits(zT1, zs[R.SPLIT])
    assert same_bits(torch.cat([y1, y2]), y) and same_bits(torch.cat([zs1, zs2]), zs) and same_bits(zT2, zT)


@pytest.mark.parametrize("ns,ni", TREES_E, ids=[tree_id(t) for t in TREES_E])
def test_e_linear_scan_split_at_step_57(ns, ni):
    """one chunk each (the scan's chunk starts come from A^L in double: only a single chunk walks the sequential arithmetic):
    bit for bit; three chunks against two and two: each half against the reference, from the first half's zT"""
    from wdf_hip import binding as wb
    key = (ns, ni, "none", "plain", 65, 131)
    c = R.case(*key)
    x, coef, _, z0, _ = dev(key)
    xa, xb = x[:, :R.SPLIT].contiguous(), x[:, R.SPLIT:].contiguous()
    y, zs, zT = wb.ss_fwd_lin_tp(x, coef, ns, ni, 1, z0=z0, want_zT=True)
    y1, zs1, zT1 = wb.ss_fwd_lin_tp(xa, coef, ns, ni, 1, z0=z0, want_zT=True)
    y2, zs2, zT2 = wb.ss_fwd_lin_tp(xb, coef, ns, ni, 1, z0=zT1, want_zT=True)
    assert same_bits(torch.cat([y1, y2]), y) and same_bits(torch.cat([zs1, zs2]), zs) and same_bits(zT2, zT)
    assert all(same_bits(a, b) for a, b in zip((y, zs, zT), seq(key)))
    y1, zs1, zT1 = wb.ss_fwd_lin_tp(xa, coef, ns, ni, 2, z0=z0, want_zT=True)
    y2, zs2, zT2 = wb.ss_fwd_lin_tp(xb, coef, ns, ni, 2, z0=zT1, want_zT=True)
    judge("E", "linear scan in two calls of two chunks", c, fig_fwd(c, torch.cat([y1, y2]), torch.cat([zs1, zs2]), zT2))


# ---- F: what is refused ------------------------------------------------------------------------------------------------------
def _args(ns, ni, root, B=4, T=16):
    rt = R.Root(root, 1.5e3)
    n = R.ncoef(ns, ni)
    dv = "cuda"
    return dict(x=torch.zeros((B, T, ni), device=dv), coef=torch.ones((n,), device=dv), rootp=None if rt.p is None else cuda(rt.p),
                z0=torch.zeros((ns, B), device=dv), zs=torch.zeros((T, ns, B), device=dv), gy=torch.zeros((T, B), device=dv),
                kw=dict(root_kind=rt.kind, n_up=rt.n_up, n_down=rt.n_down))


def _all_five(a, ns, ni, k=2, **over):
    """the five entry points on the arguments a (a dict of _args), each as a thunk; over: replacements"""
    from wdf_hip import binding as wb
    a = {**a, **over}
    kw, nl = a["kw"], a["kw"]["root_kind"] != 0
    calls = {"ss_fwd": lambda: wb.ss_fwd(a["x"], a["coef"], ns, ni, rootp=a["rootp"], z0=a["z0"], **kw),
             "ss_bwd": lambda: wb.ss_bwd(a["x"], a["coef"], ns, ni, a["zs"], a["gy"], rootp=a["rootp"], **kw),
             "ss_bwd_tp": lambda: wb.ss_bwd_tp(a["x"], a["coef"], ns, ni, a["zs"], a["gy"], k, rootp=a["rootp"], **kw)}
    if nl:
        calls["ss_fwd_tp"] = lambda: wb.ss_fwd_tp(a["x"], a["coef"], ns, ni, a["rootp"], k, 8, z0=a["z0"], **kw)
    else:
        calls["ss_fwd_lin_tp"] = lambda: wb.ss_fwd_lin_tp(a["x"], a["coef"], ns, ni, k, z0=a["z0"])
    return calls


def _refused(calls, match, only=None):
    from wdf_hip import binding as wb
    for name, f in calls.items():
        if only is None or name in only:
            with pytest.raises(wb.WdfHipError, match=match):
                f()


@pytest.mark.parametrize("root", ["none", "pair23"])
def test_f_sizes_the_library_is_not_built_for(root):
    _refused(_all_five(_args(5, 1, root), 5, 1), "ns in \\[0,4\\]")
    _refused(_all_five(_args(2, 3, root), 2, 3), "ni in \\[1,2\\]")


def test_f_two_different_diodes_on_four_states():
    _refused(_all_five(_args(4, 1, "asym"), 4, 1), "at most 3 states")
    _refused(_all_five(_args(4, 2, "asym"), 4, 2), "at most 3 states")


def test_f_diode_counts_and_missing_rootp():
    a = _args(2, 1, "pair23")
    for kw in (dict(a["kw"], n_up=17), dict(a["kw"], n_down=17), dict(a["kw"], n_up=0)):
        _refused(_all_five(a, 2, 1, kw=kw), "n_up/n_down")
    for root in ("pair11", "asym"):
        _refused(_all_five(_args(2, 1, root), 2, 1, rootp=None), "rootp")


def test_f_no_state_in_the_chunked_entry_points_and_no_root_to_speculate_on():
    from wdf_hip import binding as wb
    # (the binding sizes the workspace by the library's own answer, 0 bytes without a state: the null workspace is refused first;
    # tests/test_cabi_cpu.py has the C ABI's own message)
    _refused(_all_five(_args(0, 1, "none"), 0, 1), "without states|null", only=("ss_fwd_lin_tp", "ss_bwd_tp"))
    _refused(_all_five(_args(0, 1, "pair11"), 0, 1), "without states|null", only=("ss_fwd_tp", "ss_bwd_tp"))
    a = _args(2, 1, "none")
    with pytest.raises(wb.WdfHipError, match="nothing to speculate"):
        wb.ss_fwd_tp(a["x"], a["coef"], 2, 1, cuda([4.352e-9, 0.0493, 1.0e4]), 2, 8, root_kind=wb.ROOT_NONE)


@pytest.mark.parametrize("root", ["none", "pair11", "asym"])
def test_f_shapes_the_binding_checks(root):
    """x, coef, z0, zstash, gy and rootp of the wrong size: an out-of-bounds read if the launch went ahead"""
    ns, ni, B, T = 2, 2, 4, 16
    a = _args(ns, ni, root, B, T)
    z = lambda *s: torch.zeros(s, device="cuda")
    _refused(_all_five(a, ns, ni, x=z(B, T, 1)), "x has")
    _refused(_all_five(a, ns, ni, x=z(B, T)), "x has")
    _refused(_all_five(a, ns, ni, coef=a["coef"][:-1].contiguous()), "coef must hold")
    _refused(_all_five(a, ns, ni, coef=torch.ones((R.ncoef(ns, ni) + 1,), device="cuda")), "coef must hold")
    fwd = ("ss_fwd", "ss_fwd_lin_tp", "ss_fwd_tp")
    for bad in (z(ns, B - 1), z(ns - 1, B), z(B, ns), z(ns * B)):
        _refused(_all_five(a, ns, ni, z0=bad), "z0 must be", only=fwd)
    bwd = ("ss_bwd", "ss_bwd_tp")
    for bad in (z(T - 1, ns, B), z(T, ns - 1, B), z(T, B, ns), z(T * ns * B), None):
        _refused(_all_five(a, ns, ni, zs=bad), "zstash must be", only=bwd)
    for bad in (z(T - 1, B), z(B, T), z(T * B)):
        _refused(_all_five(a, ns, ni, gy=bad), "gy must be", only=bwd)
    if root != "none":
        _refused(_all_five(a, ns, ni, rootp=a["rootp"][:-1].contiguous()), "rootp must hold")
        _refused(_all_five(a, ns, ni, rootp=None), "rootp must hold")
