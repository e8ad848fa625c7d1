"""GPU: the MLP-root clipper kernels (csrc/wdf_mlp.h, wdf_mlp_row.h, wdf_mlp_tp.h, wdf_mlp_mfma.h behind csrc/wdf_capi_mlp.hip) at
kernel level, through wdf_hip.binding only (clipper_mlp_*, mlp_eval; no Circuit), against tests/mlp_clip_ref.py: the recursion and its
adjoint restated directly in float64, pinned on the CPU by tests/test_mlp_clip_ref_cpu.py.  The rest of the suite compares these
kernels with each other (tests/test_gpu_mlp_root.py), and they share mlp_load_consts, mlp_step_coeffs, tanh_fast, the adjoint
formulas and clipper_mlp_grad_reduce_kernel: an error in a shared piece passes all of that.

  A  sequential forward: the seven architectures x static / per-sample R x {one lane per sequence, 16-lane rows, matrix cores} at
     (B,T) = (1,1), (3,15), (4,16), (5,17), (17,33) and (66,130) from a non-zero z0.  y, zstash, zT.
  B  sequential reverse sweeps fed the REFERENCE's stash rounded to float32: clipper_mlp_bwd on the lane and the row kernels then
     clipper_mlp_wgrad, and clipper_mlp_bwd_w, same architectures and shapes.  gb, ain, lrin per step; gtheta2 (static R: both
     components; per-sample R: dC, and dR exactly 0); gw.
  C  step-parallel reverse sweep clipper_mlp_bwd_w_tp: kappa recomputed from the reference's stash, and a kappa stored by a
     want_kappa forward (then at that forward's own stash); row and matrix-core weight-gradient pass; T in {7, 8, 9, 127, 128, 129, 131,
     136, 257} (kScanChunk = 128, unrolled by 8; 131: the chunked scan's tail runs more than one step) x B in {3, 66} x chunk counts
     1, 2 and T/16 + 2; (4,4), (8,3), (16,3).  gtheta2, gw, the stored kappa itself.
  D  time-parallel forward clipper_mlp_fwd_tp, with and without want_kappa, rows and matrix cores, at (5,100), (17,257) from a
     non-zero z0, (66,130): a warm-up taken from the reference's kappa (K = 3: unequal chunks; K = 2; K = T/16 + 2, realised K from the
     library) -> clean status; the trained 2x16 / 2x8 roots under workload.dataset_resistance_batch with a warm-up of 16 -> waves
     gated, the result still the reference's to the bound + 2 tol; warm-up 0 with zinit from the reference's stash at
     binding.mlp_tp_starts -> n_bad 0, max_miss <= tol.
  E  mlp_eval: seven architectures, S in {1, 63, 64, 65, 131072 + 65} (past the grid cap of 2048 blocks), |a| up to 20.
  F  wrongly sized z0, zstash, gy, r, kappa, zinit, warmup_per_wave, w: WdfHipError before any launch.

Bounds (mlp_clip_ref; none taken from what the kernels give):
  y, zstash, zT   5e-6 max(1, max |z_ref|)                    tests/test_gpu_mlp_root.py::test_clipper_model_forward_loss_grads
  gw, dR, dC      1e-4 |ref| + 1e-5 max |ref| per component   the same test; dR and dC each judged as a vector of its own (they differ by
                                                              twelve orders of magnitude), i.e. to 1.1e-4 relative
  kappa, gb, ain, lrin, mlp_eval   8 x the case's float32 floor: max |ref32 - ref64| of the reference itself (never less than half a
                  float32 ulp of the quantity's largest value, mlp_clip_ref.floor).  The kernels use tanh_fast, fast_rcp and fast_log,
                  a few ulp each where torch's float32 is within one, and sum a layer in another order.
  after a repair  + 2 tol on y, zstash, zT and + 2 tol max |d kappa / dz| on kappa (a repaired chunk arrives within tol, not exactly)
Every check prints `FIG <section> | <case> | <what> | quantity error (floor or bound, ratio) ...` before it asserts (run with -s);
profiles/mlp_clip_kernels_digest.txt holds them from one MI355X, condensed to the worst check of every case.

Measured there (164 tests, 2327 FIG lines, 12 s in all, the references included; worst of each section): A y 0.23, zstash 0.27 of the
bound; B gb 3.7, ain 1.2, lrin 2.1 floors, dR 0.02, dC 0.04, gw 0.06 of the bound; C stored kappa 2.5 floors, gradients 0.014 of the
bound; D y 0.28 of the bound (trained 2x8, repaired), kappa 2.4 floors; E 4.4 floors.  No quantity needed a factor above 8 and no wrong
number was found.  The digest also lists five one-line wrong builds of the library and which tests here failed on each; one of the
five (t0 + 8 -> t0 + 16 in mlp_adjoint_scan_chunked_kernel) changes no bit -- the tail loop takes over the same steps -- and fails
nothing, here or anywhere.
"""
import functools
import gc

import numpy as np
import pytest

import mlp_clip_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FS = R.FS
TOL = R.TP_TOL


@pytest.fixture(scope="module", autouse=True)
def _module():
    from wdf_hip import workload
    R.set_trained_loader(workload.reference_mlp_weights)
    yield
    dev.cache_clear()
    stored_kappa_forward.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()        # (tests/test_gpu_cache_identity.py relies on the allocator handing a freed block straight back)


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def dev(c):
    """the case's inputs on the device: x, r | None, theta2, w, z0 | None, gy"""
    i = R.inputs(c, R._trained["fn"])
    return (cuda(i.x), cuda(i.R) if c.dyn else None, cuda([R.R_STATIC, R.C_CLIPPER]), cuda(i.w),
            None if i.z0 is None else cuda(i.z0), cuda(i.gy))


FAMILIES = ["lane", "row", "matrix-cores"]


@pytest.fixture
def forward_family(request, monkeypatch):
    """Which forward kernel family runs (local to this file): one lane per sequence (binding.MLP_LANE_PER_SEQUENCE), the 16-lane row
    kernel (WDF_MLP_FWD_ROW = 1) or the matrix-core kernel (WDF_MLP_FWD_ROW = 0)."""
    from wdf_hip import binding as wb
    fam = request.param
    monkeypatch.setattr(wb, "MLP_LANE_PER_SEQUENCE", fam == "lane")
    if fam == "lane":
        monkeypatch.delenv("WDF_MLP_FWD_ROW", raising=False)
    else:
        monkeypatch.setenv("WDF_MLP_FWD_ROW", "1" if fam == "row" else "0")
    return fam


class Figures:
    """one FIG line: quantities judged against a bound; print first, then assert"""

    def __init__(self, sec, case, what):
        self.head, self.items, self.bad = f"FIG {sec} | {R.case_id(case) if isinstance(case, R.Case) else case} | {what} |", [], []

    def add(self, name, err, bound, floor=None):
        ratio = err / bound if bound > 0.0 else (0.0 if err == 0.0 else float("inf"))
        extra = f"bound {bound:.2e}" if floor is None else f"floor {floor:.2e}"
        self.items.append(f"{name} {err:.2e} ({extra}, {'error/bound' if floor is None else 'error/floor'} "
                          f"{ratio if floor is None else (err / floor if floor > 0 else 0.0):.3f})")
        if not (np.isfinite(err) and err <= bound):
            self.bad.append(name)

    def forward(self, ref, y, zs, zT, extra=0.0):
        bound = R.Y_BOUND * max(1.0, float(np.max(np.abs(ref.zstash)))) + extra
        self.add("y", float(np.max(np.abs(np64(y) - ref.y))), bound)
        self.add("zstash", float(np.max(np.abs(np64(zs) - ref.zstash))), bound)
        self.add("zT", float(np.max(np.abs(np64(zT) - ref.zT))), bound)

    def floored(self, name, got, ref64, ref32, extra=0.0):
        fl = R.floor(ref32, ref64)
        self.add(name, float(np.max(np.abs(np64(got) - ref64))), R.FLOOR_FACTOR * fl + extra, floor=fl)

    def grads(self, c, ref, gth, gw):
        g = np64(gth)
        if c.dyn:
            self.add("dR (exactly 0)", abs(float(g[0])), 0.0)
        else:
            self.add("dR", R.grad_ratio([g[0]], [ref.gR]), 1.0)
        self.add("dC", R.grad_ratio([g[1]], [ref.gC]), 1.0)
        if gw is not None:
            self.add("gw", R.grad_ratio(np64(gw), ref.gw), 1.0)

    def note(self, text):
        self.items.append(text)

    def done(self):
        print(self.head + " " + "  ".join(self.items))
        assert not self.bad, (self.head, self.bad, self.items)


def arch_cases(sec, H, NL, dyn=None, B=None):
    return [c for c in R.cases(sec) if (c.H, c.NL) == (H, NL) and (dyn is None or c.dyn == dyn) and (B is None or c.B == B)]


# ------------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("forward_family", FAMILIES, indirect=True)
@pytest.mark.parametrize("dyn", [False, True], ids=["static-R", "R[B,T]"])
@pytest.mark.parametrize("H,NL", R.ARCHS)
def test_a_sequential_forward(H, NL, dyn, forward_family):
    from wdf_hip import binding as wb
    for c in arch_cases("AB", H, NL, dyn):
        x, r, th2, w, z0, _ = dev(c)
        y, zs, zT = wb.clipper_mlp_fwd(x, th2, w, H, NL, FS, r=r, z0=z0, want_zT=True)
        f = Figures("A", c, forward_family)
        f.forward(R.ref(c), y, zs, zT)
        f.done()


# ------------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("path", ["lane bwd + wgrad", "row bwd + wgrad", "bwd_w"])
@pytest.mark.parametrize("dyn", [False, True], ids=["static-R", "R[B,T]"])
@pytest.mark.parametrize("H,NL", R.ARCHS)
def test_b_sequential_reverse_sweeps(H, NL, dyn, path, monkeypatch):
    from wdf_hip import binding as wb
    monkeypatch.setattr(wb, "MLP_LANE_PER_SEQUENCE", path.startswith("lane"))
    for c in arch_cases("AB", H, NL, dyn):
        x, r, th2, w, _, gy = dev(c)
        zs = cuda(R.stash32(c))                                  # the reference's stash: a forward error can neither hide nor fail here
        s64, s32 = R.sweep_at_stash32(c), R.sweep_at_stash32(c, torch.float32)
        f = Figures("B", c, path)
        if path == "bwd_w":
            gth, gw = wb.clipper_mlp_bwd_w(x, th2, w, H, NL, FS, zs, gy, r=r)
        else:
            gth, gb, ain, lrin = wb.clipper_mlp_bwd(x, th2, w, H, NL, FS, zs, gy, r=r)
            gw = wb.clipper_mlp_wgrad(ain, lrin, gb, th2, w, H, NL, FS)
            f.floored("gb", gb, s64.gb, s32.gb)
            f.floored("ain", ain, s64.a, s32.a)
            assert (lrin is not None) == dyn
            if dyn:
                f.floored("lrin", lrin, s64.lr, s32.lr)
        f.grads(c, s64, gth, gw)
        f.done()


# ------------------------------------------------------------------------------------------------------------------ C
@functools.lru_cache(maxsize=None)
def stored_kappa_forward(c):
    """a want_kappa forward in ONE chunk (nothing speculated: the sequential result) -> zstash, kappa"""
    from wdf_hip import binding as wb
    x, r, th2, w, z0, _ = dev(c)
    _, zs, _, _, kap = wb.clipper_mlp_fwd_tp(x, th2, w, c.H, c.NL, FS, 1, 0, r=r, z0=z0, want_kappa=True)
    return zs, kap


@pytest.mark.parametrize("wgrad", ["row", "matrix-cores"])
@pytest.mark.parametrize("dyn", [False, True], ids=["static-R", "R[B,T]"])
@pytest.mark.parametrize("B", R.C_B)
@pytest.mark.parametrize("H,NL", R.C_ARCHS)
def test_c_step_parallel_reverse_sweep(H, NL, B, dyn, wgrad, monkeypatch):
    from wdf_hip import binding as wb
    monkeypatch.delenv("WDF_MLP_FWD_ROW", raising=False)
    for c in arch_cases("C", H, NL, dyn, B):
        x, r, th2, w, _, gy = dev(c)
        zs_ref = cuda(R.stash32(c))
        s64 = R.sweep_at_stash32(c)
        zs_own, kap = stored_kappa_forward(c)
        own, own32 = R.ref(c), R.ref32(c)
        f = Figures("C", c, "stored kappa")
        f.floored("kappa", kap, own.kappa, own32.kappa)
        f.done()
        for K in R.c_chunk_counts(c.T):
            # the matrix-core pass takes its own chunk count from WDF_MLP_WGRAD_MFMA: the same K, so that its grid never exceeds the row
            # grid the partial buffers are sized for (csrc/wdf_capi_mlp.hip falls back to the rows otherwise)
            monkeypatch.setenv("WDF_MLP_WGRAD_MFMA", str(K) if wgrad == "matrix-cores" else "0")
            Kr = wb.lib().wdf_clipper_mlp_tp_chunks(c.T, K)
            f = Figures("C", c, f"{wgrad} wgrad, {K} chunks asked, {Kr} run, kappa recomputed")
            gth, gw = wb.clipper_mlp_bwd_w_tp(x, th2, w, H, NL, FS, zs_ref, gy, K, r=r)
            f.grads(c, s64, gth, gw)
            f.done()
            f = Figures("C", c, f"{wgrad} wgrad, {K} chunks asked, {Kr} run, kappa stored")
            gth, gw = wb.clipper_mlp_bwd_w_tp(x, th2, w, H, NL, FS, zs_own, gy, K, r=r, kappa=kap)
            f.grads(c, own, gth, gw)
            f.done()


# ------------------------------------------------------------------------------------------------------------------ D
def _tp_forward(c, K, warm, want_kappa, zinit=None):
    from wdf_hip import binding as wb
    x, r, th2, w, z0, _ = dev(c)
    out = wb.clipper_mlp_fwd_tp(x, th2, w, c.H, c.NL, FS, K, warm, r=r, z0=z0, want_zT=True, tol=TOL, want_kappa=want_kappa,
                                zinit=zinit)
    return out[0], out[1], out[2], wb.mlp_tp_status(out[3]), (out[4] if want_kappa else None)


@pytest.mark.parametrize("forward_family", ["row", "matrix-cores"], indirect=True)
@pytest.mark.parametrize("c", R.cases("D"), ids=R.case_id)
def test_d_time_parallel_forward_synthetic(c, forward_family):
    from wdf_hip import binding as wb
    ref, ref32 = R.ref(c), R.ref32(c)
    W = R.warmup_from_kappa(ref.kappa, TOL)                      # (asserted a real warm-up on the CPU: W + 16 < T)
    for K in (3, 2, c.T // 16 + 2):
        Kr = wb.lib().wdf_clipper_mlp_tp_chunks(c.T, K)
        assert Kr > 1
        for want_kappa in (False, True):
            y, zs, zT, s, kap = _tp_forward(c, K, W, want_kappa)
            f = Figures("D", c, f"{forward_family}, warm-up {W} from kappa, {K} chunks asked, {Kr} run{', kappa' if want_kappa else ''}")
            f.forward(ref, y, zs, zT)
            if want_kappa:
                f.floored("kappa", kap, ref.kappa, ref32.kappa)
            f.note(f"status {s}")
            f.done()
            assert s["n_bad"] == 0 and s["gated_waves"] == 0 and s["sequential_waves"] == 0 and s["max_miss"] <= TOL, s
    # warm-up 0, every chunk started from the reference's state at its first sample
    K = 3
    starts = wb.mlp_tp_starts(c.T, K, 0)
    assert len(starts) == wb.lib().wdf_clipper_mlp_tp_chunks(c.T, K) and starts[0] == 0 and all(s % 16 == 0 for s in starts)
    zinit = cuda(ref.zstash[starts])
    y, zs, zT, s, kap = _tp_forward(c, K, 0, True, zinit=zinit)
    f = Figures("D", c, f"{forward_family}, zinit at {starts}, no warm-up, kappa")
    f.forward(ref, y, zs, zT)
    f.floored("kappa", kap, ref.kappa, ref32.kappa)
    f.note(f"status {s}")
    f.done()
    assert s["n_bad"] == 0 and s["gated_waves"] == 0 and s["max_miss"] <= TOL, s


@pytest.mark.parametrize("forward_family", ["row", "matrix-cores"], indirect=True)
@pytest.mark.parametrize("c", R.cases("Dt"), ids=R.case_id)
def test_d_time_parallel_forward_repairs_trained_roots(c, forward_family):
    """A warm-up of 16 under the data set's pot values with a trained root: far too short for the 75 and 99.1 kOhm sequences.  Waves
    are gated and re-run; the result is still the reference's, to the bound + 2 tol."""
    ref, ref32 = R.ref(c), R.ref32(c)
    slope = R.kappa_slope(c)
    for want_kappa in (False, True):
        y, zs, zT, s, kap = _tp_forward(c, 3, 16, want_kappa)
        f = Figures("D", c, f"{forward_family}, warm-up 16, 3 chunks{', kappa' if want_kappa else ''}")
        f.forward(ref, y, zs, zT, extra=2.0 * TOL)
        if want_kappa:
            f.floored("kappa", kap, ref.kappa, ref32.kappa, extra=2.0 * TOL * slope)
        f.note(f"max |dkappa/dz| {slope:.2f}  status {s}")
        f.done()
        assert s["n_bad"] > 0 and s["gated_waves"] > 0 and s["sequential_waves"] <= s["gated_waves"], s


# ------------------------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("H,NL", R.ARCHS)
def test_e_mlp_eval(H, NL):
    from wdf_hip import binding as wb
    seed, scale = R.SYNTH[(H, NL)]
    w = R.synthetic_mlp(H, NL, seed, scale)
    for S in R.EVAL_S:
        a, lr = R.eval_inputs(S)
        out = wb.mlp_eval(cuda(a), cuda(lr), cuda(w), H, NL)
        assert out.shape == (S,)
        f = Figures("E", f"{NL - 1}x{H}", f"S = {S}")
        f.floored("out", out, R.mlp_out(w, H, NL, a, lr), R.mlp_out(w, H, NL, a, lr, dtype=torch.float32))
        f.done()


# ------------------------------------------------------------------------------------------------------------------ F
def test_f_wrong_sizes_are_refused_before_any_launch():
    from wdf_hip import binding as wb
    H, NL, B, T = 8, 3, 5, 33
    x, th2, w = cuda(np.zeros((B, T))), cuda([R.R_STATIC, R.C_CLIPPER]), cuda(np.zeros(R.weight_count(H, NL)))
    r, z0, zs, gy = cuda(np.full((B, T), 1.0e4)), cuda(np.zeros(B)), cuda(np.zeros((T, B))), cuda(np.zeros((T, B)))
    bad_tb = cuda(np.zeros((T - 1, B)))
    E = wb.WdfHipError
    for fwd in (lambda **kw: wb.clipper_mlp_fwd(x, th2, w, H, NL, FS, **kw),
                lambda **kw: wb.clipper_mlp_fwd_tp(x, th2, w, H, NL, FS, 2, 16, **kw)):
        with pytest.raises(E, match="z0"):
            fwd(z0=cuda(np.zeros(B - 1)))
        with pytest.raises(E, match="r must be"):
            fwd(r=cuda(np.full((B, T - 1), 1.0e4)))
    with pytest.raises(E, match="weights"):
        wb.clipper_mlp_fwd(x, th2, w[:-1].contiguous(), H, NL, FS)
    with pytest.raises(E, match="theta2"):
        wb.clipper_mlp_fwd(x, th2[:1].contiguous(), w, H, NL, FS)
    for sweep in (lambda **kw: wb.clipper_mlp_bwd(x, th2, w, H, NL, FS, **kw),
                  lambda **kw: wb.clipper_mlp_bwd_w(x, th2, w, H, NL, FS, **kw),
                  lambda **kw: wb.clipper_mlp_bwd_w_tp(x, th2, w, H, NL, FS, n_chunks=2, **kw)):
        with pytest.raises(E, match="zstash"):
            sweep(zstash=bad_tb, gy=gy)
        with pytest.raises(E, match="gy"):
            sweep(zstash=zs, gy=bad_tb)
        with pytest.raises(E, match="r must be"):
            sweep(zstash=zs, gy=gy, r=cuda(np.full((B + 1, T), 1.0e4)))
    with pytest.raises(E, match="weights"):
        wb.clipper_mlp_bwd_w(x, th2, w[:-1].contiguous(), H, NL, FS, zs, gy)
    with pytest.raises(E, match="kappa"):
        wb.clipper_mlp_bwd_w_tp(x, th2, w, H, NL, FS, zs, gy, 2, kappa=bad_tb)
    with pytest.raises(E, match="zinit"):
        wb.clipper_mlp_fwd_tp(x, th2, w, H, NL, FS, 2, 0, want_kappa=True, zinit=cuda(np.zeros((3, B))))
    with pytest.raises(E, match="warmup_per_wave"):
        wb.clipper_mlp_fwd_tp(x, th2, w, H, NL, FS, 2, 16, r=r,
                              warmup_per_wave=torch.zeros(((B + 3) // 4 + 1,), dtype=torch.int32, device="cuda"))
    with pytest.raises(E, match="weights"):
        wb.mlp_eval(cuda(np.zeros(4)), cuda(np.zeros(4)), w[:-1].contiguous(), H, NL)
    # and the well-sized calls go through
    wb.clipper_mlp_fwd(x, th2, w, H, NL, FS, r=r, z0=z0)
    wb.clipper_mlp_bwd_w_tp(x, th2, w, H, NL, FS, zs, gy, 2, r=r)
    torch.cuda.synchronize()
