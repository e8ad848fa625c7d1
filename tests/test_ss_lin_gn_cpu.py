"""CPU: the reference of the linear trees' Gauss-Newton step (tests/ss_lin_gn_ref.py) has to be right before the kernel is compared
with it, and what the new entry points refuse without a device.

  1  the per-row tangents d against float64 central differences of y with respect to each coefficient;
  2  Hc symmetric and positive semidefinite; g = gscale sum e d equal to ss_lin_ref's g (and y, SSE, zT equal to its);
  3  refusals and argument validation that need no device; the new symbols in the header and in binding.SIGNATURES;
  4  wdf_hip.lm.LevenbergMarquardt driven by the float64 reference on the two fits of tests/test_gpu_circuit_lin_gn.py: the
     evaluations it needs to reach 1e-6 of the starting loss, N_ref.  Measured: 6 (lpf.py's tree), 4 (the voltage divider); the GPU
     module computes them again and allows twice as many;
  5  the bound B_H of the GPU kernel module, set the way tests/test_gpu_ss_lin_step_kernel.py sets B_G: max |Hc32 - Hc64| / magH
     of the float32 restatement over exactly the GPU cases (the reference only, never the kernel) is 5.64e-7 ((1,2) B = 2, T = 33)
     and asserted to stay under FLOOR = 5.7e-7; B_H = 8 x FLOOR + 32 x 2^-24 = 6.5e-6.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ss_lin_gn_ref as G
import ss_lin_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = G.FS


@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


SMALL = [(ns, ni, fam) for ns, ni in R.TREES for fam in (("plain",) if ns == 0 else ("plain", "neg"))]


# ---- 1, 2: the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,ni,fam", SMALL, ids=[f"ns{a}-ni{b}-{f}" for a, b, f in SMALL])
def test_tangents_against_central_differences(ns, ni, fam):
    c = R.case(ns, ni, fam, 3, 40, z0=bool(ns))
    y, d, _ = G.tangents(ns, ni, c.coef, c.x, c.z0)
    c64 = c.coef.astype(np.float64)
    worst = 0.0
    for r, idx in enumerate(R.rows(ns, ni)):
        h = 1e-6 * max(1.0, abs(c64[idx]))
        cp, cm = c64.copy(), c64.copy()
        cp[idx] += h
        cm[idx] -= h
        fd = (G.tangents(ns, ni, cp, c.x, c.z0)[0] - G.tangents(ns, ni, cm, c.x, c.z0)[0]) / (2 * h)
        err = float(np.max(np.abs(fd - d[:, r])) / max(1.0, np.max(np.abs(d[:, r]))))
        worst = max(worst, err)
    print(f"d against central differences ({ns},{ni}) {fam}: {worst:.2e}")
    assert worst < 1e-8, worst          # y is polynomial in the coefficients: O(h^2) truncation, 1e-16 / h rounding


@pytest.mark.parametrize("ns,ni,fam", SMALL, ids=[f"ns{a}-ni{b}-{f}" for a, b, f in SMALL])
def test_hc_is_a_gram_matrix_and_the_gradient_is_the_steps(ns, ni, fam):
    c = R.case(ns, ni, fam, 5, 64, z0=bool(ns))
    for dtype in (np.float64, np.float32):
        r = G.run(ns, ni, c.coef, c.x, c.target, c.gscale, z0=c.z0, dtype=dtype)
        s = R.run(ns, ni, c.coef, c.x, c.target, c.gscale, z0=c.z0, dtype=dtype)
        assert np.array_equal(r.y, s.y) and np.array_equal(r.zT, s.zT) and r.sse == s.sse
        assert np.allclose(r.g, s.g, rtol=0, atol=(1e-12 if dtype == np.float64 else 2e-6) * np.max(s.mag))
        assert np.array_equal(r.Hc, r.Hc.T) and np.all(np.abs(r.Hc) <= r.magH * (1 + 1e-12))
        assert np.min(np.linalg.eigvalsh(r.Hc)) >= -1e-6 * np.max(np.diag(r.Hc))
    r = G.run(ns, ni, c.coef, c.x, c.target, c.gscale, z0=c.z0)
    D = r.d.transpose(1, 0, 2).reshape(r.d.shape[1], -1)
    assert np.allclose(r.Hc, D @ D.T, rtol=1e-12, atol=0)
    assert np.array_equal(G.upper(r.Hc), np.array([r.Hc[i, j] for i in range(len(r.Hc)) for j in range(i, len(r.Hc))]))
    jac = np.random.default_rng(1).standard_normal((R.ncoef(ns, ni) + 1, 3))
    H = G.chain(ns, ni, r.Hc, jac, c.gscale)
    dth = np.einsum("tgb,gp->tpb", r.d, jac[R.rows(ns, ni)])
    assert np.allclose(H, float(np.float32(c.gscale)) * np.einsum("tpb,tqb->pq", dth, dth), rtol=1e-10, atol=0)
    assert np.all(np.abs(H) <= G.chain_bound(ns, ni, r.magH, jac, 1.0, c.gscale) * (1 + 1e-12))


# ---- 5: the bound ----------------------------------------------------------------------------------------------------------------
def test_the_float32_restatement_stays_under_the_floor():
    worst, at = 0.0, None
    for key in G.gpu_case_keys():
        f = G.h_distance(key)
        if f > worst:
            worst, at = f, key
    print(f"max |Hc32 - Hc64| / magH over {len(G.gpu_case_keys())} GPU cases: {worst:.3e} at {at}; FLOOR {G.FLOOR:.1e}, B_H {G.B_H:.3e}")
    assert worst <= G.FLOOR, (worst, at)
    assert G.B_H == 8 * G.FLOOR + 32 * 2.0 ** -24


def test_the_cases_are_the_issues():
    keys = G.gpu_case_keys()
    for ns, ni in R.TREES:
        for B, T, _ in [(1, 40, 1), (65, 100, 4), (130, 257, 3), (2, 33, 2)]:
            assert (ns, ni, "plain", B, T, False) in keys
    assert (2, 1, "plain", 65, 2048, False) in keys and any(k[2] == "slow" for k in keys) and any(k[5] for k in keys)
    assert G.PARAMS == [1, 2, 15]


# ---- 3: refusals -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_the_header_and_in_the_signature_table(lib):
    from wdf_hip import binding as wb
    header = open(os.path.join(REPO, "include", "wdf_hip.h")).read()
    for name in ("wdf_ss_lin_step_gn_ws_bytes", "wdf_ss_lin_step_gn"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in wb.SIGNATURES and name in wb.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert wb.SIGNATURES["wdf_ss_lin_step_gn"][1] == wb.SIGNATURES["wdf_ss_lin_step_mse"][1]
    assert callable(wb.ss_lin_step_gn)


def test_workspace_size(lib):
    ws, mse = lib.wdf_ss_lin_step_gn_ws_bytes, lib.wdf_ss_lin_step_ws_bytes
    assert ws(3, 1, 64, 64, 1) == 0 and ws(1, 0, 64, 64, 1) == 0 and ws(1, 1, 0, 64, 1) == 0 and ws(1, 1, 64, 64, 0) == 0
    assert ws(1, 1, 64, 0, 1) == 0 and ws(1, 3, 64, 64, 1) == 0 and ws(-1, 1, 64, 64, 1) == 0
    from wdf_hip import binding
    for ns, ni in R.TREES:
        for B, T, n in [(1, 40, 1), (65, 100, 4), (130, 2048, 64)]:
            K = binding.chunk_geom(T, n, 32)[1]
            g = R.kg(ns, ni)
            assert ws(ns, ni, B, T, n) - mse(ns, ni, B, T, n) == -(-B // 64) * K * (g * (g + 1) // 2) * 8, (ns, ni, B, T, n)


def test_argument_validation_without_gpu(lib):
    """every check is made before any HIP call, in the MSE step's words"""
    one = C.c_void_p(256)
    order = ["x", "coef", "jac", "n_params", "ns", "ni", "target", "gscale", "y", "ws", "out", "loss_out", "hcoef_out", "B", "T", "n_chunks",
             "z0", "zT", "stream"]
    good = dict(x=one, coef=one, jac=one, n_params=2, ns=1, ni=1, target=one, gscale=1.0, y=one, ws=one, out=one, loss_out=None,
                hcoef_out=None, B=64, T=64, n_chunks=2, z0=None, zT=None, stream=None)
    bad = [(dict(x=None), -1, b"null argument"), (dict(coef=None), -1, b"null argument"), (dict(jac=None), -1, b"null argument"),
           (dict(target=None), -1, b"null argument"), (dict(y=None), -1, b"null argument"), (dict(ws=None), -1, b"null argument"),
           (dict(out=None), -1, b"null argument"), (dict(ns=3), -3, b"ns in 0..2, ni in 1..2 (got 3, 1)"),
           (dict(ni=0), -3, b"ns in 0..2, ni in 1..2"), (dict(B=0), -1, b"B, T, n_chunks >= 1"), (dict(T=0), -1, b"B, T, n_chunks >= 1"),
           (dict(n_chunks=0), -1, b"B, T, n_chunks >= 1"), (dict(n_params=0), -1, b"1..15 parameters"),
           (dict(n_params=16), -1, b"1..15 parameters"), (dict(z0=one, zT=one), -1, b"wdf_ss_lin_step_gn: zT must not alias z0"),
           (dict(out=C.c_void_p(260)), -1, b"8-byte aligned"), (dict(hcoef_out=C.c_void_p(260)), -1, b"8-byte aligned")]
    for over, rc, words in bad:
        kw = {**good, **over}
        got = lib.wdf_ss_lin_step_gn(*[kw[k] for k in order])
        assert got == rc and words in lib.wdf_last_error(), (over, got, lib.wdf_last_error())
    # the same mistake through the MSE step: the same words (the checks are shared, not copied)
    mse_order = ["gcoef_out" if k == "hcoef_out" else k for k in order]
    for over in (dict(ns=3), dict(n_params=16), dict(x=None)):
        kw = {**good, "gcoef_out": None, **over}
        lib.wdf_ss_lin_step_gn(*[kw[k] for k in order])
        a = lib.wdf_last_error().replace(b"wdf_ss_lin_step_gn", b"")
        lib.wdf_ss_lin_step_mse(*[kw[k] for k in mse_order])
        assert a == lib.wdf_last_error().replace(b"wdf_ss_lin_step_mse", b""), over


def test_circuit_refusals_need_no_device():
    import tf_wdf as W
    from wdf_hip import binding as wb
    x, tg = np.zeros((2, 64), dtype=np.float32), np.zeros((64, 2), dtype=np.float32)
    for build in (G.build_lpf, G.build_divider):
        circ, _ = build(W)
        with pytest.raises(wb.WdfHipError, match=r"to_device\(\)"):
            circ.mse_gn(x, tg)
        with pytest.raises(wb.WdfHipError, match=r"to_device\(\)"):
            circ.gn_variables
    # a linear tree the resident step does not take keeps the refusal by name
    Rs = [W.Resistor(1.0e3, True) for _ in range(2)]
    Cs = [W.Capacitor(1.0e-7, FS, True) for _ in range(3)]
    top = W.Inverter(W.Series(Rs[0], W.Parallel(Cs[0], W.Series(Rs[1], W.Parallel(Cs[1], Cs[2])))))
    big = W.Circuit(top, W.IdealVoltageSource(), Cs[2])
    assert big.ns == 3
    with pytest.raises(wb.WdfHipError, match="IdealVoltageSource root has no Gauss-Newton step"):
        big.mse_gn(x, tg)


# ---- 4: the fits, by the float64 reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["lpf", "divider"])
def test_lm_on_the_float64_reference(which):
    path, start = G.reference_fit(which)
    n_ref = G.evaluations_to_reach(path, start, 1e-6)
    print(f"LM on the float64 reference, {which}: start {start:.3e}, (evaluations, loss) {[(n, '%.3e' % v) for n, v in path]} -> N_ref = {n_ref}")
    assert n_ref is not None and n_ref <= 10, path
    assert start > 1e-3                                           # (a fit worth the name: the start is far from the teacher)
