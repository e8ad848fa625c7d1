"""CPU: the reference of the linear one-pass MSE + ESR step (tests/ss_lin_esr_ref.py) pinned against tests/ss_lin_ref.py and against
central differences of its own loss; the caps and the no-cancellation property the GPU module's bounds rest on, over exactly its
cases; and wdf_ss_lin_step_esr_ws_bytes / the refusals of wdf_ss_lin_step_esr and wdf_ss_lin_esr_finish through the library, without
a device (as tests/test_cabi_cpu.py does)."""
import ctypes as C
import os

import numpy as np
import pytest

import ss_lin_esr_ref as E
import ss_lin_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- against ss_lin_ref ------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("ns,ni", R.TREES)
def test_helper_is_ss_lin_ref_bit_for_bit(ns, ni, dtype):
    """y and zT at any skip; at skip = 0 the P family, its magnitudes and S are ss_lin_ref.run's g, mag and sse at gscale = 1"""
    c = R.case(ns, ni, "plain", 5, 60, True)
    want = R.run(ns, ni, c.coef, c.x, c.target, 1.0, z0=c.z0, dtype=dtype)
    for skip in (0, 7, 59):
        got = E.run(ns, ni, c.coef, c.x, c.target, skip, z0=c.z0, dtype=dtype)
        assert np.array_equal(bits(got.y), bits(want.y)) and np.array_equal(bits(got.zT), bits(want.zT))
        if skip == 0:
            assert np.array_equal(bits(got.GP), bits(want.g)) and np.array_equal(bits(got.magP), bits(want.mag)) and got.S == want.sse
        else:
            assert got.S < want.sse and np.all(got.magP < want.mag)
    # the Q family is the P family of a zero target
    zero = R.run(ns, ni, c.coef, c.x, np.zeros_like(c.target), 1.0, z0=c.z0, dtype=dtype)
    got = E.run(ns, ni, c.coef, c.x, c.target, 0, z0=c.z0, dtype=dtype)
    assert np.array_equal(bits(got.GQ), bits(zero.g)) and got.E == zero.sse


# ---- against central differences ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,ni", R.TREES)
@pytest.mark.parametrize("skip", [0, 7, 23])
def test_g_against_central_differences_of_the_float64_loss(ns, ni, skip):
    """T = 24 with z0 (skip = T - 1 = 23 among them), step 1e-6 on the float64 coefficients: truncation h^2 / 6 x the third derivative
    and rounding 1e-16 / h of a loss of order 1 -- the entries agree within 1e-6 of |ga| magP_i + |gb| magQ_i (ss_lin_ref's test has
    the same bound for its loss)."""
    c = R.case(ns, ni, "plain", 3, 24, True)
    ref = E.run(ns, ni, c.coef, c.x, c.target, skip, z0=c.z0)
    c64 = c.coef.astype(np.float64)
    for i, row in enumerate(R.rows(ns, ni)):
        h = 1e-6
        cp, cm = c64.copy(), c64.copy()
        cp[row] += h
        cm[row] -= h
        fd = (E.loss_of(ns, ni, cp, c.x, c.target, skip, c.z0) - E.loss_of(ns, ni, cm, c.x, c.target, skip, c.z0)) / (2 * h)
        assert abs(ref.g[i] - fd) <= 1e-6 * ref.gmag[i], (i, ref.g[i], fd, ref.gmag[i])
    assert ref.esr > 0 and ref.gb < 0 < ref.ga


def test_an_esr_of_zero_contributes_no_gradient():
    c = R.case(1, 1, "plain", 3, 24)
    y = E.run(1, 1, c.coef, c.x, c.target, 0, dtype=np.float32).y
    r = E.run(1, 1, c.coef, c.x, y, 0, dtype=np.float32)
    assert r.S == 0.0 and r.esr == 0.0 and r.gb == 0.0 and r.ga == 2.0 / r.n and np.all(r.g == 0) and np.all(np.isfinite(r.g))


# ---- what the GPU bounds rest on ---------------------------------------------------------------------------------------------
def test_fp32_restatement_caps_and_no_cancelled_gradient_on_every_gpu_case():
    """Every call the GPU module compares: the float32 restatement against the float64 one -- y within 4e-7 max |y|, S and E within
    2e-7 relative (ss_lin_ref's caps), the P family within CAP_P = 2e-7 magP_i, the Q family within CAP_Q magQ_i.  CAP_Q is 2.2e-7,
    not 2e-7: the Q family measures 2.15e-7 on (1,1) B = 1 T = 40 (35 addends of one sequence: nothing averages out), every other
    case stays below 1.9e-7; the GPU bound 8 x 2.2e-7 + 32 x 2^-24 = 3.7e-6 still rounds up to the 4e-6 of the P family.
    And no final gradient entry g_p cancels below 3 % of |ga| magP_p + |gb| magQ_p in the float64 reference."""
    worst = dict(y=0.0, S=0.0, E=0.0, P=0.0, Q=0.0)
    least = 1.0
    cases = E.gpu_cases()
    for c in cases:
        r64, r32 = c.ref(), c.ref(np.float32)
        f = dict(y=float(np.max(np.abs(r32.y.astype(np.float64) - r64.y)) / np.max(np.abs(r64.y))),
                 S=abs(r32.S - r64.S) / r64.S, E=abs(r32.E - r64.E) / r64.E,
                 P=float(np.max(np.abs(r32.GP - r64.GP) / r64.magP)), Q=float(np.max(np.abs(r32.GQ - r64.GQ) / r64.magQ)))
        worst = {k: max(worst[k], f[k]) for k in f}
        assert f["y"] <= E.CAP_Y and f["S"] <= E.CAP_SUM and f["E"] <= E.CAP_SUM and f["P"] <= E.CAP_P and f["Q"] <= E.CAP_Q, (c, f)
        assert np.all(r64.magP > 0) and np.all(r64.magQ > 0) and r64.esr > 0, c
        frac = float(np.min(np.abs(r64.gp) / r64.gpmag))
        least = min(least, frac)
        assert frac >= 0.03, (c, frac)
    assert E.CAP_P == 2e-7 and 8 * E.CAP_Q + 32 * 2.0 ** -24 <= E.B_G
    print(f"fp32 against fp64, worst over {len(cases)} cases: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f"; least |g_p| / magnitude {least:.3f}")


def test_the_cases_cover_what_the_gpu_module_promises():
    cases = E.gpu_cases()
    keys = {c.key for c in cases}
    assert len(keys) == len(cases)
    for ns, ni in R.TREES:
        for B, T, _ in E.SHAPES_A:
            assert (ns, ni, B, T, E.SKIP_A, 3, False) in keys
    for B, T, k in E.SHAPES_B:
        L = -(-T // (k * 32)) * 32
        s = E.skips_b(T)
        assert s[0] == 0 and s[-1] == T - 1 and 2 * L <= s[4] < min(3 * L, T) and s[4] % 8 != 0
    assert any(c.n_params == 15 for c in cases) and any(c.n_params == 1 for c in cases) and any(c.n_global for c in cases)
    whole, first, second = E.carried()
    assert np.array_equal(np.concatenate([first.x, second.x]), whole.x) and first.z0 is not None and whole.skip == first.T + second.skip
    w, a, b = whole.ref(), first.ref(), second.ref()
    assert np.max(np.abs(np.concatenate([a.y, b.y]) - w.y)) <= 1e-13 and abs(b.S - w.S) <= 1e-12 * w.S and abs(b.E - w.E) <= 1e-12 * w.E


# ---- the library, without a device -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


def test_workspace_size_is_the_mse_layout_with_the_partials_doubled(lib):
    from wdf_hip import binding
    for ns, ni in R.TREES:
        for B in (1, 63, 64, 65, 130, 1340, 8192):
            for T, n in ((1, 1), (40, 1), (100, 4), (257, 3), (2048, 64), (4096, 47)):
                L, K = binding.chunk_geom(T, n, 32)
                D, G = ns * (1 + ns * ns + ns * ni), R.kg(ns, ni)
                waves = -(-B // 64) * K
                want = 256 + K * D * B * 4 + 256 + waves * 2 * (G + 1) * 8
                got = lib.wdf_ss_lin_step_esr_ws_bytes(ns, ni, B, T, n)
                mse = lib.wdf_ss_lin_step_ws_bytes(ns, ni, B, T, n)
                assert got == want and got >= mse and got - mse == waves * (G + 1) * 8, (ns, ni, B, T, n, got, want, mse)
    assert lib.wdf_ss_lin_step_esr_ws_bytes(3, 1, 64, 64, 1) == 0 and lib.wdf_ss_lin_step_esr_ws_bytes(1, 3, 64, 64, 1) == 0
    assert lib.wdf_ss_lin_step_esr_ws_bytes(1, 1, 0, 64, 1) == 0 and lib.wdf_ss_lin_step_esr_ws_bytes(1, 1, 64, 64, 0) == 0


ONE = C.c_void_p(256)      # a non-null, aligned pointer that no check dereferences


def test_every_refusal_happens_before_any_launch(lib):
    order = "x coef jac n_params ns ni target n_global eps skip y ws sums g loss3 gcoef_out B T n_chunks z0 zT stream".split()
    good = dict(x=ONE, coef=ONE, jac=ONE, n_params=2, ns=1, ni=1, target=ONE, n_global=1000.0, eps=2.2e-16, skip=50, y=ONE, ws=ONE,
                sums=ONE, g=ONE, loss3=None, gcoef_out=None, B=4, T=256, n_chunks=4, z0=None, zT=None, stream=None)
    bad = [(dict(x=None), -1, b"null"), (dict(coef=None), -1, b"null"), (dict(jac=None), -1, b"null"), (dict(target=None), -1, b"null"),
           (dict(y=None), -1, b"null"), (dict(ws=None), -1, b"null"), (dict(sums=None, g=None), -1, b"both null"),
           (dict(skip=-1), -1, b"skip"), (dict(skip=256), -1, b"skip"), (dict(skip=1 << 40), -1, b"skip"),
           (dict(n_global=0.0), -1, b"n_global"), (dict(n_global=-5.0), -1, b"n_global"), (dict(n_global=float("nan")), -1, b"n_global"),
           (dict(eps=-1.0), -1, b"eps_energy"), (dict(z0=ONE, zT=ONE), -1, b"alias"), (dict(n_params=0), -1, b"1..15"),
           (dict(n_params=16), -1, b"1..15"), (dict(ns=3), -3, b"ns in 0..2"), (dict(ns=-1), -3, None), (dict(ni=0), -3, None),
           (dict(ni=3), -3, None), (dict(B=0), -1, None), (dict(T=0), -1, None), (dict(n_chunks=0), -1, None)]
    for over, code, text in bad:
        rc = lib.wdf_ss_lin_step_esr(*[{**good, **over}[k] for k in order])
        assert rc == code, (over, rc, lib.wdf_last_error())
        assert b"wdf_ss_lin_step_esr" in lib.wdf_last_error() and (text is None or text in lib.wdf_last_error()), (over, lib.wdf_last_error())
    fin = lib.wdf_ss_lin_esr_finish
    assert fin(None, 2, 10.0, 0.0, ONE, None, None) == -1 and b"null" in lib.wdf_last_error()
    assert fin(ONE, 2, 10.0, 0.0, None, None, None) == -1 and b"null" in lib.wdf_last_error()
    assert fin(ONE, 0, 10.0, 0.0, ONE, None, None) == -1 and fin(ONE, 16, 10.0, 0.0, ONE, None, None) == -1
    assert fin(ONE, 2, 0.0, 0.0, ONE, None, None) == -1 and fin(ONE, 2, 10.0, -1.0, ONE, None, None) == -1
    assert lib.wdf_abi_version() == 6


def test_the_binding_has_the_new_names_and_refuses_without_a_gpu():
    import torch
    from wdf_hip import binding
    for s in ("wdf_ss_lin_step_esr_ws_bytes", "wdf_ss_lin_step_esr", "wdf_ss_lin_esr_finish"):
        assert s in binding.EXPORTED_SYMBOLS
    assert callable(binding.ss_lin_step_esr) and callable(binding.ss_lin_esr_finish) and binding.ESR_EPS == E.EPS
    from wdf_hip import lowering
    assert lowering.LIN_ESR_STEP_SERVES in (False, True) and hasattr(lowering.Circuit, "_mse_esr_lin_step")
    if not torch.cuda.is_available():
        with pytest.raises(binding.WdfHipError):
            binding.ss_lin_step_esr(torch.zeros(8, 1, 2), torch.zeros(9), torch.zeros(9, 2, dtype=torch.float64), torch.zeros(8, 2), 0, 1)
        with pytest.raises(binding.WdfHipError):
            binding.ss_lin_esr_finish(torch.zeros(6), 16.0)
