"""CPU: the input gradient dL/dx of the static state-space kernels -- its numpy reference (tests/ss_gx_ref.py), the two exports
(wdf_ss_bwd_gx_ws_bytes, wdf_ss_bwd_gx), their argument checks, and the routes of Circuit that refuse an x with a graph.

1. The float64 reference against central differences of L = sum(y gy), every sample of x perturbed through
   ss_static_ref.run's forward, on (B, T) = (2, 9) and (1, 1) for every (ns, ni) and root.

   The bound.  The reference's one approximation is Da, the central difference of the float64 root with step Root.H in a:
   Da_ref = b'(a) + H^2 b'''(a) / 6 + O(eps |b| / H).  The difference quotient of L in x[b,t,i] with the same step h = Root.H is
   dL/dx + h^2 L''' / 6 + O(eps sum|y gy| / h).  Both truncation terms are third derivatives of the root times H^2 / 6.  For the
   diode pair b = a - 2 V lam (mu0 omega(u0) - mu1 omega(u1)), u = l +- a / (mu V), and omega''' = omega (1 - 2 omega) / (1 + omega)^5
   lies in [-0.04, 0.05]: |b'''| <= 2 V (0.05 + 0.05) / (mu^2 V^3) <= 0.2 / V^2 with V the smaller nVt in play (0.0259 for the
   second of the two different diodes: 300; the same form bounds the exact Shockley pair, whose slope is between the two
   branches').  A perturbation of x[t][i] reaches the root at step t scaled by da[i] and the later roots through the contracting
   step map, and L''' collects b''' (da)^3 gb once per step it reaches (at most T = 9) plus the products of lower derivatives
   (|b''| <= 0.6 / V per root, at most T^2 pairs), every factor scaled by the wave scale s <= 2^3 that ss_static_ref.coefs puts
   on da and ca: |L'''| <= (9 x 300 + 81 x 24^2) x 8^3 x max|gb| < 3e7 max|gb|, so H^2 / 6 |L'''| < 5e-6 max|gb| -- against the
   channel's magnitude (>= |dy| |g| ~ max|gb| / 3) that is 2e-5 at the very worst, and the round-off terms (eps / H = 2e-10 of sum
   |y gy|, itself within 9 channel magnitudes) are below it.  FD_BOUND = 2e-5 x the channel's magnitude; a wrong or missing
   addend of gx is a whole addend, 1e4 times that.
2. The float32 mode within cap32 (CAP32 on linear trees, an eighth of G_NL under a root) over every case the GPU module runs.
3. The exports: in the header, under exports.map's pattern, in nm -D of the built library and in binding.EXPORTED_SYMBOLS; the
   ABI version; wdf_ss_bwd_gx_ws_bytes' values.
4. Argument validation through ctypes, with pointers that are never dereferenced.
5. The routes that refuse an x with a graph do so before a device is asked for.
"""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import ss_gx_ref as G
import ss_static_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_BOUND = 2e-5
NEW = ("wdf_ss_bwd_gx_ws_bytes", "wdf_ss_bwd_gx")


@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(2, 9), (1, 1)])
@pytest.mark.parametrize("root", R.ROOTS)
def test_reference_against_central_differences(root, B, T):
    worst = 0.0
    for ns, ni in R.TREES:
        if not R.built(ns, root):
            continue
        c = R.Case(ns, ni, root, "plain", B, T)
        g = G.ref(c)
        x64, gy64 = c.x.astype(np.float64), c.gy.astype(np.float64)

        def loss(x):
            return float(np.sum(R.run(ns, ni, c.coef, x, c.root, z0=c.z0).y * gy64))

        fd, h = np.empty((T, ni, B)), R.Root.H
        for b in range(B):
            for t in range(T):
                for i in range(ni):
                    xp, xm = x64.copy(), x64.copy()
                    xp[b, t, i] += h
                    xm[b, t, i] -= h
                    fd[t, i, b] = (loss(xp) - loss(xm)) / (2.0 * h)
        fig = R.ratio(np.max(np.abs(g.gx - fd), axis=(0, 2)), FD_BOUND * G.channel_mag(g.mag))
        print(f"({ns},{ni}) {root} B={B} T={T}: |gx - central differences| over FD_BOUND x channel magnitude = {fig:.3e}")
        worst = max(worst, fig)
        assert fig <= 1.0, (ns, ni, root, fig)
        assert np.all(np.abs(g.gx) <= g.mag * (1.0 + 1e-12))                   # mag bounds the sum of |addend| behind every entry
        if ns:
            assert np.allclose(g.lam0, c.ref().gz0, rtol=0, atol=1e-15)          # the same walk as run()'s
    print(f"{root} B={B} T={T}: worst {worst:.3e}")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,ni", R.TREES)
def test_float32_mode_stays_within_its_cap_over_the_gpu_cases(ns, ni):
    keys = [k for k in G.gpu_case_keys() if k[:2] == (ns, ni)]
    assert keys
    worst = 0.0
    for k in keys:
        c = G.case(*k)
        fig = G.float32_figure(c)
        worst = max(worst, fig)
        assert fig <= 1.0, (k, c.key, fig)
    print(f"({ns},{ni}): {len(keys)} cases, the float32 mode of gx at most {worst:.3f} of its cap")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_the_two_exports(lib):
    from wdf_hip import binding
    header = open(os.path.join(REPO, "include", "wdf_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    emap = open(os.path.join(REPO, "differentiable-wdfs_amd", "csrc", "exports.map")).read()
    emap = re.sub(r"/\*.*?\*/", "", emap, flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:([^}]*?)local:", emap, flags=re.S).group(1).split(";") if p.strip()]
    dyn = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in dyn.splitlines() if ln.strip()}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/wdf_hip.h"
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), f"{name} is not under exports.map's global names"
        assert name in exported, f"{name} is not in the library's dynamic symbol table"
        assert name in binding.EXPORTED_SYMBOLS and name in binding.SIGNATURES
    assert lib.wdf_abi_version() == 6 and binding.ABI_VERSION == 6
    assert "#define WDF_HIP_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header)


@pytest.mark.parametrize("ns", [0, 1, 2, 3, 4])
def test_ws_bytes(lib, ns):
    for B in (1, 64, 65, 1340):
        assert lib.wdf_ss_bwd_gx_ws_bytes(ns, B, 1) == 0
        for K in (2, 3, 16):
            assert lib.wdf_ss_bwd_gx_ws_bytes(ns, B, K) == K * ns * B * 4
    assert lib.wdf_ss_bwd_gx_ws_bytes(ns, 0, 4) == 0 and lib.wdf_ss_bwd_gx_ws_bytes(ns, 64, 0) == 0


def test_built_table_is_the_sweeps(lib):
    from wdf_hip import binding
    for ns in range(-1, 6):
        for ni in range(0, 4):
            for name, kind in R.ROOT_KIND.items():
                want = 0 <= ns <= 4 and 1 <= ni <= 2 and R.built(ns, name)
                assert binding.ss_bwd_gx_built(ns, ni, kind) == want, (ns, ni, name)
            assert not binding.ss_bwd_gx_built(ns, ni, 3) and not binding.ss_bwd_gx_built(ns, ni, 1)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
ONE = C.c_void_p(256)        # a non-null pointer that is never followed: every call below ends in its argument checks
ORDER = "x coef rootp ns ni root n_up n_down zstash gy ws_bwd_tp ws_gx gx B T n_chunks stream".split()


def _rc(lib, **over):
    good = dict(x=ONE, coef=ONE, rootp=ONE, ns=2, ni=1, root=2, n_up=1, n_down=1, zstash=ONE, gy=ONE, ws_bwd_tp=ONE, ws_gx=ONE, gx=ONE,
                B=65, T=128, n_chunks=4, stream=None)
    good.update(over)
    return lib.wdf_ss_bwd_gx(*[good[k] for k in ORDER]), lib.wdf_last_error()


@pytest.mark.parametrize("over,text", [
    (dict(x=None), b"null"), (dict(coef=None), b"null"), (dict(gy=None), b"null"), (dict(gx=None), b"null"),
    (dict(zstash=None), b"zstash"), (dict(ws_bwd_tp=None), b"workspace"), (dict(ws_gx=None), b"ws_gx"),
    (dict(gy=None, n_chunks=1, ws_bwd_tp=None, ws_gx=None), b"null"), (dict(gx=None, n_chunks=1), b"null"),
    (dict(zstash=None, n_chunks=1), b"zstash"),
    (dict(B=0), b"positive"), (dict(B=-3), b"positive"), (dict(T=0), b"positive"), (dict(T=-1), b"positive"),
    (dict(n_chunks=5), b"wdf_ss_tp_chunks"), (dict(n_chunks=0), b"does not tile"), (dict(n_chunks=-2), b"does not tile"),
    (dict(n_chunks=16, T=131), b"does not tile"),
    (dict(ns=0, zstash=None, n_chunks=2), b"without states"),
    (dict(rootp=None), b"rootp"), (dict(root=4, rootp=None), b"rootp"),
    (dict(root=1), b"unknown root"), (dict(root=2, n_up=0), b"[1,16]"),
])
def test_argument_validation_without_gpu(lib, over, text):
    rc, msg = _rc(lib, **over)
    assert rc == -1 and text in msg, (over, rc, msg)                          # WDF_EINVAL


@pytest.mark.parametrize("over", [dict(ns=5), dict(ns=-1), dict(ni=3), dict(ni=0), dict(root=4, ns=4)])
def test_unbuilt_combinations_answer_unsupported(lib, over):
    rc, msg = _rc(lib, **over)
    assert rc == -3, (over, rc, msg)                                          # WDF_EUNSUPPORTED


def test_chunk_counts_the_library_returns_pass_the_tiling_check(lib):
    """(the good case of the checks above cannot be launched here; what can be said without a device: a count wdf_ss_tp_chunks
    returns gets past the tiling check and stops at the next one)"""
    for T in (1, 9, 44, 128, 131):
        for want in (1, 2, 3, 16):
            K = lib.wdf_ss_tp_chunks(T, want)
            rc, msg = _rc(lib, T=T, n_chunks=K, gx=None)
            assert rc == -1 and msg.startswith(b"null gy/gx"), (T, want, K, msg)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
FS = 48000


def _no_gpu(monkeypatch):
    from wdf_hip import binding

    def no_gpu():
        raise AssertionError("Circuit asked for a device before it refused the input's graph")

    monkeypatch.setattr(binding, "require_gpu", no_gpu)


def _clipper(wdf):
    Vs = wdf.ResistiveVoltageSource(1.0e3, trainable=True)
    Cap = wdf.Capacitor(47.0e-9, FS, trainable=True)
    P1 = wdf.Parallel(Vs, Cap)
    return Vs, Cap, P1


def _x(torch, chans=None):
    shape = (2, 16) if chans is None else (2, 16, chans)
    return torch.zeros(shape, dtype=torch.float32, requires_grad=True)


def test_two_diode_clipper_on_its_own_kernels_refuses_before_the_device(monkeypatch):
    import tf_wdf as wdf
    import torch
    from wdf_hip import binding
    _no_gpu(monkeypatch)
    Vs, Cap, P1 = _clipper(wdf)
    root = wdf.AsymDiodePair(P1, 2.52e-9, 2.0e-6, trainable=True)
    circ = wdf.Circuit(P1, root, Cap)
    for call in (lambda x: circ(x), lambda x: circ.mse(x, torch.zeros(16, 2)), lambda x: circ.mse_esr(x, torch.zeros(16, 2)),
                 lambda x: circ.loss(x, torch.zeros(16, 2))):
        with pytest.raises(binding.WdfHipError, match="two-different-diode clipper's own kernels"):
            call(_x(torch))
    seq = wdf.Circuit(P1, root, Cap, per_sequence_R=Vs)
    with pytest.raises(binding.WdfHipError, match="per_sequence_R"):
        seq(_x(torch, 2))


def test_pot_channel_and_streamed_routes_refuse_before_the_device(monkeypatch):
    import tf_wdf as wdf
    import torch
    from wdf_hip import binding
    _no_gpu(monkeypatch)
    Vs, Cap, P1 = _clipper(wdf)
    dp = wdf.DiodePair(P1, 4.352e-9, Vt=0.0493, trainable=True)
    pot = wdf.Circuit(P1, dp, Cap, per_sample_R=Vs)
    with pytest.raises(binding.WdfHipError, match="per_sample_R"):
        pot(_x(torch, 2))
    # off the clipper topology a resistance channel is the streamed-coefficient route
    R1 = wdf.Resistor(33.0e3, True)
    Vs2 = wdf.ResistiveVoltageSource(1.0e3, trainable=True)
    C2 = wdf.Capacitor(22.0e-9, FS, True)
    top = wdf.Parallel(R1, wdf.Series(Vs2, C2))
    dp2 = wdf.DiodePair(top, 4.352e-9, Vt=0.0493, trainable=True)
    streamed = wdf.Circuit(top, dp2, R1, per_sample_R=Vs2)
    for call in (lambda x: streamed(x), lambda x: streamed.mse(x, torch.zeros(16, 2))):
        with pytest.raises(binding.WdfHipError, match="streamed-coefficient"):
            call(_x(torch, 2))


def test_a_plain_input_is_not_refused_anywhere(monkeypatch):
    """the same circuits with a plain x go on to ask for the device: nothing is refused for them"""
    import tf_wdf as wdf
    import torch
    from wdf_hip import binding

    class Reached(Exception):
        pass

    def reached():
        raise Reached()

    monkeypatch.setattr(binding, "require_gpu", reached)
    Vs, Cap, P1 = _clipper(wdf)
    root = wdf.AsymDiodePair(P1, 2.52e-9, 2.0e-6, trainable=True)
    circ = wdf.Circuit(P1, root, Cap)
    with pytest.raises(Reached):
        circ(torch.zeros((2, 16)))
    with torch.no_grad(), pytest.raises(Reached):
        circ(_x(torch))                                                        # grad mode off: no gradient is wanted, none is dropped
