"""CPU: the one-pass MSE and MSE + ESR step of small trees under the two-different-diode root (wdf_ss_asym_step_mse / _esr,
csrc/wdf_ss_asym_step.h) as far as it can be checked without a GPU -- the symbols in the header, the export list and the
library; the workspace size; the C ABI's argument validation (through ctypes: no pointer is dereferenced, validation fails
first); the conditions the GPU tests' references rest on (tests/ss_asym_step_cases.py); what Circuit._asym_step_tree refuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ss_asym_step_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wdf_ss_asym_step_ws_bytes", "wdf_ss_asym_step_esr_ws_bytes", "wdf_ss_asym_step_mse", "wdf_ss_asym_step_esr")
BUILT = [(1, 1), (1, 2), (2, 1), (2, 2)]            # both losses; three states are not built (the chunk kernel spills)


@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


def test_symbols_declared_exported_and_listed(lib):
    from wdf_hip import binding
    hdr = open(os.path.join(REPO, "include", "wdf_hip.h")).read()
    exp = open(os.path.join(REPO, "differentiable-wdfs_amd", "csrc", "exports.map")).read()
    dyn = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH], text=True)
    assert re.search(r"global:\s*wdf_\*;", exp)                  # the export list is the wdf_ prefix
    for name in NAMES:
        assert re.search(r"^(int|size_t)\s+%s\s*\(" % name, hdr, re.M), name
        assert re.search(r"\bT %s$" % name, dyn, re.M), name
        assert name in binding.EXPORTED_SYMBOLS, name
    assert "#define WDF_HIP_ABI_VERSION 6" in hdr and lib.wdf_abi_version() == 6


def test_workspace_size(lib):
    f, fe = lib.wdf_ss_asym_step_ws_bytes, lib.wdf_ss_asym_step_esr_ws_bytes
    for ns, ni in BUILT:
        assert f(ns, ni, 64, 64, 1) > 0 and fe(ns, ni, 64, 64, 1) == f(ns, ni, 64, 64, 1), (ns, ni)
        assert 0 < f(ns, ni, 64, 4096, 1) < f(ns, ni, 64, 4096, 2) < f(ns, ni, 64, 4096, 8) < f(ns, ni, 130, 4096, 8) \
            < f(ns, ni, 8192, 4096, 8), (ns, ni)
        assert f(ns, ni, 0, 64, 1) == 0 and f(ns, ni, 64, 0, 1) == 0 and f(ns, ni, 64, 64, 0) == 0
        assert f(ns, ni, 64, 64, 5) == 0                         # 5 chunks do not tile 64 steps in 8-step units
    for ns, ni in [(3, 1), (3, 2), (0, 1), (4, 1), (1, 0), (1, 3)]:
        assert f(ns, ni, 64, 64, 1) == 0 and fe(ns, ni, 64, 64, 1) == 0, (ns, ni)
    # the records alone: per sequence and chunk Psi, the nT tangents and H, HQ
    nt = 2 * 2 + 2 * 1 + 2 + 2 + 1 + 5
    assert f(2, 1, 8192, 4096, 16) >= 16 * (4 + nt * 2 + 4) * 8192 * 4
    from wdf_hip import binding
    assert binding.ss_asym_step_built(2, 2, "mse") and binding.ss_asym_step_built(2, 2, "mse_esr")
    assert not binding.ss_asym_step_built(3, 1, "mse") and not binding.ss_asym_step_built(3, 1, "mse_esr")


def _args(**kw):
    one = C.c_void_p(16)   # never dereferenced
    a = dict(x=one, coef=one, rootp=one, ns=1, ni=1, target=one, gscale=1.0, n_global=256.0, eps_energy=2.2e-16, skip=0, y=one,
             z0=None, zT=None, B=4, T=64, K=2, W=8, tol=1e-6, ws=one, status=one, out=one, sums=one, g=None, loss3=None)
    a.update(kw)
    return a


def _mse(lib, **kw):
    a = _args(**kw)
    rc = lib.wdf_ss_asym_step_mse(a["x"], a["coef"], a["rootp"], a["ns"], a["ni"], a["target"], a["gscale"], a["y"], a["z0"], a["zT"],
                                  a["B"], a["T"], a["K"], a["W"], a["tol"], a["ws"], a["status"], a["out"], None)
    return rc, lib.wdf_last_error()


def _esr(lib, **kw):
    a = _args(**kw)
    rc = lib.wdf_ss_asym_step_esr(a["x"], a["coef"], a["rootp"], a["ns"], a["ni"], a["target"], a["n_global"], a["eps_energy"],
                                  a["skip"], a["y"], a["z0"], a["zT"], a["B"], a["T"], a["K"], a["W"], a["tol"], a["ws"], a["status"],
                                  a["sums"], a["g"], a["loss3"], None)
    return rc, lib.wdf_last_error()


@pytest.mark.parametrize("arg", ["x", "coef", "rootp", "target", "y", "ws", "status", "out", "sums"])
def test_null_pointers_are_rejected(lib, arg):
    for call, own in [(_mse, "out"), (_esr, "sums")]:
        if arg in ("out", "sums") and arg != own:
            continue
        rc, err = call(lib, **{arg: None})
        assert rc == -1 and b"null" in err, (arg, rc, err)


def test_shared_arguments_are_rejected(lib):
    for call in (_mse, _esr):
        for kw, code, word in [(dict(ns=0), -3, b"ns in [1,3]"), (dict(ns=4), -3, b"ns in [1,3]"), (dict(ni=0), -3, b"ni in [1,2]"),
                               (dict(ni=3), -3, b"ni in [1,2]"), (dict(ns=3), -3, b"not built"), (dict(ns=3, ni=2), -3, b"not built"),
                               (dict(B=0), -1, b"B and T"), (dict(T=-1), -1, b"B and T"),
                               (dict(K=0), -1, b"n_chunks"), (dict(K=70000), -1, b"n_chunks"),
                               (dict(K=5, T=64), -1, b"wdf_ss_tp_chunks"), (dict(W=-1), -1, b"warmup"),
                               (dict(W=40, K=2, T=64), -1, b"longer than a chunk"), (dict(W=33, K=2, T=64), -1, b"longer than a chunk"),
                               (dict(tol=-1.0), -1, b"tol"), (dict(tol=float("nan")), -1, b"tol"),
                               (dict(ws=C.c_void_p(20)), -1, b"aligned"),
                               (dict(z0=C.c_void_p(32), zT=C.c_void_p(32)), -1, b"alias")]:
            rc, err = call(lib, **kw)
            assert rc == code and word in err, (kw, rc, err)


def test_loss_arguments_are_rejected(lib):
    for kw, word in [(dict(n_global=0.0), b"n_global"), (dict(n_global=-4.0), b"n_global"), (dict(n_global=float("nan")), b"n_global"),
                     (dict(eps_energy=-1e-30), b"eps_energy"), (dict(skip=-1), b"skip"), (dict(skip=64), b"skip"),
                     (dict(skip=1000), b"skip"), (dict(loss3=C.c_void_p(64)), b"loss3")]:
        rc, err = _esr(lib, **kw)
        assert rc == -1 and word in err, (kw, rc, err)


# ---- the references the GPU tests stand on --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs(oracle):
    memo = {}

    def get(case):
        if case not in memo:
            memo[case] = sc.Reference(oracle, case)
        return memo[case]
    return get


@pytest.mark.parametrize("case", sc.ALL)
def test_teacher_and_balance_conditions(refs, case):
    """The target differs from the model's output (S > 0), the output carries energy (E > 0), and no gradient component is a
    sum of cancelling per-sequence terms, for MSE and for MSE + ESR at skip 50."""
    r = refs(case)
    for kind, skip in [("mse", 0), ("mse_esr", 50)]:
        S, E = r.sums(skip)
        g, bal = r.grad_and_balance(kind, skip)
        print(f"{case} {kind} skip {skip}: S = {S:.4g}, E = {E:.4g}, loss = {r.loss(kind, skip):.5g}, min balance = {bal.min():.3g}")
        assert S > 0.0 and E > 0.0
        assert np.all(np.isfinite(g)) and np.all(bal >= sc.BALANCE), (case, kind, bal)


def test_new_trees_have_the_sizes_they_cover_and_the_planner_speculates():
    """hpf2 (1,2), a (2,1), b (2,2); for these the planner cuts 1536 steps in two chunks (a contracting step at both ends of
    the root's slope); two_state does not speculate."""
    import tf_wdf
    from wdf_hip import lowering, binding
    want = {"hpf2": 712, "a": 760, "b": 760}
    for case in ("hpf2", "a", "b", "two_state"):
        circ, params = sc.BUILD[case](tf_wdf, "auto")
        assert (circ.ns, circ.ni) == sc.NS_NI[case] and circ._asym_generic
        assert len(params) == sc.REFS[case]()[2].size
        coef64, _ = circ.matrices()
        plan = lowering.plan_ss_time_parallel(coef64, circ.ns, circ.ni, binding.ROOT_ASYM_PAIR, 130, 1536)
        if case == "two_state":
            assert plan is None or plan.k_fwd == 1
        else:
            assert plan.k_fwd == 2 and plan.warmup == want[case], (case, plan)


def test_asym_step_tree_refuses_what_it_must():
    import tf_wdf
    import torch
    x, t = torch.zeros(4, 64), torch.zeros(64, 4)
    circ, _ = sc.BUILD["hpf"](tf_wdf)
    assert circ._asym_step_tree(x, t, "mse") and circ._asym_step_tree(x, t, "mse_esr", 0) and circ._asym_step_tree(x, t, "mse_esr", 63)
    assert circ._asym_step_tree(x.reshape(4, 64, 1), t, "mse")
    assert not circ._asym_step_tree(x, t, "mse_esr", 64) and not circ._asym_step_tree(x, t, "mse_esr", -1)      # skip out of range
    assert not circ._asym_step_tree(x.numpy(), t, "mse") and not circ._asym_step_tree(x, t.numpy(), "mse")       # tensors only
    assert not circ._asym_step_tree(torch.zeros(4, 64, 2), t, "mse")                                             # one source
    assert not circ._asym_step_tree(x, t, "mae")
    own, _ = sc.cases.clipper(tf_wdf, None, any_tree=False)                                                      # the clipper's own kernels
    assert not own._asym_generic and not own._asym_step_tree(x, t, "mse")
    Vs, Cc = tf_wdf.ResistiveVoltageSource(45.0e3), tf_wdf.Capacitor(4.7e-9, sc.FS)
    top = tf_wdf.Parallel(Vs, Cc)
    om = tf_wdf.Circuit(top, tf_wdf.AsymDiodePair(top, 4.352e-9, 2.0e-6, solver="omega_f32"), Cc)               # the closed form
    assert not om._asym_step_tree(x, t, "mse")
    three, _ = sc.BUILD["three_state"](tf_wdf)                                                                   # not built
    assert three._asym_generic and not three._asym_step_tree(x, t, "mse") and not three._asym_step_tree(x, t, "mse_esr", 0)
    two, _ = sc.BUILD["b"](tf_wdf)
    assert two._asym_step_tree(torch.zeros(4, 64, 2), t, "mse_esr", 5)
