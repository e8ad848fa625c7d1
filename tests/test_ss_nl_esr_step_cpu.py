"""CPU: the one-pass MSE + ESR step of small diode-root trees (wdf_ss_nl_step_esr, csrc/wdf_ss_nl_step.h) as far as it goes
without a GPU: the two new symbols in the header, the library and the binding; the workspace size; the argument checks that
come before any device work; and the conditions under which Circuit.mse_esr takes the step (a stub stands for the resident
tree object)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 48000
NEW = ("wdf_ss_nl_step_esr_ws_bytes", "wdf_ss_nl_step_esr")


@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


def test_header_library_and_binding_name_the_two_symbols(lib):
    from wdf_hip import binding
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wdf_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in binding.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert "wdf_*" in open(os.path.join(REPO, "differentiable-wdfs_amd", "csrc", "exports.map")).read()
    vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
    assert lib.wdf_ss_nl_step_esr_ws_bytes.restype is C.c_size_t
    assert list(lib.wdf_ss_nl_step_esr_ws_bytes.argtypes) == [ci, ci, i64, i64, ci]
    assert lib.wdf_ss_nl_step_esr.restype is ci
    # wdf_ss_nl_step_mse's arguments with (int64 skip, double eps) where gscale was
    want = list(lib.wdf_ss_nl_step_mse.argtypes)
    at = want.index(C.c_float)
    want[at:at + 1] = [i64, C.c_double]
    assert list(lib.wdf_ss_nl_step_esr.argtypes) == want
    assert lib.wdf_abi_version() == 6


def test_workspace_size(lib):
    f, g = lib.wdf_ss_nl_step_esr_ws_bytes, lib.wdf_ss_nl_step_ws_bytes
    for ns, ni in [(1, 1), (1, 2), (2, 1)]:
        for B, T in [(1, 40), (130, 1500), (8192, 4096)]:
            sizes = [f(ns, ni, B, T, k) for k in (1, 2, 4, 8)]
            assert all(s > 0 for s in sizes)
            assert all(b > a for a, b in zip(sizes, sizes[1:])) or T < 64, sizes
            assert all(f(ns, ni, B, T, k) >= g(ns, ni, B, T, k) for k in (1, 2, 4, 8))
    assert f(1, 1, 130, 1500, 8) > f(1, 1, 130, 1500, 4) > f(1, 1, 130, 1500, 1)
    assert f(3, 1, 128, 1024, 4) == 0 and b"ns in 1..2" in lib.wdf_last_error()
    assert f(1, 3, 128, 1024, 4) == 0
    # two states WITH two sources: the MSE step has kernels, the MSE + ESR step has none
    assert g(2, 2, 128, 1024, 4) > 0 and f(2, 2, 128, 1024, 4) == 0 and b"ns * ni <= 2" in lib.wdf_last_error()
    assert f(1, 1, 0, 1024, 4) == 0 and f(1, 1, 128, 1024, 0) == 0


def test_arguments_are_checked_before_any_device_work(lib):
    one = C.c_void_p(16)                                    # never dereferenced: validation fails first
    esr = lib.wdf_ss_nl_step_esr

    def call(x=one, ns=1, ni=1, skip=50, eps=1e-16, loss3=one, T=1024, n_tree=3, ws=one):
        return esr(x, one, one, one, n_tree, ns, ni, 1, 1, one, skip, eps, one, ws, one, loss3, 128, T, 4, None)

    assert call(skip=1024) == -1 and b"skip" in lib.wdf_last_error()
    assert call(skip=-1) == -1 and b"skip" in lib.wdf_last_error()
    assert call(skip=5000) == -1
    assert call(x=None) == -1 and b"null" in lib.wdf_last_error()
    assert call(loss3=None) == -1 and call(ws=None) == -1
    assert call(eps=-1.0) == -1
    assert call(ns=3) == -3 and call(ni=3) == -3 and call(ns=0) == -3          # WDF_EUNSUPPORTED
    assert call(ns=2, ni=2) == -3 and b"ns * ni <= 2" in lib.wdf_last_error()
    assert call(n_tree=0) == -1 and call(T=0) == -1


# ---- Circuit.mse_esr's routing ------------------------------------------------------------------------------------------
def hpf(wdf, root="diode", **kw):
    R = wdf.Resistor(33.0e3, True)
    Vs = wdf.ResistiveVoltageSource(1.0e3, trainable=True)
    Cp = wdf.Capacitor(22.0e-9, FS, True)
    top = wdf.Parallel(R, wdf.Series(Vs, Cp))
    if root == "diode":
        r = wdf.DiodePair(top, 4.352e-9, Vt=25.85e-3 * 1.906, nDiodes=1.0, N_up=2, N_down=3, trainable=True)
    else:
        r = wdf.IdealVoltageSource()
    return wdf.Circuit(top, r, R, **kw)


def test_routing_predicate():
    import tf_wdf as wdf
    x, t = torch.zeros((4, 256)), torch.zeros((256, 4))
    stub = object()                                          # stands for the resident tree object to_device() would make
    circ = hpf(wdf)
    assert (circ.root_kind, circ.ns, circ.ni) == ("DiodePair", 1, 1)
    assert circ._nl_step_tree(x, t, 50) is None              # not resident: today's path
    circ._tree = stub
    assert circ._nl_step_tree(x, t, 50) is stub              # resident HPF clipper: the step
    assert circ._nl_step_tree(x, t, 0) is stub and circ._nl_step_tree(x, t, 255) is stub
    assert circ._nl_step_tree(x, t, 256) is None and circ._nl_step_tree(x, t, 1000) is None and circ._nl_step_tree(x, t, -1) is None
    assert circ._nl_step_tree(x, t, 50, z0=torch.zeros((1, 4))) is None
    assert circ._nl_step_tree(x, t, 50, carry_state=True) is None
    assert circ._nl_step_tree(x.numpy(), t, 50) is None and circ._nl_step_tree(x, np.zeros((256, 4)), 50) is None
    generic = hpf(wdf, force_generic=True)
    generic._tree = stub
    assert generic._nl_step_tree(x, t, 50) is None
    lin = hpf(wdf, root="source")
    lin._tree = stub
    assert lin.root_kind == "IdealVoltageSource" and lin._nl_step_tree(x, t, 50) is None
    # two capacitors WITH two sources: no MSE + ESR kernels (WDF_EUNSUPPORTED) -> today's path; either alone -> the step
    Va, Vb = wdf.ResistiveVoltageSource(1.0e3, trainable=True), wdf.ResistiveVoltageSource(4.7e3, trainable=True)
    Ca, Cb = wdf.Capacitor(4.7e-8, FS, True), wdf.Capacitor(2.2e-8, FS, True)
    top = wdf.Parallel(wdf.Series(Va, Ca), wdf.Series(Vb, Cb))
    big = wdf.Circuit(top, wdf.DiodePair(top, 2.52e-9, Vt=25.85e-3, nDiodes=1.752, trainable=True), Ca)
    big._tree = stub
    assert (big.ns, big.ni) == (2, 2) and big._nl_step_tree(torch.zeros((4, 256, 2)), t, 50) is None


def test_resident_entries_are_keyed_on_loss_and_skip(monkeypatch):
    """An MSE and an ESR loop over the same (x, target) do not share a workspace: _LinResident.entry keys its entries on
    (loss, skip) too.  The planning launch is stubbed out; everything else is entry()'s own code."""
    from types import SimpleNamespace
    from wdf_hip import lowering
    from wdf_hip.tensor_cache import EntryCache
    res = lowering._LinResident.__new__(lowering._LinResident)
    res.circ = SimpleNamespace(ns=1, ni=1, root_kind="DiodePair")
    res.pb = SimpleNamespace(block=torch.zeros(5), n=5)
    res.cache = EntryCache()
    planned = []

    def plan(B, T, k, dev, cold_floor=0):
        planned.append((B, T, k))
        return torch.zeros(8, dtype=torch.uint8)
    monkeypatch.setattr(res, "_plan_nl", plan)
    x, t = torch.zeros((4, 256)), torch.zeros((256, 4))
    mse = res.entry(x, t)
    esr50 = res.entry(x, t, "mse+esr", 50)
    esr0 = res.entry(x, t, "mse+esr", 0)
    assert mse is not esr50 and esr50 is not esr0 and mse is not esr0 and len(planned) == 3 and len(res.cache) == 3
    assert res.entry(x, t) is mse and res.entry(x, t, "mse+esr", 50) is esr50 and res.entry(x, t, "mse+esr", 0) is esr0
    assert len(planned) == 3
    assert mse["ws"] is not esr50["ws"] and mse["y"] is not esr50["y"]
    assert (esr50["loss"], esr50["skip"], esr0["skip"], mse["loss"]) == ("mse+esr", 50, 0, "mse")
    assert mse["ring"].shape[1] == 2 + 5 and esr50["ring"].shape[1] == 4 + 5      # {S, gradients} + loss / + {mse, esr, mse + esr}
