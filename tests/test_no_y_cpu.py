"""CPU: the one-pass steps without the y store -- WDF_NO_Y_STORE on wdf_clipper_step_mse_tp / _esr_tp and the exports
wdf_ss_lin_step_mse_noy / _esr_noy -- as the header, the binding's table, the export map and the built library declare them,
and every refusal that happens before a launch.  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOY = ("wdf_ss_lin_step_mse_noy", "wdf_ss_lin_step_esr_noy")
NO_Y = 1 << 7
E, EUNSUP = -1, -3


@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wdf_hip.h")).read(), flags=re.S)


def test_header_declares_the_flag_and_the_exports():
    from wdf_hip import binding
    src = header()
    m = re.search(r"\bWDF_NO_Y_STORE\s*=\s*1\s*<<\s*(\d+)", src)
    assert m and 1 << int(m.group(1)) == NO_Y == binding.WDF_NO_Y_STORE
    others = {n: 1 << int(s) for n, s in re.findall(r"\b(WDF_[A-Z0-9_]+)\s*=\s*1\s*<<\s*(\d+)", src) if n != "WDF_NO_Y_STORE"}
    assert NO_Y not in others.values(), others                      # a bit of its own
    for name in NOY:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    assert re.search(r"#define\s+WDF_HIP_ABI_VERSION\s+6\b", open(os.path.join(REPO, "include", "wdf_hip.h")).read())


def test_noy_signatures_are_their_bases_without_y():
    """The header's parameter lists: the twin's is the base's with the one parameter named y taken out; the binding's table agrees."""
    from wdf_hip import binding
    src = header()

    def params(name):
        args = re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", src).group(1)
        return [" ".join(a.split()) for a in args.split(",")]

    for name in NOY:
        base = name[:-len("_noy")]
        assert "float* y" in params(base)
        assert params(name) == [p for p in params(base) if p != "float* y"]
        at = params(base).index("float* y")
        rb, ab = binding.SIGNATURES[base]
        assert binding.SIGNATURES[name] == (rb, ab[:at] + ab[at + 1:])


def test_table_export_map_and_library_agree(lib):
    from wdf_hip import binding
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    emap = open(os.path.join(REPO, "differentiable-wdfs_amd", "csrc", "exports.map")).read()
    globs = re.search(r"global:\s*([^;]+);", emap).group(1).split()
    for name in NOY:
        assert name in binding.SIGNATURES and name in binding.EXPORTED_SYMBOLS
        assert name in exported
        assert any(re.fullmatch(g.replace("*", ".*"), name) for g in globs), (name, globs)
        assert hasattr(lib, name)
    assert lib.wdf_abi_version() == 6


def test_clipper_flag_refusals_without_gpu(lib):
    """The flag with a y handed in: -1 and a message that names y, on both entry points; without the flag a null y is refused as
    before; every other entry point keeps refusing the bit."""
    one = C.c_void_p(16)     # never dereferenced: validation fails first

    def call_mse(y, flags, target=one):
        return lib.wdf_clipper_step_mse_tp(one, None, one, 48000.0, 1, 1, target, 1.0, 0, y, None, None, 128, 256, 2, 32, 1e-6, one, one, None,
                                           0, one, one, 0, None, None, None, None, 0.9, 0.999, 1e-7, None, None, flags, None)

    def call_esr(y, flags, target=one):
        return lib.wdf_clipper_step_esr_tp(one, None, one, 48000.0, 1, 1, target, 1000.0, 2.2e-16, 50, y, None, None, 128, 256, 2, 32, 1e-6,
                                           one, one, None, 0, one, None, None, None, None, None, None, 0.9, 0.999, 1e-7, None, None, flags,
                                           None)

    for call in (call_mse, call_esr):
        assert call(one, NO_Y) == E
        msg = lib.wdf_last_error().decode()
        assert re.search(r"\by\b", msg) and "WDF_NO_Y_STORE" in msg, msg
        assert call(one, NO_Y | 1) == E and re.search(r"\by must be NULL\b", lib.wdf_last_error().decode())
        assert call(None, 0) == E and b"null" in lib.wdf_last_error()          # without the flag: as before
        # with the flag and no y the other checks still run: a null target is the next refusal, not a launch
        assert call(None, NO_Y, target=None) == E and b"null" in lib.wdf_last_error()
        assert call(None, NO_Y | (1 << 8)) == E and b"unknown flag" in lib.wdf_last_error()
    f = lib.wdf_clipper_fwd
    assert f(one, None, one, 48000.0, 1, 1, one, None, None, None, 4, 4, NO_Y, None) == E and b"unknown flag" in lib.wdf_last_error()
    assert lib.wdf_clipper_fwd_tp(one, None, one, 48000.0, 1, 1, one, None, None, None, 64, 64, 2, 32, 1e-6, one, one, NO_Y, None) == E
    assert b"unknown flag" in lib.wdf_last_error()
    assert lib.wdf_clipper_bwd_mse_tp(one, None, one, 48000.0, 1, 1, one, one, one, 1.0, one, one, one, None, 0, 64, 64, 2, NO_Y, None) == E
    assert b"unknown flag" in lib.wdf_last_error()


def _lin_calls(lib):
    one = C.c_void_p(16)
    two = C.c_void_p(32)

    def mse(noy, x=one, target=one, ws=one, out=one, ns=1, ni=1, B=64, T=64, K=2, n_params=2, z0=None, zT=None):
        y = () if noy else (one,)
        fn = lib.wdf_ss_lin_step_mse_noy if noy else lib.wdf_ss_lin_step_mse
        return fn(x, one, one, n_params, ns, ni, target, 1.0, *y, ws, out, None, None, B, T, K, z0, zT, None)

    def esr(noy, x=one, target=one, ws=one, sums=one, g=one, ns=1, ni=1, B=64, T=64, K=2, n_params=2, z0=None, zT=None, skip=0, n=100.0,
            eps=0.0):
        y = () if noy else (one,)
        fn = lib.wdf_ss_lin_step_esr_noy if noy else lib.wdf_ss_lin_step_esr
        return fn(x, one, one, n_params, ns, ni, target, n, eps, skip, *y, ws, sums, g, None, None, B, T, K, z0, zT, None)

    return one, two, mse, esr


def test_lin_noy_refusals_match_their_bases_without_gpu(lib):
    one, two, mse, esr = _lin_calls(lib)
    bad = [dict(x=None), dict(target=None), dict(ws=None), dict(z0=two, zT=two), dict(ns=3), dict(ns=-1), dict(ni=0), dict(ni=3),
           dict(n_params=0), dict(n_params=16), dict(B=0), dict(T=0), dict(K=0)]
    for kw in bad:
        for fn in (mse, esr):
            base = fn(False, **kw)
            assert base in (E, EUNSUP), kw
            assert fn(True, **kw) == base, kw
            assert lib.wdf_last_error() != b""
    assert mse(True, ns=3) == EUNSUP and esr(True, ni=3) == EUNSUP
    assert mse(True, out=None) == mse(False, out=None) == E
    for kw in (dict(skip=-1), dict(skip=64), dict(n=0.0), dict(n=-1.0), dict(eps=-1.0), dict(sums=None, g=None)):
        assert esr(True, **kw) == esr(False, **kw) == E, kw
    assert esr(True, sums=None, g=None) == E and b"both null" in lib.wdf_last_error()
    assert mse(True, z0=two, zT=two) == E and b"wdf_ss_lin_step_mse_noy" in lib.wdf_last_error()
    assert esr(True, z0=two, zT=two) == E and b"wdf_ss_lin_step_esr_noy" in lib.wdf_last_error()


def test_binding_refuses_y_with_store_y_false_without_gpu():
    """Before anything else is looked at: no GPU, no library call, no allocation."""
    import torch
    from wdf_hip import binding
    y = torch.zeros((4, 4))
    x = torch.zeros((4, 4))
    calls = [lambda: binding.clipper_step_mse_tp(x, x, 48000.0, x, 1.0, 1, 0, y=y, store_y=False),
             lambda: binding.clipper_step_esr_tp(x, x, 48000.0, x, 16.0, 0.0, 0, 1, 0, y=y, store_y=False),
             lambda: binding.ss_lin_step_mse(x, x, x, x, 1.0, 1, y=y, store_y=False),
             lambda: binding.ss_lin_step_esr(x, x, x, x, 0, 1, y=y, store_y=False)]
    for call in calls:
        with pytest.raises(binding.WdfHipError, match=r"y= .*store_y=False"):
            call()


def test_engine_and_circuit_take_store_output():
    import inspect
    from wdf_hip import engine, lowering
    assert inspect.signature(engine.MseStep.__init__).parameters["store_output"].default is True
    assert inspect.signature(lowering.Circuit.mse).parameters["store_output"].default is True
    assert inspect.signature(lowering.Circuit.mse_esr).parameters["store_output"].default is True
