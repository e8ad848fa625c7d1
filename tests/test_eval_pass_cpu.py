"""CPU: the clipper's loss-only evaluation pass -- wdf_clipper_eval_tp, _ws_bytes, _ws_init -- as the header, the binding's table,
the export map and the built library declare it, every refusal that happens before a HIP call (on pointers that are never
dereferenced), and the `grad` keyword of Circuit.mse / mse_esr.  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wdf_clipper_eval_tp_ws_bytes", "wdf_clipper_eval_tp_ws_init", "wdf_clipper_eval_tp")
TM, GENERAL, ONE_PER_LANE, R_PER_SEQ, NO_Y = 1 << 0, 1 << 3, 1 << 5, 1 << 6, 1 << 7
E = -1


@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wdf_hip.h")).read(), flags=re.S)


def test_header_table_export_map_and_library_agree(lib):
    from wdf_hip import binding
    src = header()
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    emap = open(os.path.join(REPO, "differentiable-wdfs_amd", "csrc", "exports.map")).read()
    globs = re.search(r"global:\s*([^;]+);", emap).group(1).split()
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", src), name
        assert name in binding.SIGNATURES and name in binding.EXPORTED_SYMBOLS
        assert name in exported
        assert any(re.fullmatch(g.replace("*", ".*"), name) for g in globs), (name, globs)
        assert hasattr(lib, name)
    # the header's parameter list against the table's, parameter by parameter
    args = [" ".join(a.split()) for a in re.search(r"\bwdf_clipper_eval_tp\s*\(([^()]*)\)\s*;", src).group(1).split(",")]
    kinds = {"float": C.c_float, "double": C.c_double, "int": C.c_int, "int64_t": C.c_int64}
    want = [C.c_void_p if "*" in a else kinds[a.split()[0]] for a in args]
    assert binding.SIGNATURES["wdf_clipper_eval_tp"] == (C.c_int, want)
    assert "const float* theta" in args and "double* sums" in args          # no optimizer: theta is const; sums are doubles
    assert binding.SIGNATURES["wdf_clipper_eval_tp_ws_bytes"] == (C.c_size_t, [C.c_int64, C.c_int])


def test_abi_version_stays_6(lib):
    assert lib.wdf_abi_version() == 6
    assert re.search(r"#define\s+WDF_HIP_ABI_VERSION\s+6\b", open(os.path.join(REPO, "include", "wdf_hip.h")).read())


def _call(lib):
    one = C.c_void_p(16)     # never dereferenced: validation fails first

    def call(x=one, r=None, theta=one, fs=48000.0, n_up=1, n_down=1, target=one, n=1000.0, eps=2.2e-16, skip=50, y=one, B=128, T=256,
             K=2, warmup=32, tol=1e-6, ws=one, status=one, state=None, mwt=0, sums=one, loss3=None, flags=0):
        return lib.wdf_clipper_eval_tp(x, r, theta, fs, n_up, n_down, target, n, eps, skip, y, None, None, B, T, K, warmup, tol, ws, status,
                                       state, mwt, sums, loss3, flags, None)
    return one, call


def test_every_refusal_is_minus_one_with_a_message(lib):
    one, call = _call(lib)
    bad = [dict(x=None), dict(theta=None), dict(target=None), dict(ws=None), dict(status=None), dict(sums=None),       # null pointers
           dict(skip=-1), dict(skip=256), dict(skip=1000),                                                               # skip outside [0, T)
           dict(n=0.0), dict(n=-3.0), dict(eps=-1.0e-9),
           dict(K=0), dict(K=5), dict(K=9),                        # counts wdf_clipper_tp_chunks(256, .) does not return (4 and 8)
           dict(flags=R_PER_SEQ),                                  # one r per sequence without an r
           dict(B=0), dict(T=0), dict(fs=0.0), dict(n_up=0), dict(n_down=17), dict(warmup=-1), dict(tol=-1.0),
           dict(state=one, mwt=0), dict(state=one, mwt=33), dict(state=one, mwt=9)]                                      # 9 x 16 > the 128-step chunk
    for kw in bad:
        lib.wdf_last_error()
        assert call(**kw) == E, kw
        assert lib.wdf_last_error() not in (None, b""), kw
    assert lib.wdf_clipper_tp_chunks(256, 5) == 4 and lib.wdf_clipper_tp_chunks(256, 9) == 8
    assert call(K=5) == E and b"wdf_clipper_tp_chunks" in lib.wdf_last_error()
    assert call(skip=256) == E and b"skip" in lib.wdf_last_error()
    assert call(sums=None) == E and b"null" in lib.wdf_last_error()
    assert call(n=0.0) == E and b"n_global" in lib.wdf_last_error()
    assert call(eps=-1.0) == E and b"eps_energy" in lib.wdf_last_error()
    assert call(flags=R_PER_SEQ) == E and b"WDF_R_PER_SEQUENCE" in lib.wdf_last_error()


def test_unknown_flags(lib):
    one, call = _call(lib)
    for flags in (NO_Y, 1 << 8, NO_Y | TM, (1 << 8) | GENERAL, 1 << 1, 1 << 4):
        assert call(flags=flags) == E, flags
        assert b"unknown flag" in lib.wdf_last_error(), flags
        assert call(flags=flags, y=None) == E and b"unknown flag" in lib.wdf_last_error()      # (y = NULL is how no y is said)


def test_workspace_size(lib):
    for K in (1, 2, 32):
        assert lib.wdf_clipper_eval_tp_ws_bytes(0, K) == 0
    assert lib.wdf_clipper_eval_tp_ws_bytes(128, 0) == 0
    a, b = lib.wdf_clipper_eval_tp_ws_bytes(128, 4), lib.wdf_clipper_eval_tp_ws_bytes(256, 4)
    assert 0 < a < b
    # no records, no group areas: smaller than the training step's
    assert lib.wdf_clipper_eval_tp_ws_bytes(8192, 32) < lib.wdf_clipper_step_mse_tp_ws_bytes(8192, 32)
    assert lib.wdf_clipper_eval_tp_ws_init(None, 128, 4, None) == E


def test_binding_refuses_y_with_store_y_false_without_gpu():
    """Before anything else is looked at: no GPU, no library call, no allocation."""
    import torch
    from wdf_hip import binding
    x = torch.zeros((4, 4))
    with pytest.raises(binding.WdfHipError, match=r"y= .*store_y=False"):
        binding.clipper_eval_tp(x, x, 48000.0, x, 16.0, 0.0, 0, 1, 0, y=torch.zeros((4, 4)), store_y=False)


def test_circuit_losses_take_grad_defaulting_to_true():
    import inspect
    from wdf_hip import engine, lowering
    assert inspect.signature(lowering.Circuit.mse).parameters["grad"].default is True
    assert inspect.signature(lowering.Circuit.mse_esr).parameters["grad"].default is True
    assert callable(engine.MseStep.eval_fused)
