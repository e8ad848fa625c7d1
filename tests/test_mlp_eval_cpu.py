"""CPU: the MLP-root clipper's loss-only evaluation pass -- wdf_clipper_mlp_eval -- as the header, the binding's table, the export
map and the built library declare it, every refusal that happens before a HIP call (on pointers that are never dereferenced), and
the routing flag of Circuit.mse_esr(..., grad=False).  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wdf_clipper_mlp_eval"
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
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", src)
    assert NAME in binding.SIGNATURES and NAME in binding.EXPORTED_SYMBOLS
    assert NAME in exported
    assert any(re.fullmatch(g.replace("*", ".*"), NAME) for g in globs), globs
    assert hasattr(lib, NAME)
    # the header's parameter list against the table's, parameter by parameter
    args = [" ".join(a.split()) for a in re.search(r"\b" + NAME + r"\s*\(([^()]*)\)\s*;", src).group(1).split(",")]
    kinds = {"float": C.c_float, "double": C.c_double, "int": C.c_int, "int64_t": C.c_int64}
    want = [C.c_void_p if "*" in a else kinds[a.split()[0]] for a in args]
    assert len(want) == 21
    assert binding.SIGNATURES[NAME] == (C.c_int, want)
    assert [a.split()[-1].lstrip("*") for a in args] == ["x", "p", "lr", "theta2", "w", "hidden", "n_layers", "activation", "fs", "target",
                                                         "skip", "n_global", "eps_energy", "y", "state", "B", "T", "n_items", "sums", "loss3",
                                                         "stream"]
    assert "const float* w" in args and "double* sums" in args             # no optimizer: w is const; sums are doubles
    # the head is the resident step's own, up to y
    assert binding.SIGNATURES[NAME][1][:14] == binding.SIGNATURES["wdf_clipper_mlp_step"][1][:14]


def test_abi_version_stays_6(lib):
    assert lib.wdf_abi_version() == 6
    assert re.search(r"#define\s+WDF_HIP_ABI_VERSION\s+6\b", open(os.path.join(REPO, "include", "wdf_hip.h")).read())


def _call(lib):
    one = C.c_void_p(16)     # never dereferenced: validation fails first; 16-byte aligned
    odd = C.c_void_p(20)

    def call(x=one, p=one, lr=one, theta2=one, w=one, hidden=16, n_layers=3, activation=0, fs=48000.0, target=one, skip=50, n=1000.0,
             eps=2.2e-16, y=one, state=one, B=32, T=256, n_items=4, sums=one, loss3=None):
        return lib.wdf_clipper_mlp_eval(x, p, lr, theta2, w, hidden, n_layers, activation, fs, target, skip, n, eps, y, state, B, T, n_items,
                                        sums, loss3, None)
    return one, odd, call


def test_every_refusal_is_minus_one_with_a_message(lib):
    one, odd, call = _call(lib)
    bad = [dict(x=None), dict(w=None), dict(target=None), dict(state=None), dict(sums=None),                         # null pointers
           dict(p=None), dict(lr=None),                                                                                # p and lr go together
           dict(p=None, lr=None, theta2=None),                                                                         # static R without theta2
           dict(fs=0.0), dict(fs=-1.0), dict(skip=-1), dict(n=0.0), dict(n=-3.0), dict(eps=-1.0e-9),
           dict(x=odd), dict(p=odd), dict(lr=odd)]                                                                     # not 16-byte aligned
    for kw in bad:
        lib.wdf_last_error()
        assert call(**kw) == E, kw
        assert lib.wdf_last_error() not in (None, b""), kw
    assert call(sums=None) == E and b"null" in lib.wdf_last_error()
    assert call(p=None) == E and b"go together" in lib.wdf_last_error()
    assert call(p=None, lr=None, theta2=None) == E and b"theta2" in lib.wdf_last_error()
    assert call(skip=-1) == E and b"skip" in lib.wdf_last_error()
    assert call(n=0.0) == E and b"n_global" in lib.wdf_last_error()
    assert call(eps=-1.0) == E and b"eps_energy" in lib.wdf_last_error()
    assert call(x=odd) == E and b"aligned" in lib.wdf_last_error()


def test_what_the_step_refuses_of_a_shape_the_pass_refuses(lib):
    one, odd, call = _call(lib)
    # the network, T, the plan's size -- step_check_shape's rules, all WDF_EINVAL here
    for kw in [dict(hidden=12), dict(n_layers=2), dict(n_layers=6), dict(activation=2), dict(T=250), dict(T=0), dict(B=0), dict(n_items=1),
               dict(B=33, n_items=2)]:
        lib.wdf_last_error()
        assert call(**kw) == E, kw
        assert lib.wdf_last_error() not in (None, b""), kw
        assert lib.wdf_clipper_mlp_step_state_bytes(kw.get("hidden", 16), kw.get("n_layers", 3), kw.get("B", 32), kw.get("T", 256),
                                                    kw.get("n_items", 4), 1) == 0 or "activation" in kw


def test_routing_flag_and_the_pass_class_exist():
    from wdf_hip import lowering, mlp_root
    assert isinstance(lowering.MLP_EVAL_PASS_SERVES, bool)
    assert issubclass(mlp_root.MlpEvalPass, mlp_root._MlpResident) and issubclass(mlp_root.MlpTrainStep, mlp_root._MlpResident)
    for name in ("run", "read", "set_wcol", "set_controller", "freeze", "warmup_peaks", "replan", "of"):
        assert callable(getattr(mlp_root.MlpEvalPass, name)), name
    # shared through the base, not copied
    for name in ("read", "set_wcol", "set_controller", "freeze", "warmup_peaks", "replan"):
        assert getattr(mlp_root.MlpEvalPass, name) is getattr(mlp_root.MlpTrainStep, name), name
