"""CPU: the loss-only evaluation pass of linear trees (wdf_ss_lin_eval*, csrc/wdf_ss_lin_eval.h) as far as it goes without a GPU:
the two symbols in the header, the signature table, the library and the export map; the header's parameter lists against the
table's; every refusal that comes before any device work; the workspace size; the binding's own refusal of a wrong y; the routing
constant."""
import ctypes as C
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wdf_ss_lin_eval_ws_bytes", "wdf_ss_lin_eval")
WDF_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wdf_hip.h")).read(), flags=re.S)


def test_header_table_library_and_export_map_name_the_two_symbols(lib):
    from wdf_hip import binding
    src = header()
    dyn = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in binding.SIGNATURES and name in binding.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert name in exported, name
    assert "wdf_*" in open(os.path.join(REPO, "differentiable-wdfs_amd", "csrc", "exports.map")).read()
    assert lib.wdf_abi_version() == 6
    assert re.search(r"#define\s+WDF_HIP_ABI_VERSION\s+6\b", open(os.path.join(REPO, "include", "wdf_hip.h")).read())
    assert callable(binding.ss_lin_eval)


def ctype_class(decl):
    """one C parameter declaration -> the class of ctypes type the table must hold for it"""
    decl = decl.strip()
    if "*" in decl:
        return "pointer"
    word = re.sub(r"\b(const|unsigned)\b", "", decl).split()[0]
    return {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int32_t": C.c_int32}[word]


def table_class(t):
    return "pointer" if t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents") or issubclass(t, C._Pointer) else t


def test_the_headers_parameter_lists_equal_the_tables(lib):
    from wdf_hip import binding
    src = header()
    for name in NEW:
        m = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        want = [ctype_class(p) for p in m.group(2).split(",")]
        restype, argtypes = binding.SIGNATURES[name]
        assert [table_class(t) for t in argtypes] == want, name
        assert restype is {"size_t": C.c_size_t, "int": C.c_int}[m.group(1)]
    assert len(binding.SIGNATURES["wdf_ss_lin_eval"][1]) == 20 and len(binding.SIGNATURES["wdf_ss_lin_eval_ws_bytes"][1]) == 5


def test_every_refusal_comes_before_any_device_work(lib):
    one, two = C.c_void_p(16), C.c_void_p(32)               # never dereferenced: validation fails first
    ev = lib.wdf_ss_lin_eval

    def call(x=one, coef=one, ns=1, ni=1, target=one, skip=50, n_global=1000.0, eps=1e-16, gscale=1.0, y=one, ws=one, sums=one, loss3=one,
             loss_out=one, B=128, T=1024, k=4, z0=None, zT=None):
        return ev(x, coef, ns, ni, target, skip, n_global, eps, gscale, y, ws, sums, loss3, loss_out, B, T, k, z0, zT, None)

    def refused(what, **kw):
        rc = call(**kw)
        msg = lib.wdf_last_error()
        assert rc == WDF_EINVAL and msg, (kw, rc, msg)
        assert what in msg, (kw, msg)

    for name in ("x", "coef", "target", "ws"):
        refused(b"null", **{name: None})
    refused(b"null", sums=None, loss3=None, loss_out=None)
    for kw in (dict(ns=-1), dict(ns=3), dict(ni=0), dict(ni=3)):
        refused(b"ns in 0..2", **kw)
    refused(b"B, T", B=0)
    refused(b"B, T", T=0)
    refused(b"n_chunks", k=0)
    refused(b"n_chunks", k=-3)
    refused(b"skip", skip=1024)
    refused(b"skip", skip=-1)
    refused(b"skip", skip=5000)
    refused(b"n_global", n_global=0.0)
    refused(b"n_global", n_global=-1.0)
    refused(b"eps", eps=-1.0)
    refused(b"alias", z0=two, zT=two)


def test_workspace_size(lib):
    f = lib.wdf_ss_lin_eval_ws_bytes
    for ns, ni in [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2)]:
        by_k = [f(ns, ni, 8192, 2048, k) for k in (1, 2, 8, 32, 64)]
        assert all(s > 0 for s in by_k) and all(b > a for a, b in zip(by_k, by_k[1:])), (ns, ni, by_k)
        by_b = [f(ns, ni, B, 1501, 12) for B in (1, 70, 130, 8192)]
        assert all(b >= a for a, b in zip(by_b, by_b[1:])) and by_b[-1] > by_b[0], (ns, ni, by_b)
    assert f(2, 1, 130, 1501, 12) > f(1, 1, 130, 1501, 12) > f(0, 1, 130, 1501, 12)
    # no tangents: smaller than either step's
    assert 0 < f(1, 1, 8192, 4096, 32) < lib.wdf_ss_lin_step_ws_bytes(1, 1, 8192, 4096, 32) < lib.wdf_ss_lin_step_esr_ws_bytes(1, 1, 8192, 4096, 32)
    for bad in [(3, 1, 128, 1024, 4), (-1, 1, 128, 1024, 4), (1, 3, 128, 1024, 4), (1, 0, 128, 1024, 4), (1, 1, 0, 1024, 4), (1, 1, 128, 0, 4),
                (1, 1, 128, 1024, 0)]:
        assert f(*bad) == 0 and lib.wdf_last_error(), bad


def test_the_binding_refuses_a_wrong_y_without_a_gpu(lib):
    from wdf_hip import binding
    x, coef, target = torch.zeros((8, 1, 4)), torch.zeros(9), torch.zeros((8, 4))
    with pytest.raises(binding.WdfHipError, match="store_y=False"):
        binding.ss_lin_eval(x, coef, target, 1, y=torch.zeros((8, 4)), store_y=False)
    with pytest.raises(binding.WdfHipError, match=r"y must be a \[T,B\] = \[8, 4\] tensor"):
        binding.ss_lin_eval(x, coef, target, 1, y=torch.zeros((4, 8)))
    with pytest.raises(binding.WdfHipError, match="on x_tm's device"):
        binding.ss_lin_eval(x, coef, target, 1, y=torch.zeros((8, 4), device="meta"))
    with pytest.raises(binding.WdfHipError, match="y must be"):
        binding.ss_lin_eval(x, coef, target, 1, y=[[0.0] * 4] * 8)


def test_the_routing_constant_is_a_bool():
    from wdf_hip import lowering
    assert isinstance(lowering.LIN_EVAL_PASS_SERVES, bool)
    assert isinstance(lowering._LIN_EVAL_OCC, int) and lowering._LIN_EVAL_OCC >= 1
    if "WDF_LIN_EVAL_OCC" not in os.environ:
        assert lowering._LIN_EVAL_OCC == lowering._LIN_OCC       # (the chunk count decides the bits: the default is the step's)
