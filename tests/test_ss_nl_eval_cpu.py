"""CPU: the loss-only evaluation pass of small diode-root trees (wdf_ss_nl_eval*, csrc/wdf_ss_nl_eval.h) as far as it goes
without a GPU: the five symbols in the header, the signature table, the library and the export map; the header's parameter
lists against the table's; every refusal that comes before any device work; the workspace size; the binding's own refusal of a
y handed in with store_y=False; the routing constant."""
import ctypes as C
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wdf_ss_nl_eval_ws_bytes", "wdf_ss_nl_eval_plan", "wdf_ss_nl_eval_set", "wdf_ss_nl_eval_read", "wdf_ss_nl_eval")


@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wdf_hip.h")).read(), flags=re.S)


def test_header_table_library_and_export_map_name_the_five_symbols(lib):
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
    assert len(binding.SIGNATURES["wdf_ss_nl_eval"][1]) == 20


def test_every_refusal_comes_before_any_device_work(lib):
    one = C.c_void_p(16)                                    # never dereferenced: validation fails first
    ev = lib.wdf_ss_nl_eval

    def call(x=one, coef=one, params=one, n_tree=3, ns=1, ni=1, n_up=1, n_down=1, target=one, skip=50, n_global=1000.0, eps=1e-16, y=one,
             ws=one, sums=one, loss3=one, B=128, T=1024, k=4):
        return ev(x, coef, params, n_tree, ns, ni, n_up, n_down, target, skip, n_global, eps, y, ws, sums, loss3, B, T, k, None)

    def refused(what, **kw):
        rc = call(**kw)
        msg = lib.wdf_last_error()
        assert rc == -1 and msg, (kw, rc, msg)
        assert what in msg, (kw, msg)

    for name in ("x", "coef", "params", "target", "ws", "sums"):
        refused(b"null", **{name: None})
    refused(b"skip", skip=1024)
    refused(b"skip", skip=-1)
    refused(b"skip", skip=5000)
    refused(b"n_global", n_global=0.0)
    refused(b"n_global", n_global=-1.0)
    refused(b"eps", eps=-1.0)
    for kw in (dict(ns=0), dict(ns=3), dict(ni=0), dict(ni=3)):
        refused(b"ns in 1..2", **kw)
    # (K - 1) L < T <= K L must hold: 1024 steps in 5 chunks of 224 are right, 1000 steps "in 33" take 32 chunks of 32
    assert lib.wdf_ss_nl_step_chunk_len(1024, 5) == 224
    refused(b"n_chunks", T=1000, k=33)
    refused(b"n_chunks", T=40, k=3)
    refused(b"n_chunks", k=0)
    refused(b"n_up", n_up=0)
    refused(b"n_up", n_down=0)
    refused(b"component values", n_tree=0)
    assert lib.wdf_ss_nl_eval_plan(None, 1, 1, 128, 1024, 4, 64, 64, 16, 256, 1e-6, None) == -1 and b"null" in lib.wdf_last_error()
    assert lib.wdf_ss_nl_eval_plan(one, 1, 1, 128, 1024, 4, 64, 24, 16, 256, 1e-6, None) == -1 and b"multiple" in lib.wdf_last_error()
    assert lib.wdf_ss_nl_eval_plan(one, 1, 1, 128, 1024, 4, 64, 64, 16, 256, 0.0, None) == -1
    assert lib.wdf_ss_nl_eval_plan(one, 3, 1, 128, 1024, 4, 64, 64, 16, 256, 1e-6, None) == -1
    assert lib.wdf_ss_nl_eval_set(None, 8, 1.0, None) == -1
    assert lib.wdf_ss_nl_eval_set(one, 1, 1.0, None) == -1 and lib.wdf_ss_nl_eval_set(one, 13, 1.0, None) == -1
    assert lib.wdf_ss_nl_eval_read(None, one, None) == -1 and lib.wdf_ss_nl_eval_read(one, None, None) == -1


def test_workspace_size(lib):
    f = lib.wdf_ss_nl_eval_ws_bytes
    for ns, ni in [(1, 1), (1, 2), (2, 1), (2, 2)]:
        sizes = [f(ns, ni, B, 1501, 12) for B in (1, 70, 130, 131, 8192)]
        assert all(s > 0 for s in sizes) and all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    assert f(2, 1, 130, 1501, 12) > f(1, 1, 130, 1501, 12)
    # no tangents, no records: smaller than the step's
    assert 0 < f(1, 1, 8192, 4096, 32) < lib.wdf_ss_nl_step_ws_bytes(1, 1, 8192, 4096, 32)
    for bad in [(3, 1, 128, 1024, 4), (1, 3, 128, 1024, 4), (0, 1, 128, 1024, 4), (1, 1, 0, 1024, 4), (1, 1, 128, 0, 4), (1, 1, 128, 1024, 0),
                (1, 1, 128, 1000, 33)]:
        assert f(*bad) == 0 and lib.wdf_last_error(), bad


def test_the_binding_refuses_a_y_with_store_y_false_without_a_gpu():
    from wdf_hip import binding
    z = torch.zeros(1)
    with pytest.raises(binding.WdfHipError, match="store_y=False"):
        binding.ss_nl_eval(z, z, z, 3, 1, 1, z, 1, z, y=torch.zeros((4, 4)), store_y=False)


def test_the_routing_constant_is_a_bool():
    from wdf_hip import lowering
    assert isinstance(lowering.NL_EVAL_PASS_SERVES, bool)
    assert isinstance(lowering._NL_EVAL_OCC, int) and lowering._NL_EVAL_OCC >= 1
