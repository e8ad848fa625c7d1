#!/usr/bin/env python3
"""What a build of libwdf_hip.so IS, in two sections that two builds can be diffed on (no GPU needed):

  (a) kernels: the sorted set of (kernel symbol, sha256 of its normalised gfx950 disassembly) over every translation unit.
      Source: the code objects ROCm's `llvm-objdump --offloading` extracts from build/<tu>.o (or from the library itself),
      disassembled with `llvm-objdump -d`; a line is normalised by dropping everything from `//` on (addresses, encodings),
      and a kernel ends at its last `s_endpgm`: the filler behind it (`s_code_end`, zero words that decode as instructions,
      objdump's `...` for a run of either) depends on the kernel's neighbour in the unit.
      Identical pairs from several units (static kernels of shared headers) count once.
  (b) host-only exports: every *_ws_bytes / *_state_bytes / *_tp_chunks / *_tp_starts / chunk_len / row_len / count export of
      include/wdf_hip.h over a fixed grid of arguments -- one line per export: points, sha256 of the values (--values: all of them).

usage: lib_digest.py <libwdf_hip.so | build dir holding the .o files> [--lib libwdf_hip.so] [--values] [--only a|b]
A build dir takes (a) from its objects and (b) from --lib (default: lib/wdf_hip/libwdf_hip.so beside csrc/).
"""
import argparse
import ctypes
import glob
import hashlib
import itertools
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "wdf_hip.h")

GRID = {
    "B": [1, 63, 64, 129, 1340, 8192], "S": [1, 63, 64, 129, 1340, 8192], "T": [1, 31, 257, 2048, 4096],
    "n_chunks": [1, 2, 5, 32, 47], "wgrad_chunks": [1, 2, 5, 32, 47], "warmup": [0, 7, 64], "max_warm_tiles": [1, 4],
    "n_params": [1, 4, 7], "root": [0, 1, 2, 3, 4],                              # (root: the WDF_ROOT_* values and one that is none)
}
SS_SHAPES = [(ns, ni) for ni in (1, 2) for ns in range(0, 9)]                 # every export answers 0 outside its own range
MLP_ARCHS = [(4, 3), (8, 3), (16, 3), (4, 4), (8, 4), (4, 5), (8, 5), (16, 5), (2, 3)]
HOST_ONLY = re.compile(r"^(size_t|int64_t|int)\s+(wdf_\w*(?:_ws_bytes|_state_bytes|_tp_chunks|_tp_starts|_chunk_len|_row_len|"
                       r"_weight_count|_ncoef|_matrix_core_chunks|_warm_unit))\(([^)]*)\)", re.M)


def llvm_tool(name):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin", os.environ.get("ROCM_PATH", "/opt/rocm") + "/lib/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    sys.exit(f"{name}: not found under ROCM_PATH")


def kernels_of(binary):
    """{(symbol, digest)} of the gfx950 code objects bundled in one object file or shared library."""
    out = set()
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, os.path.basename(binary))
        shutil.copy(binary, local)
        subprocess.run([llvm_tool("llvm-objdump"), "--offloading", local], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
        for co in sorted(glob.glob(local + ".*gfx950*")):
            syms = subprocess.run([llvm_tool("llvm-objdump"), "-t", co], check=True, capture_output=True, text=True).stdout
            kernels = {ln.split()[-1][:-3] for ln in syms.splitlines() if ln.endswith(".kd")}     # (a kernel has a descriptor)
            dis = subprocess.run([llvm_tool("llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
            name, body = None, []
            for ln in dis.splitlines() + ["0 <end>:"]:
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
                if m:
                    if name in kernels:
                        ends = [i for i, b in enumerate(body) if b == "s_endpgm"]
                        body = body[:ends[-1] + 1] if ends else body     # (what follows is alignment filler, decoded as code)
                        out.add((name, hashlib.sha256("\n".join(body).encode()).hexdigest()))
                    name, body = m.group(1), []
                elif name is not None:
                    ln = ln.split("//")[0].strip()
                    if ln and ln not in ("...", "s_code_end"):       # (the filler behind a kernel depends on what follows it in the unit)
                        body.append(ln)
    return out


def section_a(path):
    files = sorted(glob.glob(os.path.join(path, "*.o"))) if os.path.isdir(path) else [path]
    if not files:
        sys.exit(f"{path}: no object files")
    pairs = set()
    for f in files:
        pairs |= kernels_of(f)
    print(f"# (a) kernels: {len(pairs)} (symbol, sha256 of the normalised disassembly) pairs from {len(files)} file(s); "
          f"sha256 of this section: {hashlib.sha256(repr(sorted(pairs)).encode()).hexdigest()}")
    for name, digest in sorted(pairs):
        print(f"{digest}  {name}")


def points(params):
    """The grid for one export's parameter list [(ctype, name)]: shapes and architectures travel as pairs."""
    names = [n for _, n in params]
    axes = []
    for n in names:
        if n in ("ni", "n_tanh_layers", "n_layers"):
            continue                                                            # set by its pair's first half
        if n == "ns":
            axes.append([dict(ns=a, ni=b) for a, b in SS_SHAPES] if "ni" in names else [dict(ns=a) for a in range(0, 9)])
        elif n == "hidden":
            depth = "n_tanh_layers" if "n_tanh_layers" in names else "n_layers"
            axes.append([{"hidden": h, depth: d} for h, d in MLP_ARCHS])
        elif n == "n_items":
            axes.append([dict(n_items=0), dict(n_items=1), dict(n_items=2)])    # x ceil(B / 16), filled in below
        elif n == "starts":
            axes.append([dict()])
        else:
            axes.append([{n: v} for v in GRID[n]])
    for combo in itertools.product(*axes):
        pt = {}
        for d in combo:
            pt.update(d)
        if "n_items" in pt:
            pt["n_items"] *= (pt["B"] + 15) // 16
        yield pt


def section_b(lib_path, values):
    lib = ctypes.CDLL(lib_path)
    ctype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}
    protos = HOST_ONLY.findall(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    print(f"# (b) host-only exports: {len(protos)}; per export: grid points, sha256 of the values in grid order")
    for ret, name, arglist in sorted(protos, key=lambda p: p[1]):
        params = [] if arglist.strip() == "void" else [tuple(a.replace("*", " * ").split()[i] for i in (0, -1)) for a in arglist.split(",")]
        fn = getattr(lib, name)
        fn.restype = ctype[ret]
        fn.argtypes = [ctypes.POINTER(ctypes.c_int64) if n == "starts" else ctype[t] for t, n in params]
        rows = []
        for pt in points(params):
            if any(n == "starts" for _, n in params):
                buf = (ctypes.c_int64 * max(pt["n_chunks"], 1))(*([-1] * max(pt["n_chunks"], 1)))
                rc = fn(*[buf if n == "starts" else pt[n] for _, n in params])
                val = (rc, list(buf))
            else:
                val = fn(*[pt[n] for _, n in params])
            rows.append(f"{name}({', '.join(f'{k}={v}' for k, v in pt.items())}) = {val}")
        print(f"{hashlib.sha256(chr(10).join(rows).encode()).hexdigest()}  {name}  {len(rows)} points")
        if values:
            print("\n".join("    " + r for r in rows))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("path")
    ap.add_argument("--lib")
    ap.add_argument("--values", action="store_true")
    ap.add_argument("--only", choices=["a", "b"])
    a = ap.parse_args()
    lib = a.lib or (a.path if not os.path.isdir(a.path) else os.path.join(os.path.abspath(a.path), "..", "..", "lib", "wdf_hip", "libwdf_hip.so"))
    if a.only != "b":
        section_a(a.path)
    if a.only != "a":
        section_b(os.path.abspath(lib), a.values)


if __name__ == "__main__":
    main()
