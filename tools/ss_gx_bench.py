"""What the input gradient costs next to the forward and the reverse sweep it follows (csrc/wdf_statespace.h: ss_bwd_gx_kernel), on
one MI355X, at the level _StateSpaceFn works at: the binding calls it makes for one forward + backward, with and without dL/dx.

Trees: the HPF tree of HPFDiodeClipper.h:28-32 under DiodePair (2 up, 3 down) and the RC low-pass of lpf.py, coefficients from
Circuit.matrices().  Shapes 8192 x 4096 and 1340 x 2048.  Variants, per tree and shape:
  sequential        ss_fwd + ss_bwd                                   one lane walks a sequence
  sequential_gx     ... + ss_bwd_gx(n_chunks=1)
  chunks            the planner's plan (plan_ss_time_parallel; a linear tree's forward: _StateSpaceFn's own chunk rule):
                    ss_fwd_lin_tp | ss_fwd_tp | ss_fwd, then ss_bwd_tp
  chunks_gx         ... + ss_bwd_gx(n_chunks = the sweep's, its workspace)
The pass reads 4 ni + 4 ns + 4 bytes per sample and writes 4 ni; it evaluates the root again.

Method: ONE process.  Every variant is warmed before anything is timed; then REPS rounds, each round every variant in turn, INNER
calls between two device events.  A variant reports the median of its REPS samples and their min-max.  Measured, no threshold:
nothing in the engine depends on the number.

Fails without a GPU.  Writes profiles/ss_gx_cost.jsonl (or --out), every line stamped with the library's sha256.  The ratios go to
DESIGN section 4."""
import argparse
import hashlib
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "ss_gx_cost.jsonl")
REPS, INNER, WARMUP = 20, 5, 4
FS = 48000


def main(shapes, reps=REPS, out=OUT, write=True):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib"))
    import tf_wdf as wdf
    from wdf_hip import binding as wb
    from wdf_hip import lowering, workload

    wb.require_gpu()                                             # (no GPU: WdfHipError, nothing written)
    lib_sha = hashlib.sha256(open(wb.LIB_PATH, "rb").read()).hexdigest()
    dev = torch.device("cuda", 0)

    def hpf():
        R = wdf.Resistor(33.0e3, True)
        Vs = wdf.ResistiveVoltageSource(1.0e3, trainable=True)
        C = wdf.Capacitor(22.0e-9, FS, True)
        top = wdf.Parallel(R, wdf.Series(Vs, C))
        dp = wdf.DiodePair(top, 4.352e-9, Vt=25.85e-3, nDiodes=1.906, N_up=2, N_down=3, trainable=True)
        circ = wdf.Circuit(top, dp, R)
        coef64, r_port = circ.matrices()
        rootp = torch.tensor([float(dp.Is), float(dp.nVt), float(r_port)], dtype=torch.float32, device=dev)
        return circ, coef64.detach(), rootp, wb.ROOT_DIODE_PAIR, 2, 3

    def lpf():
        R1, C1 = wdf.Resistor(1000.0, True), wdf.Capacitor(1.0e-6, FS, True)
        circ = wdf.Circuit(wdf.Inverter(wdf.Series(R1, C1)), wdf.IdealVoltageSource(), C1)
        coef64, _ = circ.matrices()
        return circ, coef64.detach(), None, wb.ROOT_NONE, 1, 1

    rows = []
    for tree, make in (("HPF diode tree", hpf), ("RC low-pass", lpf)):
        circ, coef64, rootp, kind, n_up, n_down = make()
        ns, ni = circ.ns, circ.ni
        coef = coef64.to(device=dev, dtype=torch.float32)
        for B, T in shapes:
            x = torch.as_tensor(workload.sweep_batch(B, T, seed=4), device=dev).reshape(B, T, ni).contiguous()
            gy = torch.as_tensor(np.random.default_rng(1).standard_normal((T, B)).astype(np.float32) / (B * T), device=dev)
            plan = lowering.plan_ss_time_parallel(coef64, ns, ni, kind, B, T)
            k_lin = min(T // 64, (2 * 1024) // max(1, -(-B // 64))) if kind == wb.ROOT_NONE else 0
            rk = dict(root_kind=kind, rootp=rootp, n_up=n_up, n_down=n_down)
            gxbuf = torch.empty((T, ni, B), dtype=torch.float32, device=dev)

            def sequential(want_gx):
                def run():
                    _, zs, _ = wb.ss_fwd(x, coef, ns, ni, want_stash=True, **rk)
                    wb.ss_bwd(x, coef, ns, ni, zs, gy, **rk)
                    if want_gx:
                        wb.ss_bwd_gx(x, coef, ns, ni, zs, gy, gx=gxbuf, **rk)
                return run

            def chunks(want_gx):
                def run():
                    if k_lin >= 2:
                        _, zs, _ = wb.ss_fwd_lin_tp(x, coef, ns, ni, k_lin, want_stash=True)
                    elif plan is not None and plan.k_fwd >= 2 and kind != wb.ROOT_NONE:
                        _, zs, _, _ = wb.ss_fwd_tp(x, coef, ns, ni, rootp, plan.k_fwd, plan.warmup, plan.tol, n_up, n_down, want_stash=True,
                                                   root_kind=kind)
                    else:
                        _, zs, _ = wb.ss_fwd(x, coef, ns, ni, want_stash=True, **rk)
                    k = plan.k_bwd if plan is not None else 1
                    if k >= 2:
                        *_, ws = wb.ss_bwd_tp(x, coef, ns, ni, zs, gy, k, return_ws=True, **rk)
                    else:
                        ws = None
                        wb.ss_bwd(x, coef, ns, ni, zs, gy, **rk)
                    if want_gx:
                        wb.ss_bwd_gx(x, coef, ns, ni, zs, gy, n_chunks=k, ws_bwd_tp=ws, gx=gxbuf, **rk)
                return run

            fns = {"sequential": sequential(False), "sequential_gx": sequential(True), "chunks": chunks(False), "chunks_gx": chunks(True)}
            for fn in fns.values():
                for _ in range(WARMUP):
                    fn()
            torch.cuda.synchronize()
            samples = {v: [] for v in fns}
            for _ in range(reps):
                for v, fn in fns.items():
                    e0, e1 = wb.Event(), wb.Event()
                    e0.record()
                    for _ in range(INNER):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    samples[v].append(e0.elapsed_ms(e1) / INNER)
            row = {"config": f"{tree} {B}x{T}", "tree": tree, "ns": ns, "ni": ni, "B": B, "T": T,
                   "plan": None if plan is None else {"k_fwd": plan.k_fwd, "warmup": plan.warmup, "k_bwd": plan.k_bwd}, "k_lin": k_lin,
                   "gx_bytes_per_sample": {"read": 4 * ni + 4 * ns + 4, "written": 4 * ni}}
            for v, ms in samples.items():
                med = float(np.median(ms))
                row[v] = {"ms": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": len(ms), "calls_per_rep": INNER}
            for v in ("sequential", "chunks"):
                row[f"ratio_{v}_gx_to_{v}"] = row[v + "_gx"]["ms"] / row[v]["ms"]
                row[f"gx_ms_{v}"] = row[v + "_gx"]["ms"] - row[v]["ms"]
            row["device"] = wb.device_info(0)[0]
            row["library_sha256"] = lib_sha
            print(json.dumps(row), flush=True)
            rows.append(json.dumps(row))
            del x, gy, gxbuf, fns
            torch.cuda.empty_cache()
    if write:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(rows) + "\n")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", nargs=2, type=int, action="append", metavar=("B", "T"), help="a shape of one's own (prints its line, writes nothing)")
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    sys.exit(main([tuple(s) for s in a.shape] if a.shape else [(8192, 4096), (1340, 2048)], a.reps, a.out, write=not a.shape))
