"""What the Gauss-Newton matrix costs in the two-different-diode clipper's one-pass step, on one MI355X: engine.AsymGnStep.run
(wdf_clipper_asym_step_gn: the MSE step plus 28 fp64 accumulators and their FMAs per sample, a 43-double record) against
engine.AsymMseStep.step_fused (wdf_clipper_asym_step_mse) at 8192 x 4096 and 1340 x 2048, both Newton modes in turn, both with
the planner's plan, neither with an optimizer.  No routing depends on the figure: it is recorded.

Timing as tools/asym_step_bench.py: the two rows of a mode are warmed up, then timed in turn, REPS rounds of INNER calls each
between two device events; a row reports the median of its REPS samples and their min-max.  Parity from the same run: max
|y - oracle| on a fixed sample of sequences, out28[0:7] against the MSE step's out7.  Writes one JSON line per row to --out
(default profiles/asym_gn_step.jsonl) and prints it."""
import argparse
import json
import os
import sys

import numpy as np
import torch

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib")); sys.path.insert(0, os.path.join(_R, "oracle"))
from wdf_hip import binding as wb, engine, workload
import oracle as O

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--out", default=os.path.join(_R, "profiles", "asym_gn_step.jsonl"))
args = ap.parse_args()

FS = workload.FS
THETA6 = np.array([4.352e-9, 25.85e-3 * 1.906, 2.0e-6, 25.85e-3 * 1.4, 45.0e3, 4.7e-9])
SHAPES = [(8192, 4096), (1340, 2048)]
REPS, INNER, WARMUP = 20, 5, 3

wb.require_gpu()
th = torch.tensor(THETA6, dtype=torch.float32, device="cuda")
t32 = THETA6.astype(np.float32).astype(np.float64)


def time_group(fns):
    for fn in fns:
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    samples = [[] for _ in fns]
    for _ in range(REPS):
        for i, fn in enumerate(fns):
            e0, e1 = wb.Event(), wb.Event()
            e0.record()
            for _ in range(INNER):
                fn()
            e1.record()
            torch.cuda.synchronize()
            samples[i].append(e0.elapsed_ms(e1) / INNER)
    return samples


def timing(ms, n):
    med = float(np.median(ms))
    return {"ms": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": len(ms), "calls_per_rep": INNER,
            "samples_per_s": n / med * 1e3}


out = open(args.out, "w")


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


for B, T in SHAPES:
    x = workload.sweep_batch(B, T)
    xd = torch.as_tensor(x, device="cuda")
    pick = np.random.default_rng(0).choice(B, 32, replace=False)
    ref = O.clipper_asym_fwd(t32, FS, x[pick].astype(np.float64))
    pk = torch.as_tensor(pick, device="cuda")
    plan = engine.plan_asym_time_parallel(B, T, THETA6[4], THETA6[5], FS)
    # the target: this clipper at "teacher" parameters (every component x 1.25), computed on the device
    tgd, _, _, _ = wb.clipper_asym_fwd_tp(xd, torch.tensor(THETA6 * 1.25, dtype=torch.float32, device="cuda"), FS, wb.ASYM_NEWTON_F64,
                                          plan.k_fwd, plan.warmup)

    def yerr(y):
        return float(np.max(np.abs(y[:, pk].cpu().numpy().astype(np.float64) - ref)))

    for name, mode in (("fp32 Newton", wb.ASYM_NEWTON_F32), ("fp64 Newton", wb.ASYM_NEWTON_F64)):
        mse = engine.AsymMseStep(B, T, FS, plan, xd.device, mode=mode)
        gn = engine.AsymGnStep(B, T, FS, plan, xd.device, mode=mode)
        sm, sg = time_group([lambda: mse.step_fused(th, xd, tgd), lambda: gn.run(th, xd, tgd)])
        tm, tg = timing(sm, B * T), timing(sg, B * T)
        o7, o28 = mse.out.cpu().numpy(), gn.out.cpu().numpy()
        ulps = np.abs(o28[:7].astype(np.float64) - o7.astype(np.float64)) / np.spacing(np.abs(o7)).astype(np.float64)
        common = {"root": name, "B": B, "T": T, "plan": {"k_fwd": plan.k_fwd, "warmup": plan.warmup}}
        emit({**common, "step": "MSE: AsymMseStep.step_fused (wdf_clipper_asym_step_mse)", **tm, "max_abs_err_vs_exact": yerr(mse.y),
              "loss": float(o7[0]) / (B * T), "status": wb.mlp_tp_status(mse.status), "ws_bytes": int(mse.ws.numel())})
        emit({**common, "step": "Gauss-Newton: AsymGnStep.run (wdf_clipper_asym_step_gn)", **tg, "max_abs_err_vs_exact": yerr(gn.y),
              "loss": float(o28[0]) / (B * T), "status": wb.mlp_tp_status(gn.status), "ws_bytes": int(gn.ws.numel()),
              "out28_0_7_vs_out7_max_ulp": float(np.max(ulps)), "out28_0_7_bit_for_bit": bool(np.array_equal(o28[:7], o7)),
              "cost_ratio_median": tg["ms"] / tm["ms"], "gap_ms": tg["ms"] - tm["ms"],
              "sum_of_spreads_ms": (tm["ms_max"] - tm["ms_min"]) + (tg["ms_max"] - tg["ms_min"])})
        del mse, gn
        torch.cuda.empty_cache()
out.close()
