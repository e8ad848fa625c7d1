"""The two-different-diode clipper's MSE training step at 8192 x 4096 on one MI355X, both Newton modes in turn:
(a) the composed step as Circuit.mse ran it before the one-pass step existed -- engine.clipper_asym forward (x in, y + stash
out), torch's mean((y - target)^2) forward and backward, the reverse sweep -- and (b) engine.AsymMseStep.step_fused, both
with the planner's plan, both without the optimizer.

Timing as tools/c5_sweep.py: the two rows of a mode are warmed up, then timed in turn, REPS rounds of INNER calls each
between two device events; a row reports the median of its REPS samples and their min-max.  Parity from the same run:
max |y - oracle| on a fixed sample of sequences, and the step's loss and gradient against the composed path's.  Prints one
JSON line per row; copy the output under profiles/."""
import json
import os
import sys

import numpy as np
import torch

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib")); sys.path.insert(0, os.path.join(_R, "oracle"))
from wdf_hip import binding as wb, engine, workload
import oracle as O

FS = workload.FS
THETA6 = np.array([4.352e-9, 25.85e-3 * 1.906, 2.0e-6, 25.85e-3 * 1.4, 45.0e3, 4.7e-9])
B, T = 8192, 4096
REPS, INNER, WARMUP = 20, 5, 3

wb.require_gpu()
x = workload.sweep_batch(B, T)
xd = torch.as_tensor(x, device="cuda")
th = torch.tensor(THETA6, dtype=torch.float32, device="cuda")
t32 = THETA6.astype(np.float32).astype(np.float64)
pick = np.random.default_rng(0).choice(B, 32, replace=False)
ref = O.clipper_asym_fwd(t32, FS, x[pick].astype(np.float64))
pk = torch.as_tensor(pick, device="cuda")
plan = engine.plan_asym_time_parallel(B, T, THETA6[4], THETA6[5], FS)
# the target: this clipper at "teacher" parameters (every component x 1.25), computed on the device
tgd, _, _, _ = wb.clipper_asym_fwd_tp(xd, torch.tensor(THETA6 * 1.25, dtype=torch.float32, device="cuda"), FS, wb.ASYM_NEWTON_F64,
                                      plan.k_fwd, plan.warmup)


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


def timing(ms):
    med = float(np.median(ms))
    return {"ms": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": len(ms), "calls_per_rep": INNER,
            "samples_per_s": B * T / med * 1e3}


def yerr(y):
    return float(np.max(np.abs(y[:, pk].cpu().numpy().astype(np.float64) - ref)))


for name, mode in (("fp32 Newton", wb.ASYM_NEWTON_F32), ("fp64 Newton", wb.ASYM_NEWTON_F64)):
    keep = {}

    def composed():
        tv = th.clone().requires_grad_(True)
        y = engine.clipper_asym(tv, xd, FS, tp=plan, mode=mode)
        loss = torch.mean((y - tgd) ** 2)
        loss.backward()
        keep["c"] = (loss.detach(), tv.grad, y.detach())

    st = engine.AsymMseStep(B, T, FS, plan, xd.device, mode=mode)

    def one_pass():
        st.step_fused(th, xd, tgd)

    sc, ss = time_group([composed, one_pass])
    loss_c, g_c, y_c = keep["c"]
    loss_s, g_s = float(st.sse) / (B * T), st.gtheta.cpu().numpy().astype(np.float64)
    status = wb.mlp_tp_status(st.status)
    g_c = g_c.cpu().numpy().astype(np.float64)
    tc, ts = timing(sc), timing(ss)
    common = {"root": name, "B": B, "T": T, "plan": {"k_fwd": plan.k_fwd, "warmup": plan.warmup, "k_bwd": plan.k_bwd}}
    print(json.dumps({**common, "step": "composed: forward + torch MSE + reverse sweep", **tc, "max_abs_err_vs_exact": yerr(y_c),
                      "loss": float(loss_c)}), flush=True)
    print(json.dumps({**common, "step": "one pass: AsymMseStep.step_fused", **ts, "max_abs_err_vs_exact": yerr(st.y),
                      "loss": loss_s, "loss_rel_to_composed": abs(loss_s - float(loss_c)) / float(loss_c),
                      "grad_max_rel_to_composed": float(np.max(np.abs(g_s - g_c) / np.abs(g_c))), "status": status,
                      "speedup_median": tc["ms"] / ts["ms"],
                      "gap_ms": tc["ms"] - ts["ms"],
                      "sum_of_spreads_ms": (tc["ms_max"] - tc["ms_min"]) + (ts["ms_max"] - ts["ms_min"])}), flush=True)
    del st, keep
    torch.cuda.empty_cache()
