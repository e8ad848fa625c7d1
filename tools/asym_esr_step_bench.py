"""The two-different-diode clipper's MSE + ESR training step at 8192 x 4096 on one MI355X, with the planner's plan and
without the optimizer.  Per Newton mode, three rows timed in turn in ONE process:
(a) the one-pass MSE + ESR step, engine.AsymEsrStep.step_fused (skip = 50);
(b) the one-pass MSE step, engine.AsymMseStep.step_fused;
(c) the composed mse_esr path as Circuit.mse_esr ran it before the one-pass step existed -- engine.clipper_asym forward (x in,
    y + stash out), the torch loss on y[skip:] (four reductions) forward and backward, the reverse sweep.

Without arguments this is the driver: it starts one worker process per mode (`--mode newton_f32`, then `--mode newton_f64`), each
under its own `timeout`, stops at the first one that fails, prints the workers' JSON rows and writes them to
profiles/r09_asym_esr_step.jsonl.  The driver itself never opens the GPU.

Timing as tools/asym_step_bench.py: the rows of a mode are warmed up, then timed in turn, REPS rounds of INNER calls each
between two device events; a row reports the median of its REPS samples and their min-max.  Parity from the same run:
max |y - oracle| on a fixed sample of sequences, and the step's loss and gradient against the composed path's."""
import argparse
import json
import os
import subprocess
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "r09_asym_esr_step.jsonl")
MODES = ("newton_f32", "newton_f64")
B, T, SKIP = 8192, 4096, 50
REPS, INNER, WARMUP = 20, 5, 3
WORKER_TIMEOUT_S = 300


def drive():
    rows = []
    for mode in MODES:
        cmd = ["timeout", "-k", "10", str(WORKER_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--mode", mode]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"asym_esr_step_bench: the {mode} worker ended with status {p.returncode}; nothing more is started, "
                  f"{OUT} is left as it was", file=sys.stderr)
            return p.returncode
        rows += [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    with open(OUT, "w") as f:
        f.write("\n".join(rows) + "\n")
    return 0


def work(mode_name):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib")); sys.path.insert(0, os.path.join(_R, "oracle"))
    from wdf_hip import binding as wb, engine, workload
    import oracle as O

    FS = workload.FS
    THETA6 = np.array([4.352e-9, 25.85e-3 * 1.906, 2.0e-6, 25.85e-3 * 1.4, 45.0e3, 4.7e-9])
    EPS = float(np.finfo(float).eps)
    name, mode = {"newton_f32": ("fp32 Newton", wb.ASYM_NEWTON_F32), "newton_f64": ("fp64 Newton", wb.ASYM_NEWTON_F64)}[mode_name]
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

    keep = {}

    def composed():
        tv = th.clone().requires_grad_(True)
        y = engine.clipper_asym(tv, xd, FS, tp=plan, mode=mode)
        o, t = y[SKIP:], tgd[SKIP:]
        S, E, n = torch.sum((o - t) ** 2), torch.sum(o ** 2) + EPS, float(o.numel())
        loss = S / n + torch.sqrt(S / E / n)
        loss.backward()
        keep["c"] = (loss.detach(), tv.grad, y.detach())

    se = engine.AsymEsrStep(B, T, FS, plan, xd.device, mode=mode, skip=SKIP)
    sm = engine.AsymMseStep(B, T, FS, plan, xd.device, mode=mode)

    def one_pass_esr():
        se.step_fused(th, xd, tgd)

    def one_pass_mse():
        sm.step_fused(th, xd, tgd)

    s_e, s_m, s_c = time_group([one_pass_esr, one_pass_mse, composed])
    loss_c, g_c, y_c = keep["c"]
    loss_e, g_e = float(se.loss3[2]), se.gtheta.cpu().numpy().astype(np.float64)
    g_c = g_c.cpu().numpy().astype(np.float64)
    te, tm, tc = timing(s_e), timing(s_m), timing(s_c)
    common = {"root": name, "B": B, "T": T, "skip": SKIP, "plan": {"k_fwd": plan.k_fwd, "warmup": plan.warmup, "k_bwd": plan.k_bwd}}
    spread = lambda a: a["ms_max"] - a["ms_min"]
    print(json.dumps({**common, "step": "one pass MSE + ESR: AsymEsrStep.step_fused", **te, "max_abs_err_vs_exact": yerr(se.y),
                      "loss": loss_e, "loss_rel_to_composed": abs(loss_e - float(loss_c)) / float(loss_c),
                      "grad_max_rel_to_composed": float(np.max(np.abs(g_e - g_c) / np.abs(g_c))), "status": wb.mlp_tp_status(se.status),
                      "speedup_median_vs_composed": tc["ms"] / te["ms"], "gap_ms_vs_composed": tc["ms"] - te["ms"],
                      "sum_of_spreads_ms_vs_composed": spread(tc) + spread(te),
                      "ratio_median_to_mse_step": te["ms"] / tm["ms"]}), flush=True)
    print(json.dumps({**common, "step": "one pass MSE: AsymMseStep.step_fused", **tm, "max_abs_err_vs_exact": yerr(sm.y),
                      "loss": float(sm.sse) / (B * T), "status": wb.mlp_tp_status(sm.status)}), flush=True)
    print(json.dumps({**common, "step": "composed: forward + torch MSE + ESR + reverse sweep", **tc, "max_abs_err_vs_exact": yerr(y_c),
                      "loss": float(loss_c)}), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=MODES, help="worker: time this mode's three rows in this process")
    a = ap.parse_args()
    sys.exit(work(a.mode) if a.mode else drive())
