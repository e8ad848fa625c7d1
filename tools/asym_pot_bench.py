"""The two-different-diode clipper's training steps with one pot resistance per sequence on one MI355X, at 8192 x 4096 and
8192 x 2048 (BASELINE configs[3]'s shape), with the planner's plan and without the optimizer.  Per shape and Newton mode, six
rows timed in turn in ONE process:
(a) the pot MSE + ESR step, engine.AsymEsrStep.step_fused(r=...) (skip = 50);   (b) its static twin at R = 45 kOhm;
(c) the pot MSE step, engine.AsymMseStep.step_fused(r=...);                     (d) its static twin at R = 45 kOhm;
(e), (f) the composed pot path for either loss -- engine.clipper_asym(r=...) forward (x in, y + stash out), the torch loss
    forward and backward, the reverse sweep wdf_clipper_asym_bwd_tp_rseq.
Pots: uniform in 10-99.1 kOhm per sequence (seed 0); the pot rows' plan comes from the largest of them, the static rows' from 45 kOhm.

Without arguments this is the driver: it starts one worker process per shape and mode, each under its own `timeout`, stops at
the first one that fails, prints the workers' JSON rows and writes them to profiles/r10_asym_pot.jsonl.  The driver itself
never opens the GPU.

Timing as tools/asym_esr_step_bench.py: the rows of a worker are warmed up, then timed in turn, REPS rounds of INNER calls each
between two device events; a row reports the median of its REPS samples and their min-max.  The pot rows carry the two
ratios the routing and the register question rest on: to the static twin and to the composed pot path, same process."""
import argparse
import json
import os
import subprocess
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "r10_asym_pot.jsonl")
MODES = ("newton_f32", "newton_f64")
SHAPES = ((8192, 4096), (8192, 2048))
SKIP = 50
REPS, INNER, WARMUP = 20, 5, 3
WORKER_TIMEOUT_S = 300


def drive():
    rows = []
    for B, T in SHAPES:
        for mode in MODES:
            cmd = ["timeout", "-k", "10", str(WORKER_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--mode", mode,
                   "--shape", f"{B}x{T}"]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode != 0:
                print(f"asym_pot_bench: the {mode} {B}x{T} worker ended with status {p.returncode}; nothing more is started, "
                      f"{OUT} is left as it was", file=sys.stderr)
                return p.returncode
            rows += [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    with open(OUT, "w") as f:
        f.write("\n".join(rows) + "\n")
    return 0


def work(mode_name, B, T):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib"))
    from wdf_hip import binding as wb, engine, workload

    FS = workload.FS
    THETA6 = np.array([4.352e-9, 25.85e-3 * 1.906, 2.0e-6, 25.85e-3 * 1.4, 45.0e3, 4.7e-9])
    EPS = float(np.finfo(float).eps)
    name, mode = {"newton_f32": ("fp32 Newton", wb.ASYM_NEWTON_F32), "newton_f64": ("fp64 Newton", wb.ASYM_NEWTON_F64)}[mode_name]
    wb.require_gpu()
    xd = torch.as_tensor(workload.sweep_batch(B, T), device="cuda")
    th = torch.tensor(THETA6, dtype=torch.float32, device="cuda")
    r = np.random.default_rng(0).uniform(10.0e3, 99.1e3, B).astype(np.float32)
    rd = torch.as_tensor(r, device="cuda")
    plan_pot = engine.plan_asym_time_parallel(B, T, float(r.max()), THETA6[5], FS)
    plan_st = engine.plan_asym_time_parallel(B, T, THETA6[4], THETA6[5], FS)
    # the targets: this clipper at "teacher" parameters (the diodes and C x 1.25), with and without the pots, computed on the device
    teacher = torch.tensor(THETA6 * np.array([1.25, 1.25, 1.25, 1.25, 1.0, 1.25]), dtype=torch.float32, device="cuda")
    tg_pot = wb.clipper_asym_fwd_tp_rseq(xd, rd, teacher, FS, wb.ASYM_NEWTON_F64, plan_pot.k_fwd, plan_pot.warmup)[0]
    tg_st = wb.clipper_asym_fwd_tp(xd, teacher, FS, wb.ASYM_NEWTON_F64, plan_st.k_fwd, plan_st.warmup)[0]

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

    keep = {}

    def composed(skip):
        def run():
            tv = th.clone().requires_grad_(True)
            y = engine.clipper_asym(tv, xd, FS, tp=plan_pot, mode=mode, r=rd)
            if skip is None:
                loss = torch.mean((y - tg_pot) ** 2)
            else:
                o, t = y[skip:], tg_pot[skip:]
                S, E, n = torch.sum((o - t) ** 2), torch.sum(o ** 2) + EPS, float(o.numel())
                loss = S / n + torch.sqrt(S / E / n)
            loss.backward()
            keep[skip] = (float(loss.detach()), tv.grad.cpu().numpy().astype(np.float64))
        return run

    pe = engine.AsymEsrStep(B, T, FS, plan_pot, xd.device, mode=mode, skip=SKIP)
    pm = engine.AsymMseStep(B, T, FS, plan_pot, xd.device, mode=mode)
    se = engine.AsymEsrStep(B, T, FS, plan_st, xd.device, mode=mode, skip=SKIP)
    sm = engine.AsymMseStep(B, T, FS, plan_st, xd.device, mode=mode)
    fns = [lambda: pe.step_fused(th, xd, tg_pot, r=rd), lambda: se.step_fused(th, xd, tg_st),
           lambda: pm.step_fused(th, xd, tg_pot, r=rd), lambda: sm.step_fused(th, xd, tg_st),
           composed(SKIP), composed(None)]
    t_pe, t_se, t_pm, t_sm, t_ce, t_cm = [timing(s) for s in time_group(fns)]
    plan_of = lambda p: {"k_fwd": p.k_fwd, "warmup": p.warmup, "k_bwd": p.k_bwd}
    common = {"root": name, "B": B, "T": T, "skip": SKIP, "pots_ohm": [float(r.min()), float(r.max())]}
    tr = [0, 1, 2, 3, 5]

    def pot_row(step, t, t_static, t_comp, stp, loss, g, key):
        loss_c, g_c = keep[key]
        return {**common, "step": step, "plan": plan_of(plan_pot), **t, "status": wb.mlp_tp_status(stp.status), "loss": loss,
                "loss_rel_to_composed": abs(loss - loss_c) / loss_c,
                "grad_max_rel_to_composed": float(np.max(np.abs(g[tr] - g_c[tr]) / np.abs(g_c[tr]))), "grad_R": float(g[4]),
                "ratio_median_to_static_twin": t["ms"] / t_static["ms"], "ratio_median_to_composed_pot_path": t["ms"] / t_comp["ms"],
                "sum_of_spreads_ms_vs_composed": (t["ms_max"] - t["ms_min"]) + (t_comp["ms_max"] - t_comp["ms_min"])}
    rows = [
        pot_row("pot, one pass MSE + ESR: AsymEsrStep.step_fused(r=)", t_pe, t_se, t_ce, pe, float(pe.loss3[2]),
                pe.gtheta.cpu().numpy().astype(np.float64), SKIP),
        {**common, "step": "static twin at 45 kOhm, one pass MSE + ESR", "plan": plan_of(plan_st), **t_se, "status": wb.mlp_tp_status(se.status)},
        pot_row("pot, one pass MSE: AsymMseStep.step_fused(r=)", t_pm, t_sm, t_cm, pm, float(pm.sse) / (B * T),
                pm.gtheta.cpu().numpy().astype(np.float64), None),
        {**common, "step": "static twin at 45 kOhm, one pass MSE", "plan": plan_of(plan_st), **t_sm, "status": wb.mlp_tp_status(sm.status)},
        {**common, "step": "pot, composed MSE + ESR: forward + torch loss + bwd_tp_rseq", "plan": plan_of(plan_pot), **t_ce, "loss": keep[SKIP][0]},
        {**common, "step": "pot, composed MSE: forward + torch loss + bwd_tp_rseq", "plan": plan_of(plan_pot), **t_cm, "loss": keep[None][0]},
    ]
    for row in rows:
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=MODES, help="worker: time this mode's six rows in this process")
    ap.add_argument("--shape", default="8192x4096", help="worker: BxT")
    a = ap.parse_args()
    sys.exit(work(a.mode, *[int(v) for v in a.shape.split("x")]) if a.mode else drive())
