"""The one-pass training step of a tree under tf_wdf.AsymDiodePair(any_tree=True) (csrc/wdf_ss_asym_step.h: Circuit._asym_tree_step)
against the composed path -- forward with stash, the loss in torch, the reverse sweep (what Circuit.mse / mse_esr do without
the step) -- on the HPF tree Parallel(R, Series(Vs, C)) probed at R, both losses (MSE; MSE + ESR past 50 samples), at
8192 x 4096 and at 1340 x 2048, on one MI355X.  Each row ends with the gradients of the seven components read back.

Circuit.mse / mse_esr take the step for a loss (lowering.ASYM_TREE_STEP_SERVES) only if the step's SLOWEST sample beats the
composed path's FASTEST at both shapes: the rows carry `step_max_below_composed_min`.

Without arguments this is the driver: one worker process under its own `timeout`; it prints the worker's JSON rows and writes them
to profiles/r13_ss_asym_step.jsonl.  The driver never opens the GPU.

Timing as tools/ss_asym_bench.py: all rows are warmed up, then timed in turn in one process, REPS rounds of INNER calls each
between two device events; a row reports the median of its REPS samples and their min and max."""
import argparse
import json
import os
import subprocess
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "r13_ss_asym_step.jsonl")
SHAPES = [(8192, 4096), (1340, 2048)]
SKIP = 50
REPS, INNER, WARMUP = 20, 3, 3
WORKER_TIMEOUT_S = 420
FS = 48000
DIODES = dict(Is_up=4.352e-9, Is_down=2.0e-6, nDiodes_up=1.906, nDiodes_down=1.4)


def drive():
    cmd = ["timeout", "-k", "10", str(WORKER_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--worker"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode != 0:
        print(f"ss_asym_step_bench: the worker ended with status {p.returncode}; {OUT} is left as it was", file=sys.stderr)
        return p.returncode
    with open(OUT, "w") as f:
        f.write("\n".join(ln for ln in p.stdout.splitlines() if ln.startswith("{")) + "\n")
    return 0


def work():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib"))
    import tf_wdf as wdf
    from wdf_hip import binding as wb, lowering

    tf = wdf.tf
    wb.require_gpu()
    eps = float(np.finfo(float).eps)

    def hpf():
        R = wdf.Resistor(33.0e3, True)
        Vs = wdf.ResistiveVoltageSource(1.0e3, trainable=True)
        C = wdf.Capacitor(22.0e-9, FS, True)
        top = wdf.Parallel(R, wdf.Series(Vs, C))
        dp = wdf.AsymDiodePair(top, trainable=True, any_tree=True, **DIODES)
        return wdf.Circuit(top, dp, R), [R.R, Vs.R, C.C, dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down]

    rows, fns = [], []
    for B, T in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(77)
        x = (torch.randn((B, T), generator=g) * 1.2).cuda()
        tgt = (torch.randn((T, B), generator=g) * 0.1).cuda()
        for kind, skip in (("mse", 0), ("mse_esr", SKIP)):
            circ, params = hpf()
            info = {}

            def composed(circ=circ, params=params, info=info, x=x, tgt=tgt, kind=kind, skip=skip):
                y = circ(x)
                o, t = y[skip:], tgt[skip:]
                S, n = tf.reduce_sum(tf.square(o - t)), float(o.numel())
                loss = S / n if kind == "mse" else S / n + tf.sqrt(S / (tf.reduce_sum(tf.square(o)) + eps) / n)
                info["g"] = [float(v) for v in tf.GradientTape().gradient(loss, params)]
                info["loss"] = float(loss)

            def step(circ=circ, params=params, info=info, x=x, tgt=tgt, kind=kind, skip=skip):
                loss = circ._asym_tree_step(x, tgt, kind, skip)
                info["g"] = [float(v) for v in tf.GradientTape().gradient(loss, params)]
                info["loss"] = float(loss)

            for path, fn in (("composed", composed), ("one-pass step", step)):
                rows.append({"circuit": "HPF tree, AsymDiodePair(any_tree=True)", "loss": kind, "skip": skip, "path": path, "B": B, "T": T,
                             "info": info})
                fns.append(fn)

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
    for i, (row, fn) in enumerate(zip(rows, fns)):
        lowering.LAST_SS_TP_STATUS.update(status=None, chunks_used=None, warmup_used=None)
        fn()                                                     # once more, to read this row's own verdict and results
        torch.cuda.synchronize()
        st = lowering.LAST_SS_TP_STATUS
        info = row.pop("info")
        j = i + 1 if i % 2 == 0 else i - 1                       # rows come in pairs: composed, step
        out = dict(row)
        out.update({"ms": float(np.median(samples[i])), "ms_min": float(np.min(samples[i])), "ms_max": float(np.max(samples[i])),
                    "reps": REPS, "calls_per_rep": INNER, "chunks_used": st.get("chunks_used"), "warmup_used": st.get("warmup_used"),
                    "status": None if st.get("status") is None else wb.ss_tp_status(st["status"]),
                    "loss_value": info["loss"], "gradients": info["g"],
                    "ms_ratio_to_other_path": float(np.median(samples[i]) / np.median(samples[j]))})
        s, c = (i, j) if row["path"] == "one-pass step" else (j, i)
        out["step_max_below_composed_min"] = bool(np.max(samples[s]) < np.min(samples[c]))
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--worker", action="store_true", help="time the rows in this process")
    a = ap.parse_args()
    sys.exit(work() if a.worker else drive())
