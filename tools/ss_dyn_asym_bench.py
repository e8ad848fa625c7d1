"""The two-different-diode root on the streamed-coefficient kernels (tf_wdf.AsymDiodePair(streamed=True), root kind
WDF_ROOT_ASYM_PAIR of csrc/wdf_ss_dyn.h) at 1340 x 2048 on one MI355X, next to the symmetric DiodePair root (N_up = N_down = 1,
the Wright-omega closed form) on the same kernels, the same data and the same plan: the HPF tree Parallel(R, Series(Vs, C))
with the pot on Vs, once constant along every sequence (one coefficient row per sequence) and once moving per sample.
Per (pot, root) four rows: the forward alone (no gradient asked for: no stash) and forward + reverse sweep to every live
component (sum(y gy)), each sequentially (time_parallel=None) and in the planner's chunks (the cold plan of the two-diode
circuit handed to both roots, warm_start=False so that every call runs that plan).  Each row names the plan, the device's
verdict and max |y - sequential|, and the ratio of its time to the symmetric root's row.

Without arguments this is the driver: one worker process under its own `timeout`; it prints the worker's JSON rows and writes them
to profiles/r15_ss_dyn_asym.jsonl.  The driver never opens the GPU.

Timing as tools/ss_asym_bench.py: all rows are warmed up, then timed in turn (the two roots alternate), REPS rounds of INNER
calls each between two device events; a row reports the median of its REPS samples and their min-max."""
import argparse
import json
import os
import subprocess
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "r15_ss_dyn_asym.jsonl")
B, T = 1340, 2048
REPS, INNER, WARMUP = 20, 5, 3
WORKER_TIMEOUT_S = 420
FS = 48000
DIODES = dict(Is_up=4.352e-9, Is_down=2.0e-6, nDiodes_up=1.906, nDiodes_down=1.4)


def drive():
    cmd = ["timeout", "-k", "10", str(WORKER_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--worker"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode != 0:
        print(f"ss_dyn_asym_bench: the worker ended with status {p.returncode}; {OUT} is left as it was", file=sys.stderr)
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

    def hpf(asym, **kw):
        R = wdf.Resistor(33.0e3, True)
        Vs = wdf.ResistiveVoltageSource(1.0e3, trainable=True)
        C = wdf.Capacitor(22.0e-9, FS, True)
        top = wdf.Parallel(R, wdf.Series(Vs, C))
        if asym:
            dp = wdf.AsymDiodePair(top, trainable=True, streamed=True, **DIODES)
            dv = [dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down]
        else:
            dp = wdf.DiodePair(top, 4.352e-9, Vt=25.85e-3, nDiodes=1.906, trainable=True)
            dv = [dp.Is, dp.nVt]
        return wdf.Circuit(top, dp, R, per_sample_R=Vs, warm_start=False, **kw), [R.R, C.C] + dv

    rng = np.random.default_rng(77)
    x = (rng.standard_normal((B, T)) * 1.2).astype(np.float32)
    gy = torch.as_tensor((rng.standard_normal((T, B)) / (B * T)).astype(np.float32)).cuda()
    level = np.exp(rng.uniform(np.log(300.0), np.log(5.0e3), B))
    wob = 1.0 + 0.3 * np.sin(2 * np.pi * np.arange(T)[None, :] / rng.uniform(200, 900, B)[:, None] + rng.uniform(0, 6, B)[:, None])
    pots = {"one value per sequence": np.repeat(level[:, None], T, axis=1).astype(np.float32),
            "a value per sample": (level[:, None] * wob).astype(np.float32)}

    rows, fns = [], []
    for pot, r in pots.items():
        xin = torch.as_tensor(np.stack([x, r], axis=-1)).cuda()
        planner = hpf(True, time_parallel="auto")[0]
        with torch.no_grad():
            planner(xin)
        plan = next(iter(planner._dyn_plans.values()))[0]
        for mode, tp in (("sequential", None), ("the planner's chunks", plan)):
            for asym in (True, False):
                circ, params = hpf(asym, time_parallel=tp)
                with torch.no_grad():
                    y_seq = hpf(asym, time_parallel=None)[0](xin).as_subclass(torch.Tensor)
                info = {}

                def fwd(circ=circ, info=info, xin=xin):
                    with torch.no_grad():
                        info["y"] = circ(xin)

                def fwd_bwd(circ=circ, params=params, info=info, xin=xin):
                    y = circ(xin)
                    info["y"], info["g"] = y, tf.GradientTape().gradient(tf.reduce_sum(y * gy), params)

                for what, fn in (("forward", fwd), ("forward + reverse sweep", fwd_bwd)):
                    rows.append({"root": "AsymDiodePair(streamed=True), root kind 4" if asym else "DiodePair N 1/1, root kind 2",
                                 "pot": pot, "mode": mode, "what": what, "B": B, "T": T, "plan": None if tp is None else plan._asdict(),
                                 "y_seq": y_seq, "info": info, "asym": asym, "circ": circ})
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
    med = [float(np.median(s)) for s in samples]
    for i, (row, fn) in enumerate(zip(rows, fns)):
        lowering.LAST_SS_TP_STATUS.update(status=None, chunks_used=None, warmup_used=None)      # (what a sequential forward leaves)
        fn()                                                     # once more, to read this row's own verdict
        torch.cuda.synchronize()
        st = lowering.LAST_SS_TP_STATUS
        y = row.pop("info")["y"].as_subclass(torch.Tensor).detach()
        asym = row.pop("asym")
        row["rows_per_sequence"] = bool(list(row.pop("circ")._dyn_chan_const.values())[0])
        out = {k: v for k, v in row.items() if k != "y_seq"}
        out.update({"ms": med[i], "ms_min": float(np.min(samples[i])), "ms_max": float(np.max(samples[i])), "reps": REPS,
                    "calls_per_rep": INNER, "samples_per_s": B * T / med[i] * 1e3, "chunks_used": st.get("chunks_used"),
                    "warmup_used": st.get("warmup_used"),
                    "status": None if st.get("status") is None else wb.ss_tp_status(st["status"]),
                    "max_abs_y_minus_sequential": float((y - row["y_seq"]).abs().max())})
        # rows come as (asym forward, asym forward + sweep, symmetric forward, symmetric forward + sweep)
        j = i + 2 if asym else i - 2
        out["ms_ratio_to_symmetric_root"] = med[i] / med[j] if asym else 1.0
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--worker", action="store_true", help="time the rows in this process")
    a = ap.parse_args()
    sys.exit(work() if a.worker else drive())
