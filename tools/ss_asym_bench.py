"""The two-different-diode root on the generic state-space kernels (tf_wdf.AsymDiodePair(any_tree=True), root kind
WDF_ROOT_ASYM_PAIR of csrc/wdf_statespace.h) at 8192 x 4096 on one MI355X, next to what it can be compared with:
(a) the HPF tree Parallel(R, Series(Vs, C)) under AsymDiodePair(any_tree=True) and under DiodePair (N_up = N_down = 1, the
    Wright-omega closed form) -- the same kernels, the same planner, only the root differs;
(b) the clipper tree Parallel(Vs, C) under AsymDiodePair through force_generic=True and on its own kernels (csrc/wdf_asym.h).
Per circuit two rows: the forward alone (no gradient asked for: no stash) and forward + reverse sweep to every component
(sum(y gy)); each row names the plan, the chunks and warm-up the last call used, the device's verdict, and max |y - sequential|
(time_parallel=None on the same circuit).

Without arguments this is the driver: one worker process under its own `timeout`; it prints the worker's JSON rows and writes them
to profiles/r12_ss_asym.jsonl.  The driver never opens the GPU.

Timing as tools/ss_nl_esr_step_bench.py: all rows are warmed up, then timed in turn (the two roots alternate), REPS rounds of
INNER calls each between two device events; a row reports the median of its REPS samples and their min-max."""
import argparse
import json
import os
import subprocess
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "r12_ss_asym.jsonl")
B, T = 8192, 4096
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
        print(f"ss_asym_bench: the worker ended with status {p.returncode}; {OUT} is left as it was", file=sys.stderr)
        return p.returncode
    with open(OUT, "w") as f:
        f.write("\n".join(ln for ln in p.stdout.splitlines() if ln.startswith("{")) + "\n")
    return 0


def work():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib"))
    import tf_wdf as wdf
    from wdf_hip import binding as wb, engine, lowering

    tf = wdf.tf
    wb.require_gpu()

    def hpf(asym, **kw):
        R = wdf.Resistor(33.0e3, True)
        Vs = wdf.ResistiveVoltageSource(1.0e3, trainable=True)
        C = wdf.Capacitor(22.0e-9, FS, True)
        top = wdf.Parallel(R, wdf.Series(Vs, C))
        if asym:
            dp = wdf.AsymDiodePair(top, trainable=True, any_tree=True, **DIODES)
            dv = [dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down]
        else:
            dp = wdf.DiodePair(top, 4.352e-9, Vt=25.85e-3, nDiodes=1.906, trainable=True)
            dv = [dp.Is, dp.nVt]
        return wdf.Circuit(top, dp, R, **kw), [R.R, Vs.R, C.C] + dv

    def clipper(generic, **kw):
        Vs = wdf.ResistiveVoltageSource(45.0e3, trainable=True)
        C = wdf.Capacitor(4.7e-9, FS, trainable=True)
        top = wdf.Parallel(Vs, C)
        dp = wdf.AsymDiodePair(top, trainable=True, any_tree=generic, **DIODES)
        return wdf.Circuit(top, dp, C, force_generic=generic, **kw), [Vs.R, C.C, dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down]

    g = torch.Generator(device="cpu").manual_seed(77)
    x = (torch.randn((B, T), generator=g) * 1.2).cuda()
    gy = (torch.randn((T, B), generator=g) / (B * T)).cuda()

    builds = [("HPF tree, AsymDiodePair(any_tree=True): generic kernels, root kind 4", lambda **kw: hpf(True, **kw), True),
              ("HPF tree, DiodePair N 1/1: generic kernels, root kind 2", lambda **kw: hpf(False, **kw), True),
              ("clipper tree, AsymDiodePair through force_generic=True: generic kernels, root kind 4", lambda **kw: clipper(True, **kw), True),
              ("clipper tree, AsymDiodePair on its own kernels (csrc/wdf_asym.h)", lambda **kw: clipper(False, **kw), False)]
    rows, fns = [], []
    for name, build, generic in builds:
        circ, params = build()
        with torch.no_grad():
            y_seq = build(time_parallel=None)[0](x).as_subclass(torch.Tensor)
        info = {}

        def fwd(circ=circ, info=info):
            with torch.no_grad():
                info["y"] = circ(x)

        def fwd_bwd(circ=circ, params=params, info=info):
            y = circ(x)
            info["y"], info["g"] = y, tf.GradientTape().gradient(tf.reduce_sum(y * gy), params)

        for kind, fn in (("forward", fwd), ("forward + reverse sweep", fwd_bwd)):
            rows.append({"circuit": name, "what": kind, "B": B, "T": T, "generic": generic, "y_seq": y_seq, "info": info, "circ": circ})
            fns.append(fn)

    def status_of(row):
        if row["generic"]:
            st = lowering.LAST_SS_TP_STATUS
            return {"chunks_used": st.get("chunks_used"), "warmup_used": st.get("warmup_used"),
                    "status": None if st.get("status") is None else wb.ss_tp_status(st["status"])}
        st = engine.LAST_TP_STATUS.get("status")
        return {"status": None if st is None else wb.mlp_tp_status(st)}

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
        engine.LAST_TP_STATUS["status"] = None
        fn()                                                     # once more, to read this row's own verdict
        torch.cuda.synchronize()
        circ = row.pop("circ")
        plan = None
        if row["generic"]:
            kind = wb.ROOT_ASYM_PAIR if circ.root_kind == "AsymDiodePair" else wb.ROOT_DIODE_PAIR
            plan = lowering.plan_ss_time_parallel(circ.matrices()[0], circ.ns, circ.ni, kind, B, T)
            plan = None if plan is None else plan._asdict()
        y = row.pop("info")["y"].as_subclass(torch.Tensor).detach()
        out = {k: v for k, v in row.items() if k not in ("y_seq", "generic")}
        out.update({"ms": med[i], "ms_min": float(np.min(samples[i])), "ms_max": float(np.max(samples[i])), "reps": REPS,
                    "calls_per_rep": INNER, "samples_per_s": B * T / med[i] * 1e3, "cold_plan": plan, **status_of(row),
                    "max_abs_y_minus_sequential": float((y - row["y_seq"]).abs().max())})
        # rows come in pairs of circuits (asym, its neighbour): the ratio of this row to the same row of the other circuit
        j = i + 2 if (i // 2) % 2 == 0 else i - 2
        out["ms_ratio_to_neighbour"] = med[i] / med[j]
        out["neighbour"] = rows[j]["circuit"] if "circuit" in rows[j] else None
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--worker", action="store_true", help="time the rows in this process")
    a = ap.parse_args()
    sys.exit(work() if a.worker else drive())
