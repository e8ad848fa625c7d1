"""The one-pass training steps with and without the y store, side by side on one MI355X (csrc/wdf_clipper_fused.h STORE_Y,
csrc/wdf_ss_step.h STORE_Y): what dropping 4 of the 12 (clipper) / 16 (linear tree) bytes per sample buys.

Configurations, each one JSON line:
  clipper 8192 x 4096   MSE and MSE + ESR (skip 50), x time-major and batch-major, engine.tuned_plan's plan, a warm-start state
                        per variant (engine.MseStep(..., warm=True, store_output=...).step_fused at constant theta)
  clipper 8192 x 2048   MSE + ESR with one pot value per sequence (BASELINE configs[3]: 1340 x 2048 tiled, the recordings' grid)
  RC low-pass           MSE and MSE + ESR at 8192 x 4096 and 1340 x 2048: Circuit.mse / mse_esr(..., store_output=...) on a resident
                        circuit + tape.gradient to R and C (the probe launch rides in both variants)

Method: ONE process.  Every configuration is built and both of its variants warmed (WARMUP calls each) before anything is timed;
then per configuration REPS rounds, each round the storing variant and then the no-y variant, INNER calls between two device
events.  A variant reports the median of its REPS samples and their min-max.  Per line: the bytes the algorithm moves per sample
(from the shapes: x, target [, y]; a pot that is constant along a sequence is not streamed), the rate over the 8 TB/s roof, the
ratio no-y / storing of the medians, and whether the no-y median lies inside the storing variant's own min-max spread.

Fails without a GPU.  Writes profiles/no_y_step.jsonl, every line stamped with the library's sha256.  No threshold: the figures
go to DESIGN section 4."""
import argparse
import hashlib
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "no_y_step.jsonl")
SKIP = 50
REPS, INNER, WARMUP = 20, 5, 6
HBM_PEAK_GBS = 8000.0
FS_LIN = 48000


def main(only=None, reps=REPS):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib"))
    import tf_wdf as wdf
    from wdf_hip import binding as wb
    from wdf_hip import engine, workload

    wb.require_gpu()                                             # (no GPU: WdfHipError, nothing written)
    lib_sha = hashlib.sha256(open(wb.LIB_PATH, "rb").read()).hexdigest()
    dev = torch.device("cuda", 0)
    fs = workload.FS
    configs = []                                                 # (name, common fields, {variant: fn}, bytes {variant: B/sample})

    def clipper(B, T, loss, time_major, pot):
        th = workload.clipper_theta()
        if pot:
            idx = np.arange(B) % 1340
            x_host, r_host = workload.sweep_batch(1340, T, seed=4)[idx], workload.dataset_resistance_batch(1340, T)[idx]
        else:
            x_host, r_host = workload.sweep_batch(B, T), None
        x = torch.as_tensor(x_host, device=dev)
        r = None if r_host is None else torch.as_tensor(r_host, device=dev)
        tgt, _, _ = wb.clipper_fwd(x, torch.tensor(workload.target_theta(), dtype=torch.float32, device=dev), fs, r=r, want_stash=False)
        if time_major:
            x, r = x.t().contiguous(), None if r is None else r.t().contiguous()
        theta = torch.tensor(th, dtype=torch.float32, device=dev)
        R_plan = float(th[2]) if r is None else float(r_host.max())
        plan = engine.tuned_plan(theta, x, r, fs, R_plan, float(th[3]), time_major=time_major,
                                 R_min=None if r is None else float(r_host.min()), fused=True)
        kw = dict(time_major=time_major, loss=loss, warm=True, **({"skip": SKIP} if loss == "mse+esr" else {}))
        st = {v: engine.MseStep(B, T, fs, plan, dev, store_output=(v == "storing"), **kw) for v in ("storing", "no_y")}
        fns = {v: (lambda s=s: s.step_fused(theta, x, tgt, r=r)) for v, s in st.items()}
        name = f"clipper {B}x{T} {loss} {'time-major' if time_major else 'batch-major'} x" + (", one pot value per sequence" if pot else "")
        common = {"config": name, "B": B, "T": T, "loss": loss, "layout": "time-major" if time_major else "batch-major",
                  "plan": {"k_fwd": plan.k_fwd, "warmup": plan.warmup, "tol": plan.tol}, "pot_per_sequence": bool(pot)}

        def after():
            bad = {v: wb.tp_status(s.status)["n_bad"] for v, s in st.items()}
            g = {v: s.gtheta.cpu().numpy().astype(np.float64) for v, s in st.items()}
            ok = g["storing"] != 0
            return {"n_bad": bad, "y_buffers": {v: s.y is not None for v, s in st.items()},
                    "grad_max_rel_no_y_to_storing": float(np.max(np.abs(g["no_y"][ok] - g["storing"][ok]) / np.abs(g["storing"][ok])))}
        configs.append((name, common, fns, {"storing": 12, "no_y": 8}, after))

    def lowpass(B, T, loss):
        tf = wdf.tf

        def lpf(R=1000.0, C=1.0e-6):
            R1, C1 = wdf.Resistor(R, True), wdf.Capacitor(C, FS_LIN, True)
            return wdf.Circuit(wdf.Inverter(wdf.Series(R1, C1)), wdf.IdealVoltageSource(), C1), [R1.R, C1.C]
        g = torch.Generator(device="cpu").manual_seed(77)
        x = (torch.randn((B, T), generator=g) * 1.2).to(dev)
        teacher, _ = lpf(315.0, 0.7e-6)
        with torch.no_grad():
            tgt = teacher(x).as_subclass(torch.Tensor).detach().contiguous()
        circ = {v: lpf() for v in ("storing", "no_y")}
        for c, _ in circ.values():
            c.to_device()
        keep = {}

        def run(v):
            c, params = circ[v]

            def fn():
                with tf.GradientTape() as tape:
                    l = c.mse(x, tgt, store_output=(v == "storing")) if loss == "mse" else c.mse_esr(x, tgt, SKIP, store_output=(v == "storing"))
                keep[v] = (l, tape.gradient(l, params))
            return fn
        name = f"RC low-pass {B}x{T} {loss}"
        common = {"config": name, "B": B, "T": T, "loss": loss, "layout": "time-major (resident)"}

        def after():
            gr = {v: np.array([float(t) for t in keep[v][1]]) for v in keep}
            return {"loss": {v: float(keep[v][0]) for v in keep}, "last_output": {v: circ[v][0].last_output is not None for v in circ},
                    "grad_max_rel_no_y_to_storing": float(np.max(np.abs(gr["no_y"] - gr["storing"]) / np.abs(gr["storing"])))}
        configs.append((name, common, {v: run(v) for v in circ}, {"storing": 16, "no_y": 12}, after))

    want = lambda tag: only is None or tag in only
    if want("clipper"):
        for time_major in (True, False):
            for loss in ("mse", "mse+esr"):
                clipper(8192, 4096, loss, time_major, False)
        clipper(8192, 2048, "mse+esr", True, True)
    if want("lowpass"):
        for B, T in ((8192, 4096), (1340, 2048)):
            for loss in ("mse", "mse+esr"):
                lowpass(B, T, loss)

    for _, _, fns, _, _ in configs:                              # every shape warm before anything is timed
        for fn in fns.values():
            for _ in range(WARMUP):
                fn()
    torch.cuda.synchronize()
    rows = []
    for name, common, fns, nbytes, after in configs:
        samples = {v: [] for v in fns}
        for _ in range(reps):
            for v in ("storing", "no_y"):
                e0, e1 = wb.Event(), wb.Event()
                e0.record()
                for _ in range(INNER):
                    fns[v]()
                e1.record()
                torch.cuda.synchronize()
                samples[v].append(e0.elapsed_ms(e1) / INNER)
        B, T = common["B"], common["T"]
        row = dict(common)
        for v, ms in samples.items():
            med = float(np.median(ms))
            gbs = nbytes[v] * B * T / (med * 1e-3) / 1e9
            row[v] = {"ms": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": len(ms), "calls_per_rep": INNER,
                      "algorithmic_bytes_per_sample": nbytes[v], "GB_per_s": gbs, "frac_of_8TBs": gbs / HBM_PEAK_GBS,
                      "samples_per_s": B * T / med * 1e3}
        row["ratio_no_y_to_storing"] = row["no_y"]["ms"] / row["storing"]["ms"]
        row["no_y_median_inside_storing_spread"] = bool(row["storing"]["ms_min"] <= row["no_y"]["ms"] <= row["storing"]["ms_max"])
        row.update(after())
        row["device"] = wb.device_info(0)[0]
        row["library_sha256"] = lib_sha
        print(json.dumps(row), flush=True)
        rows.append(json.dumps(row))
    if only is None:
        with open(OUT, "w") as f:
            f.write("\n".join(rows) + "\n")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", nargs="+", choices=["clipper", "lowpass"], help="a subset (prints its lines, writes nothing)")
    ap.add_argument("--reps", type=int, default=REPS)
    a = ap.parse_args()
    sys.exit(main(a.only, a.reps))
