"""The loss-only evaluation pass (csrc/wdf_clipper_eval.h) against the one-pass training step and against today's gradient-free
composition, side by side on one MI355X: what a validation pass costs when nobody reads the gradient.

Configurations, each one JSON line:
  clipper 8192 x 4096   MSE + ESR (skip 50), x time-major and batch-major, engine.tuned_plan's plan, a warm-start state per variant
                        at constant theta:
                          (a) step        engine.MseStep.step_fused, storing y              12 B/sample
                          (b) step_no_y   the same step without the y store                   8
                          (c) eval        engine.MseStep.eval_fused, storing y               12
                          (d) eval_no_y   the same pass without the y store                   8
                          (e) composed    MseStep.forward + binding.loss_sums + binding.esr_coef (y written, then y and the
                                          target read again: 8 + 12 = 20; the forward also writes its 4-byte state stash)
  clipper 8192 x 2048   the same five with one pot value per sequence (the recordings' grid: 1340 x 2048 tiled)
  MLP-root 1340 x 2048  clipper_pot.py's shape: the resident training step (mlp_root.MlpTrainStep.step, no optimizer) against its
                        forward and loss-sum phases + binding.esr_coef (what Circuit.mse_esr(grad=False) runs)

Method: ONE process.  Every configuration is built and all of its variants warmed (WARMUP calls each) before anything is timed;
then per configuration REPS rounds, each round every variant in turn, INNER calls between two device events.  A variant reports
the median of its REPS samples and their min-max.  Per line: the bytes the algorithm moves per sample, the rate over the 8 TB/s
roof, the ratios eval / step, and the criterion of the Circuit layer: (c) below (a) and (d) below (b), each by more than (a)'s
or (b)'s own min-max spread over the rounds (`eval_pass_serves`).

Fails without a GPU.  Writes profiles/eval_pass.jsonl (or --out), every line stamped with the library's sha256.  No time is fixed
in advance: the yardstick is the training step in the same process.  The figures go to DESIGN section 4."""
import argparse
import hashlib
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "eval_pass.jsonl")
SKIP = 50
REPS, INNER, WARMUP = 20, 5, 6
HBM_PEAK_GBS = 8000.0


def main(only=None, reps=REPS, out=OUT):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib"))
    from wdf_hip import binding as wb
    from wdf_hip import engine, mlp_root, workload

    wb.require_gpu()                                             # (no GPU: WdfHipError, nothing written)
    lib_sha = hashlib.sha256(open(wb.LIB_PATH, "rb").read()).hexdigest()
    dev = torch.device("cuda", 0)
    fs = workload.FS
    eps = float(np.finfo(float).eps)
    configs = []                                                 # (common fields, {variant: fn}, {variant: B/sample}, after)

    def clipper(B, T, time_major, pot):
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
        kw = dict(time_major=time_major, loss="mse+esr", warm=True, skip=SKIP)
        store = {"step": True, "step_no_y": False, "eval": True, "eval_no_y": False, "composed": True}
        st = {v: engine.MseStep(B, T, fs, plan, dev, store_output=s, **kw) for v, s in store.items()}
        n = float(B * (T - SKIP))

        def composed(s=st["composed"]):
            s.forward(theta, x, r)
            wb.loss_sums(s.y, tgt, SKIP, sums=s.sums, ws=s.ws_l)
            wb.esr_coef(s.sums, n, eps, s.gcoef, s.loss)
        fns = {v: (lambda s=st[v]: s.step_fused(theta, x, tgt, r=r)) for v in ("step", "step_no_y")}
        fns.update({v: (lambda s=st[v]: s.eval_fused(theta, x, tgt, r=r)) for v in ("eval", "eval_no_y")})
        fns["composed"] = composed
        name = f"clipper {B}x{T} mse+esr {'time-major' if time_major else 'batch-major'} x" + (", one pot value per sequence" if pot else "")
        common = {"config": name, "B": B, "T": T, "loss": "mse+esr", "layout": "time-major" if time_major else "batch-major",
                  "plan": {"k_fwd": plan.k_fwd, "warmup": plan.warmup, "tol": plan.tol}, "pot_per_sequence": bool(pot)}

        def after():
            loss = {"step": float(st["step"].loss[2]), "step_no_y": float(st["step_no_y"].loss[2]), "eval": float(st["eval"].loss_eval[2]),
                    "eval_no_y": float(st["eval_no_y"].loss_eval[2]), "composed": float(st["composed"].loss[2])}
            return {"n_bad": {v: wb.tp_status(s.status)["n_bad"] for v, s in st.items()}, "loss": loss,
                    "loss_max_rel_to_step": max(abs(l - loss["step"]) / abs(loss["step"]) for l in loss.values())}
        configs.append((common, fns, {"step": 12, "step_no_y": 8, "eval": 12, "eval_no_y": 8, "composed": 20}, after, ("step", "eval")))

    def mlp(B, T, net="2x16_pre"):
        x = torch.as_tensor(workload.sweep_batch(B, T, seed=4) * 0.6, device=dev)
        r = torch.as_tensor(workload.dataset_resistance_batch(B, T), device=dev)
        wh, hidden, n_layers = workload.reference_mlp_weights(net)
        th4 = torch.tensor(workload.clipper_theta(), dtype=torch.float32, device=dev)
        target, _, _ = wb.clipper_fwd(x, th4, fs, r=r, want_stash=False)
        st = {v: mlp_root.MlpTrainStep(x, r, target, torch.tensor(wh, device=dev), hidden, n_layers, fs, workload.C_CLIPPER, skip=SKIP)
              for v in ("step", "eval")}
        gcoef, loss3 = torch.zeros(2, device=dev), torch.zeros(3, device=dev)

        def ev(s=st["eval"]):
            s._call(mlp_root.PHASE_FWD | mlp_root.PHASE_SUMS, None)
            wb.esr_coef(s.sums, s.n_global, s.eps_energy, gcoef=gcoef, loss=loss3)
        common = {"config": f"MLP-root clipper {net} {B}x{T} mse+esr", "B": B, "T": T, "loss": "mse+esr", "layout": "batch-major"}

        def after():
            return {"loss": {"step": float(st["step"].loss3[2]), "eval": float(loss3[2])}}
        configs.append((common, {"step": st["step"].step, "eval": ev}, {"step": 16, "eval": 16}, after, ("step", "eval")))

    want = lambda tag: only is None or tag in only
    if want("clipper"):
        clipper(8192, 4096, True, False)
        clipper(8192, 4096, False, False)
        clipper(8192, 2048, True, True)
    if want("mlp"):
        mlp(1340, 2048)

    for _, fns, _, _, _ in configs:                              # every shape warm before anything is timed
        for fn in fns.values():
            for _ in range(WARMUP):
                fn()
    torch.cuda.synchronize()
    rows = []
    for common, fns, nbytes, after, _ in configs:
        samples = {v: [] for v in fns}
        for _ in range(reps):
            for v in fns:
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
        below = lambda ev, stp: bool(row[ev]["ms"] < row[stp]["ms"] - (row[stp]["ms_max"] - row[stp]["ms_min"]))
        row["ratio_eval_to_step"] = row["eval"]["ms"] / row["step"]["ms"]
        row["eval_below_step_by_more_than_its_spread"] = below("eval", "step")
        if "eval_no_y" in row:
            row["ratio_eval_no_y_to_step_no_y"] = row["eval_no_y"]["ms"] / row["step_no_y"]["ms"]
            row["ratio_eval_to_composed"] = row["eval"]["ms"] / row["composed"]["ms"]
            row["eval_no_y_below_step_no_y_by_more_than_its_spread"] = below("eval_no_y", "step_no_y")
            row["eval_pass_serves"] = bool(row["eval_below_step_by_more_than_its_spread"] and
                                           row["eval_no_y_below_step_no_y_by_more_than_its_spread"])
        row.update(after())
        row["device"] = wb.device_info(0)[0]
        row["library_sha256"] = lib_sha
        print(json.dumps(row), flush=True)
        rows.append(json.dumps(row))
    if only is None:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(rows) + "\n")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", nargs="+", choices=["clipper", "mlp"], help="a subset (prints its lines, writes nothing)")
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    sys.exit(main(a.only, a.reps, a.out))
