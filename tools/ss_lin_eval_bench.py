"""The loss-only evaluation pass of resident linear trees (csrc/wdf_ss_lin_eval.h) against what Circuit.mse / mse_esr(grad=False) run
without it, side by side on one MI355X: what a validation call costs on the RC low-pass of lpf.py after to_device().

Shapes 8192 x 4096 and 1340 x 2048; per shape one JSON line with the variants
  (a) step_mse        Circuit.mse(grad=False) with LIN_EVAL_PASS_SERVES off: probe + the one-pass MSE step, detached      16 B/sample
  (b) step_esr        Circuit.mse_esr(skip=50, grad=False) with it off: probe + the one-pass MSE + ESR step, detached      16
  (c) eval            Circuit.mse_esr(skip=50, grad=False) through the pass, storing y (the same kernel serves mse)         16
  (d) eval_no_y       the same with store_output=False                                                                     12
  (c), (d) also as eval_occN / eval_no_y_occN at WDF_LIN_EVAL_OCC = N in 2, 4, 8 (the default is the step's WDF_LIN_OCC): reported only.
Every variant runs on a circuit of its own built alike (its own entry and workspace) at constant parameters.

Method: ONE process.  Every variant is warmed (WARMUP calls) before anything is timed; then REPS rounds, each round every variant in
turn, INNER calls between two device events.  A variant reports the median of its REPS samples and their min-max: per call as
Circuit makes it (the probe launch and the host's part included).  Criterion of the Circuit layer (`lin_eval_pass_serves`): (c)
below (a) by more than (a)'s own min-max spread AND below (b) by more than (b)'s, at both shapes.  No threshold on (d) or on the
occupancy sweep.

Fails without a GPU.  Writes profiles/ss_lin_eval_pass.jsonl (or --out), every line stamped with the library's sha256.  The figures
go to DESIGN section 4."""
import argparse
import hashlib
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "ss_lin_eval_pass.jsonl")
SKIP = 50
REPS, INNER, WARMUP = 20, 5, 8
OCCS = (2, 4, 8)
FS = 48000


def main(shapes, reps=REPS, out=OUT, write=True):
    import numpy as np
    import torch
    for p in (os.path.join(_R, "differentiable-wdfs_amd", "lib"),):
        sys.path.insert(0, p)
    import tf_wdf as wdf
    from wdf_hip import binding as wb
    from wdf_hip import lowering, workload

    wb.require_gpu()                                             # (no GPU: WdfHipError, nothing written)
    lib_sha = hashlib.sha256(open(wb.LIB_PATH, "rb").read()).hexdigest()
    dev = torch.device("cuda", 0)

    def lpf(scale=1.0):
        R1, C1 = wdf.Resistor(1000.0 * scale, True), wdf.Capacitor(1.0e-6 / scale, FS, True)
        circ = wdf.Circuit(wdf.Inverter(wdf.Series(R1, C1)), wdf.IdealVoltageSource(), C1)
        circ.to_device()
        assert circ._lin is not None
        return circ

    def call(circ, serves, occ, fn):
        def run():
            lowering.LIN_EVAL_PASS_SERVES, lowering._LIN_EVAL_OCC = serves, occ
            return fn(circ)
        return run

    rows = []
    was = lowering.LIN_EVAL_PASS_SERVES, lowering._LIN_EVAL_OCC
    try:
        for B, T in shapes:
            x = torch.as_tensor(workload.sweep_batch(B, T, seed=4), device=dev)
            other = lpf(1.12)                                    # the target: the same circuit at other component values
            lowering.LIN_EVAL_PASS_SERVES = False
            other.mse(x, torch.zeros((T, B), device=dev), grad=False)
            tgt = other.last_output.detach().clone()
            del other
            fns, circs, nbytes = {}, {}, {}
            circs["step_mse"] = lpf()
            fns["step_mse"] = call(circs["step_mse"], False, was[1], lambda c: c.mse(x, tgt, grad=False))
            circs["step_esr"] = lpf()
            fns["step_esr"] = call(circs["step_esr"], False, was[1], lambda c: c.mse_esr(x, tgt, skip=SKIP, grad=False))
            nbytes.update({"step_mse": 16, "step_esr": 16})
            for occ in (None,) + OCCS:
                for name, store in (("eval", True), ("eval_no_y", False)):
                    v = name if occ is None else f"{name}_occ{occ}"
                    circs[v] = lpf()
                    fns[v] = call(circs[v], True, was[1] if occ is None else occ,
                                  lambda c, s=store: c.mse_esr(x, tgt, skip=SKIP, grad=False, store_output=s))
                    fns[v]()                                     # (the entry is made under this OCC)
                    nbytes[v] = 16 if store else 12
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
            row = {"config": f"RC low-pass {B}x{T}", "B": B, "T": T, "skip": SKIP, "lin_occ": lowering._LIN_OCC}
            for v, ms in samples.items():
                med = float(np.median(ms))
                row[v] = {"ms": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": len(ms), "calls_per_rep": INNER,
                          "samples_per_s": B * T / med * 1e3, "algorithmic_bytes_per_sample": nbytes[v],
                          "GB_per_s": nbytes[v] * B * T / (med * 1e-3) / 1e9}
                ents = list(circs[v]._lin.cache.values())
                row[v]["chunks"] = int(ents[0]["k"]) if ents else None
            below = lambda ev, ref: bool(row[ev]["ms"] < row[ref]["ms"] - (row[ref]["ms_max"] - row[ref]["ms_min"]))
            for c in ["eval", "eval_no_y"] + [f"{n}_occ{o}" for o in OCCS for n in ("eval", "eval_no_y")]:
                row[f"ratio_{c}_to_step_mse"] = row[c]["ms"] / row["step_mse"]["ms"]
                row[f"ratio_{c}_to_step_esr"] = row[c]["ms"] / row["step_esr"]["ms"]
            row["lin_eval_pass_serves"] = below("eval", "step_mse") and below("eval", "step_esr")
            row["device"] = wb.device_info(0)[0]
            row["library_sha256"] = lib_sha
            print(json.dumps(row), flush=True)
            rows.append(json.dumps(row))
            del fns, circs
            torch.cuda.empty_cache()
    finally:
        lowering.LIN_EVAL_PASS_SERVES, lowering._LIN_EVAL_OCC = was
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
