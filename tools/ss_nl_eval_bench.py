"""The loss-only evaluation pass of resident diode-root trees (csrc/wdf_ss_nl_eval.h) against what Circuit.mse / mse_esr(grad=False)
run without it, side by side on one MI355X: what a validation call costs on the HPF diode clipper (HPFDiodeClipper.h:28-32).

Shapes 8192 x 4096 and 1340 x 2048; per shape one JSON line with the variants
  (a) step_mse       Circuit.mse(grad=False) with NL_EVAL_PASS_SERVES off: probe + the tangent-carried MSE step          12 B/sample
  (b) composed_esr   Circuit.mse_esr(skip=50, grad=False) with it off: probe + forward + loss sums + reverse sweep
  (c) eval_occN      Circuit.mse_esr(skip=50, grad=False) through the pass, storing y, WDF_NL_EVAL_OCC = N in 1, 2, 4  12
  (d) eval_no_y_occN the same with store_output=False                                                                    8
Every variant runs on a circuit of its own built alike (its own entry, workspace and warm state) at constant parameters.

Method: ONE process.  Every variant is warmed (WARMUP calls) before anything is timed; then REPS rounds, each round every variant in
turn, INNER calls between two device events.  A variant reports the median of its REPS samples and their min-max, and the w_used
its controller settled on.  Criterion of the Circuit layer (`nl_eval_pass_serves`, per N): (c) below (a) by more than (a)'s own
min-max spread AND below (b) by more than (b)'s.  No threshold on (d).

Then, per shape, the secant: two more circuits, the switch on and off, the parameters moved by one Adam-sized step (1e-3 of
themselves, fixed signs) before each of 40 calls; the w_used each settles on, the groups repaired, the median time of a call.

Fails without a GPU.  Writes profiles/ss_nl_eval_pass.jsonl (or --out), every line stamped with the library's sha256.  The
figures go to DESIGN section 4."""
import argparse
import hashlib
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "ss_nl_eval_pass.jsonl")
SKIP = 50
REPS, INNER, WARMUP = 20, 5, 8
OCCS = (1, 2, 4)
FS = 48000
THETA = (33.0e3, 1.0e3, 22.0e-9, 4.352e-9, 25.85e-3 * 1.906)      # R, Rs, C, Is, nVt


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

    def hpf(scale=1.0):
        R = wdf.Resistor(THETA[0] * scale, True)
        Vs = wdf.ResistiveVoltageSource(THETA[1], trainable=True)
        C = wdf.Capacitor(THETA[2] / scale, FS, True)
        top = wdf.Parallel(R, wdf.Series(Vs, C))
        dp = wdf.DiodePair(top, THETA[3], Vt=THETA[4], nDiodes=1.0, N_up=1, N_down=1, trainable=True)
        circ = wdf.Circuit(top, dp, R)
        circ.to_device()
        return circ, [R.R, Vs.R, C.C, dp.Is, dp.nVt]

    def call(circ, serves, fn):
        def run():
            lowering.NL_EVAL_PASS_SERVES = serves
            return fn(circ)
        return run

    rows = []
    was = lowering.NL_EVAL_PASS_SERVES, lowering._NL_EVAL_OCC
    try:
        for B, T in shapes:
            x = torch.as_tensor(workload.sweep_batch(B, T, seed=4), device=dev)
            other, _ = hpf(1.05)                                 # the target: the same circuit at other component values
            lowering.NL_EVAL_PASS_SERVES = False
            other.mse(x, torch.zeros((T, B), device=dev), grad=False)
            tgt = other.last_output.detach().clone()
            del other
            fns, circs, nbytes = {}, {}, {}
            circs["step_mse"], _ = hpf()
            fns["step_mse"] = call(circs["step_mse"], False, lambda c: c.mse(x, tgt, grad=False))
            circs["composed_esr"], _ = hpf()
            fns["composed_esr"] = call(circs["composed_esr"], False, lambda c: c.mse_esr(x, tgt, skip=SKIP, grad=False))
            nbytes.update({"step_mse": 12, "composed_esr": None})
            for occ in OCCS:
                for name, store in (("eval", True), ("eval_no_y", False)):
                    v = f"{name}_occ{occ}"
                    circs[v], _ = hpf()
                    lowering._NL_EVAL_OCC, lowering.NL_EVAL_PASS_SERVES = occ, True
                    circs[v].mse_esr(x, tgt, skip=SKIP, grad=False, store_output=store)       # (the entry is made under this OCC)
                    fns[v] = call(circs[v], True, lambda c, s=store: c.mse_esr(x, tgt, skip=SKIP, grad=False, store_output=s))
                    nbytes[v] = 12 if store else 8
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
            row = {"config": f"HPF diode clipper {B}x{T}", "B": B, "T": T, "skip": SKIP}
            for v, ms in samples.items():
                med = float(np.median(ms))
                row[v] = {"ms": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": len(ms), "calls_per_rep": INNER,
                          "samples_per_s": B * T / med * 1e3}
                if nbytes[v]:
                    row[v].update({"algorithmic_bytes_per_sample": nbytes[v], "GB_per_s": nbytes[v] * B * T / (med * 1e-3) / 1e9})
                tree = circs[v]._tree
                evs = [e for e in tree.cache.values() if "sums" in e]
                if evs:
                    ctl = tree.read_eval_ctl(evs[0])
                    row[v].update({"chunks": tree._nl_eval_k(T, evs[0]["k"]), "w_used": ctl["w_used"], "total_gated": ctl["total_gated"],
                                   "replans": evs[0]["replans"]})
            below = lambda ev, ref: bool(row[ev]["ms"] < row[ref]["ms"] - (row[ref]["ms_max"] - row[ref]["ms_min"]))
            for occ in OCCS:
                c = f"eval_occ{occ}"
                row[f"ratio_{c}_to_step_mse"] = row[c]["ms"] / row["step_mse"]["ms"]
                row[f"ratio_{c}_to_composed_esr"] = row[c]["ms"] / row["composed_esr"]["ms"]
                row[f"nl_eval_pass_serves_occ{occ}"] = below(c, "step_mse") and below(c, "composed_esr")
            # ---- the secant on / off under moving parameters
            moving = {}
            for secant in (True, False):
                lowering._NL_EVAL_OCC, lowering.NL_EVAL_PASS_SERVES = was[1], True
                circ, params = hpf()
                ent = circ._tree.eval_entry(x, tgt)
                wb.ss_nl_eval_set(ent["ws"], wb.NL_EVAL_SECANT, 1 if secant else 0)
                ms, used = [], []
                for i in range(40):
                    for j, p in enumerate(params):
                        p.assign(float(p) * (1.0 + (1.0e-3 if j % 2 == 0 else -1.0e-3)))
                    torch.cuda.synchronize()
                    e0, e1 = wb.Event(), wb.Event()
                    e0.record()
                    circ.mse_esr(x, tgt, skip=SKIP, grad=False)
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_ms(e1))
                    used.append(circ._tree.read_eval_ctl(ent)["w_used"])
                ctl = circ._tree.read_eval_ctl(ent)
                moving["secant_on" if secant else "secant_off"] = {"ms_median_after_10": float(np.median(ms[10:])), "w_used": used,
                                                                    "w_used_last": used[-1], "total_gated": ctl["total_gated"]}
            row["moving_parameters"] = moving
            row["device"] = wb.device_info(0)[0]
            row["library_sha256"] = lib_sha
            print(json.dumps(row), flush=True)
            rows.append(json.dumps(row))
            del fns, circs
            torch.cuda.empty_cache()
    finally:
        lowering.NL_EVAL_PASS_SERVES, lowering._NL_EVAL_OCC = was
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
