"""What the Gauss-Newton matrix costs in the linear trees' one-pass step, on one MI355X: _LinResident.gn_step (wdf_ss_probe_adam +
wdf_ss_lin_step_gn: the MSE step plus kG (kG + 1) / 2 sums of tangent products per row) against _LinResident.step (wdf_ss_probe_adam
+ wdf_ss_lin_step_mse, whose kernels this change leaves as the parent built them: profiles/lin_gn_digest.txt) at 8192 x 4096 and
1340 x 2048, on lpf.py's tree (one capacitor, one source: kG = 4, 10 new sums) and on a tree of two capacitors and one source
(kG = 9, 45 new sums), each on the chunk count its own entry plans.  No routing depends on the figure and no ratio was set in
advance: a Gauss-Newton pass replaces tens of Adam passes, so its cost is recorded.

The clock: device events on the current stream around INNER consecutive calls (probe and step launches included, no host
synchronisation inside), after WARMUP calls of each row; the two rows of a tree and shape are timed in turn, REPS rounds; a row
reports the median of its REPS samples and their min-max.  Parity from the same run: the SSE and the gradient of the two steps.
Writes one JSON line per row to --out (default profiles/lin_gn_step.jsonl) and prints it."""
import argparse
import json
import os
import sys

import numpy as np
import torch

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib"))
import tf_wdf as W
from wdf_hip import binding as wb

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--out", default=os.path.join(_R, "profiles", "lin_gn_step.jsonl"))
ap.add_argument("--shapes", default="8192x4096,1340x2048")
args = ap.parse_args()

FS = 48000
SHAPES = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
REPS, INNER, WARMUP = 20, 20, 3


def lpf():
    R1, C1 = W.Resistor(1000.0, True), W.Capacitor(1.0e-6, FS, True)
    return W.Circuit(W.Inverter(W.Series(R1, C1)), W.IdealVoltageSource(), C1)


def two_capacitors():
    Ra, Rb = W.Resistor(1.0e3, True), W.Resistor(2.2e3, True)
    Ca, Cb = W.Capacitor(1.0e-7, FS, True), W.Capacitor(2.2e-7, FS, True)
    return W.Circuit(W.Inverter(W.Series(Ra, W.Parallel(Ca, W.Series(Rb, Cb)))), W.IdealVoltageSource(), Cb)


TREES = [("lpf.py's tree", lpf), ("two capacitors, one source", two_capacitors)]


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


def timing(ms, n):
    med = float(np.median(ms))
    return {"ms": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": len(ms), "calls_per_rep": INNER,
            "samples_per_s": n / med * 1e3}


wb.require_gpu()
out = open(args.out, "w")


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


for B, T in SHAPES:
    rng = np.random.default_rng([B, T])
    x = torch.as_tensor(rng.standard_normal((B, T)).astype(np.float32), device="cuda")
    for name, build in TREES:
        circ = build().to_device()
        lin = circ._lin
        assert lin is not None
        tgt = (0.5 * x.t() + 0.05 * torch.as_tensor(rng.standard_normal((T, B)).astype(np.float32), device="cuda")).contiguous()
        with torch.no_grad(), torch._C.DisableTorchFunctionSubclass():
            em, eg = lin.entry(x, tgt), lin.gn_entry(x, tgt)
            res = {}

            def run_mse():
                res["mse"] = lin.step(em)

            def run_gn():
                res["gn"] = lin.gn_step(eg)

            sm, sg = time_group([run_mse, run_gn])
            tm, tg = timing(sm, B * T), timing(sg, B * T)
            om, og = res["mse"][0].cpu().numpy(), res["gn"].cpu().numpy()
        n = lin.pb.n
        same = bool(np.array_equal(og[:1 + n].astype(np.float32), om))
        rel = float(np.max(np.abs(og[:1 + n] - om.astype(np.float64)) / np.abs(om.astype(np.float64))))
        kG = circ.ns * circ.ns + circ.ns * circ.ni + circ.ns + circ.ni
        common = {"tree": name, "ns": circ.ns, "ni": circ.ni, "kG": kG, "new_sums": kG * (kG + 1) // 2, "n_params": n, "B": B, "T": T,
                  "clock": f"device events around {INNER} consecutive calls (probe + step), median of {REPS} after {WARMUP} warm-up calls"}
        emit({**common, "step": "MSE: _LinResident.step (wdf_ss_probe_adam + wdf_ss_lin_step_mse)", **tm, "n_chunks": em["k"],
              "loss": float(om[0]) / (B * T), "ws_bytes": int(em["ws"].numel())})
        emit({**common, "step": "Gauss-Newton: _LinResident.gn_step (wdf_ss_probe_adam + wdf_ss_lin_step_gn)", **tg, "n_chunks": eg["k"],
              "loss": float(og[0]) / (B * T), "ws_bytes": int(eg["ws"].numel()), "sse_and_gradient_bit_for_bit_after_float_rounding": same,
              "sse_and_gradient_max_rel_diff": rel, "cost_ratio_median": tg["ms"] / tm["ms"], "gap_ms": tg["ms"] - tm["ms"],
              "sum_of_spreads_ms": (tm["ms_max"] - tm["ms_min"]) + (tg["ms_max"] - tg["ms_min"])})
        del circ, lin, em, eg, tgt
        torch.cuda.empty_cache()
out.close()
