"""The MLP-root clipper's loss-only evaluation pass (csrc/wdf_mlp_eval.h, mlp_root.MlpEvalPass) against what a validation call costs
without it, side by side on one MI355X, in a training loop whose weights MOVE (the warm-ups settle against a moving trajectory: a
fixed-weights figure would flatter the pass).

Setting: clipper_pot.py's shape, 1340 x 2048, the committed 2x16 weights.  Pair A (sweeps of seed 4) is trained with the resident
step and Adam(1e-4, beta_1 0.5), one step per epoch.  Pair B (seed 5) is evaluated once per epoch by each of four variants, every
variant on an entry of its own (its own state block, snapshots and warm-up controller), all reading the weights pair A trains:
    (a) step        the full training step on B (forward, reverse sweep, reduce; no optimizer: the weights are A's to move)
    (b) fwd_sums    the step's forward and loss-sum phases + wdf_esr_coef: Circuit.mse_esr(grad=False) with MLP_EVAL_PASS_SERVES off
    (c) eval        the pass, storing y
    (d) eval_no_y   the pass without the y store
Every entry is re-planned once after its 24th call, as the Circuit layer does.

Method: ONE process.  DISCARD epochs first (everything runs, nothing is timed); then REPS rounds of INNER epochs.  In every epoch
each variant's call on B runs between two device events of its own, the variants in an order that rotates from epoch to epoch; a
variant's sample for a round is the mean of its INNER timings.  A variant reports the median of its REPS samples and their min-max,
and its entry's read-back (warm-up units per column, chunks flagged and columns gone sequential since the start).

Criterion of the Circuit layer (lowering.MLP_EVAL_PASS_SERVES): (c) below (b) and below (a), each by more than the compared
variant's own min-max spread over the rounds, and the same for (d).

Fails without a GPU.  Writes profiles/mlp_eval_pass.jsonl (or --out): one line per variant and a verdict line, each stamped with the
library's sha256.  No time is fixed in advance.  The figures go to DESIGN section 4."""
import argparse
import hashlib
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "mlp_eval_pass.jsonl")
SKIP = 50
REPS, INNER, DISCARD, REPLAN_AT = 20, 5, 40, 24


def main(B=1340, T=2048, net="2x16_pre", reps=REPS, out=OUT):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib"))
    from wdf_hip import binding as wb
    from wdf_hip import mlp_root, workload

    wb.require_gpu()                                             # (no GPU: WdfHipError, nothing written)
    lib_sha = hashlib.sha256(open(wb.LIB_PATH, "rb").read()).hexdigest()
    dev = torch.device("cuda", 0)
    fs = workload.FS
    wh, hidden, n_layers = workload.reference_mlp_weights(net)
    w = torch.tensor(wh, dtype=torch.float32, device=dev)        # ONE weight vector: A trains it, everything on B reads it
    th4 = torch.tensor(workload.clipper_theta(), dtype=torch.float32, device=dev)

    def pair(seed):
        x = torch.as_tensor(workload.sweep_batch(B, T, seed=seed) * 0.6, device=dev)
        r = torch.as_tensor(workload.dataset_resistance_batch(B, T), device=dev)
        target, _, _ = wb.clipper_fwd(x, th4, fs, r=r, want_stash=False)
        return x, r, target

    xa, ra, ta = pair(4)
    xb, rb, tb = pair(5)
    adam = wb.Adam(w.numel(), lr=1.0e-4, beta_1=0.5, device=dev)
    train = mlp_root.MlpTrainStep(xa, ra, ta, w, hidden, n_layers, fs, workload.C_CLIPPER, skip=SKIP, adam=adam)
    step_b = mlp_root.MlpTrainStep(xb, rb, tb, w, hidden, n_layers, fs, workload.C_CLIPPER, skip=SKIP, adam=None)
    fwd_b = mlp_root.MlpTrainStep(xb, rb, tb, w, hidden, n_layers, fs, workload.C_CLIPPER, skip=SKIP, adam=None)
    eval_b, eval_no_y_b = mlp_root.MlpEvalPass.of(fwd_b), mlp_root.MlpEvalPass.of(fwd_b)
    gcoef, loss3 = torch.zeros(2, device=dev), torch.zeros(3, device=dev)

    def fwd_sums():
        fwd_b._call(mlp_root.PHASE_FWD | mlp_root.PHASE_SUMS, None)
        wb.esr_coef(fwd_b.sums, fwd_b.n_global, fwd_b.eps_energy, gcoef=gcoef, loss=loss3)

    variants = {"step": (step_b, step_b.step), "fwd_sums": (fwd_b, fwd_sums), "eval": (eval_b, eval_b.run),
                "eval_no_y": (eval_no_y_b, lambda: eval_no_y_b.run(store_output=False))}
    names = list(variants)
    calls = {"train": 0}
    events = {v: (wb.Event(), wb.Event()) for v in names}

    def epoch(k, timed):
        train.step()
        calls["train"] += 1
        if calls["train"] == REPLAN_AT:
            train.replan()
            for ent, _ in variants.values():
                ent.replan()                                     # (every variant has made REPLAN_AT calls too)
        order = names[k % 4:] + names[:k % 4]
        for v in order:
            e0, e1 = events[v]
            e0.record()
            variants[v][1]()
            e1.record()
        if not timed:
            return None
        torch.cuda.synchronize()
        return {v: events[v][0].elapsed_ms(events[v][1]) for v in names}

    for k in range(DISCARD):
        epoch(k, False)
    torch.cuda.synchronize()
    w_after_discard = w.clone()
    samples = {v: [] for v in names}
    k = DISCARD
    for _ in range(reps):
        acc = {v: 0.0 for v in names}
        for _ in range(INNER):
            ms = epoch(k, True)
            k += 1
            for v in names:
                acc[v] += ms[v]
        for v in names:
            samples[v].append(acc[v] / INNER)
    torch.cuda.synchronize()
    moved = float((w - w_after_discard).abs().max())
    losses = {"step": float(step_b.loss3[2]), "fwd_sums": float(loss3[2]), "eval": float(eval_b.loss3[2]), "eval_no_y": float(eval_no_y_b.loss3[2])}
    common = {"config": f"MLP-root clipper {net} {B}x{T} mse+esr, validation call on pair B while pair A trains", "B": B, "T": T, "net": net,
              "epochs_discarded": DISCARD, "rounds": reps, "epochs_per_round": INNER, "largest_weight_move_while_timed": moved,
              "device": wb.device_info(0)[0], "library_sha256": lib_sha}
    rows, stat = [], {}
    for v in names:
        ms = samples[v]
        info, wc = variants[v][0].read()
        stat[v] = {"ms": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}
        rows.append(dict(common, variant=v, **stat[v], loss=losses[v], warmup_units=wc.tolist(), calls=info["calls"], have_snap=info["have_snap"],
                         total_flagged=info["total_flagged"], total_sequential=info["total_sequential"], n_items=variants[v][0].n_items))
    spread = lambda v: stat[v]["ms_max"] - stat[v]["ms_min"]
    below = lambda a, b: bool(stat[a]["ms"] < stat[b]["ms"] - spread(b))
    verdict = {f"{a}_below_{b}_by_more_than_its_spread": below(a, b) for a in ("eval", "eval_no_y") for b in ("fwd_sums", "step")}
    verdict["mlp_eval_pass_serves"] = all(verdict.values())
    verdict.update({"ratio_eval_to_fwd_sums": stat["eval"]["ms"] / stat["fwd_sums"]["ms"], "ratio_eval_to_step": stat["eval"]["ms"] / stat["step"]["ms"],
                    "ratio_eval_no_y_to_fwd_sums": stat["eval_no_y"]["ms"] / stat["fwd_sums"]["ms"],
                    "ratio_eval_no_y_to_step": stat["eval_no_y"]["ms"] / stat["step"]["ms"],
                    "loss_max_rel_to_step": max(abs(l - losses["step"]) / abs(losses["step"]) for l in losses.values())})
    rows.append(dict(common, variant="verdict", **verdict))
    for row in rows:
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(json.dumps(row) for row in rows) + "\n")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    sys.exit(main(reps=a.reps, out=a.out))
