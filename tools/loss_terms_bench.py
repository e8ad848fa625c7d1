"""The weighted loss family (MSE, ESR, pre-emphasised ESR, mean: wdf_loss_terms_sums / _coef / _grad, csrc/wdf_elementwise.h) on
one MI355X next to the torch composition of the same four terms on the same y, at 8192 x 4096 and 1340 x 2048 (B x T), skip 50,
weights (1, 1, 1, 1), c = 0.85.  Per shape four rows:
  stage: sums + coef + grad        the training step's loss stage: loss, terms and dL/dy [T,B]
  stage: sums + coef               the validation pass: loss and terms only
  torch: loss + autograd dL/dy     the four terms by torch element-wise operations on [T',B] arrays in float32, then
                                   torch.autograd.grad to y
  torch: loss only                 the same under torch.no_grad()
Each stage row also reports the bytes its kernels must move at the least (sums: 8 B per kept sample; grad: 8 B read per kept
sample + 4 B written per sample) and the rate that is of the time measured -- the HBM roof is the yardstick.

Without arguments this is the driver: one worker process under its own `timeout`; it prints the worker's JSON rows and writes them
to profiles/r14_loss_terms.jsonl.  The driver never opens the GPU.  No routing and no test depends on the figures.

Timing as tools/ss_asym_bench.py: all rows are warmed up, then timed in turn, REPS rounds of INNER calls each between two device
events; a row reports the median of its REPS samples and their min-max."""
import argparse
import json
import os
import subprocess
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "r14_loss_terms.jsonl")
SHAPES = [(8192, 4096), (1340, 2048)]            # (B, T)
SKIP = 50
WEIGHTS = (1.0, 1.0, 1.0, 1.0)
COEFF = 0.85
REPS, INNER, WARMUP = 20, 3, 3
WORKER_TIMEOUT_S = 300


def drive():
    cmd = ["timeout", "-k", "10", str(WORKER_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--worker"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode != 0:
        print(f"loss_terms_bench: the worker ended with status {p.returncode}; {OUT} is left as it was", file=sys.stderr)
        return p.returncode
    with open(OUT, "w") as f:
        f.write("\n".join(ln for ln in p.stdout.splitlines() if ln.startswith("{")) + "\n")
    return 0


def work():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib"))
    from wdf_hip import binding as wb

    wb.require_gpu()
    eps = float(np.finfo(float).eps)
    rows, fns = [], []
    for B, T in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(14)
        ramp = 0.05 * torch.arange(T, dtype=torch.float32)[:, None] + 0.3 * torch.arange(B, dtype=torch.float32)[None, :]
        y = (0.5 * torch.sin(ramp) + 0.05 * torch.randn((T, B), generator=g)).cuda()
        target = (0.9 * y.cpu() + 0.02 * torch.randn((T, B), generator=g) + 0.01).cuda()
        n = float((T - SKIP) * B)
        ws = torch.empty((wb.lib().wdf_loss_terms_ws_bytes(),), dtype=torch.uint8, device="cuda")
        sums6 = torch.empty((6,), dtype=torch.float64, device="cuda")
        gcoef = torch.empty((6,), dtype=torch.float32, device="cuda")
        terms = torch.empty((5,), dtype=torch.float32, device="cuda")
        gy = torch.empty_like(y)
        info = {}

        def stage(grad, y=y, target=target, n=n, ws=ws, sums6=sums6, gcoef=gcoef, terms=terms, gy=gy, info=info):
            wb.loss_terms_sums(y, target, SKIP, COEFF, sums6=sums6, ws=ws)
            wb.loss_terms_coef(sums6, n, eps, WEIGHTS, COEFF, gcoef=gcoef, terms=terms)
            if grad:
                wb.loss_terms_grad(y, target, gcoef, SKIP, COEFF, gy=gy)
            info["stage"] = terms

        def composed(grad, y=y, target=target, n=n, info=info):
            yv = y.detach().requires_grad_(grad)
            with torch.set_grad_enabled(grad):
                o, t = yv[SKIP:], target[SKIP:]
                e = o - t
                S, E = torch.sum(e * e), torch.sum(o * o) + eps
                fo = torch.cat([o[:1], o[1:] - COEFF * o[:-1]])
                fe = torch.cat([e[:1], e[1:] - COEFF * e[:-1]])
                Sp, Ep = torch.sum(fe * fe), torch.sum(fo * fo) + eps
                loss = (WEIGHTS[0] * S / n + WEIGHTS[1] * torch.sqrt(S / E / n) + WEIGHTS[2] * torch.sqrt(Sp / Ep / n)
                        + WEIGHTS[3] * torch.abs(torch.sum(o) - torch.sum(t)) / n)
                if grad:
                    info["gy_torch"], = torch.autograd.grad(loss, yv)
            info["torch"] = loss.detach()

        kept, every = (T - SKIP) * B, T * B
        for name, fn, least in (("stage: sums + coef + grad", lambda s=stage: s(True), 8 * kept + 8 * kept + 4 * every),
                                ("stage: sums + coef", lambda s=stage: s(False), 8 * kept),
                                ("torch: loss + autograd dL/dy", lambda c=composed: c(True), None),
                                ("torch: loss only", lambda c=composed: c(False), None)):
            rows.append({"what": name, "B": B, "T": T, "skip": SKIP, "weights": WEIGHTS, "coeff": COEFF, "least_bytes": least, "info": info})
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
    for i, row in enumerate(rows):
        info = row.pop("info")
        med = float(np.median(samples[i]))
        row.update({"ms": med, "ms_min": float(np.min(samples[i])), "ms_max": float(np.max(samples[i])), "reps": REPS,
                    "calls_per_rep": INNER, "loss_stage": float(info["stage"][4]), "loss_torch_f32": float(info["torch"])})
        if row["least_bytes"] is not None:
            row["least_bytes_per_s"] = row["least_bytes"] / med * 1e3
        j = i + 2 if i % 4 < 2 else i - 2                     # the row of the other implementation, same shape, same work
        row["ms_ratio_to_other"] = med / float(np.median(samples[j]))
        row["other"] = rows[j]["what"]
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--worker", action="store_true", help="time the rows in this process")
    a = ap.parse_args()
    sys.exit(work() if a.worker else drive())
