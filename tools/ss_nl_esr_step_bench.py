"""The HPF diode clipper's MSE + ESR training step (a small tree under a DiodePair root, csrc/wdf_ss_nl_step.h) at 8192 x 4096
and 1340 x 2048 on one MI355X, skip = 50, resident component values, without the optimizers.  Per shape, three rows timed in
turn in ONE process:
(a) the one-pass MSE + ESR step of the resident tree, Circuit._mse_esr_nl_step (wdf_ss_probe_adam + wdf_ss_nl_step_esr);
(b) the one-pass MSE step, Circuit.mse on a resident circuit (wdf_ss_probe_adam + wdf_ss_nl_step_mse);
(c) the composed mse_esr path as Circuit.mse_esr ran it before the one-pass step existed -- a resident circuit built with
    force_generic=True: the device probe, the forward, torch's reductions on y[skip:], the reverse sweep.
Every row includes tape.gradient to the five components.

Without arguments this is the driver: it starts one worker process per shape (`--shape 8192x4096`, then `--shape 1340x2048`), each
under its own `timeout`, stops at the first one that fails, prints the workers' JSON rows and writes them to
profiles/r11_ss_nl_esr_step.jsonl.  The driver itself never opens the GPU.

Timing as tools/asym_esr_step_bench.py: the rows of a shape are warmed up, then timed in turn, REPS rounds of INNER calls each
between two device events; a row reports the median of its REPS samples and their min-max."""
import argparse
import json
import os
import subprocess
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "r11_ss_nl_esr_step.jsonl")
SHAPES = ("8192x4096", "1340x2048")
SKIP = 50
REPS, INNER, WARMUP = 20, 5, 3
WORKER_TIMEOUT_S = 300
FS = 48000
THETA = (33.0e3, 1.0e3, 22.0e-9, 4.352e-9, 25.85e-3 * 1.906)


def drive():
    rows = []
    for shape in SHAPES:
        cmd = ["timeout", "-k", "10", str(WORKER_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--shape", shape]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"ss_nl_esr_step_bench: the {shape} worker ended with status {p.returncode}; nothing more is started, "
                  f"{OUT} is left as it was", file=sys.stderr)
            return p.returncode
        rows += [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    with open(OUT, "w") as f:
        f.write("\n".join(rows) + "\n")
    return 0


def work(shape):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib"))
    import tf_wdf as wdf
    from wdf_hip import binding as wb

    tf = wdf.tf
    B, T = (int(v) for v in shape.split("x"))
    wb.require_gpu()

    def hpf(**kw):
        R = wdf.Resistor(THETA[0], True)
        Vs = wdf.ResistiveVoltageSource(THETA[1], trainable=True)
        C = wdf.Capacitor(THETA[2], FS, True)
        top = wdf.Parallel(R, wdf.Series(Vs, C))
        dp = wdf.DiodePair(top, THETA[3], Vt=THETA[4], nDiodes=1.0, N_up=1, N_down=1, trainable=True)
        return wdf.Circuit(top, dp, R, **kw), [R.R, Vs.R, C.C, dp.Is, dp.nVt]

    g = torch.Generator(device="cpu").manual_seed(77)
    x = (torch.randn((B, T), generator=g) * 1.2).cuda()
    teacher, _ = hpf()
    tgt = (teacher(x) * 0.8).as_subclass(torch.Tensor).detach().contiguous()

    circuits = {name: hpf(**kw) for name, kw in (("esr", {}), ("mse", {}), ("composed", {"force_generic": True}))}
    for c, _ in circuits.values():
        c.to_device()
    keep = {}

    def run(name, loss_of):
        circ, params = circuits[name]

        def fn():
            with tf.GradientTape() as tape:
                loss = loss_of(circ)
            keep[name] = (loss, tape.gradient(loss, params))
        return fn

    fns = [run("esr", lambda c: c._mse_esr_nl_step(c._nl_step_tree(x, tgt, SKIP), x, tgt, SKIP)), run("mse", lambda c: c.mse(x, tgt)),
           run("composed", lambda c: c.mse_esr(x, tgt, skip=SKIP))]

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

    def timing(ms):
        med = float(np.median(ms))
        return {"ms": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": len(ms), "calls_per_rep": INNER,
                "samples_per_s": B * T / med * 1e3}

    te, tm, tc = (timing(s) for s in samples)
    grads = {k: np.array([float(v) for v in keep[k][1]]) for k in keep}
    loss = {k: float(keep[k][0]) for k in keep}
    assert getattr(keep["esr"][0], "_wdf_fused", None) is not None and getattr(keep["composed"][0], "_wdf_fused", None) is None
    tree = circuits["esr"][0]._tree
    ctl = tree.read_ctl([e for e in tree.cache.values() if e.get("loss") == "mse+esr"][0])
    common = {"circuit": "HPF diode clipper, N 1/1", "B": B, "T": T, "skip": SKIP}
    print(json.dumps({**common, "step": "one pass MSE + ESR: Circuit._mse_esr_nl_step, resident", **te, "loss": loss["esr"],
                      "loss_rel_to_composed": abs(loss["esr"] - loss["composed"]) / loss["composed"],
                      "grad_max_rel_to_composed": float(np.max(np.abs(grads["esr"] - grads["composed"]) / np.abs(grads["composed"]))),
                      "ctl": ctl, "slowest_vs_composed_fastest": te["ms_max"] / tc["ms_min"],
                      "speedup_median_vs_composed": tc["ms"] / te["ms"], "ratio_median_to_mse_step": te["ms"] / tm["ms"]}), flush=True)
    print(json.dumps({**common, "step": "one pass MSE: Circuit.mse, resident", **tm, "loss": loss["mse"]}), flush=True)
    print(json.dumps({**common, "step": "composed: resident probe + forward + torch MSE + ESR + reverse sweep (force_generic)", **tc,
                      "loss": loss["composed"]}), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", choices=SHAPES, help="worker: time this shape's three rows in this process")
    a = ap.parse_args()
    sys.exit(work(a.shape) if a.shape else drive())
