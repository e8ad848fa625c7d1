"""The RC low-pass's MSE + ESR training step (lpf.py's tree: a linear tree under the ideal source, csrc/wdf_ss_step.h) at
8192 x 4096 and 1340 x 2048 on one MI355X, skip = 50, resident component values, without the optimizers.  Per shape, three rows
timed in turn in ONE process, each `circ.mse_esr(x, target, 50)` (or `circ.mse`) + tape.gradient to R and C:
(a) Circuit.mse_esr with lowering.LIN_ESR_STEP_SERVES on: the one-pass MSE + ESR step (wdf_ss_probe_adam + wdf_ss_lin_step_esr);
(b) the one-pass MSE step, Circuit.mse (wdf_ss_probe_adam + wdf_ss_lin_step_mse);
(c) Circuit.mse_esr with the flag off: the composed path -- the device probe, the forward with its stash, torch's reductions on
    y[skip:], the reverse sweep, the probe's chain rule -- which is what mse_esr ran on this circuit before the step existed.

Without arguments this is the driver: it starts one worker process per shape (`--shape 8192x4096`, then `--shape 1340x2048`), each
under its own `timeout`, stops at the first one that fails, prints the workers' JSON rows and writes them to
profiles/r17_ss_lin_esr_step.jsonl.  The driver itself never opens the GPU.

Timing as tools/ss_nl_esr_step_bench.py: the rows of a shape are warmed up, then timed in turn, REPS rounds of INNER calls each
between two device events; a row reports the median of its REPS samples and their min-max.  The flag goes to True only if row (a)'s
slowest sample beats row (c)'s fastest at both shapes (`slowest_vs_composed_fastest` < 1)."""
import argparse
import json
import os
import subprocess
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(_R, "profiles", "r17_ss_lin_esr_step.jsonl")
SHAPES = ("8192x4096", "1340x2048")
SKIP = 50
REPS, INNER, WARMUP = 20, 5, 3
WORKER_TIMEOUT_S = 300
FS = 48000


def drive():
    rows = []
    for shape in SHAPES:
        cmd = ["timeout", "-k", "10", str(WORKER_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--shape", shape]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"ss_lin_esr_step_bench: the {shape} worker ended with status {p.returncode}; nothing more is started, "
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
    from wdf_hip import lowering

    tf = wdf.tf
    B, T = (int(v) for v in shape.split("x"))
    wb.require_gpu()

    def lpf(R=1000.0, C=1.0e-6):
        R1, C1 = wdf.Resistor(R, True), wdf.Capacitor(C, FS, True)
        return wdf.Circuit(wdf.Inverter(wdf.Series(R1, C1)), wdf.IdealVoltageSource(), C1), [R1.R, C1.C]

    g = torch.Generator(device="cpu").manual_seed(77)
    x = (torch.randn((B, T), generator=g) * 1.2).cuda()
    teacher, _ = lpf(315.0, 0.7e-6)                               # (the values lpf.py aims for: fc = 720 Hz)
    with torch.no_grad():
        tgt = teacher(x).as_subclass(torch.Tensor).detach().contiguous()

    circuits = {name: lpf() for name in ("esr", "mse", "composed")}
    for c, _ in circuits.values():
        c.to_device()
    keep = {}

    def run(name, loss_of, serves):
        circ, params = circuits[name]

        def fn():
            lowering.LIN_ESR_STEP_SERVES = serves
            with tf.GradientTape() as tape:
                loss = loss_of(circ)
            keep[name] = (loss, tape.gradient(loss, params))
        return fn

    fns = [run("esr", lambda c: c.mse_esr(x, tgt, SKIP), True), run("mse", lambda c: c.mse(x, tgt), False),
           run("composed", lambda c: c.mse_esr(x, tgt, SKIP), False)]

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
    common = {"circuit": "RC low-pass (lpf.py)", "B": B, "T": T, "skip": SKIP}
    print(json.dumps({**common, "step": "one pass MSE + ESR: Circuit.mse_esr with LIN_ESR_STEP_SERVES, resident", **te, "loss": loss["esr"],
                      "loss_rel_to_composed": abs(loss["esr"] - loss["composed"]) / loss["composed"],
                      "grad_max_rel_to_composed": float(np.max(np.abs(grads["esr"] - grads["composed"]) / np.abs(grads["composed"]))),
                      "slowest_vs_composed_fastest": te["ms_max"] / tc["ms_min"],
                      "speedup_median_vs_composed": tc["ms"] / te["ms"], "ratio_median_to_mse_step": te["ms"] / tm["ms"]}), flush=True)
    print(json.dumps({**common, "step": "one pass MSE: Circuit.mse, resident", **tm, "loss": loss["mse"]}), flush=True)
    print(json.dumps({**common, "step": "composed: Circuit.mse_esr with the flag off (resident probe + forward + torch MSE + ESR + "
                                        "reverse sweep)", **tc, "loss": loss["composed"]}), flush=True)
    return 0


def kernels(shape):
    """--kernel: pass 2 alone (ss_lin_step_kernel, between the events the C call brackets it with) through binding.ss_lin_step_mse /
    ss_lin_step_esr on the two-capacitor instantiations no circuit of this tool reaches: (2,2) at one and two sequences per lane,
    (2,1) at two; one per lane is chosen by a y buffer at 4 mod 8 bytes.  One JSON row per (tree, width, loss), nothing written."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib"))
    from wdf_hip import binding as wb

    B, T = (int(v) for v in shape.split("x"))
    wb.require_gpu()
    rng = np.random.default_rng(11)
    target = torch.as_tensor(rng.standard_normal((T, B)).astype(np.float32), device="cuda")
    for ns, ni, width in ((2, 2, 1), (2, 2, 2), (2, 1, 2)):
        q = np.array([[1.0, 0.4], [-0.3, 1.0]])
        A = q @ np.diag([0.98, 0.6]) @ np.linalg.inv(q)
        n_coef = wb.lib().wdf_ss_ncoef(ns, ni)
        coef = np.zeros(n_coef + 1)                              # SSCoef order: A, Bx, E, ca, da, cy, dy, fy (+ the port resistance)
        coef[:ns * ns] = A.reshape(-1)
        coef[ns * ns:ns * ns + ns * ni] = 0.02 * rng.uniform(-1.0, 1.0, ns * ni)
        o_cy = ns * ns + ns * ni + 2 * ns + ni
        coef[o_cy:o_cy + ns + ni] = rng.uniform(-1.0, 1.0, ns + ni)
        coef_d = torch.as_tensor(coef.astype(np.float32), device="cuda")
        jac = torch.as_tensor(rng.uniform(-1.0, 1.0, (n_coef + 1, 3)), device="cuda")
        x = torch.as_tensor(rng.standard_normal((T, ni, B)).astype(np.float32), device="cuda")
        y = torch.empty((T * B + 2,), dtype=torch.float32, device="cuda")[(2 if width == 2 else 1):][:T * B].view(T, B)
        assert y.data_ptr() % 8 == (0 if width == 2 else 4)
        n_chunks = max(1, min(T // 32, (4 * 256 * 64 * width) // B))
        steps = {"mse": lambda ws: wb.ss_lin_step_mse(x, coef_d, jac, target, 2.0 / (B * T), n_chunks, ws=ws, y=y),
                 "mse+esr": lambda ws: wb.ss_lin_step_esr(x, coef_d, jac, target, SKIP, n_chunks, ws=ws, y=y)}
        for loss, fn in steps.items():
            ws = fn(None)["ws"]
            for _ in range(WARMUP):
                fn(ws)
            ms = []
            for _ in range(REPS):
                e0, e1 = wb.Event(), wb.Event()
                wb.Event.bracket_next(e0, e1)
                fn(ws)
                torch.cuda.synchronize()
                ms.append(e0.elapsed_ms(e1))
            print(json.dumps({"kernel": f"ss_lin_step_kernel<{ns},{ni},{'v2f' if width == 2 else 'float'}>", "loss": loss, "B": B, "T": T,
                              "n_chunks": n_chunks, "ms": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)),
                              "reps": len(ms)}), flush=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", choices=SHAPES, help="worker: time this shape's three rows in this process")
    ap.add_argument("--kernel", action="store_true", help="with --shape: time pass 2 alone on the two-capacitor instantiations instead")
    a = ap.parse_args()
    if a.kernel and not a.shape:
        ap.error("--kernel needs --shape")
    sys.exit((kernels(a.shape) if a.kernel else work(a.shape)) if a.shape else drive())
