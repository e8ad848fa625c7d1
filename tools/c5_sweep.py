"""BASELINE config 5: asymmetric (two-different-diode) clipper -- Newton on the exact pair in fp64 (tolerance sweep) and in
fp32, and the fp32 Wright-omega closed form (a model approximation, kept for comparison): error against the oracle's exact
solve and samples/s on one MI355X, forward sequential, forward in time chunks, forward + reverse sweep.

Timing: the rows of a group are warmed up, then timed in turn, REPS rounds of INNER calls each between two device events
(so the rows of a group see the same machine in the same seconds); a row reports the median of its REPS samples and their
min-max.  Prints one JSON line per row; copy the output under profiles/."""
import json
import sys
import numpy as np
import torch
import os
_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_R, "differentiable-wdfs_amd", "lib")); sys.path.insert(0, os.path.join(_R, "oracle"))
from wdf_hip import binding as wb, workload
import oracle as O

FS = workload.FS
THETA6 = np.array([4.352e-9, 25.85e-3 * 1.906, 2.0e-6, 25.85e-3 * 1.4, 45.0e3, 4.7e-9])
B, T = 8192, 4096
x = workload.sweep_batch(B, T)
xd = torch.as_tensor(x, device="cuda")
th = torch.tensor(THETA6, dtype=torch.float32, device="cuda")
t32 = THETA6.astype(np.float32).astype(np.float64)
pick = np.random.default_rng(0).choice(B, 32, replace=False)
ref = O.clipper_asym_fwd(t32, FS, x[pick].astype(np.float64))
pk = torch.as_tensor(pick, device="cuda")


REPS, INNER, WARMUP = 20, 5, 3
rows = []


def time_group(fns):
    """[ms samples] per callable: WARMUP calls of each, then REPS rounds over the group, INNER calls per sample"""
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


def timing(ms):
    med = float(np.median(ms))
    return {"ms": med, "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": len(ms), "calls_per_rep": INNER,
            "samples_per_s": B * T / med * 1e3, "samples_per_s_min": B * T / float(np.max(ms)) * 1e3,
            "samples_per_s_max": B * T / float(np.min(ms)) * 1e3}


def yerr(y):
    return float(np.max(np.abs(y[:, pk].cpu().numpy() - ref)))


# ---- forward, sequential --------------------------------------------------------------------------------------------------
seq = [("fp32 Wright-omega closed form (1 FSC step; a model approximation)", wb.ASYM_OMEGA_F32, 1e-12, 1)]
seq += [(f"fp64 Newton tol={tol:g}", wb.ASYM_NEWTON_F64, tol, 50) for tol in (1e-4, 1e-6, 1e-8, 1e-10, 1e-12, 1e-14)]
seq += [(f"fp32 Newton tol={tol:g} (floor 4.8e-7)", wb.ASYM_NEWTON_F32, tol, 50) for tol in (1e-4, 1e-12)]
times = time_group([(lambda m=m, tol=tol, mi=mi: wb.clipper_asym_fwd(xd, th, FS, m, tol=tol, max_iter=mi)) for _, m, tol, mi in seq])
for (name, m, tol, mi), ms in zip(seq, times):
    y, _, it = wb.clipper_asym_fwd(xd, th, FS, m, tol=tol, max_iter=mi, want_iters=True)
    row = {"root": name, "step": "forward, sequential", **timing(ms), "max_abs_err_vs_exact": yerr(y)}
    if m != wb.ASYM_OMEGA_F32:
        row["mean_newton_iters_per_wave_step"] = float(it.sum()) / (it.numel() * T)
    rows.append(row)

# ---- forward in K time chunks (wdf_clipper_asym_fwd_tp: verified on the device) ------------------------------------------
W = 192
tpc = []
for K in (4, 8, 16, 32):
    tpc.append((f"fp32 Wright-omega closed form, {K} time chunks", wb.ASYM_OMEGA_F32, 1e-12, 1, K))
    tpc += [(f"fp64 Newton tol={tol:g}, {K} time chunks", wb.ASYM_NEWTON_F64, tol, 50, K) for tol in (1e-6, 1e-12)]
    tpc.append((f"fp32 Newton tol=1e-12 (floor 4.8e-7), {K} time chunks", wb.ASYM_NEWTON_F32, 1e-12, 50, K))
times = time_group([(lambda m=m, tol=tol, mi=mi, K=K: wb.clipper_asym_fwd_tp(xd, th, FS, m, K, W, tol=tol, max_iter=mi))
                    for _, m, tol, mi, K in tpc])
for (name, m, tol, mi, K), ms in zip(tpc, times):
    y, _, _, st = wb.clipper_asym_fwd_tp(xd, th, FS, m, K, W, tol=tol, max_iter=mi)
    rows.append({"root": name, "step": "forward, time chunks", **timing(ms), "max_abs_err_vs_exact": yerr(y),
                 "verify": wb.mlp_tp_status(st)})


# ---- forward + reverse sweep (gradients to all six parameters of L = mean((y - y*)^2)) --------------------------------------
# error columns: the gradient on 32 picked sequences against fp64 central differences of the oracle's exact forward (Newton
# mode: the model being differentiated; OMEGA mode differentiates its own closed form, so its distance to the exact model's
# gradient is MODEL error) and, Newton mode, the time-parallel sweep against the sequential one that re-solves every root.
th_star = torch.tensor(THETA6 * np.array([1.2, 0.95, 0.8, 1.05, 0.9, 1.1]), dtype=torch.float32, device="cuda")
tgt, _, _ = wb.clipper_asym_fwd(xd, th_star, FS, wb.ASYM_NEWTON_F64, tol=1e-12)
tgt_pick = tgt[:, pk].cpu().numpy().astype(np.float64)
x_pick = x[pick].astype(np.float64)


def fd_grad():
    g = np.zeros(6)
    for i in range(6):
        h = 1e-6 * t32[i]
        tp_, tm_ = t32.copy(), t32.copy()
        tp_[i] += h
        tm_[i] -= h
        lp = np.mean((O.clipper_asym_fwd(tp_, FS, x_pick) - tgt_pick) ** 2)
        lm = np.mean((O.clipper_asym_fwd(tm_, FS, x_pick) - tgt_pick) ** 2)
        g[i] = (lp - lm) / (2 * h)
    return g


g_fd = fd_grad()
xp_d = xd[pk].contiguous()


def picked_grad(mode, kb):
    """gradient and forward error on the 32 picked sequences"""
    y, zT, _, zs = wb.clipper_asym_fwd(xp_d, th, FS, mode, tol=1e-12, want_zT=True, want_stash=True)
    gy = (2.0 * (y - tgt[:, pk]) / y.numel()).contiguous()
    err = float(np.max(np.abs(y.cpu().numpy() - ref)))
    if kb == 0:
        return wb.clipper_asym_bwd(xp_d, th, FS, zs, gy).cpu().numpy().astype(np.float64), err
    return wb.clipper_asym_bwd_tp(xp_d, th, FS, mode, zs, zT, gy, kb).cpu().numpy().astype(np.float64), err


def fwd_bwd(mode, kf, kb, tol=1e-12):
    def once():
        if kf > 1:
            y, zT, zs, _ = wb.clipper_asym_fwd_tp(xd, th, FS, mode, kf, W, tol=tol, want_stash=True, want_zT=True)
        else:
            y, zT, _, zs = wb.clipper_asym_fwd(xd, th, FS, mode, tol=tol, want_stash=True, want_zT=True)
        gy = (y - tgt) * (2.0 / y.numel())
        if kb == 0:
            return wb.clipper_asym_bwd(xd, th, FS, zs, gy, tol=tol)
        return wb.clipper_asym_bwd_tp(xd, th, FS, mode, zs, zT, gy, kb)
    return once


g_seq_pick, _ = picked_grad(wb.ASYM_NEWTON_F64, 0)
MODES = (("fp64 Newton tol=1e-12", wb.ASYM_NEWTON_F64), ("fp32 Newton tol=1e-12 (floor 4.8e-7)", wb.ASYM_NEWTON_F32),
         ("fp32 Wright-omega closed form (a model approximation)", wb.ASYM_OMEGA_F32))
# the sequential reverse sweep (fp64 Newton re-solve per step, 10 ms a call) is timed in a group of its own
slow = [("fp64 Newton tol=1e-12", wb.ASYM_NEWTON_F64, kf, 0) for kf in (1, 16)]
# all modes side by side, the same plans, timed in turn
fast = [(name, mode, kf, kb) for kf, kb in ((1, 1), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32)) for name, mode in MODES]
for group in (slow, fast):
    times = time_group([fwd_bwd(mode, kf, kb) for _, mode, kf, kb in group])
    for (name, mode, kf, kb), ms in zip(group, times):
        gp, err = picked_grad(mode, kb)
        row = {"root": name, "step": "forward + reverse sweep", "fwd_chunks": kf,
               "reverse": "sequential, Newton re-solve per step" if kb == 0 else f"time-parallel, {kb} chunks, no re-solve",
               **timing(ms), "max_abs_err_vs_exact": err,
               "max_rel_grad_err_vs_fd_of_exact_model_32seq": float(np.max(np.abs(gp - g_fd) / np.abs(g_fd)))}
        if mode != wb.ASYM_OMEGA_F32:
            row["max_rel_grad_err_vs_sequential_sweep_32seq"] = float(np.max(np.abs(gp - g_seq_pick) / np.abs(g_seq_pick)))
        rows.append(row)
for r in rows:
    print(json.dumps(r))
