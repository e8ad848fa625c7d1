#!/usr/bin/env python3
"""bench.py -- the BASELINE.json metric on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" = one pass of the hot path over one batch: diode-clipper forward over
B x T samples (y written), MSE against synthetic targets, the gradient dL/d{Is, nVt, R, C}, (N > 1)
one RCCL all-reduce of the fused [loss, grads] buffer, and the on-device Adam update.  By default forward,
loss and gradient run as ONE pass over the data (wdf_clipper_step_mse_tp: the gradient is carried forward in
time as the state's tangent, no state stash); --two-kernel runs the forward kernel + reverse-sweep kernel
pair instead.  --loss mse+esr (the scripts' training loss past 50 samples) takes the same one-pass form.
Workload = BASELINE.json configs[2]: 1N4148 diode clipper fwd+bwd, batch 8192 sequences x 4096
samples @ 48 kHz per GPU ("scaling": "weak": every rank holds its own 8192-sequence shard of the
global batch; --scaling strong splits ONE 8192-sequence batch over the ranks instead).
Inputs are resident in HBM before the timed region.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the line: the contract fields, the step's
configuration, `kernel_ms` (min / median / max of the HIP-event times of the recurrence kernel(s) of the
timed steps) and the HBM roofline priced with them.  --full adds the measurements that take runs of
their own: `parity` (the bench path's y and fused gradient at full size against the CPU oracle, checked
after the timed region), `value_batch_major` (the same step with x handed over as [B,T], the reference
scripts' layout), the other scaling curve (N > 1), value_cold, strong_proxy, value_sustained,
value_fwd_1024, the copy bandwidth beside the roofline and the CPU baseline.

--dump-outputs DIR writes what the last timed step computed, as float32 .npy files: sse [1], grad [4]
(dL/d{Is, nVt, R, C}), theta [4] (the parameters after that step's update) and y_sample [256, T] (y of
256 sequences of rank 0's shard, picked with a fixed seed).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "differentiable-wdfs_amd", "lib"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from wdf_hip import binding, dist as wdist, engine, workload  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec
PMC_TRAFFIC_GLOB = os.path.join(REPO, "profiles", "*_pmc_traffic.json")
BYTES_FWD = 12                 # x 4 + y 4 + z-stash 4   (fwd 8 B + 4 B stash)
BYTES_BWD = 12                 # x 4 + z-stash 4 + target 4: the fused-MSE sweep rebuilds y from the stash and forms
                               # dL/dy from the target itself (SURVEY 8d counts x, z and dL/dy: the same 12 B)
BYTES_STEP = 24                # SURVEY 8d's figure for forward + backward, the unit one launch of the one-pass step processes
BYTES_STEP_MOVED = 12          # what that kernel itself has to move: x 4 + target 4 + y 4 (no stash, x read once)
N_SIMD = 1024                  # 256 CUs x 4
VALU_CLOCK_GHZ = 2.4           # MI355X_MICROARCH.md: peak engine clock (the chip sustains ~1.9-2.0 under this kernel: DVFS)
SQ_GLOB = os.path.join(REPO, "profiles", "*_sq_counters.json")


def measured_traffic(kernel, cfg):
    """(HBM bytes per launch of `kernel`, source file) from the committed rocprofv3 PMC passes of
    this same command (profiles/*_pmc_traffic.json: FETCH_SIZE x2 + WRITE_SIZE, see their _doc,
    collected by tools/pmc_traffic.sh) -- only from a file taken on the configuration being run;
    otherwise (None, None)."""
    return _committed_pass(PMC_TRAFFIC_GLOB, kernel, cfg, lambda k: k["traffic_bytes"])


def measured_valu_cycles(kernel, cfg):
    """(VALU-active cycles per launch of `kernel`, summed over all waves; source file) from the committed SQ pass of this
    command (profiles/*_sq_counters.json, tools/pmc_sq.sh: SQ_ACTIVE_INST_VALU counts quad-cycles) on the configuration
    being run; otherwise (None, None)."""
    return _committed_pass(SQ_GLOB, kernel, cfg, lambda k: 4.0 * k["SQ_ACTIVE_INST_VALU"])


def library_identity():
    """What the committed counter passes are matched on: the first 16 hex digits of the sha256 of the library this process
    loaded, and of the sources the diode-clipper translation unit's DEVICE code is compiled from -- its .hip file, the kernel
    headers it includes, the Makefile's flags; not include/wdf_hip.h, whose declarations of other families' entry points do
    not reach a kernel -- so a pass stays valid when only ANOTHER kernel family changed."""
    import hashlib
    out = {"path": os.path.relpath(binding.LIB_PATH, REPO), "sha16": None, "clipper_src_sha16": None}
    try:
        out["sha16"] = hashlib.sha256(open(binding.LIB_PATH, "rb").read()).hexdigest()[:16]
    except OSError:
        pass
    csrc = os.path.join(REPO, "differentiable-wdfs_amd", "csrc")
    h = hashlib.sha256()
    try:
        for name in ("Makefile", "wdf_capi_clipper.hip", "wdf_capi_common.h", "wdf_clipper.h", "wdf_clipper_fused.h", "wdf_omega.h",
                     "wdf_omega64.h", "wdf_asym.h", "wdf_vec.h", "wdf_optim.h", "wdf_elementwise.h"):
            h.update(open(os.path.join(csrc, name), "rb").read())
        out["clipper_src_sha16"] = h.hexdigest()[:16]
    except OSError:
        pass
    return out


def _committed_pass(pattern, kernel, cfg, value):
    """The newest committed counter file taken ON THIS LIBRARY (the file's stamp -- library sha or the clipper translation
    unit's source sha -- must equal this run's: a pass of another build is refused) whose configuration is the one being
    run: batch, layout, loss and the kernel's own chunk count must match; among those the one whose warm-up (the device
    controller moves it by a few 16-step units from run to run: < 3 % of the kernel's work) is closest."""
    import glob
    ident = library_identity()
    best = None
    paths = sorted(glob.glob(pattern), reverse=True) + sorted(glob.glob(pattern.replace(os.sep + "profiles" + os.sep, os.sep + "gpurun_out" + os.sep)), reverse=True)
    for path in paths:
        try:
            d = json.load(open(path))
            c = d.get("config")
            lib = d.get("library") or {}
            same_build = (lib.get("sha16") is not None and lib.get("sha16") == ident["sha16"]) or \
                         (lib.get("clipper_src_sha16") is not None and lib.get("clipper_src_sha16") == ident["clipper_src_sha16"])
            if not c or not same_build or kernel not in d["kernels"]:
                continue
            if all(c.get(k, "mse" if k == "loss" else None) == v for k, v in cfg.items() if k != "fwd_warmup_steps"):
                dist = abs((c.get("fwd_warmup_steps") or 0) - (cfg.get("fwd_warmup_steps") or 0))
                if best is None or dist < best[0]:
                    best = (dist, value(d["kernels"][kernel]), os.path.relpath(path, REPO))
        except (OSError, ValueError, KeyError, TypeError):
            pass
    return (None, None) if best is None else (best[1], best[2])


def _oracle():
    """The CPU oracle: CHECKER and reported baseline only (never on the measured path)."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import oracle as O
    return O


def cgroup_cpu_quota():
    """(text of the cgroup's CPU limit, cores it allows or None): cgroup v2 `cpu.max` ("max 100000" / "<quota> <period>"),
    else v1 `cpu.cfs_quota_us` / `cpu.cfs_period_us`.  What a box exposes (`sched_getaffinity`) and what its cgroup lets
    run are two numbers; the line prints both."""
    try:
        txt = open("/sys/fs/cgroup/cpu.max").read().strip()
        q, per = txt.split()
        return txt, (None if q == "max" else float(q) / float(per))
    except (OSError, ValueError):
        pass
    try:
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return f"{q} {per} (cgroup v1)", (None if q <= 0 else q / per)
    except (OSError, ValueError):
        return None, None


def cpu_baseline(T, fs, hold_s=4.0, warm_floor_s=2.0):
    """The oracle's fused fwd + MSE + bwd step ("port": C restatement of the reference algorithm, OpenMP over sequences)
    timed on the host cores on a bounded sample of the same workload.  Checker code used as a reported baseline only.

    The thread count is CALIBRATED, and every candidate is measured warm: the first passes at a new thread count pay for the
    OpenMP pool's threads and for the page faults of the per-thread tapes and the output array (measured in the build
    container, 8 threads: 5.6, 6.6, 5.5, 4.7, 5.5, 17, 48, 54, 54 M samples/s pass after pass), so a candidate's passes are
    discarded for at least 2 s and until two in a row agree within 10 %, and its figure is the best of three timed runs of >= 0.25 s each, with
    >= 32 sequences per thread.  Reported: the best figure (`value`, `cores`), the figure with every allowed core running
    (`all_cores`), one core (`value_one_core`), the cgroup's quota next to the affinity count, and the whole table."""
    O = _oracle()
    avail = len(os.sched_getaffinity(0))
    quota_txt, quota_cores = cgroup_cpu_quota()
    th = workload.clipper_theta()
    cands = {max(1, avail >> k) for k in range(0, 9)}
    if quota_cores is not None:
        cands.add(max(1, min(avail, int(round(quota_cores)))))
    cands = sorted(cands, reverse=True)
    # a cold plateau lasts over a second (the container: five 0.2 s passes at a tenth of the warm rate, then a jump), and looks
    # steady while it lasts: every multi-thread candidate is warmed for at least this long
    # (`warm_floor_s`, default 2 s; the CPU suite passes a shorter one)
    data = {}

    def batch(nt):
        Bs = min(8192, max(64, 32 * nt))
        if Bs not in data:
            x = workload.sweep_batch(8192, T, b0=0, b1=Bs)
            data[Bs] = (x, O.clipper_fwd(workload.target_theta(), fs, x, dtype=np.float32, n_threads=avail))
        return (Bs,) + data[Bs]

    def timed(nt, Bs, x, tgt, min_s):
        t0 = time.perf_counter()
        n = 0
        while True:
            O.clipper_mse_step(th, fs, x, tgt, n_threads=nt)
            n += 1
            dt = time.perf_counter() - t0
            if dt >= min_s:
                return Bs * T * n / dt

    table = []
    for nt in cands:
        Bs, x, tgt = batch(nt)
        t_c = time.perf_counter()
        prev, n_warm = None, 0
        warm_s = 0.5 if nt == 1 else warm_floor_s
        while True:                                                           # warm: discarded passes
            r = timed(nt, Bs, x, tgt, 0.0)
            n_warm += 1
            el = time.perf_counter() - t_c
            if (el >= warm_s and prev is not None and abs(r - prev) <= 0.1 * max(r, prev)) or el >= 2.5 * warm_s:
                break
            prev = r
        runs = [timed(nt, Bs, x, tgt, 0.25) for _ in range(3)]
        table.append({"threads": nt, "sequences": Bs, "warm_passes_discarded": n_warm,
                      "best": max(runs), "median": sorted(runs)[1]})
    best = max(table, key=lambda e: e["best"])
    allc = next(e for e in table if e["threads"] == avail)
    one = next(e for e in table if e["threads"] == 1)
    # the reported figure: the best thread count held for the rest of the budget (warm already)
    Bs, x, tgt = batch(best["threads"])
    t0 = time.perf_counter()
    value = max(best["best"], timed(best["threads"], Bs, x, tgt, hold_s))
    dt = time.perf_counter() - t0
    return {"value": value, "unit": "samples/s", "cores": best["threads"], "kind": "port",
            "logical_cpus": avail, "cgroup_cpu_max": quota_txt, "cgroup_cores": quota_cores,
            "cores_note": (f"{avail} logical CPUs in the affinity mask, cgroup quota "
                           f"{'none' if quota_cores is None else f'{quota_cores:g} cores'}; best throughput at {best['threads']} "
                           f"OpenMP threads"),
            "all_cores": {"threads": avail, "value": allc["best"], "median": allc["median"]},
            "value_one_core": one["best"],
            "calibration": table,
            "sample": f"oracle_clipper_mse_step_f32 (fused fwd + MSE + bwd) on {Bs} sequences x {T} samples of the same sweep "
                      f"workload, OpenMP {best['threads']} threads: best of three warm >= 0.25 s runs and a {dt:.1f} s hold; every "
                      f"candidate of {cands} measured the same way (>= 32 sequences per thread, passes discarded for >= 2 s and until two agree "
                      f"within 10 %)"}


def parity_check(stepper, theta, xk, x_host, target, fs, n_global, fused, g_first=None):
    """After the timed region: one more step (no update) of the BENCH PATH ITSELF (same
    stepper, same plan, same warm-start state, no update) at the parameters training has reached, against
    the fp64 CPU oracle over the whole batch: every output sample and the four gradient components."""
    O = _oracle()
    th_host = theta.detach().cpu().numpy().astype(np.float64)
    if fused:
        sse, g = stepper.step_fused(theta, xk, target)
    else:
        stepper.forward(theta, xk)
        sse, g = stepper.backward(theta, xk, target)
    torch.cuda.synchronize()
    y = stepper.y.cpu().numpy()
    t0 = time.perf_counter()
    loss_ref, g_ref, y_ref = O.clipper_mse_step(th_host, fs, x_host.astype(np.float64), target.cpu().numpy().astype(np.float64),
                                                dtype=np.float64, n_threads=len(os.sched_getaffinity(0)))
    got = g.cpu().numpy().astype(np.float64)
    # max_rel_grad: every component against its OWN magnitude at the final theta -- after a long run the gradient has shrunk
    # towards 0 (the loss is near its minimum) and this ratio grows with the cancellation in the sum;
    # max_grad_err_vs_first_step: the same absolute errors against the components' magnitudes at the run's first step
    return {"max_abs_y": float(np.max(np.abs(y - y_ref))),
            "max_rel_grad": float(np.max(np.abs(got - g_ref) / np.abs(g_ref))),
            "max_grad_err_vs_first_step": None if g_first is None else float(np.max(np.abs(got - g_ref) / np.abs(g_first))),
            "grad_shrunk_to": None if g_first is None else [float(v) for v in np.abs(g_ref) / np.abs(g_first)],
            "rel_loss": float(abs(float(sse) / n_global - loss_ref) / loss_ref),
            "checked": f"all {y.shape[1]} sequences x {y.shape[0]} samples of the bench path's y and its fused gradient "
                       f"d(mean squared error)/d(Is,nVt,R,C), vs oracle_clipper_mse_step_f64 at the final theta "
                       f"({time.perf_counter() - t0:.1f} s of CPU)"}


def mlp_components(hidden, n_tanh, stride):
    """Indices into the flat weight vector: every bias, the whole first and last layer, every `stride`-th entry of the
    hidden kernels (the oracle differentiates by complex step: one pass over the picked sequences per component)."""
    idx, o, n_in = [], 0, 2
    for layer in range(n_tanh):
        nk = n_in * hidden
        idx += list(range(o, o + nk, 1 if layer == 0 else stride))
        idx += list(range(o + nk, o + nk + hidden))
        o += nk + hidden
        n_in = hidden
    return np.array(idx + list(range(o, o + hidden + 1)))


def mlp_parity_check(run_step, w, theta2, x, r, x_host, r_host, target, fs, hidden, n_tanh, skip, n_global, eps):
    """After the timed region, at the weights training has reached: one more forward + loss + reverse sweep of the BENCH
    PATH ITSELF (same plan, same warm start, same kernels; no update), checked three ways --
      y of EVERY sequence and the loss against the fp64 oracle (generic tree interpreter, MLP root: clipper_pot.py:94-127);
      the gradient of the loss restricted to 8 picked sequences (dLoss/dy of the real loss, zeroed elsewhere) against the
        oracle's complex-step derivative, per component;
      the whole-batch gradient against the sequential row sweep (another kernel family: no chunks, no matrix cores)."""
    O = _oracle()
    B, T = x.shape
    t0 = time.perf_counter()
    y, gy, loss3 = run_step()                                   # y keeps its autograd graph
    (gw,) = torch.autograd.grad(y, [w], grad_outputs=gy, retain_graph=True)
    pick = np.unique(np.linspace(0, B - 1, 8).astype(np.int64))
    mask = torch.zeros((1, B), dtype=torch.float32, device=x.device)
    mask[0, torch.as_tensor(pick, device=x.device)] = 1.0
    (gw_pick,) = torch.autograd.grad(y, [w], grad_outputs=gy * mask)
    wd = w.detach()
    y_seq, zs_seq, _ = binding.clipper_mlp_fwd(x, theta2, wd, hidden, n_tanh, fs, r=r)
    _, gw_seq = binding.clipper_mlp_bwd_w(x, theta2, wd, hidden, n_tanh, fs, zs_seq, gy, r=r)
    torch.cuda.synchronize()
    sizes, acts = [2] + [hidden] * n_tanh + [1], [O.ACT_TANH] * n_tanh + [O.ACT_NONE]
    oc = O.clipper_mlp_circuit(fs, sizes, acts)
    theta = np.concatenate([theta2.cpu().numpy().astype(np.float64), wd.cpu().numpy().astype(np.float64)])
    y_ref = O.tree_fwd(oc, theta, np.stack([x_host.astype(np.float64), r_host.astype(np.float64)], axis=-1))
    o, t = y_ref[skip:], target.cpu().numpy().astype(np.float64)[skip:]
    S, E = float(np.sum((o - t) ** 2)), float(np.sum(o ** 2)) + eps
    loss_ref = S / n_global + float(np.sqrt(S / E / n_global))
    comp = mlp_components(hidden, n_tanh, 8)
    gy_host = gy.cpu().numpy().astype(np.float64)[:, pick]
    xin = np.stack([x_host[pick].astype(np.float64), r_host[pick].astype(np.float64)], axis=-1)
    g_ref = O.tree_grad(oc, theta, xin, gy_host, params=list(2 + comp))
    got = gw_pick.cpu().numpy().astype(np.float64)[comp]
    yh = y.detach().cpu().numpy()
    return {"max_abs_y": float(np.max(np.abs(yh - y_ref))),
            "rel_loss": abs(float(loss3[2]) - loss_ref) / loss_ref,
            "max_grad_err_vs_oracle": float(np.max(np.abs(got - g_ref) / (np.abs(g_ref) + 0.1 * np.max(np.abs(g_ref))))),
            "max_grad_err_vs_sequential_sweep": float((gw - gw_seq).abs().max() / gw_seq.abs().max()),
            "max_abs_y_vs_sequential_kernel": float((y.detach() - y_seq).abs().max()),
            "checked": f"y of all {B} x {T} samples and the MSE+ESR loss vs the fp64 oracle (tree interpreter, MLP root); "
                       f"d loss/d w restricted to sequences {pick.tolist()} vs the oracle's complex-step derivative on "
                       f"{len(comp)} of {w.numel()} components (all biases, first and last layer, every 8th hidden-kernel "
                       f"entry; error relative to |component| + 0.1 max|component|); the whole-batch gradient, all components, "
                       f"vs the sequential row sweep (error relative to the largest component) "
                       f"({time.perf_counter() - t0:.1f} s)"}


MFMA_F32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 at 64 FLOP/clk/SIMD (= the fp32 vector rate)


def copy_bandwidth_gbs(dev, nbytes=1 << 29, reps=10):
    """Achievable HBM bandwidth on this box: a device-to-device copy of `nbytes` (read + write
    counted), HIP events on the launch stream.  SURVEY 8d's second roofline denominator."""
    a = torch.empty(nbytes // 4, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = binding.Event(), binding.Event()
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    ms = e0.elapsed_ms(e1) / reps
    return 2.0 * nbytes / (ms * 1e-3) / 1e9


class Trainer:
    """The step of the training loop on one layout of x."""

    def __init__(self, args, x, target, fs, B, T, n_global, world, dev, time_major, cold=None):
        self.args, self.world, self.tm = args, world, time_major
        cold = args.cold_forward if cold is None else cold
        self.xk = x.t().contiguous() if time_major else x      # one-off: the engine keeps its training inputs resident time-major
        th_host = workload.clipper_theta()
        self.theta = torch.tensor(th_host, dtype=torch.float32, device=dev)
        self.target = target
        skip = 50 if args.loss == "mse+esr" else 0               # skip_samples, clipper_pot.py:232
        tp = None if args.sequential else engine.plan_time_parallel(B, T, th_host[2], th_host[3], fs, time_major=time_major)
        if tp is not None and args.plan:
            kf, w, kb = (int(v) for v in args.plan.split(","))
            tp = tp._replace(k_fwd=kf, warmup=w, k_bwd=kb)
        self.fused = not args.two_kernel
        if tp is not None and args.plan:
            pass
        elif tp is not None and self.fused:     # part of the untimed set-up: pick the chunk count on this box
            tp = engine.autotune_fused(self.theta, self.xk, target, fs, tp, time_major=time_major, warm=not cold)
        elif tp is not None:
            tp = engine.autotune_time_parallel(self.theta, self.xk, target, fs, tp, time_major=time_major)
        self.tp = tp
        self.stepper = engine.MseStep(B, T, fs, tp, dev, n_global=n_global, time_major=time_major, loss=args.loss, skip=skip,
                                      sums_allreduce=wdist.allreduce_sum_ if (world > 1 or args.force_dist) else None,
                                      warm=not cold)
        # the update that closes a training step (lpf.py:93-94: one Adam per component, its learning
        # rate scaled to the component; tf_wdf.py:74,104 clip constraints), on the device
        self.adam = None if args.no_optimizer else binding.Adam(
            4, lr=[1e-3 * float(v) for v in th_host], lo=[1e-15, 1e-3, 180.0, 1e-13], hi=[1e-3, 1.0, 1.0e6, 1.0], device=dev)
        self.first_sse = None
        self.keep_outputs = False      # run(): copy what the last timed step computed (--dump-outputs)
        self.outputs = None
        self.ev = [binding.Event() for _ in range(4)]
        self.t_fwd, self.t_bwd = [], []
        self.loop_events = []          # (start, stop[, start, stop]) around the recurrence kernel(s) of every 4th timed step

    def step(self, timed=False, ev=None):
        # one pass: forward (x -> y), MSE and the gradient in ONE kernel (-> SSE, dSSE-mean/dtheta); or, two kernels:
        # forward (x -> y, state stash), then the MSE-fused reverse sweep; then ONE fused all-reduce of
        # [SSE, grads] (no-op on 1 GPU unless --force-dist)
        # timed: events bracket exactly the recurrence kernel(s) (what rocprofv3 lists under that name)
        # ev: events of the caller's own (no read-back here: the timed loop collects them after its closing synchronize)
        st, args = self.stepper, self.args
        read_back = timed and ev is None               # (timed=True: bracket with the trainer's own events and wait for them)
        timed = timed or ev is not None
        ev = self.ev if ev is None else ev
        # one rank: the update rides in the step's own last waves (one-pass step: either loss; kernel pair: plain MSE);
        # otherwise all-reduce, then update
        fold = self.adam is not None and self.world == 1 and not args.force_dist and (self.fused or args.loss == "mse")
        if self.fused:
            if timed:
                binding.Event.bracket_next(ev[0], ev[1])
            st.step_fused(self.theta, self.xk, self.target, adam=self.adam if fold else None)
        else:
            if timed:
                binding.Event.bracket_next(ev[0], ev[1])
            st.forward(self.theta, self.xk)
            if timed:
                binding.Event.bracket_next(ev[2], ev[3])
            st.backward(self.theta, self.xk, self.target, adam=self.adam if fold else None)
        buf = st.out                                   # [SSE, grads]: the kernels wrote it in place
        if not (self.fused and args.loss == "mse+esr"):   # (the one-pass MSE + ESR step all-reduces its ten sums itself)
            wdist.allreduce_sum_(buf)
        if self.adam is not None:
            if self.first_sse is None:
                self.first_sse = buf[0:1].clone()          # SSE of the very first step, for the report
                self.first_grad = buf[1:].clone()
            if not fold:
                self.adam.apply(self.theta, buf[1:])
        if read_back:
            self.t_fwd.append(ev[0].elapsed_ms(ev[1]))
            if not self.fused:
                self.t_bwd.append(ev[2].elapsed_ms(ev[3]))
        return buf[0], buf[1:]

    def last_outputs(self, n_seq=256, seed=2024):
        """What the step hands its caller, as the last step left it: sse [1], grad [4], theta [4] (after the update) and y of
        n_seq sequences (a fixed, seeded pick) as [n_seq, T]; float32 host arrays."""
        st = self.stepper
        idx = np.sort(np.random.default_rng(seed).choice(st.B, size=min(n_seq, st.B), replace=False))
        y = st.y[:, torch.as_tensor(idx, device=st.y.device)].t()
        return {"sse": st.sse.cpu().numpy(), "grad": st.gtheta.cpu().numpy(), "theta": self.theta.cpu().numpy(),
                "y_sample": y.cpu().numpy()}

    def run(self, warmup, steps, dev):
        """W untimed steps, then exactly K steps between barrier + synchronize; max over ranks."""
        n_ev = 2 if self.fused else 4
        warm_evs = []
        for i in range(warmup):
            # (graph mode: the replayed steps cannot carry per-kernel events, so the kernel durations reported are those of
            #  the warm-up steps' kernels, recorded here and read after the timed region)
            e = [binding.Event() for _ in range(n_ev)] if self.args.graph else None
            warm_evs.append(e)
            self.step(ev=e)
        # HIP events around the recurrence kernel of every 4th step (every n-th past 4096 steps), recorded INSIDE the timed region on the launch stream
        # and read only after its closing synchronize (no host wait in between): kernel time and step time from one loop
        graph = None
        if self.args.graph:
            # One training step -- kernel(s), (N > 1) the RCCL all-reduce, the update -- captured once as a HIP graph and
            # replayed: the host then spends one launch per step instead of 2..5 plus torch.distributed's dispatch (which,
            # not the GPU, bounds the multi-rank step when driven eagerly).  Everything a step reads or writes lives in
            # device buffers that do not move (theta, Adam moments and step count, warm-start state, workspaces).
            if warmup < 1:                                     # (first-use allocations happen outside the capture)
                warm_evs.append([binding.Event() for _ in range(n_ev)])
                self.step(ev=warm_evs[-1])
            torch.cuda.synchronize()
            try:
                graph = torch.cuda.CUDAGraph()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    with torch.cuda.graph(graph, stream=side):
                        loss, grad = self.step()
                torch.cuda.current_stream().wait_stream(side)
                self.step_graph = graph
            except Exception as exc:        # (a runtime that cannot capture the collective: the same step, launched eagerly)
                print(f"bench: HIP-graph capture of the step failed ({type(exc).__name__}: {exc}); eager launches instead",
                      file=sys.stderr, flush=True)
                graph, self.args.graph = None, False
                torch.cuda.synchronize()
        # Inside the timed region every 4th step carries events (a pair of event records costs the stream ~9 us of dispatch
        # gap: bracketing EVERY step of a 20-step run made the run 8 % slower than the loop it measures); a short run gets
        # its full sample of kernel durations from a pass of bracketed steps AFTER the closing synchronize (--full only).
        every = max(1, min(4, steps)) if steps <= 64 else max(4, -(-steps // 1024))
        evs = [[binding.Event() for _ in range(n_ev)] if (i % every == 0 and graph is None) else None for i in range(steps)]
        self.n_in_region = sum(1 for e in evs if e is not None)     # (the first n_in_region entries of t_fwd are the timed region's own)
        wdist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if graph is not None:
            for i in range(steps):
                graph.replay()
        else:
            for i in range(steps):
                loss, grad = self.step(ev=evs[i])
        torch.cuda.synchronize()
        wdist.barrier()
        dt = time.perf_counter() - t0
        self.dt_local = dt
        # the warm-start controller as the TIMED steps left it (the untimed continuation below puts the parameters back afterwards:
        # a jump the controller answers with more warm-up -- not what the timed region ran with)
        self.warm_after_timed = None if self.stepper.warm is None else self.stepper.warm.info()
        if self.keep_outputs:
            self.outputs = self.last_outputs()
        if graph is not None:                                  # kernel durations: the warm-up steps' (their last ones: past the cold call)
            evs = [e for e in warm_evs if e is not None][-8:] + evs
            self.n_in_region = 0
        elif steps <= 64 and self.args.full:                   # (untimed: the same loop continued, every step bracketed)
            post = [[binding.Event() for _ in range(n_ev)] for _ in range(steps)]
            keep = [t.clone() for t in ([self.theta] + ([self.adam.m, self.adam.v, self.adam.step] if self.adam is not None else []))]
            for e in post:
                self.step(ev=e)
            torch.cuda.synchronize()
            for t, k in zip([self.theta] + ([self.adam.m, self.adam.v, self.adam.step] if self.adam is not None else []), keep):
                t.copy_(k)                                     # (the report's loss / theta are those of the timed steps)
            evs = evs + post
        for e in evs:
            if e is not None:
                self.t_fwd.append(e[0].elapsed_ms(e[1]))
                if not self.fused:
                    self.t_bwd.append(e[2].elapsed_ms(e[3]))
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        if self.world > 1:
            torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
        return float(tmax), loss, grad


def sustained_rate(trainer, Bg, T, ms_step, seconds=2.5):
    """The same training loop kept running for `seconds` (the headline's timed region is a few milliseconds: the chip is
    still cool and at its boost clock there).  Two clock stamps (s_memtime, read by a one-lane kernel on the launch stream)
    bracket the loop: shader cycles / elapsed time = the clock the chip sustained."""
    dev = trainer.theta.device
    n = max(200, int(seconds / (ms_step * 1e-3)))
    s0 = torch.zeros(2, dtype=torch.int64, device=dev)
    s1 = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    binding.clock_stamp(s0)
    for _ in range(n):
        trainer.step()
    binding.clock_stamp(s1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    a, b = s0.cpu().numpy(), s1.cpu().numpy()
    wall = float(b[1] - a[1]) / 100.0e6                         # s_memrealtime: 100 MHz
    return {"value": Bg * T / (dt / n), "ms_per_step": dt / n * 1e3, "steps": n, "seconds": dt,
            "shader_clock_mhz": None if wall <= 0 else float(b[0] - a[0]) / wall / 1e6,
            "note": "the headline loop continued (same trainer, same state) for this long; clock = s_memtime ticks / s_memrealtime"}


def forward_only(args, dev, fs, B=1024, T=4096, steps=100, warmup=10):
    """BASELINE configs[1]: 1N4148 diode clipper FORWARD ONLY, 1024 sequences x 4096 samples: y written, no stash, nothing
    carried between calls (every call warms its chunks up from z = 0: inference sees other data every call).  The chunk
    count is picked by timing; y of the whole batch is checked against the fp64 oracle."""
    x_host = workload.sweep_batch(B, T, seed=3)
    x = torch.as_tensor(x_host, device=dev)
    xk = x.t().contiguous()                                       # the engine's resident layout
    theta = torch.tensor(workload.clipper_theta(), dtype=torch.float32, device=dev)
    th_host = workload.clipper_theta()
    plan = engine.plan_time_parallel(B, T, th_host[2], th_host[3], fs, time_major=True)
    e0, e1 = binding.Event(), binding.Event()

    def timed(k, n):
        ws = torch.empty((max(16, binding.lib().wdf_clipper_fwd_tp_ws_bytes(B, k)),), dtype=torch.uint8, device=dev)
        st = torch.zeros((4,), dtype=torch.int32, device=dev)
        run = lambda: binding.clipper_fwd_tp(xk, theta, fs, k, plan.warmup, plan.tol, want_stash=False, ws=ws, status=st, time_major=True)  # noqa: E731
        for _ in range(3):
            out = run()
        e0.record()
        for _ in range(n):
            out = run()
        e1.record()
        return e0.elapsed_ms(e1) / n, out[0], st

    # (1024 sequences are 8 waves per chunk on a 1024-SIMD chip: the call is a latency chain of T / k + W steps, so many short chunks)
    cands = sorted({k for k in (plan.k_fwd // 2, plan.k_fwd, plan.k_fwd * 2, plan.k_fwd * 4, plan.k_fwd * 8) if 2 <= k <= T // 32})
    times = {k: timed(k, 10)[0] for k in cands}
    k = min(times, key=times.get)
    # ... and the warm-up, as engine.autotune_time_parallel does for the training pair: the planned W shrinks a 10 V error below
    # 1e-7; on real data the diodes hold the state within ~1 V, so W - 32 is tried while the device's own verification reports a
    # miss 8x inside the tolerance and the call gets faster (every call is verified and repaired whatever W is)
    W_planned = plan.warmup
    t_now = times[k]
    for _ in range(6):
        if plan.warmup < 96:
            break
        shorter = plan._replace(warmup=plan.warmup - 32)
        keep = plan
        plan = shorter
        t_short, _, st_short = timed(k, 10)
        stat = binding.tp_status(st_short)
        if not (stat["n_bad"] == 0 and stat["max_miss"] <= plan.tol / 8.0 and t_short < 0.98 * t_now):
            plan = keep
            break
        t_now = t_short
    for k2 in (k * 2, k * 3 // 2):                               # (a shorter warm-up moves the best chunk count up)
        if k2 <= T // 32 and k2 not in times:
            t2, _, st2 = timed(k2, 10)
            times[k2] = t2
            if binding.tp_status(st2)["n_bad"] == 0 and t2 < 0.98 * t_now:
                k, t_now = k2, t2
    for _ in range(warmup):
        binding.clipper_fwd_tp(xk, theta, fs, k, plan.warmup, plan.tol, want_stash=False, time_major=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ms_ev, y, st = timed(k, steps)
    torch.cuda.synchronize()
    out = {"value": B * T / (ms_ev * 1e-3), "unit": "samples/s", "ms_per_call": ms_ev, "chunks": k, "warmup_steps": plan.warmup,
           "warmup_steps_planned": W_planned,
           "chunk_sweep_ms": {str(kk): v for kk, v in times.items()}, "verify_status": binding.tp_status(st),
           "bytes_per_sample": 8, "hbm_frac": 8.0 * B * T / (ms_ev * 1e-3) / 1e9 / HBM_PEAK_GBS,
           "workload": f"1N4148 diode clipper forward only, {B} sequences x {T} samples @ {int(fs)} Hz (BASELINE configs[1]); x resident "
                       f"time-major, y written, stateless calls"}
    if not args.no_parity:
        O = _oracle()
        y_ref = O.clipper_fwd(th_host.astype(np.float32).astype(np.float64), fs, x_host.astype(np.float64))
        out["max_abs_y_vs_oracle"] = float(np.max(np.abs(y.cpu().numpy() - y_ref)))
    return out


def valu_cycle_model(B, T, k, w_used):
    """VALU-active cycles per launch of the one-pass kernel when no committed SQ pass matches the autotuned plan: the count
    is deterministic in the work -- a wave (128 sequences, two per lane) runs T / k + W steps per chunk -- and the committed
    passes fit  SQ_ACTIVE_INST_VALU = c quad-cycles per wave-step + 210 per wave:  c = 124.65 until round 5
    (profiles/r03_c_sq_counters.json: 32 chunks; r03_c16: 16 chunks; warm-up 16 steps both; to better than 0.1 %), c = 109.4
    since round 6's LEAN root tier (profiles/r06_m_sq_counters.json: 32.686 M per launch of 2048 waves x 144 steps)."""
    waves = (B + 127) // 128 * k
    return 4.0 * (109.4 * waves * (T / k + w_used) + 210.0 * waves)


def run_mlp_step(args, world, rank, local):
    """--root mlp2x16 (and friends), the default form: the path clipper_pot.py actually trains -- the pot clipper with a
    DenseRootModel root -- at the reference's training-set shape (BASELINE configs[3]: 1340 sequences x 2048 samples per
    GPU, pot value per sample in the loader's layout, committed reference weights) through the RESIDENT training step
    (csrc/wdf_mlp_step.h, wdf_clipper_mlp_step): forward in verified time chunks (per-column chunk counts and warm-ups,
    steered on the device), MSE + ESR past 50 samples, exact reverse sweep to all weights, Adam(1e-4, beta_1 0.5) -- five
    launches per step; N > 1: the two loss sums and the weight gradient are all-reduced in between.  One JSON line."""
    from wdf_hip import mlp_root
    dev = torch.device("cuda", local)
    fs, T, B = workload.FS, 2048, (args.batch if args.batch != 8192 else 1340)
    Bg = B * world
    b0, b1 = wdist.shard_range(Bg, rank, world)
    x_host = workload.sweep_batch(Bg, T, b0=b0, b1=b1, seed=4) * 0.6
    r_host = workload.dataset_resistance_batch(Bg, T, b0=b0, b1=b1)
    x, r = torch.as_tensor(x_host, device=dev), torch.as_tensor(r_host, device=dev)
    net = args.root[3:] + "_pre" if args.root == "mlp2x16" else args.root[3:]
    wh, hidden, n_layers = workload.reference_mlp_weights(net, path=args.mlp_weights)
    w = torch.tensor(wh, device=dev)
    th4 = torch.tensor(workload.clipper_theta(), dtype=torch.float32, device=dev)
    target, _, _ = binding.clipper_fwd(x, th4, fs, r=r, want_stash=False)        # "measurement": the analytic diode pair
    skip, eps = 50, float(np.finfo(float).eps)
    n_global = float(Bg * (T - skip))
    adam = binding.Adam(w.numel(), lr=1.0e-4, beta_1=0.5, device=dev)
    dist_on = world > 1 or args.force_dist
    st = mlp_root.MlpTrainStep(x, r, target, w, hidden, n_layers, fs, workload.C_CLIPPER, skip=skip, adam=adam,
                               n_global=n_global, eps_energy=eps,
                               sums_allreduce=wdist.allreduce_sum_ if dist_on else None,
                               grad_allreduce=wdist.allreduce_sum_ if dist_on else None)
    # untimed set-up (as the diode line autotunes its chunk count): the cold call and the controller settling (24 steps), then
    # the chunk plan picked by measurement among six candidates, 16 training steps each (MlpTrainStep.autotune); then the
    # contract's W untimed steps
    tuned = None
    if not args.plan:
        for _ in range(24):
            st.step()
        tuned = st.autotune()
    for i in range(args.warmup):
        st.step()
    graph = None
    if args.graph:
        torch.cuda.synchronize()
        try:
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    st.step()
            torch.cuda.current_stream().wait_stream(side)
        except Exception as exc:
            print(f"bench: HIP-graph capture of the step failed ({type(exc).__name__}: {exc}); eager launches instead",
                  file=sys.stderr, flush=True)
            graph, args.graph = None, False
            torch.cuda.synchronize()
    info0, _ = st.read()
    wdist.barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    if graph is not None:
        for _ in range(args.steps):
            graph.replay()
    else:
        for _ in range(args.steps):
            st.step()
    torch.cuda.synchronize(); wdist.barrier()
    dt = time.perf_counter() - t0
    ranks = ranks_report(world, dev, dt, args.steps)
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
    dt = float(tmax)
    info1, wcol = st.read()
    loss_last = [float(v) for v in st.loss3]
    # kernel times: the same step launched in its two phases, events around the chunked forward and the reverse sweep
    ev = [binding.Event() for _ in range(4)]
    t_fk, t_wk = [], []
    if not dist_on:
        for _ in range(min(args.steps, 16)):
            binding.Event.bracket_next(ev[0], ev[1])
            st.forward_only()
            binding.Event.bracket_next(ev[2], ev[3])
            st.backward_only()
            torch.cuda.synchronize()
            t_fk.append(ev[0].elapsed_ms(ev[1])); t_wk.append(ev[2].elapsed_ms(ev[3]))
    parity = None
    if rank == 0 and world == 1 and not args.no_parity:
        parity = mlp_step_parity(st, x_host, r_host, target, net, fs, skip, eps)
    if rank == 0:
        items = st.items
        w_steps = 16 * wcol[items[:, 0]].astype(np.int64)
        run = np.where(items[:, 1] > 0, np.minimum(w_steps, items[:, 2]), 0) + (items[:, 3] - items[:, 2])
        fk_ms = float(np.mean(t_fk)) if t_fk else None
        wk_ms = float(np.mean(t_wk)) if t_wk else None
        # the reverse sweep on the matrix cores: per wave (16 sequences) and step 4 (NL - 1) + 1 forward MFMAs, 4 (NL - 1) for
        # the delta chain and 4 (NL - 1) outer products (v_mfma_f32_16x16x4_f32, 2048 flop each)
        n_mfma = 12 * (n_layers - 1) + 1
        flops = (B + 15) // 16 * T * n_mfma * 2048
        out = {"metric": f"samples/sec fwd+bwd, MLP-root ({args.root[3:]}) pot clipper, clipper_pot.py training-set shape",
               "value": Bg * T / (dt / args.steps), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "f32", "data": "synthetic",
               "config": {"workload": f"pot clipper with DenseRootModel {args.root[3:]} root (reference weights), MSE+ESR past 50 "
                                      f"samples, Adam(1e-4, beta_1 0.5), {B} sequences x {T} samples per GPU, pot value per sample "
                                      f"(BASELINE configs[3] shape)",
                          "global_batch": Bg, "seq_len": T, "parallelism": f"dp{world}", "loss": loss_last[2],
                          "collective": None if not dist_on else "all-reduce of the two loss sums, then of the weight gradient",
                          "step": "resident training step (wdf_clipper_mlp_step): five launches, steered on the device",
                          "time_parallel": {"forward_items": int(st.n_items), "reverse_chunks": int(st.wgrad_chunks),
                                            "plan": None if tuned is None else {"picked": tuned[0], "ms_per_step_while_tuning": tuned[1]},
                                            "chunks_per_column": {"min": int(np.bincount(items[:, 0]).min()), "max": int(np.bincount(items[:, 0]).max())},
                                            "warmup_steps_per_column": {"min": int(16 * wcol.min()), "mean": float(16 * wcol.mean()), "max": int(16 * wcol.max())},
                                            "forward_steps_per_wave": {"mean": float(run.mean()), "max": int(run.max()), "owned_mean": float(T * st.ncol / st.n_items)},
                                            "verify_tol": st.tol,
                                            "verdict_last_call": {k: info1[k] for k in ("n_bad", "max_miss", "flagged_columns", "sequential_columns")},
                                            "in_timed_region": {"boundaries_repaired": info1["total_flagged"] - info0["total_flagged"],
                                                                "columns_sequential": info1["total_sequential"] - info0["total_sequential"]}}},
               "ranks_seen": ranks["ranks_seen"], "ranks": ranks, "library": library_identity(),
               "step_launch": "one HIP-graph replay per step" if graph is not None else "eager launches",
               "kernel_ms": None if fk_ms is None else {"forward_chunks": spread(t_fk), "reverse_sweep": spread(t_wk)},
               "parity": parity,
               "roofline": None if wk_ms is None else
               {"bound": "mfma", "kernel": "mlp_step_wgrad_kernel", "achieved": flops / (wk_ms * 1e-3) / 1e12,
                "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": flops / (wk_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS,
                "traffic": None, "mfma_per_wave_step": n_mfma,
                "forward": {"kernel": "mlp_step_fwd_kernel", "ms": fk_ms,
                            "useful_fraction_of_steps": float(T * st.ncol / run.sum()),
                            "note": "one wave per SIMD, every wave a dependent chain of steps (18 MFMAs + ~150 VALU + 24 transcendentals "
                                    "per owned step, 9 MFMAs per warm-up step): bound by issue, not by a throughput roof"},
                "note": "fp32-input MFMA (v_mfma_f32_16x16x4_f32, 2048 flop, 32 cycles per SIMD): issued MFMA flops of the reverse "
                        "sweep / its kernel time / the fp32 matrix peak"}}
        print(json.dumps(out), flush=True)
    if world > 1 or args.force_dist:
        wdist.barrier()
        torch.distributed.destroy_process_group()


def mlp_step_parity(st, x_host, r_host, target, net, fs, skip, eps):
    """After the timed region, at the weights training has reached, no update: (1) one more step of the BENCH PATH ITSELF
    (same state, same plan): y of every sequence and the loss against the fp64 oracle (tree interpreter, MLP root:
    clipper_pot.py:94-127,141-177); its whole-batch gradient against the sequential row sweep (another kernel family: no
    chunks, no matrix cores) fed with dLoss/dy of that loss; (2) the same kernels on 8 picked sequences as a batch of their
    own: the gradient of THEIR MSE + ESR loss against the oracle's complex-step derivative, per component."""
    from wdf_hip import mlp_root
    O = _oracle()
    t0 = time.perf_counter()
    B, T = st.B, st.T
    adam, st.adam = st.adam, None
    hooks = (st.sums_allreduce, st.grad_allreduce)
    st.sums_allreduce = st.grad_allreduce = None
    st.step()
    torch.cuda.synchronize()
    st.adam, (st.sums_allreduce, st.grad_allreduce) = adam, hooks
    hidden, n_layers = st.hidden, st.n_layers
    wd = st.w.detach().clone()
    sizes, acts = [2] + [hidden] * n_layers + [1], [O.ACT_TANH] * n_layers + [O.ACT_NONE]
    oc = O.clipper_mlp_circuit(fs, sizes, acts)
    theta = np.concatenate([[45.0e3, float(np.float32(workload.C_CLIPPER))], wd.cpu().numpy().astype(np.float64)])
    y_ref = O.tree_fwd(oc, theta, np.stack([x_host.astype(np.float64), r_host.astype(np.float64)], axis=-1))
    tgt = target.cpu().numpy().astype(np.float64)

    def loss_of(yr, tr):
        o, t = yr[skip:], tr[skip:]
        n = float(o.size)
        S, E = float(np.sum((o - t) ** 2)), float(np.sum(o ** 2)) + eps
        esr = float(np.sqrt(S / E / n))
        gy = np.zeros_like(yr)
        gy[skip:] = (2.0 / n + 1.0 / (esr * E * n)) * (o - t) - esr / E * o
        return S / n + esr, gy

    loss_ref, gy_ref = loss_of(y_ref, tgt)
    yh = st.y.cpu().numpy()
    th2 = torch.tensor([45.0e3, workload.C_CLIPPER], dtype=torch.float32, device=st.x.device)
    gy_own = torch.as_tensor(loss_of(yh.astype(np.float64), tgt)[1].astype(np.float32), device=st.x.device)
    _, gw_seq = binding.clipper_mlp_bwd_w(st.x, th2, wd, hidden, n_layers, fs, st.zstash, gy_own, r=st.r)
    # (2) the picked sequences as their own training set
    pick = np.unique(np.linspace(0, B - 1, 8).astype(np.int64))
    pk = torch.as_tensor(pick, device=st.x.device)
    st8 = mlp_root.MlpTrainStep(st.x[pk].contiguous(), st.r[pk].contiguous(), target[:, pk].contiguous(), wd, hidden, n_layers, fs,
                                workload.C_CLIPPER, skip=skip, adam=None, eps_energy=eps, n_items=16, wgrad_chunks=16)
    st8.step()
    st8.step()                                                   # (the second call starts its chunks from snapshots)
    torch.cuda.synchronize()
    xin = np.stack([x_host[pick].astype(np.float64), r_host[pick].astype(np.float64)], axis=-1)
    loss8, gy8 = loss_of(y_ref[:, pick], tgt[:, pick])
    comp = mlp_components(hidden, n_layers, 8)
    g_ref = O.tree_grad(oc, theta, xin, gy8, params=list(2 + comp))
    got = st8.gw.cpu().numpy().astype(np.float64)[comp]
    return {"max_abs_y": float(np.max(np.abs(yh - y_ref))),
            "rel_loss": abs(float(st.loss3[2]) - loss_ref) / loss_ref,
            "max_grad_err_vs_oracle": float(np.max(np.abs(got - g_ref) / (np.abs(g_ref) + 0.1 * np.max(np.abs(g_ref))))),
            "rel_loss_picked": abs(float(st8.loss3[2]) - loss8) / loss8,
            "max_grad_err_vs_sequential_sweep": float((st.gw - gw_seq).abs().max() / gw_seq.abs().max()),
            "checked": f"y of all {B} x {T} samples and the MSE+ESR loss of the bench path's own step vs the fp64 oracle (tree "
                       f"interpreter, MLP root); its whole-batch gradient, all {wd.numel()} components, vs the sequential row sweep "
                       f"(error relative to the largest component); the same kernels on sequences {pick.tolist()} as a batch of "
                       f"their own: d(their MSE+ESR loss)/dw vs the oracle's complex-step derivative on {len(comp)} components "
                       f"(all biases, first and last layer, every 8th hidden-kernel entry; error relative to |component| + 0.1 "
                       f"max|component|) ({time.perf_counter() - t0:.1f} s)"}


def run_mlp_root(args, world, rank, local):
    """--mlp-path unfused: the round-2/3 pipeline (~20 launches steered from the host), kept for A/B.
    --root mlp2x16 (and friends): the path clipper_pot.py actually trains -- the pot clipper with a
    DenseRootModel root -- at the reference's training-set shape (BASELINE configs[3]: 1340 sequences x 2048
    samples per GPU, pot value per sample in the loader's layout, committed reference weights): forward
    (time-parallel, verified), MSE + ESR past 50 samples, exact step-parallel reverse sweep to all weights,
    all-reduce of the weight gradient, Adam(1e-4, beta_1 0.5) on the device.  One JSON line."""
    from wdf_hip import mlp_root
    dev = torch.device("cuda", local)
    fs, T, B = workload.FS, 2048, (args.batch if args.batch != 8192 else 1340)
    Bg = B * world
    b0, b1 = wdist.shard_range(Bg, rank, world)
    x = torch.as_tensor(workload.sweep_batch(Bg, T, b0=b0, b1=b1, seed=4) * 0.6, device=dev)
    r = torch.as_tensor(workload.dataset_resistance_batch(Bg, T, b0=b0, b1=b1), device=dev)
    wh, hidden, n_tanh = workload.reference_mlp_weights(args.root[3:] + "_pre" if args.root == "mlp2x16" else args.root[3:])
    w = torch.tensor(wh, device=dev, requires_grad=True)
    theta2 = torch.tensor([45.0e3, workload.C_CLIPPER], dtype=torch.float32, device=dev)
    th4 = torch.tensor(workload.clipper_theta(), dtype=torch.float32, device=dev)
    target, _, _ = binding.clipper_fwd(x, th4, fs, r=r, want_stash=False)        # "measurement": the analytic diode pair
    skip, eps = 50, float(np.finfo(float).eps)
    n_global = float(Bg * (T - skip))
    plan = None if args.sequential else mlp_root.plan_mlp_time_parallel(B, T, r, None, workload.C_CLIPPER, fs, hidden=hidden, n_tanh=n_tanh)
    adam = binding.Adam(w.numel(), lr=1.0e-4, beta_1=0.5, device=dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    gcoef, loss3 = torch.zeros(2, dtype=torch.float32, device=dev), torch.zeros(3, dtype=torch.float32, device=dev)
    loss_ws = torch.empty((binding.lib().wdf_loss_sums_ws_bytes(),), dtype=torch.uint8, device=dev)
    gy_buf = torch.empty((T, B), dtype=torch.float32, device=dev)
    ev = [binding.Event() for _ in range(8)]
    t_f, t_b, t_fk, t_wk = [], [], [], []

    def forward_and_loss():
        """forward -> (y with its autograd graph, dLoss/dy, the three loss values); the loss on the device
        (include/wdf_hip.h: wdf_loss_sums / wdf_esr_coef / wdf_loss_esr_grad)"""
        y, _ = mlp_root.clipper_mlp(theta2, w, x, r, None, fs, hidden, n_tanh, workload.C_CLIPPER, time_parallel=plan)
        yd = y.detach()
        binding.loss_sums(yd, target, skip, sums=sums, ws=loss_ws)
        wdist.allreduce_sum_(sums)
        binding.esr_coef(sums, n_global, eps, gcoef=gcoef, loss=loss3)
        return y, binding.loss_esr_grad(yd, target, gcoef, skip, gy=gy_buf), loss3

    def step(timed=False):
        if timed:                 # events around the whole forward / reverse call (kernels + their helpers), and
            ev[0].record()        # brackets around the forward kernel and the weight-gradient kernel alone
            binding.Event.bracket_next(ev[4], ev[5])
        y, _ = mlp_root.clipper_mlp(theta2, w, x, r, None, fs, hidden, n_tanh, workload.C_CLIPPER, time_parallel=plan)
        if timed:
            ev[1].record()
        # the loss on the device (include/wdf_hip.h: wdf_loss_sums / wdf_esr_coef / wdf_loss_esr_grad): the two sums,
        # global; then loss = S/n + sqrt(S/(E+eps)/n) and d loss / d y = ga (y - t) + gb y past `skip`
        yd = y.detach()
        binding.loss_sums(yd, target, skip, sums=sums, ws=loss_ws)
        wdist.allreduce_sum_(sums)
        binding.esr_coef(sums, n_global, eps, gcoef=gcoef, loss=loss3)
        gy = binding.loss_esr_grad(yd, target, gcoef, skip, gy=gy_buf)
        if timed:
            ev[2].record()
            binding.Event.bracket_next(ev[6], ev[7])
        (gw,) = torch.autograd.grad(y, [w], grad_outputs=gy)
        if timed:
            ev[3].record()
        wdist.allreduce_sum_(gw)                                       # the weight gradient, global
        with torch.no_grad():
            adam.apply(w, gw)
        if timed:
            t_f.append(ev[0].elapsed_ms(ev[1])); t_b.append(ev[2].elapsed_ms(ev[3]))
            t_fk.append(ev[4].elapsed_ms(ev[5])); t_wk.append(ev[6].elapsed_ms(ev[7]))
        return loss3[2]

    for _ in range(args.warmup):
        loss0 = step()
    wdist.barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize(); wdist.barrier()
    dt = time.perf_counter() - t0
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
    dt = float(tmax)
    for _ in range(min(args.steps, 10)):
        step(True)
    torch.cuda.synchronize()
    parity = None
    if rank == 0 and world == 1 and not args.no_parity:
        x_host = workload.sweep_batch(Bg, T, b0=b0, b1=b1, seed=4) * 0.6
        r_host = workload.dataset_resistance_batch(Bg, T, b0=b0, b1=b1)
        parity = mlp_parity_check(forward_and_loss, w, theta2, x, r, x_host, r_host, target, fs, hidden, n_tanh, skip, n_global, eps)
    if rank == 0:
        st = None if mlp_root.LAST_TP_STATUS["status"] is None else binding.mlp_tp_status(mlp_root.LAST_TP_STATUS["status"])
        f_ms, b_ms = float(np.mean(t_f)), float(np.mean(t_b))
        fk_ms, wk_ms = float(np.mean(t_fk)), float(np.mean(t_wk))
        # The dominant kernels: the forward (a latency chain: steps x (MFMA chain + tanh), one wave per SIMD) and the
        # weight-gradient pass of the reverse sweep.  On the matrix cores (16-sequence waves, csrc/wdf_mlp_mfma.h) the
        # latter issues, per wave and step, (NL - 1) x 4 + 1 forward MFMAs, the same again transposed for the deltas and
        # 4 outer-product MFMAs per layer: 27 v_mfma_f32_16x16x4_f32 (2048 flop each) for three tanh layers.
        # (which kernel ran: the library is asked, csrc/wdf_capi_mlp.hip wdf_clipper_mlp_wgrad_matrix_core_chunks)
        wg_mfma = plan is not None and plan.k_bwd > 1 and binding.lib().wdf_clipper_mlp_wgrad_matrix_core_chunks(B, T) > 0
        n_mfma = 12 * (n_tanh - 1) + 3     # forward 4 (NL-1) + 1, deltas + outer products 8 (NL-1), d/da and d/dlr sums 2
        flops = (B + 15) // 16 * T * n_mfma * 2048
        achieved_tf = flops / (wk_ms * 1e-3) / 1e12
        out = {"metric": f"samples/sec fwd+bwd, MLP-root ({args.root[3:]}) pot clipper, clipper_pot.py training-set shape",
               "value": Bg * T / (dt / args.steps), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "f32", "data": "synthetic",
               "config": {"workload": f"pot clipper with DenseRootModel {args.root[3:]} root (reference weights), MSE+ESR past 50 "
                                      f"samples, {B} sequences x {T} samples per GPU, pot value per sample (BASELINE configs[3] shape)",
                          "global_batch": Bg, "seq_len": T, "parallelism": f"dp{world}", "loss": float(loss),
                          "time_parallel": None if plan is None else {"fwd_chunks": plan.k_fwd, "fwd_warmup_steps_planned": plan.warmup,
                                                                      "fwd_warmup_steps_used": mlp_root.LAST_TP_STATUS.get("warmup_used", max(v["warmup"] for v in mlp_root._WARMUP_ADAPT.values())),
                                                                      "fwd_warmup_steps_cold": max(v["warmup"] for v in mlp_root._WARMUP_ADAPT.values()),
                                                                      "fwd_warm_start": bool(mlp_root._WARM_START),
                                                                      **({"fwd_warmup_trace": [w for w, _ in mlp_root._TRACE_WARMUP]} if mlp_root._TRACE_WARMUP else {}),
                                                                      "verify_tol": plan.tol, "bwd_chunks": plan.k_bwd,
                                                                      "verify_status": st}},
               "call_ms": {"forward": spread(t_f), "reverse": spread(t_b)},
               "kernel_ms": {"forward_chunks": spread(t_fk), "weight_gradient": spread(t_wk)},
               "parity": parity,
               "roofline": ({"bound": "mfma", "kernel": "clipper_mlp_mfma_wgrad_tp_kernel", "achieved": achieved_tf,
                             "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved_tf / MFMA_F32_PEAK_TFLOPS,
                             "traffic": None,
                             "mfma_per_wave_step": n_mfma,
                             "note": "fp32-input MFMA (v_mfma_f32_16x16x4_f32, 2048 flop, 32 cycles per SIMD): issued MFMA flops "
                                     "of the weight-gradient pass / its kernel time / the fp32 matrix peak.  The forward "
                                     "kernel is a latency chain (dependent MFMAs + tanh per step, one wave per SIMD), "
                                     "not a throughput-bound kernel: see kernel_ms"} if wg_mfma else
                            {"bound": "valu", "kernel": "clipper_mlp_row_wgrad_tp_kernel", "achieved": None, "peak": None,
                             "unit": "instr/s", "frac": None, "traffic": None,
                             "note": "row kernels: VALU-issue bound (~250 instructions per step and 4-sequence wave)"})}
        print(json.dumps(out), flush=True)
    if world > 1:
        wdist.barrier()
        torch.distributed.destroy_process_group()


def run_tree_step(args, rank, local, kind):
    """--config lpf | hpf: a secondary line -- lpf.py:86-99's training loop (GradientTape -> circ.mse -> tape.gradient -> one
    Adam per component) through the element API with the component values resident on the device (Circuit.to_device()):
    the one-pass step of a LINEAR tree (lpf: RC lowpass, lpf.py:20-49; csrc/wdf_ss_step.h) or of a DIODE-ROOT tree (hpf:
    HPFDiodeClipper.h:28-32's circuit; csrc/wdf_ss_nl_step.h) at --batch x --seq-len."""
    import tf_wdf as wdf
    from tf_wdf import tf
    dev = torch.device("cuda", local)
    fs, B, T = 48000, args.batch, args.seq_len
    g = torch.Generator(device="cpu").manual_seed(1234)

    def build(values):
        if kind == "lpf":
            R1, C1 = wdf.Resistor(values[0], True), wdf.Capacitor(values[1], fs, True)
            return wdf.Circuit(wdf.Inverter(wdf.Series(R1, C1)), wdf.IdealVoltageSource(), C1), [R1.R, C1.C]
        R = wdf.Resistor(values[0], True); Vs = wdf.ResistiveVoltageSource(values[1], trainable=True)   # noqa: E702
        C = wdf.Capacitor(values[2], fs, True)
        top = wdf.Parallel(R, wdf.Series(Vs, C))
        dp = wdf.DiodePair(top, values[3], Vt=values[4], nDiodes=1.0, trainable=True)
        return wdf.Circuit(top, dp, R), [R.R, Vs.R, C.C, dp.Is, dp.nVt]

    start = [1000.0, 1.0e-6] if kind == "lpf" else [33.0e3, 1.0e3, 22.0e-9, 4.352e-9, 25.85e-3 * 1.906]
    teacher = [1800.0, 0.6e-6] if kind == "lpf" else [39.0e3, 1.5e3, 15.0e-9, 2.52e-9, 25.85e-3 * 1.752]
    x = (torch.randn((B, T), generator=g) * (1.0 if kind == "lpf" else 1.2)).to(dev)
    with torch.no_grad():
        tgt = build(teacher)[0](x).as_subclass(torch.Tensor).detach().clone()      # [T,B]: the same circuit, other components
    circ, params = build(start)
    circ.to_device()
    opts = [tf.keras.optimizers.Adam(learning_rate=1.0e-3 * float(p)) for p in params]
    res = getattr(circ, "_lin", None) or circ._tree

    def step():
        with tf.GradientTape() as tape:
            loss = circ.mse(x, tgt)
        grads = tape.gradient(loss, params)
        for o, gr, p in zip(opts, grads, params):
            o.apply_gradients([(gr, p)])
        return loss

    for _ in range(max(args.warmup, 2)):
        step()
    every = max(1, min(4, args.steps)) if args.steps <= 64 else max(4, -(-args.steps // 1024))
    evs = [(binding.Event(), binding.Event()) if i % every == 0 else None for i in range(args.steps)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        if evs[i] is not None:
            binding.Event.bracket_next(evs[i][0], evs[i][1])
        loss = step()
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    k_ms = [e[0].elapsed_ms(e[1]) for e in evs if e is not None]
    ms = dt / args.steps * 1e3
    ent = next(iter(res.cache.values()))
    ctl = res.read_ctl(ent) if kind == "hpf" else None

    # ---- parity: y of 64 sequences of the last timed step, and a cold step on 256 sequences at the final components ----
    parity = None
    if not args.no_parity:
        O = _oracle()
        theta_end = np.array([float(p) for p in params], dtype=np.float32).astype(np.float64)
        if kind == "lpf":
            nodes = [(O.NODE_RESISTOR, -1, -1, 0, -1, -1), (O.NODE_CAPACITOR, -1, -1, 1, -1, -1), (O.NODE_SERIES, 0, 1, -1, -1, -1),
                     (O.NODE_INVERTER, 2, -1, -1, -1, -1)]
            oc = O.Circuit(nodes, top=3, probe=1, n_in=1, root_kind=O.ROOT_IDEAL_VSOURCE, fs=fs, root_vin=0)
        else:
            nodes = [(O.NODE_RESISTOR, -1, -1, 0, -1, -1), (O.NODE_RES_VSOURCE, -1, -1, 1, 0, -1), (O.NODE_CAPACITOR, -1, -1, 2, -1, -1),
                     (O.NODE_SERIES, 1, 2, -1, -1, -1), (O.NODE_PARALLEL, 0, 3, -1, -1, -1)]
            oc = O.Circuit(nodes, top=4, probe=0, n_in=1, root_kind=O.ROOT_DIODE_PAIR, fs=fs, p_is=3, p_nvt=4, n_up=1, n_down=1)
        nb = min(B, 256)
        xs = x[:nb].cpu().numpy().astype(np.float64)
        # (against a target the circuit cannot meet: near the teacher the residual is at fp32's resolution of y and the
        #  gradient a sum of cancelling terms -- no measure of the kernels)
        tpar = (0.3 * torch.randn((T, nb), generator=g)).to(dev)
        ts = tpar.cpu().numpy().astype(np.float64)
        c2, p2 = build([float(v) for v in theta_end])
        c2.to_device()
        with tf.GradientTape() as tape:
            l2 = c2.mse(x[:nb].contiguous(), tpar)
        g2 = np.array([float(v) for v in tape.gradient(l2, p2)])
        yref = O.tree_fwd(oc, theta_end, xs)
        e = yref - ts
        gref = O.tree_grad(oc, theta_end, xs, 2.0 * e / e.size)
        y2 = c2.last_output.detach().cpu().numpy()
        parity = {"sequences": nb, "max_abs_y": float(np.max(np.abs(y2 - yref))),
                  "loss_rel": abs(float(l2) - float(np.mean(e * e))) / float(np.mean(e * e)),
                  "grad_max_rel": float(np.max(np.abs(g2 - gref) / np.abs(gref))),
                  "note": "the same kernels on the first 256 sequences at the components the timed loop ended with (a cold call, "
                          "noise target of 0.3 rms), vs oracle tree_fwd / tree_grad in fp64"}
    if rank != 0:
        return
    n = B * T
    kname = "ss_lin_step_kernel" if kind == "lpf" else "ss_nl_step_kernel"
    kmean = float(np.mean(k_ms))
    traffic = None                 # PMC bytes per launch of this kernel: a committed counter pass at the bench shape (tools/pmc_ss_step.sh)
    try:
        pm = json.load(open(os.path.join(REPO, "profiles", "r04_ss_step_pmc.json")))
        if pm.get("samples") == n:
            traffic = pm["kernels"][kname]["traffic_bytes"]
    except (OSError, KeyError, ValueError):
        pass
    out = {"metric": f"samples/sec training step (forward + MSE + gradient + Adam per component), "
                     f"{'RC lowpass (lpf.py:20-49)' if kind == 'lpf' else 'HPF diode clipper (HPFDiodeClipper.h:28-32)'} @48kHz "
                     f"through Circuit.to_device() / circ.mse",
           "value": n / (dt / args.steps), "unit": "samples/s", "n_gpus": 1, "steps": args.steps, "warmup": max(args.warmup, 2),
           "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"{kind}: {B} sequences x {T} samples, {len(params)} trainable components, target = the same circuit "
                                  f"with other component values", "chunks": ent["k"]},
           "host_ms_per_step": t_host / args.steps * 1e3,
           "kernel_ms": {kname: spread(k_ms)},
           "parity": parity,
           "roofline": {"bound": "hbm" if kind == "lpf" else "valu", "kernel": kname,
                        "achieved": 12.0 * n / (kmean * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": 12.0 * n / (kmean * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": traffic,
                        "traffic_source": None if traffic is None else "profiles/r04_ss_step_pmc.json (a committed counter pass of this shape)",
                        "note": "algorithmic bytes of this kernel: x, target read, y written = 12 B per sample" +
                                ("" if kind == "lpf" else "; the kernel is VALU-issue-bound (171 instructions per step of two "
                                                          "sequences at one wave per SIMD), the HBM fraction is what it moves")}}
    if ctl is not None:
        out["control"] = {k_: ctl[k_] for k_ in ("call", "w_used", "w_snap", "max_miss", "gated_groups", "total_gated")}
        out["control"]["replans"] = ent["replans"]
    print(json.dumps(out), flush=True)


def run_c4(args, rank, local):
    """--config c4: BASELINE configs[3]'s per-GPU share as a line of its own -- the dataset-style training loop: the reference's
    training set shape (1340 sequences of 2048 samples, .MISSING_LARGE_BLOBS:1-5 / clipper_pot.py:58) tiled to --batch (8192)
    sequences, one pot value per sequence on the recordings' grid laid out as the loader leaves it (dataimport.py:82-137: four
    contiguous blocks), the pot streamed as input channel 1 (clipper_pot.py:114-117), loss MSE + ESR past 50 samples
    (clipper_pot.py:146-156,177,232,248), Adam on {Is, nVt, C} in the step's own launch (R is data).  The diode-pair root of the
    north star; one GPU (the 8-GPU run shards the batch and all-reduces ten floats per step: --gpus N --loss mse+esr)."""
    dev = torch.device("cuda", local)
    fs, B0, T, skip = workload.FS, 1340, 2048, 50
    B = args.batch
    idx = np.arange(B) % B0
    x_host = workload.sweep_batch(B0, T, seed=4)[idx]
    r_host = workload.dataset_resistance_batch(B0, T)[idx]
    x, r = torch.as_tensor(x_host, device=dev), torch.as_tensor(r_host, device=dev)
    xt, rt = x.t().contiguous(), r.t().contiguous()              # the engine's resident layout (one-off, at data load)
    th0 = workload.clipper_theta()
    tgt, _, _ = binding.clipper_fwd(x, torch.tensor(workload.target_theta(), dtype=torch.float32, device=dev), fs, r=r, want_stash=False)
    plan = engine.plan_time_parallel(B, T, float(r_host.max()), th0[3], fs, time_major=True, R_min=float(r_host.min()))
    best = None
    for k in sorted({k for k in (plan.k_fwd, plan.k_fwd * 2, plan.k_fwd * 4, plan.k_fwd * 8) if 2 <= k <= T // 64}):
        theta = torch.tensor(th0, dtype=torch.float32, device=dev)
        adam = binding.Adam(4, lr=[1e-3 * float(v) for v in th0], lo=[1e-15, 1e-3, 180.0, 1e-13], hi=[1e-3, 1.0, 1.0e6, 1.0], device=dev)
        st = engine.MseStep(B, T, fs, plan._replace(k_fwd=k), dev, time_major=True, loss="mse+esr", skip=skip, warm=True)
        for _ in range(12):
            st.step_fused(theta, xt, tgt, r=rt, adam=adam)
        e0, e1 = binding.Event(), binding.Event()
        e0.record()
        for _ in range(10):
            st.step_fused(theta, xt, tgt, r=rt, adam=adam)
        e1.record()
        ms = e0.elapsed_ms(e1) / 10
        if binding.tp_status(st.status)["n_bad"] == 0 and (best is None or ms < best[0]):
            best = (ms, k)
    k = best[1] if best else plan.k_fwd
    theta = torch.tensor(th0, dtype=torch.float32, device=dev)
    adam = binding.Adam(4, lr=[1e-3 * float(v) for v in th0], lo=[1e-15, 1e-3, 180.0, 1e-13], hi=[1e-3, 1.0, 1.0e6, 1.0], device=dev)
    st = engine.MseStep(B, T, fs, plan._replace(k_fwd=k), dev, time_major=True, loss="mse+esr", skip=skip, warm=True)
    losses, g_first = [], None
    for i in range(args.warmup):
        st.step_fused(theta, xt, tgt, r=rt, adam=adam)
        if i == 0:
            losses.append(float(st.loss[2]))
            g_first = st.gtheta.cpu().numpy().astype(np.float64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        st.step_fused(theta, xt, tgt, r=rt, adam=adam)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    losses.append(float(st.loss[2]))
    stat = binding.tp_status(st.status)
    parity = None
    if not args.no_parity:
        # one more step (its parameters kept aside) against the fp64 oracle over the whole batch: y, the three loss values, the gradient
        O = _oracle()
        th_before = theta.clone()
        st.step_fused(theta, xt, tgt, r=rt, adam=adam)
        torch.cuda.synchronize()
        n, eps = B * (T - skip), float(np.finfo(float).eps)
        th64 = th_before.cpu().numpy().astype(np.float64)
        x64, r64, t64 = x_host.astype(np.float64), r_host.astype(np.float64), tgt.cpu().numpy().astype(np.float64)
        y64 = O.clipper_fwd(th64, fs, x64, r=r64)
        o, t = y64[skip:], t64[skip:]
        S, E = float(np.sum((o - t) ** 2)), float(np.sum(o * o)) + eps
        mse, esr = S / n, float(np.sqrt(S / E / n))
        gy = np.zeros_like(y64)
        gy[skip:] = (2.0 / n + (1.0 / (esr * E * n) if esr > 0 else 0.0)) * (o - t) - esr / E * o
        _, g64 = O.clipper_fwd_bwd(th64, fs, x64, gy, r=r64)
        got, l3 = st.gtheta.cpu().numpy().astype(np.float64), st.loss.cpu().numpy().astype(np.float64)
        parity = {"max_abs_y": float(np.max(np.abs(st.y.cpu().numpy() - y64))),
                  # (every component against its OWN magnitude at the final parameters -- the loss has fallen by three orders of
                  #  magnitude by then and the gradient is what is left of a cancellation -- and against its magnitude at the first step)
                  "max_rel_grad": float(max(abs(got[i] - g64[i]) / abs(g64[i]) for i in (0, 1, 3))),
                  "max_grad_err_vs_first_step": None if g_first is None else float(max(abs(got[i] - g64[i]) / abs(g_first[i]) for i in (0, 1, 3))),
                  "grad_shrunk_to": None if g_first is None else [float(abs(g64[i]) / abs(g_first[i])) for i in (0, 1, 3)],
                  "rel_loss": float(abs(l3[2] - (mse + esr)) / (mse + esr)),
                  "checked": "y of all sequences, mse + esr and d loss / d{Is, nVt, C} of one more step, vs the fp64 oracle at that step's parameters"}
    ms = dt / args.steps * 1e3
    moved = 12.0 * B * T / (ms * 1e-3) / 1e9
    if rank == 0:
        print(json.dumps({
            "metric": "samples/sec fwd+bwd, 1N4148 diode clipper, dataset-style training step (BASELINE configs[3], per-GPU share)",
            "value": B * T / (ms * 1e-3), "unit": "samples/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"1N4148 diode clipper, {B} sequences x {T} samples (1340 x 2048 tiled), one pot value per sequence on "
                                   "{10.0k, 25.2k, 75.0k, 99.1k} streamed as channel 1, MSE + ESR past 50 samples, Adam on {Is, nVt, C} in the step",
                       "global_batch": B, "seq_len": T, "chunks": k, "resistance_channel": "one value per sequence (WDF_R_PER_SEQUENCE)"
                       if binding.r_is_per_sequence(rt, True) else "per sample",
                       "loss_first_step": losses[0] if losses else None, "loss_last_step": losses[-1], "verify_status": stat,
                       "warm_start": st.warm.info() if st.warm is not None else None},
            "parity": parity, "library": library_identity(),
            "roofline": {"bound": "hbm", "kernel": "clipper_fused_tp_kernel", "achieved": moved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": moved / HBM_PEAK_GBS, "traffic": None, "algorithmic_bytes_per_sample": 12,
                         "note": "whole step (chunk kernel + finish launch) over x 4 + target 4 + y 4 bytes per sample"}}), flush=True)


def self_launch(n, argv, rehearse):
    """`python bench.py --gpus N` with no launcher around it: start the N ranks here -- torch.distributed.run, one process per
    GPU, rendezvous on 127.0.0.1 at a free port -- and hand their exit status back.  (Under a launcher WORLD_SIZE is set
    and this is skipped: the driver's `python -m torch.distributed.run ... bench.py --gpus N` form is untouched.)"""
    import socket
    import subprocess
    if not rehearse and torch.cuda.is_available() and torch.cuda.device_count() < n and "--launch-check" not in argv:
        print(f"bench: --gpus {n} but this node shows {torch.cuda.device_count()} GPU(s) (--rehearse-on-one-gpu runs the {n}-rank "
              f"code path on one)", file=sys.stderr, flush=True)
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # (dmabuf IPC: what RCCL needs on this driver)
    env.setdefault("OMP_NUM_THREADS", str(max(1, len(os.sched_getaffinity(0)) // n)))
    env["WDF_BENCH_SELF_LAUNCHED"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


def ranks_report(world, dev, dt_local, steps):
    """What the line says about the ranks that really took part: `ranks_seen` = an all-reduce of ones on the step's own
    process group (the collective's answer, not the environment's), the backend string, the distinct devices, and every
    rank's own time per step (the line's ms_per_step is their max)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return {"ranks_seen": 1, "collective_backend": None, "devices_seen": 1,
                "ms_per_step_per_rank": {"min": dt_local / steps * 1e3, "max": dt_local / steps * 1e3}}
    ones = torch.ones(1, dtype=torch.float32, device=dev)
    dist.all_reduce(ones, op=dist.ReduceOp.SUM)
    mine = torch.tensor([dt_local / steps * 1e3], dtype=torch.float64, device=dev)
    every = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(every, mine)
    if dev.type == "cuda":
        props = torch.cuda.get_device_properties(dev)
        ident = f"{os.uname().nodename}:{getattr(props, 'uuid', None) or getattr(props, 'pci_bus_id', dev.index)}:{dev.index}"
    else:
        ident = f"{os.uname().nodename}:cpu"
    idents = [None] * dist.get_world_size()
    dist.all_gather_object(idents, ident)
    backend = dist.get_backend()
    ver = None
    if backend == "nccl":
        try:
            ver = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            pass
    per = [float(t) for t in every]
    return {"ranks_seen": int(round(float(ones))), "world_size": dist.get_world_size(),
            "collective_backend": backend + (f" (RCCL {ver}: torch.distributed's nccl backend on ROCm)" if backend == "nccl" else
                                             " (rehearsal: every rank on cuda:0)" if backend == "gloo" and dev.type == "cuda" else
                                             " (no GPU: host ranks)" if backend == "gloo" else ""),
            "devices_seen": len(set(idents)),
            "ms_per_step_per_rank": {"min": min(per), "max": max(per), "all": per},
            "launcher": "bench.py started the ranks itself (torch.distributed.run)" if os.environ.get("WDF_BENCH_SELF_LAUNCHED")
                        else "started under an external launcher (WORLD_SIZE in the environment)"}


def spread(ts):
    ts = sorted(ts)
    return {"min": ts[0], "median": ts[len(ts) // 2], "max": ts[-1], "n": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps (default 200: at ~0.1 ms per step a 20-step region is one scheduler hiccup wide)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed steps before them (default 20)")
    ap.add_argument("--batch", type=int, default=8192, help="sequences per GPU (weak scaling) or in total (strong)")
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: --batch sequences on every rank (default).  strong: ONE batch of --batch sequences "
                         "split over the ranks (SURVEY 8e: global B = 8192 fixed)")
    ap.add_argument("--launch-check", action="store_true",
                    help="pre-flight: start / join the ranks, count them with an all-reduce on the step's process group, print the "
                         "`ranks` block and exit (no kernels; without a GPU the ranks meet over gloo)")
    ap.add_argument("--no-companion", action="store_true",
                    help="N > 1: skip the second measurement on the other scaling curve (strong next to a weak headline and vice versa)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the after-the-run check of y and the gradient against the oracle")
    ap.add_argument("--no-batch-major", action="store_true", help="skip the second measurement with x as [B,T]")
    ap.add_argument("--no-cold", action="store_true", help="skip the third measurement: the stateless step (value_cold)")
    ap.add_argument("--no-strong-proxy", action="store_true",
                    help="skip strong_proxy: the per-rank step of the 8-rank strong-scaling run (1/8 of the batch) timed on this GPU")
    ap.add_argument("--no-sustained", action="store_true", help="skip value_sustained: the headline loop kept running for ~2.5 s")
    ap.add_argument("--no-fwd-1024", action="store_true", help="skip value_fwd_1024: BASELINE configs[1], forward only at 1024 x 4096")
    ap.add_argument("--config", default=None, choices=["c2", "c4", "lpf", "hpf"],
                    help="c2: ONLY BASELINE configs[1] (1N4148 diode clipper forward-only, 1024 sequences x 4096 samples), its own JSON line.  "
                         "c4: BASELINE configs[3]'s per-GPU share (dataset-shaped batch, pot value per sequence, MSE + ESR, Adam).  "
                         "lpf / hpf: secondary lines -- lpf.py's training loop through the element API with resident components "
                         "(RC lowpass: linear one-pass step; HPF diode clipper: diode-root one-pass step)")
    ap.add_argument("--graph", default="auto", choices=["auto", "on", "off"],
                    help="capture one training step (kernels, all-reduce, update) as a HIP graph and replay it in the timed loop. "
                         "auto: on for the one-rank RCCL step of --force-dist and for the five-launch MLP-root step on one rank; off "
                         "for the single-rank one-launch diode step and -- until it has run on a node -- for N > 1 (`on` opts in)")
    ap.add_argument("--no-optimizer", action="store_true",
                    help="skip the on-device Adam update of {Is, nVt, R, C} that closes every step")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="testing aid: run the multi-rank code path (sharding, all-reduce, max-over-ranks timing) with "
                         "every rank on cuda:0 and the gloo backend, where only one GPU is available")
    ap.add_argument("--force-dist", action="store_true",
                    help="world size 1 only: create a one-rank RCCL (nccl) process group and run the fused-buffer "
                         "all-reduce + separate Adam launch of the N > 1 path, so that branch executes on a one-GPU box")
    ap.add_argument("--loss", default="mse", choices=["mse", "mse+esr"],
                    help="mse: the metric's loss (default). mse+esr: clipper_pot.py's training loss past 50 samples "
                         "(one-pass step: both tangent-weighted sums in the same pass; --two-kernel: one extra streaming "
                         "pass for the two loss sums)")
    ap.add_argument("--plan", default=None, metavar="KF,W,KB",
                    help="pin the time-parallel plan (forward chunks, cold warm-up steps, reverse chunks) instead of "
                         "autotuning it; used to profile one configuration across several rocprofv3 passes")
    ap.add_argument("--sequential", action="store_true", help="one lane per sequence, no time-parallel chunks")
    ap.add_argument("--two-kernel", action="store_true",
                    help="forward kernel + reverse-sweep kernel (24 B/sample through HBM, state stash) instead of the "
                         "one-pass step (12 B/sample)")
    ap.add_argument("--cold-forward", action="store_true",
                    help="every forward warms its chunks up from z = 0 (no state kept between steps) instead of "
                         "starting them from the previous step's snapshots")
    ap.add_argument("--root", default="diode", choices=["diode", "mlp2x16", "mlp2x8", "mlp4x8"],
                    help="diode: the metric's analytic diode-pair root (default).  mlp*: a secondary line -- the pot clipper "
                         "with the reference's DenseRootModel root at the training-set shape 1340 x 2048 (--batch to change)")
    ap.add_argument("--mlp-weights", default=None, metavar="PATH",
                    help="--root mlp*: the network's weights from this file (a model JSON in the reference's schema, or an .npz with "
                         "<net>_theta / <net>_sizes) instead of the package's copy of the reference's committed networks")
    ap.add_argument("--mlp-path", default="step", choices=["step", "unfused"],
                    help="--root mlp*: step = the resident training step (five launches, default); unfused = the round-3 pipeline")
    ap.add_argument("--x-batch-major", action="store_true",
                    help="make the [B,T] layout (the reference scripts') the HEADLINE measurement instead of the engine's "
                         "resident time-major copy")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, the measurements and checks that take runs of their own: parity against the "
                         "oracle, the other layout, the other scaling curve, the cold step, strong_proxy, the sustained loop, "
                         "forward-only at 1024 x 4096, copy bandwidth, the CPU baseline, kernel_ms of a short run continued "
                         "untimed (the --no-* options leave parts out)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed to DIR/<name>.npy (sse, grad, theta, y_sample; float32)")
    args = ap.parse_args()
    if args.dump_outputs and (args.config is not None or args.root != "diode"):
        raise SystemExit("--dump-outputs writes the headline step's outputs: not with --config or --root")
    # auto: replay where it has been exercised on hardware -- one rank (the five-launch MLP-root step; the one-rank RCCL step of
    # --force-dist).  N > 1 launches eagerly by default: a collective inside a captured graph has only ever run on ONE rank
    # (0.1232 eager against 0.1201 ms replayed there: 3 %), and a capture that went wrong on some ranks of a node would hang the
    # first real scaling run instead of slowing it; `--graph on` opts in.
    args.graph = (args.graph == "on") or (args.graph == "auto" and not args.rehearse_on_one_gpu and args.gpus == 1 and
                                          (args.force_dist or (args.root != "diode" and args.mlp_path == "step")))
    args.steps = 200 if args.steps is None else args.steps
    args.warmup = 20 if args.warmup is None else args.warmup

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher around us: start the ranks ourselves (one process per GPU) and pass their line and status through
        raise SystemExit(self_launch(args.gpus, sys.argv[1:], args.rehearse_on_one_gpu))
    if args.rehearse_on_one_gpu:
        os.environ["LOCAL_RANK"] = "0"
        world, rank, local = wdist.init(backend="gloo")
    else:
        world, rank, local = wdist.init(backend="nccl" if args.force_dist else None, force=args.force_dist)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.force_dist and world != 1:
        raise SystemExit("--force-dist is for world size 1")
    if args.launch_check:
        # pre-flight of the multi-rank entry point: the ranks are up (started here or by a launcher), the collective counts
        # them, rank 0 prints what it saw -- seconds on an 8-GPU node, and (gloo, no kernels) runnable without a GPU
        has_gpu = torch.cuda.is_available()
        dev = torch.device("cuda", local) if has_gpu else torch.device("cpu")
        r = ranks_report(world, dev, 0.0, 1)
        if rank == 0:
            print(json.dumps({"launch_check": True, "n_gpus": world, "ranks_seen": r["ranks_seen"], "ranks": r,
                              "ok": r["ranks_seen"] == world}), flush=True)
        if world > 1:
            wdist.barrier()
            torch.distributed.destroy_process_group()
        raise SystemExit(0 if r["ranks_seen"] == world else 3)
    binding.require_gpu()
    if args.config == "c2":
        dev = torch.device("cuda", local)
        r_ = forward_only(args, dev, workload.FS, steps=args.steps, warmup=args.warmup)
        if rank == 0:
            print(json.dumps({"metric": "samples/sec forward-only, 1N4148 diode clipper @48kHz, 1024 sequences x 4096 samples (BASELINE configs[1])",
                              "value": r_["value"], "unit": "samples/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                              "ms_per_step": r_["ms_per_call"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                              "dtype": "f32", "data": "synthetic", "config": {"workload": r_["workload"], "chunks": r_["chunks"],
                                                                            "warmup_steps": r_["warmup_steps"]},
                              "parity": {"max_abs_y": r_.get("max_abs_y_vs_oracle")},
                              "roofline": {"bound": "hbm", "kernel": "clipper_fwd_tp_kernel", "achieved": 8.0 * r_["value"] / 1e9,
                                           "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": r_["hbm_frac"], "traffic": None},
                              "detail": r_}), flush=True)
        return
    if args.config == "c4":
        if world != 1:
            raise SystemExit("--config c4 is the per-GPU share as a one-GPU line (the sharded run: --gpus N --loss mse+esr)")
        return run_c4(args, rank, local)
    if args.config in ("lpf", "hpf"):
        if world != 1:
            raise SystemExit("--config lpf / hpf are one-GPU lines (the element API's resident loops do not shard)")
        return run_tree_step(args, rank, local, args.config)
    if args.root != "diode":
        return (run_mlp_root if args.mlp_path == "unfused" else run_mlp_step)(args, world, rank, local)
    dev = torch.device("cuda", local)
    fs, T = workload.FS, args.seq_len
    Bg = args.batch * world if args.scaling == "weak" else args.batch
    b0, b1 = wdist.shard_range(Bg, rank, world)
    B = b1 - b0
    if B < 1:
        raise SystemExit("more ranks than sequences")

    # ---- resident inputs ---------------------------------------------------------------
    x_host = workload.sweep_batch(Bg, T, b0=b0, b1=b1)
    x = torch.as_tensor(x_host, device=dev)                                           # [B,T] as the scripts hold it
    theta_star = torch.tensor(workload.target_theta(), dtype=torch.float32, device=dev)
    target, _, _ = binding.clipper_fwd(x, theta_star, fs, want_stash=False)
    skip = 50 if args.loss == "mse+esr" else 0
    n_global = float(Bg * (T - skip))
    tm = not args.x_batch_major

    main_run = Trainer(args, x, target, fs, B, T, n_global, world, dev, tm)
    main_run.keep_outputs = bool(args.dump_outputs) and rank == 0
    dt, loss, grad = main_run.run(args.warmup, args.steps, dev)
    if main_run.outputs is not None:
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in main_run.outputs.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), np.ascontiguousarray(arr, dtype=np.float32))

    ranks = ranks_report(world, dev, main_run.dt_local, args.steps)
    if ranks["ranks_seen"] != world:
        raise SystemExit(f"the collective saw {ranks['ranks_seen']} ranks, WORLD_SIZE is {world}")

    # the OTHER scaling curve from the same invocation: the headline is per-GPU work fixed at --batch sequences ("weak", the
    # contract's default); SURVEY 8e's strong curve -- ONE batch of --batch sequences split over the ranks -- is timed right
    # behind it with the same K / W (at N = 1 the two are the same run)
    companion = None
    if args.full and world > 1 and not args.no_companion and args.loss == "mse":
        other_kind = "strong" if args.scaling == "weak" else "weak"
        Bg2 = args.batch if other_kind == "strong" else args.batch * world
        c0, c1 = wdist.shard_range(Bg2, rank, world)
        if c1 - c0 >= 1:
            x2_host = workload.sweep_batch(Bg2, T, b0=c0, b1=c1)
            x2 = torch.as_tensor(x2_host, device=dev)
            t2, _, _ = binding.clipper_fwd(x2, theta_star, fs, want_stash=False)
            run2 = Trainer(args, x2, t2, fs, c1 - c0, T, float(Bg2 * T), world, dev, tm)
            dt2, _, _ = run2.run(args.warmup, args.steps, dev)
            r2 = ranks_report(world, dev, run2.dt_local, args.steps)
            companion = {"scaling": other_kind, "value": Bg2 * T / (dt2 / args.steps), "unit": "samples/s",
                         "ms_per_step": dt2 / args.steps * 1e3, "global_batch": Bg2, "sequences_per_rank": c1 - c0,
                         "chunks": None if run2.tp is None else run2.tp.k_fwd,
                         "ms_per_step_per_rank": r2["ms_per_step_per_rank"], "steps": args.steps, "warmup": args.warmup}
            del run2, x2, t2

    # (per-launch durations: HIP events recorded inside the timed loop, Trainer.run)
    tp, stepper = main_run.tp, main_run.stepper
    tp_stat = binding.tp_status(stepper.status) if tp is not None and tp.k_fwd > 1 else None
    buf_last = stepper.out.clone()
    theta_final = [float(v) for v in main_run.theta]

    # the other layout, same step, same clock
    other = None
    if args.full and not args.no_batch_major and args.loss == "mse":
        alt = Trainer(args, x, target, fs, B, T, n_global, world, dev, not tm)
        dt_alt, _, _ = alt.run(args.warmup, args.steps, dev)
        other = Bg * T / (dt_alt / args.steps)
        del alt

    parity = None
    if args.full and rank == 0 and world == 1 and not args.no_parity and args.loss == "mse":
        g_first = None if main_run.first_sse is None else main_run.first_grad.cpu().numpy().astype(np.float64)
        parity = parity_check(stepper, main_run.theta, main_run.xk, x_host, target, fs, n_global, main_run.fused, g_first)

    # the STATELESS step: nothing carried from call to call, every chunk warms up from z = 0 (what a loop that presents
    # other data every step gets); same step otherwise, its own autotuned chunk count
    cold = None
    if args.full and not args.no_cold and not args.cold_forward and not args.sequential and main_run.fused:
        cr = Trainer(args, x, target, fs, B, T, n_global, world, dev, tm, cold=True)
        dt_c, _, _ = cr.run(args.warmup, args.steps, dev)
        cold = {"value": Bg * T / (dt_c / args.steps), "ms_per_step": dt_c / args.steps * 1e3,
                "chunks": None if cr.tp is None else cr.tp.k_fwd, "warmup_steps": None if cr.tp is None else cr.tp.warmup}
        del cr

    # SURVEY 8(e)'s strong-scaling curve, priced on ONE GPU: rank 0's shard of the 8192-sequence global batch under 8 ranks
    # (its first 1024 sequences), the same step, the same K / W -- what a rank of the 8-GPU strong run computes between two
    # all-reduces (the collective itself -- 20 bytes -- is not in it)
    strong_proxy = None
    if args.full and rank == 0 and world == 1 and not args.no_strong_proxy and args.loss == "mse" and main_run.fused and \
            B % 8 == 0 and B // 8 >= 128:
        Bs = B // 8
        xs, ts = x[:Bs].contiguous(), target[:, :Bs].contiguous()
        sp = Trainer(args, xs, ts, fs, Bs, T, n_global, world, dev, tm)
        dt_s, _, _ = sp.run(args.warmup, args.steps, dev)
        ms_e = dt_s / args.steps * 1e3
        stat_e = None if sp.tp is None or sp.tp.k_fwd < 2 else binding.tp_status(sp.stepper.status)
        k_e = None if sp.tp is None else sp.tp.k_fwd
        # the same step replayed as a HIP graph: at ~45 us per step the eager loop is bound by the HOST (two launches and the
        # torch glue of a step cost it ~55 us: a 200-step run shows it, a 20-step run hides it in the launch queue)
        import copy
        ga = copy.copy(args)
        ga.graph, ga.plan = True, (args.plan if args.plan else (None if sp.tp is None else f"{sp.tp.k_fwd},{sp.tp.warmup},{sp.tp.k_bwd}"))
        del sp
        sg = Trainer(ga, xs, ts, fs, Bs, T, n_global, world, dev, tm)
        dt_g, _, _ = sg.run(max(args.warmup, 8), args.steps, dev)
        ms_g = dt_g / args.steps * 1e3 if ga.graph else None       # (a failed capture falls back to eager launches: not a graph figure)
        ms_s = ms_e if ms_g is None else min(ms_e, ms_g)
        strong_proxy = {"ranks": 8, "B_per_rank": Bs, "ms_per_step": ms_s, "ms_per_step_eager": ms_e, "ms_per_step_graph_replay": ms_g,
                        "chunks": k_e, "verify_status": stat_e,
                        "verify_status_graph_replay": None if sg.tp is None or sg.tp.k_fwd < 2 else binding.tp_status(sg.stepper.status),
                        "projected_value_8": Bg * T / (ms_s * 1e-3), "projected_speedup_8": (dt / args.steps * 1e3) / ms_s,
                        "note": "one-GPU proxy of the per-rank step of the 8-rank STRONG run (global batch fixed): compute only, "
                                "the 20-byte all-reduce per step is not in it; ms_per_step = the better of eager launches and "
                                "HIP-graph replay of the same step (--graph on is how a rank would run it)"}
        del sg, xs, ts

    # the loop kept running (after the headline's burst of a few milliseconds), and BASELINE configs[1] (forward only)
    sustained = fwd1024 = None
    if args.full and rank == 0 and world == 1 and not args.no_sustained and main_run.fused and not args.graph:
        sustained = sustained_rate(main_run, Bg, T, dt / args.steps * 1e3)
    if args.full and rank == 0 and world == 1 and not args.no_fwd_1024 and args.loss == "mse":
        fwd1024 = forward_only(args, dev, fs)

    if rank == 0:
        copy_gbs = copy_bandwidth_gbs(dev) if args.full else None
        ms_step = dt / args.steps * 1e3
        value = Bg * T / (dt / args.steps)
        t_fwd, t_bwd = main_run.t_fwd, main_run.t_bwd
        fused = main_run.fused
        # the kernel's duration the roofline is priced with: the mean over the samples taken INSIDE the timed region (HIP
        # events on the launch stream); the untimed continuation's samples are reported beside them, never mixed in
        n_in = main_run.n_in_region if getattr(main_run, "n_in_region", 0) else len(t_fwd)
        f_in, b_in = t_fwd[:n_in], t_bwd[:n_in]
        f_ms = float(np.mean(f_in))
        b_ms = float(np.mean(b_in)) if t_bwd else None
        warm = getattr(main_run, "warm_after_timed", None) or (None if stepper.warm is None else stepper.warm.info())
        # a kernel's traffic depends on the batch, the layout and its OWN chunking only
        key = {"B": B, "T": T, "x_layout": "time-major" if tm else "batch-major", "loss": args.loss}
        w_used = None if tp is None else (tp.warmup if warm is None else warm["warm_unit_steps"] * max(0, warm["last_warm_tiles"]))
        if fused:
            # (round 6) the one-pass step's ALGORITHMIC bytes are the 12 B/sample it has to move -- x 4 + target 4 in, y 4 out:
            # no stash, x read once -- so `achieved` / `frac` are rates the memory system really sees and
            # can never exceed 1; SURVEY 8(d)'s 24 B/sample (the two-pass algorithm it assumed) is reported beside it
            dom, dom_ms, dom_bytes = "clipper_fused_tp_kernel", f_ms, BYTES_STEP_MOVED
            if tp is not None:
                key.update({"fused_chunks": tp.k_fwd, "fwd_warmup_steps": w_used})
        else:
            fname = "clipper_fwd_tp_kernel" if (tp is not None and tp.k_fwd > 1) else "clipper_fwd_kernel"
            dom, dom_ms, dom_bytes = (fname, f_ms, BYTES_FWD) if f_ms >= b_ms else ("clipper_bwd_tp_kernel", b_ms, BYTES_BWD)
            if tp is not None:
                if dom.startswith("clipper_fwd"):
                    key.update({"fwd_chunks": tp.k_fwd, "fwd_warmup_steps": w_used})
                else:
                    key.update({"bwd_chunks": tp.k_bwd})
        achieved = dom_bytes * B * T / (dom_ms * 1e-3) / 1e9
        traffic, traffic_src = (None, None) if tp is None else measured_traffic(dom, key)
        layout_names = {True: "time-major [T,B] resident copy (one-off transpose at data load, outside the timed region)",
                        False: "batch-major [B,T] as the reference scripts hold it"}
        curves = {args.scaling: {"value": value, "ms_per_step": ms_step, "global_batch": Bg, "sequences_per_rank": B}}
        if companion is not None:
            curves[companion["scaling"]] = companion
        elif world == 1:
            curves["strong" if args.scaling == "weak" else "weak"] = {"value": value, "ms_per_step": ms_step, "global_batch": Bg,
                                                                       "sequences_per_rank": B, "note": "N = 1: the same run"}
        curves = {k: curves[k] for k in ("strong", "weak") if k in curves}      # SURVEY 8(e) names the strong curve first
        if strong_proxy is not None:
            curves["strong"]["one_gpu_proxy_of_8_ranks"] = strong_proxy
        out = {
            "metric": "samples/sec fwd+bwd, 1N4148 diode clipper @48kHz batch=8192; 1->8 GPU scaling",
            "value": value, "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_step, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"1N4148 diode clipper fwd+bwd (grads wrt Is,nVt,R,C), {args.loss.upper()} loss, "
                                   f"{B} sequences x {T} samples @ {int(fs)} Hz per GPU (BASELINE configs[2])",
                       "global_batch": Bg, "seq_len": T, "parallelism": f"dp{world}",
                       "collective": ("RCCL all-reduce of the fused 5-float [SSE, grads] buffer on a one-rank nccl group "
                                      "(--force-dist)") if args.force_dist else
                                     (None if world == 1 else "all-reduce of the fused 5-float [SSE, grads] buffer per step"),
                       "loss": float(loss) / n_global, "grad": [float(g) for g in grad],
                       "optimizer": None if main_run.adam is None else
                       {"kind": "Adam on device (wdf_adam_step), lr = 1e-3 x component value, clip constraints",
                        "loss_first_step": float(main_run.first_sse) / n_global,
                        "loss_last_step": float(buf_last[0]) / n_global,
                        "theta_final": theta_final},
                       "x_layout": layout_names[tm],
                       "time_parallel": None if tp is None else
                       {"fwd_chunks": tp.k_fwd, "fwd_warmup_steps": tp.warmup, "verify_tol": tp.tol,
                        "bwd_chunks": None if fused else tp.k_bwd, "verify_status": tp_stat, "warm_start": warm}},
            # the ranks that took part, as the collective itself counted them; both scaling curves from this invocation:
            # `value` is the curve named by `scaling` (weak by default: --batch sequences on EVERY rank, the contract's
            # "per-GPU work fixed"); scaling_curves.strong is SURVEY 8e's global batch of --batch sequences split over the ranks
            "ranks_seen": ranks["ranks_seen"], "ranks": ranks,
            "headline_curve": f"{args.scaling}: `value` counts {Bg} sequences x {T} samples per step over {world} rank(s)",
            "scaling_curves": curves,
            "value_batch_major" if tm else "value_time_major": other,
            "step_launch": "one HIP-graph replay per step" if args.graph else "eager launches",
            "step_kernels": ("one pass: clipper_fused_tp_kernel (forward + loss + tangent-carried gradient, per-chunk records) and "
                             "clipper_fused_finish_kernel behind it (boundary verification, repair of missed tiles, record walk on "
                             "8 waves per tile, reduction, chain rule, warm-start steering, Adam)") if fused else
                            "two kernels: clipper_fwd_tp_kernel (+ gated repair) and clipper_bwd_tp_kernel (MSE-fused reverse sweep)",
            "kernel_ms": {"fused_step": spread(t_fwd)} if fused else {"fwd": spread(t_fwd), "bwd": spread(t_bwd)},
            "kernel_ms_in_region": ({"fused_step": spread(f_in)} if fused else {"fwd": spread(f_in), "bwd": spread(b_in)}),
            "kernel_ms_sampling": {"bracketed_in_timed_region": n_in, "all_samples": len(t_fwd),
                                   "note": "kernel_ms_in_region: HIP events around the kernel of every 4th TIMED step (these price the "
                                           "roofline); kernel_ms: those plus -- with --full, for runs of <= 64 steps -- the same loop continued "
                                           "untimed with every step bracketed (parameters and optimizer state restored afterwards); "
                                           "HIP-graph replay: the warm-up steps' kernels (a replayed step carries no events)"},
            "library": library_identity(),
            "parity": parity,
            "strong_proxy": strong_proxy,
            "value_cold": None if cold is None else cold["value"],
            "cold": cold,
            "value_sustained": None if sustained is None else sustained["value"],
            "sustained": sustained,
            "value_fwd_1024": None if fwd1024 is None else fwd1024["value"],
            "fwd_1024": fwd1024,
            "roofline": {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "traffic_source": traffic_src,
                         "algorithmic_bytes_per_sample": dom_bytes, "kernel_ms_used": dom_ms,
                         "copy_bandwidth": copy_gbs, "frac_of_copy_bandwidth": None if copy_gbs is None else achieved / copy_gbs},
        }
        if fused:
            # SURVEY 8(d)'s contract: frac = ALGORITHMIC bytes of forward + backward (24 B/sample) x the samples one launch
            # processes / the kernel's mean duration in the timed region / the 8 TB/s HBM peak.  The one-pass kernel does that
            # work moving 12 B/sample (x, target read; y written), so beside `frac` the block carries what the kernel itself
            # moves (hbm.frac_moved), what the counters saw (hbm.frac_traffic, from a committed PMC pass OF THIS BUILD, else
            # null) and the VALU-issue fraction (valu.frac: measured SQ pass of this build, else -- and it says so -- the
            # instruction-count model) -- the kernel's practical bound.
            moved = BYTES_STEP_MOVED * B * T / (dom_ms * 1e-3) / 1e9
            valu, valu_src = (None, None) if tp is None else measured_valu_cycles(dom, key)
            valu_kind = "measured: VALU-active cycles of a committed SQ counter pass of this build and configuration / this run's kernel time"
            if valu is None and tp is not None and key.get("x_layout") == "time-major" and args.loss == "mse":
                valu, valu_src = valu_cycle_model(B, T, tp.k_fwd, w_used or 0), "instruction-count model (bench.py valu_cycle_model)"
                valu_kind = "MODEL, not a measurement: VALU-active cycles from the instruction count fitted to earlier SQ passes / this run's kernel time"
            peak = N_SIMD * VALU_CLOCK_GHZ
            ach = None if valu is None else valu / (dom_ms * 1e-3) / 1e9
            survey = BYTES_STEP * B * T / (dom_ms * 1e-3) / 1e9
            out["roofline"].update({
                "frac_kind": "algorithmic bytes of the ONE-PASS step (x 4 + target 4 + y 4 = 12 B/sample) x samples per launch / mean "
                             "duration of clipper_fused_tp_kernel in the timed region / 8 TB/s.  The step's second launch "
                             "(clipper_fused_finish_kernel: verification, chunk records, reduction, Adam) is in ms_per_step, not in "
                             "this kernel's time; second_launch_ms is the difference",
                "second_launch_ms": ms_step - dom_ms,
                "survey_8d_two_pass_equivalent": {"bytes_per_sample": BYTES_STEP, "achieved": survey, "frac": survey / HBM_PEAK_GBS,
                                                  "note": "SURVEY 8(d) prices forward + backward at 24 B/sample (stash written and "
                                                          "read back, x read twice); this kernel does that work moving 12, so "
                                                          "the figure is nominal and may exceed 1"},
                "hbm": {"bytes_moved_per_sample": BYTES_STEP_MOVED, "moved": moved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac_moved": moved / HBM_PEAK_GBS,
                        "frac_traffic": None if traffic is None else traffic / (dom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        "traffic_over_moved": None if traffic is None else traffic / (BYTES_STEP_MOVED * B * T),
                        "frac_moved_of_copy_bandwidth": None if copy_gbs is None else moved / copy_gbs},
                "valu": {"frac": None if ach is None else ach / peak, "achieved": ach, "peak": peak,
                         "unit": "G VALU-active cycles/s (chip: 1024 SIMDs x 2.4 GHz)", "source": valu_src, "kind": valu_kind},
                "practical_bound": "VALU issue: ~110 instructions per two sample-steps (69 packed) at 2 waves per SIMD; valu.frac uses the "
                                   "2.4 GHz peak clock, the chip sustains ~1.9-2.2 GHz under this kernel (sustained.shader_clock_mhz)"})
        else:
            out["roofline"].update({"fwd_kernel_ms": f_ms, "bwd_kernel_ms": b_ms})
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(T, fs)
            out["speedup_vs_cpu"] = {"vs_best": value / out["cpu_baseline"]["value"],
                                     "vs_all_cores": value / out["cpu_baseline"]["all_cores"]["value"],
                                     "vs_one_core": value / out["cpu_baseline"]["value_one_core"],
                                     "target": 100.0, "met": value / out["cpu_baseline"]["value"] >= 100.0}
        print(json.dumps(out), flush=True)
    if world > 1 or args.force_dist:
        wdist.barrier()                      # rank 0 finishes its report before any communicator goes away
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
