"""Lowering of a tf_wdf element tree + root to the HIP kernels (the fast tier).

Circuit(top, root, probe) walks the tree the user built from tf_wdf elements, probes ONE
time step of it with unit vectors -- every adaptor / one-port is linear in the waves
(tf_wdf.py:31-214), so that step is a = ca.z + da.x ; b = root(a) ; z' = A z + Bx x + E b ;
y = cy.z + dy.x + fy b -- and runs the T-step recursion for the whole batch in one launch of
csrc/wdf_statespace.h (or csrc/wdf_clipper.h for the diode-clipper topology, which also
takes the per-sample resistance channel of clipper_pot.py:116-117).  The probe runs the
elements' own calc_impedance / reflected / incident code on tiny float64 torch vectors, so
the matrices carry the autograd graph back to R and C: the reverse-sweep kernel returns
dL/d(matrices) and torch chains it to the component values -- which is what
tape.gradient(loss, model.trainable_variables) is in the reference (lpf.py:87-90).
"""
import collections
import ctypes
import math
import os
from collections import namedtuple

import numpy as np
import torch

from . import binding
from . import compat_tf as tf
from . import warmstart
from .tensor_cache import EntryCache, ObjectMemo, tensor_key  # noqa: F401  (tensor_key: re-exported)


# ------------------------------------------------------------------------------ autograd glue
SsTpPlan = namedtuple("SsTpPlan", ["k_fwd", "warmup", "tol", "k_bwd"])
LAST_SS_TP_STATUS = {"status": None}
N_SIMD = 1024            # MI355X: 256 CUs x 4
# Whether Circuit.mse / mse_esr take the one-pass step of csrc/wdf_ss_asym_step.h on a tree under AsymDiodePair(any_tree=True):
# decided per loss by tools/ss_asym_step_bench.py (the step's slowest sample against the composed path's fastest, at both of its
# shapes; profiles/r13_ss_asym_step.jsonl).  Circuit._asym_tree_step is the step either way.
ASYM_TREE_STEP_SERVES = {"mse": False, "mse_esr": False}
# Whether Circuit.mse_esr() takes the one-pass MSE + ESR step of a resident LINEAR tree (csrc/wdf_ss_step.h: wdf_ss_lin_step_esr;
# Circuit._mse_esr_lin_step reaches it either way).  The project's standing criterion for a step: True only where the step's slowest
# sample beats the composed path's fastest at both shapes of tools/ss_lin_esr_step_bench.py (the linear step's section).
# Measured (profiles/r17_ss_lin_esr_step.jsonl): 0.142 ms against 0.905 ms at 8192 x 4096, 0.079 ms against 0.620 ms at 1340 x 2048.
LIN_ESR_STEP_SERVES = True
# Whether Circuit.mse / mse_esr(..., grad=False) take the loss-only evaluation pass on a resident diode-pair clipper
# (csrc/wdf_clipper_eval.h; Circuit._eval_resident reaches it either way).  True only where tools/eval_pass_bench.py shows the pass
# below the one-pass training step in the same process, storing y and not, each by more than the step's own min-max spread over
# the rounds (profiles/eval_pass.jsonl).  False: grad=False runs the step and detaches.
EVAL_PASS_SERVES = True
# Whether Circuit.mse_esr(..., grad=False) takes the MLP-root clipper's loss-only evaluation pass (csrc/wdf_mlp_eval.h:
# wdf_clipper_mlp_eval, mlp_root.MlpEvalPass) on a resident MLP-root clipper.  True only where tools/mlp_eval_pass_bench.py shows the
# pass, storing y and not, below BOTH the full training step and the step's forward + loss-sum phases followed by wdf_esr_coef, each
# by more than the compared variant's own min-max spread over the rounds, in a loop whose weights move
# (profiles/mlp_eval_pass.jsonl).  False: grad=False runs the step's forward and loss-sum phases.
# Measured at 1340 x 2048, 2x16 (median, min-max over 20 rounds): step 0.390 ms (0.382-0.408), forward + sums + esr_coef 0.373
# (0.372-0.374), the pass 0.188 (0.175-0.195) storing y and 0.189 (0.177-0.197) without: below both by more than their spreads.
MLP_EVAL_PASS_SERVES = True
# grad=False on a resident diode-root tree: the loss-only evaluation pass (csrc/wdf_ss_nl_eval.h) instead of the training step.
# Decided by tools/ss_nl_eval_bench.py (profiles/ss_nl_eval_pass.jsonl): the storing pass is below the MSE step
# and below the composed MSE + ESR route, each by more than the other's own min-max spread, at both shapes.
NL_EVAL_PASS_SERVES = True
# grad=False on a resident LINEAR tree: the loss-only evaluation pass (csrc/wdf_ss_lin_eval.h) instead of the one-pass training step.
# True only if tools/ss_lin_eval_bench.py shows the storing pass below the MSE step and below the MSE + ESR step at both shapes, each
# by more than the compared step's own min-max spread (profiles/ss_lin_eval_pass.jsonl).  _LinResident.evaluate
# reaches the pass either way.
# Measured on one MI355X, RC low-pass, ms per call, median [min-max] over 20 rounds of 5 calls:
#   8192 x 4096: MSE step 0.1165 [0.1151-0.1191], MSE + ESR step 0.1251 [0.1233-0.1284], the pass storing y 0.1174 [0.1167-0.1191],
#                without y 0.0959 [0.0949-0.0983]
#   1340 x 2048: MSE step 0.0481 [0.0470-0.0835], MSE + ESR step 0.0502 [0.0497-0.0591], the pass storing y 0.0417 [0.0408-0.0424],
#                without y 0.0392 [0.0377-0.0419]
# At 8192 x 4096 the storing pass is NOT below the MSE step: both move 16 B/sample at 4.6 TB/s, and on this one-capacitor tree the
# step's tangents hide under its memory time.  Below the MSE + ESR step by 0.008 ms there (its spread: 0.005); at 1340 x 2048 below
# both steps' medians by 13 % and 17 %, inside their spreads.  Hence False: grad=False runs the step and detaches, as before.
LIN_EVAL_PASS_SERVES = False


def plan_ss_time_parallel(coef64, ns, ni, root_kind, B, T, tol=1.0e-6):
    """SsTpPlan for the time-parallel state-space kernels (csrc/wdf_statespace.h), or None when the batch already fills the
    chip / the tree has no state.  Host arithmetic on the step's small matrices only (no device work, no sync).
    Reverse sweep: exact, so chunks are added until every SIMD holds ~2 waves (more only add record traffic).  Forward with a diode root: a chunk warms up
    from z = 0 for W steps; W outlasts the slowest mode of the step's Jacobian  A + Da E ca^T  at both ends of the diode's
    slope Da in [-1, 1] (off and fully conducting), with the same 0.01 tol margin as the clipper planner; chunks only while
    a chunk is at least as long as its warm-up.  The device verifies every boundary whatever the estimate."""
    if ns < 1:
        return None
    waves = max(1, -(-B // 64))
    k_bwd = min(T // 64, (2 * N_SIMD) // waves)           # (measured at 8192 x 4096: 16 chunks 0.179 ms, 32: 0.182, 64: 0.221)
    k_fwd, W = 1, 0
    if root_kind in (binding.ROOT_DIODE_PAIR, binding.ROOT_ASYM_PAIR):      # (two different diodes: Da = 2/F - 1, F >= 1 -- the same bound)
        c = coef64.detach().double().cpu().numpy()
        A = c[:ns * ns].reshape(ns, ns)
        oE = ns * ns + ns * ni
        E, ca = c[oE:oE + ns], c[oE + ns:oE + 2 * ns]
        rho = max(float(np.max(np.abs(np.linalg.eigvals(A + sgn * np.outer(E, ca))))) for sgn in (1.0, -1.0))
        if rho < 1.0 - 1e-9:
            W = 16 if rho <= 0.0 else max(16, -(-int(math.ceil(math.log(0.01 * tol) / math.log(rho))) // 8) * 8)
            k_fwd = min(T // max(W, 64), (2 * N_SIMD) // waves)
    if k_fwd < 2 and k_bwd < 2:
        return None
    return SsTpPlan(max(1, k_fwd), W, float(tol), max(1, k_bwd))


class SsWarmStart:
    """Warm-started chunks for the time-parallel state-space forward when the SAME batch is visited again with slightly
    different coefficients (a training loop: lpf.py:86-99 re-runs data_in every epoch): chunk k starts from the state the
    previous call had at the sample its warm-up begins -- the secant through the last two calls once there are two -- so a
    fraction of the cold warm-up closes the gap, and with the shorter warm-up more chunks pay.  The device verifies every
    boundary as always; warmstart.WarmUpController steers the warm-up from its verdicts.  One object per (batch, circuit);
    made by Circuit.__call__, keyed on the caller's tensor and its version."""

    def __init__(self, T, B, ns, plan, secant=True):
        self.T, self.B, self.ns, self.plan, self.secant = int(T), int(B), int(ns), plan, bool(secant)
        self.k_max = max(2, (2 * N_SIMD) // max(1, -(-self.B // 64)))
        # (misses here are real -- a diode root contracts -- so one repaired wave counts; far inside the tolerance the
        #  controller takes two units at a time)
        self.ctl = warmstart.WarmUpController(plan.warmup, plan.warmup // 4, unit=16, floor=16, miss_waves=1, wait_calls=16,
                                              bold_below=4.0, tol=plan.tol)
        self.rows, self.prev = {}, {}
        self._idx = {}
        self.trace = collections.deque(maxlen=256)      # warm-up used by the last calls (probing)

    def chunks(self, W):
        return binding.lib().wdf_ss_tp_chunks(self.T, max(2, min(self.T // max(W, 64), self.k_max)))

    def start(self):
        """-> (chunks, warm-up, zinit) for this call; (plan's, cold, None) when there is nothing to start from yet."""
        self.ctl.cold = self.plan.warmup
        W = self.ctl.begin(self.rows)
        if W is None:
            return self.plan.k_fwd, self.plan.warmup, None
        r1, r2 = self.rows[W], (self.prev.get(W) if self.secant else None)
        return self.chunks(W), W, (r1 if r2 is None else torch.lerp(r2, r1, 2.0))

    def finish(self, zs, status, was_warm, w_used):
        """After the forward: keep this call's states at the chunk starts the next call may use; queue the verdict."""
        if was_warm:
            self.ctl.end(status, w_used)
        cands = self.ctl.candidates()
        key = tuple(cands)
        if key not in self._idx:
            if len(self._idx) > 16:
                self._idx.clear()
            starts = [binding.ss_tp_starts(self.T, self.chunks(w), w) for w in cands]
            self._idx[key] = (torch.tensor([t for s_ in starts for t in s_], dtype=torch.int64, device=zs.device),
                              [len(s_) for s_ in starts])
        idx, lens = self._idx[key]
        rows = zs.index_select(0, idx).split(lens, 0)            # [sum of chunk counts, ns, B] floats; the stash is not kept
        self.prev = {w: self.rows[w] for w, n in zip(cands, lens) if w in self.rows and self.rows[w].shape[0] == n}
        self.rows = dict(zip(cands, rows))
        self.trace.append(w_used)


class DynWarmStart:
    """Warm-started chunks for the streamed-coefficient forward (csrc/wdf_ss_dyn.h) when the SAME batch is visited again with
    components one optimizer step apart: the previous call's whole state stash is kept (T ns B floats), so chunk k may start
    any number of steps W before its first owned step from the state that call had there; warmstart.WarmUpController steers
    W from the device's verdicts (a miss costs a sequential re-run of the waves concerned, never a wrong result), and with
    the shorter warm-up more chunks pay.  A tree whose cold warm-up outlasts its chunks (HPFDiodeClipper.h's: 672 steps) runs
    its first call sequentially and is chunked from the second on."""

    def __init__(self, T, B, ns, k_max, cold_W, tol):
        self.T, self.B, self.ns, self.k_max = int(T), int(B), int(ns), int(k_max)
        cap = max(32, min(int(cold_W), self.T // 2) // 16 * 16)
        self.ctl = warmstart.WarmUpController(cap, max(32, cap // 2), unit=16, floor=16, miss_waves=1, wait_calls=16, bold_below=4.0,
                                              tol=tol)
        self.prev = None
        self.trace = collections.deque(maxlen=256)

    def start(self):
        """-> (chunks, warm-up, zinit [K, ns, B]) or None (no earlier call to start from)."""
        if self.prev is None:
            return None
        W = self.ctl.begin(range(0, 1 << 30))
        K = binding.dyn_chunks(self.T, max(2, min(self.k_max, self.T // max(W, 64))))
        if K < 2:
            return None
        Lc = binding.dyn_chunk_len(self.T, K)
        key = (K, W)
        if getattr(self, "_idx_key", None) != key:
            self._idx_key = key
            self._idx = torch.tensor([max(0, k * Lc - W) for k in range(K)], dtype=torch.int64, device=self.prev.device)
        return K, W, self.prev.index_select(0, self._idx).contiguous()

    def finish(self, zs, status, was_warm, w_used):
        if was_warm and status is not None:
            self.ctl.end(status, w_used)
        self.prev = zs
        self.trace.append(w_used)


class _StateSpaceFn(torch.autograd.Function):
    """y [T,B] = statespace(coef, rootp, x [B,T,ni], z0).  tp: an SsTpPlan (time-parallel kernels) or None.
    warm: an SsWarmStart for this batch (training loops) or None.
    An x that carries a graph gets dL/dx from a pass of its own behind the reverse sweep (csrc/wdf_statespace.h:
    ss_bwd_gx_kernel); a plain x launches what it always launched.
    launches: how many times the input-gradient pass went out (tests read it)."""
    launches = {"gx": 0}

    @staticmethod
    def forward(ctx, coef, rootp, x, z0, ns, ni, root_kind, n_up, n_down, want_zT, tp=None, warm=None):
        need = coef.requires_grad or (rootp is not None and rootp.requires_grad) or (z0 is not None and z0.requires_grad)
        need = need or ctx.needs_input_grad[2]
        c = coef.detach().contiguous()
        rp = None if rootp is None else rootp.detach().contiguous()
        z0d = None if z0 is None else z0.detach().contiguous()
        B, T = x.shape[0], x.shape[1]
        k_lin = min(T // 64, (2 * 1024) // max(1, -(-B // 64))) if (root_kind == binding.ROOT_NONE and ns > 0) else 0
        if k_lin >= 2:      # linear tree, few sequences: the exact chunked scan (csrc/wdf_statespace.h) fills the chip
            y, zs, zT = binding.ss_fwd_lin_tp(x, c, ns, ni, k_lin, want_stash=need, z0=z0d, want_zT=want_zT)
        elif tp is not None and tp.k_fwd >= 2 and root_kind in (binding.ROOT_DIODE_PAIR, binding.ROOT_ASYM_PAIR):
            # nonlinear root: chunks warmed up from z = 0, verified on the device, missed waves re-run sequentially
            k, W, zinit = (tp.k_fwd, tp.warmup, None) if (warm is None or not need or z0d is not None) else warm.start()
            y, zs, zT, st = binding.ss_fwd_tp(x, c, ns, ni, rp, k, W, tp.tol, n_up, n_down, want_stash=need,
                                              z0=z0d, want_zT=want_zT, zinit=zinit, root_kind=root_kind)
            LAST_SS_TP_STATUS["status"] = st
            LAST_SS_TP_STATUS["warmup_used"], LAST_SS_TP_STATUS["chunks_used"] = W, k
            if warm is not None and need and z0d is None:
                warm.finish(zs, st, zinit is not None, W)
        else:
            y, zs, zT = binding.ss_fwd(x, c, ns, ni, root_kind, rp, n_up, n_down, want_stash=need, z0=z0d, want_zT=want_zT)
        ctx.cfg = (ns, ni, root_kind, n_up, n_down, z0 is not None, tp)
        ctx.save_for_backward(c, rp, x, zs)
        if want_zT:
            ctx.mark_non_differentiable(zT)
            return y, zT
        return y, None

    @staticmethod
    def backward(ctx, gy, _gzT):
        ns, ni, root_kind, n_up, n_down, has_z0, tp = ctx.cfg
        c, rp, x, zs = ctx.saved_tensors
        want_gx = ctx.needs_input_grad[2]
        gy = gy.contiguous()
        k, ws = 1, None
        if tp is not None and tp.k_bwd >= 2 and ns >= 1:      # exact chunked reverse sweep (any root)
            k = tp.k_bwd
            gcoef, groot, gz0, *ws = binding.ss_bwd_tp(x, c, ns, ni, zs, gy, k, root_kind, rp, n_up, n_down, want_gz0=has_z0,
                                                       return_ws=want_gx)
        else:
            gcoef, groot, gz0 = binding.ss_bwd(x, c, ns, ni, zs, gy, root_kind, rp, n_up, n_down, want_gz0=has_z0)
        gx = None
        if want_gx:
            # dL/dx: the sweep's chunks, each from the adjoint that enters it (re-walked from the records the sweep left in ws);
            # time-major [T,ni,B], handed back as a view in x's layout
            gx = binding.ss_bwd_gx(x, c, ns, ni, zs, gy, root_kind, rp, n_up, n_down, n_chunks=k,
                                   ws_bwd_tp=ws[0] if ws else None).permute(2, 0, 1)
            _StateSpaceFn.launches["gx"] += 1
        return gcoef, groot, gx, gz0, None, None, None, None, None, None, None, None


class _AsymTreeStepFn(torch.autograd.Function):
    """loss = the one-pass step of a small tree under ROOT_ASYM_PAIR (csrc/wdf_ss_asym_step.h) over (coef, rootp): forward runs
    the step and keeps d loss/d coef and d loss/d rootp, backward hands them back scaled by the incoming gradient -- the
    float64 probe's graph carries them on to R, C and the diode Variables, as it does _StateSpaceFn's.
    kind: "mse" (mean squared error) | "mse_esr" (the scripts' loss on the rows past skip).  -> loss, y [T,B], zT [ns,B] | None."""

    @staticmethod
    def forward(ctx, coef, rootp, x, target, ns, ni, kind, skip, z0, want_zT, k, W, tol):
        c, rp = coef.detach().contiguous(), rootp.detach().contiguous()
        B, T, nc = x.shape[0], x.shape[1], c.numel()
        if kind == "mse":
            n = float(B * T)
            y, zT, out, st = binding.ss_asym_step_mse(x, c, rp, ns, ni, target, 2.0 / n, k, W, tol, z0=z0, want_zT=want_zT)
            loss, g = out[0] / n, out[1:]
        else:
            n = float(B * (T - skip))
            y, zT, _, g, loss3, st = binding.ss_asym_step_esr(x, c, rp, ns, ni, target, n, float(np.finfo(float).eps), skip, k, W, tol,
                                                              z0=z0, want_zT=want_zT)
            loss = loss3[2].clone()
        LAST_SS_TP_STATUS["status"] = st
        LAST_SS_TP_STATUS["warmup_used"], LAST_SS_TP_STATUS["chunks_used"] = W, k
        ctx.save_for_backward(g[:nc], g[nc:])
        ctx.mark_non_differentiable(y)
        if zT is not None:
            ctx.mark_non_differentiable(zT)
        return loss, y, zT

    @staticmethod
    def backward(ctx, gl, _gy, _gzT):
        gcoef, groot = ctx.saved_tensors
        return (gcoef * gl, groot * gl) + (None,) * 11


class _LossTermsFn(torch.autograd.Function):
    """loss = w_mse mse + w_esr esr + w_emph esr_emph + w_avg avg of (y, target) [T,B] past `skip` (clipper_pot.py:141-165), the
    fused device stage of csrc/wdf_elementwise.h: forward launches sums -> (sums_allreduce(sums6), in place) -> coef -> grad and
    returns (loss, terms[5] = {mse, esr, esr_emph, avg, loss}); backward hands back gy times the incoming scalar, for whichever
    reverse sweep produced y.  want_grad False (a validation pass) skips the grad launch.
    launches: how many times each kernel family went out (tests read it: a validation pass leaves "grad" alone)."""
    launches = {"sums": 0, "coef": 0, "grad": 0}

    @staticmethod
    def forward(ctx, y, target, skip, weights, coeff, n, sums_allreduce, want_grad):
        yd = y.detach().contiguous()
        sums6 = binding.loss_terms_sums(yd, target, skip, coeff)
        _LossTermsFn.launches["sums"] += 1
        if sums_allreduce is not None:
            sums_allreduce(sums6)
        gcoef, terms = binding.loss_terms_coef(sums6, n, float(np.finfo(float).eps), weights, coeff)
        _LossTermsFn.launches["coef"] += 1
        gy = None
        if want_grad:
            gy = binding.loss_terms_grad(yd, target, gcoef, skip, coeff)
            _LossTermsFn.launches["grad"] += 1
        ctx.save_for_backward(gy)
        ctx.mark_non_differentiable(terms)
        return terms[4].clone(), terms

    @staticmethod
    def backward(ctx, gl, _gterms):
        gy, = ctx.saved_tensors
        if gy is None:
            raise binding.WdfHipError("Circuit.loss: this loss was evaluated without a gradient (torch.no_grad(), or nothing "
                                      "required one)")
        return gy * gl, None, None, None, None, None, None, None


# The device tape interpreter keeps a sample's node values in LDS: its time grows with the square of the tape's length, torch's
# (one launch per operation over the whole channel) linearly -- past this many operations torch runs the tape
# (tools/ss_dyn_rows_crossover.py, profiles/r05_rows_crossover.txt: 32 operations 1.6 vs 2.2 ms per step, 48: 2.5 vs 3.3, 89: 5.5 vs 5.2, 138: 12.9 vs 7.5).
DYN_ROWS_MAX_OPS = int(os.environ.get("WDF_DYN_ROWS_MAX_OPS", "80"))


class _DynRowsFn(torch.autograd.Function):
    """rows [T,n,B] (or the static row [n]) of a probed step from its tape, on the device (csrc/wdf_ss_dyn_rows.h):
    calc_impedance for every sample in one launch; backward: dLoss/d(component value) from the rows' adjoint in two."""

    @staticmethod
    def forward(ctx, rtape, chan, r, *vals):
        params = torch.stack([v.detach().double().reshape(()) for v in vals]) if vals else torch.zeros((0,), dtype=torch.float64, device=r.device)
        rows = binding.ss_dyn_rows(rtape, params, chan, r)
        ctx.rtape, ctx.chan, ctx.r, ctx.params = rtape, chan, r, params
        ctx.dtypes = [v.dtype for v in vals]
        return rows if r is not None else rows.reshape(-1)

    @staticmethod
    def backward(ctx, grows):
        g = grows.float().contiguous()
        if ctx.r is None:
            g = g.reshape(1, -1, 1)
        gp = binding.ss_dyn_rows_bwd(ctx.rtape, ctx.params, ctx.chan, ctx.r, g)
        need = ctx.needs_input_grad[3:]
        return (None, None, None) + tuple(gp[i].to(ctx.dtypes[i]) if need[i] else None for i in range(len(need)))


class _SsDynFn(torch.autograd.Function):
    """y [T,B] = the state-space recursion with streamed coefficient rows and / or the MLP root (csrc/wdf_ss_dyn.h).
    rows: [T,n,B] (per-sample impedance) or [n] (static), n = A | Bx | E | ca | da | cy | dy | fy | R_port.
    rootvec: {Is, nVt} (diode root), {Is_up, nVt_up, Is_down, nVt_down} (two different diodes), the flat weights (MLP root) or None.  The reverse sweep hands back dL/d(row entry) for
    every sample; torch chains it through the rows' own graph (the probe tape evaluated over the resistance channel) to the
    component values -- calc_impedance's chain rule per sample (tf_wdf.py:114-115,139-145,168-177)."""

    @staticmethod
    def forward(ctx, rows, rootvec, x, z0, ns, ni, kind, hidden, n_tanh, n_up, n_down, want_zT, tp=None, warm=None):
        need = rows.requires_grad or (rootvec is not None and rootvec.requires_grad) or (z0 is not None and z0.requires_grad)
        need = need or (warm is not None and ns >= 1)                         # (the next call's chunks start from this call's states)
        hot = warm.start() if (warm is not None and z0 is None) else None
        if hot is not None:
            tp = SsTpPlan(hot[0], hot[1], tp.tol if tp is not None else 1.0e-6, tp.k_bwd if tp is not None else 1)
        r = rows.detach().float().contiguous()
        rv = None if rootvec is None else rootvec.detach().float().contiguous()
        z0d = None if z0 is None else z0.detach().float().contiguous()
        rootp, w = (rv, None) if kind in (binding.ROOT_DIODE_PAIR, binding.ROOT_ASYM_PAIR) else (None, rv)
        if tp is not None and tp.k_fwd >= 2 and ns >= 1:       # verified time chunks; the waves that missed re-run sequentially
            y, zs, zT, st = binding.ss_dyn_fwd_tp(x, r, ns, ni, tp.k_fwd, tp.warmup, tp.tol, kind, rootp=rootp, w=w, hidden=hidden,
                                                  n_tanh=n_tanh, n_up=n_up, n_down=n_down, want_stash=need, z0=z0d, want_zT=want_zT,
                                                  zinit=None if hot is None else hot[2])
            LAST_SS_TP_STATUS["status"] = st
            LAST_SS_TP_STATUS["warmup_used"], LAST_SS_TP_STATUS["chunks_used"] = tp.warmup, tp.k_fwd
        else:
            st = None
            y, zs, zT = binding.ss_dyn_fwd(x, r, ns, ni, kind, rootp=rootp, w=w, hidden=hidden, n_tanh=n_tanh, n_up=n_up, n_down=n_down,
                                           want_stash=need, z0=z0d, want_zT=want_zT)
        if warm is not None and z0 is None and zs is not None:
            warm.finish(zs, st, hot is not None, tp.warmup if (tp is not None and st is not None) else 0)
        ctx.tp = tp
        ctx.cfg = (ns, ni, kind, hidden, n_tanh, n_up, n_down, z0 is not None, rows.dim() == 3)   # (3 dims: [T,n,B] or [1,n,B])
        ctx.save_for_backward(r, rv, x, zs)
        if want_zT:
            ctx.mark_non_differentiable(zT)
            return y, zT
        return y, None

    @staticmethod
    def backward(ctx, gy, _gzT):
        ns, ni, kind, hidden, n_tanh, n_up, n_down, has_z0, per_sample = ctx.cfg
        r, rv, x, zs = ctx.saved_tensors
        rootp, w = (rv, None) if kind in (binding.ROOT_DIODE_PAIR, binding.ROOT_ASYM_PAIR) else (None, rv)
        if zs is None:
            zs = torch.zeros((x.shape[1], 1, x.shape[0]), dtype=torch.float32, device=x.device)      # (ns = 0: nothing to read)
        tp = ctx.tp
        if tp is not None and tp.k_bwd >= 2 and ns >= 1:       # exact time chunks
            grows, groot, gz0 = binding.ss_dyn_bwd_tp(x, r, ns, ni, zs, gy.contiguous(), tp.k_bwd, kind, rootp=rootp, w=w, hidden=hidden,
                                                      n_tanh=n_tanh, n_up=n_up, n_down=n_down, want_gz0=has_z0)
        else:
            grows, groot, gz0 = binding.ss_dyn_bwd(x, r, ns, ni, zs, gy.contiguous(), kind, rootp=rootp, w=w, hidden=hidden, n_tanh=n_tanh,
                                                   n_up=n_up, n_down=n_down, want_gz0=has_z0)
        if not per_sample:
            # static row: the kernel summed over the steps itself (float64 accumulators, grows [1,n,B]: no [T,n,B] array of
            # per-sample products exists any more); what is left is the sum over the sequences
            grows = grows.sum(dim=(0, 2), dtype=torch.float64).float()
        return (grows, None if groot is None else groot.float(), None, (gz0[:ns] if has_z0 else None), None, None, None, None, None,
                None, None, None, None, None)


def _nbytes(*ts):
    return sum(t.numel() * t.element_size() for t in ts if isinstance(t, torch.Tensor))


# ------------------------------------------------------------------------------ resident linear trees
_LIN_OCC = int(os.environ.get("WDF_LIN_OCC", "2"))       # chunks are cut so that every SIMD gets this many waves
_NL_OCC = int(os.environ.get("WDF_NL_OCC", "1"))
_NL_WMIN = int(os.environ.get("WDF_NL_WMIN", "16"))      # the shortest warm-up the device's controller may settle on
# chunk waves per SIMD of the diode-root evaluation pass: 1, as the step (the fastest of the sweep over 1, 2, 4 at 8192 x 4096;
# at 1340 x 2048 the 64-step floor of a chunk caps the count before it matters: DESIGN section 4)
_NL_EVAL_OCC = int(os.environ.get("WDF_NL_EVAL_OCC", str(_NL_OCC)))
# chunk waves per SIMD of the linear trees' evaluation pass: the step's, and it has to stay the step's by default -- the chunk
# count decides the bits (the order of the sums, where the walk rounds), and grad=False must report what the default reports
_LIN_EVAL_OCC = int(os.environ.get("WDF_LIN_EVAL_OCC", str(_LIN_OCC)))
_ROWS = 1024                                             # result rows per slab (see _LinResident.entry)
NL_TOL = 1.0e-6                                          # boundary tolerance of the diode-root one-pass step (plan_ss_time_parallel's)
ESR_EPS = float(np.finfo(float).eps)                     # what the scripts' esr_loss adds to the energy (clipper_pot.py:146-156)


class _LinResident:
    """A linear tree (ideal-source root) whose component values live on the device: the probed step as a device tape
    (probe_tape.py), and per (x, target) pair the buffers of the one-pass MSE step (csrc/wdf_ss_step.h)."""

    def __init__(self, circ, device):
        from . import probe_tape
        self.circ = circ
        own = {"Resistor": "R", "ResistiveVoltageSource": "R", "Capacitor": "C"}
        self.params = []                                          # (element, attribute) of every component value, tree order
        for e in circ.elements:
            name = own.get(_kind(e))
            if name is not None:
                self.params.append((e, name))
        pvars = [e.__dict__[n] for e, n in self.params]
        self.n_tree = len(pvars)                                  # the component values the tape sees; then the root's own
        if circ.root_kind == "DiodePair":
            self.params += [(circ.root, "Is"), (circ.root, "nVt")]
            pvars += [circ.root.Is, circ.root.nVt]
        if not 1 <= len(pvars) <= probe_tape.MAX_PARAMS:
            raise binding.WdfHipError(f"Circuit.to_device: 1..{probe_tape.MAX_PARAMS} component values (this tree has {len(pvars)})")
        for (e, n), v in zip(self.params, pvars):
            # what the resident step would silently freeze is refused (as on the clipper path): a value computed from other
            # Variables would get no gradient and never move; a Variable another circuit's block already holds
            if isinstance(v, torch.Tensor) and not getattr(v, "_is_tf_variable", False) and (v.requires_grad or v.grad_fn is not None):
                raise binding.WdfHipError(f"Circuit.to_device: {type(e).__name__}.{n} is a tensor computed from other Variables; the "
                                          "resident step would freeze it -- keep this circuit on the host path")
            if isinstance(v, torch.Tensor) and getattr(v, "_wdf_block", None) is not None:
                raise binding.WdfHipError("Circuit.to_device: a component Variable already lives in another circuit's block")
        # the tape is recorded (and its size checked) BEFORE any Variable moves: a circuit the device probe cannot hold
        # leaves its Variables where they were
        tape, outs, rport = probe_tape.record(circ, pvars[:self.n_tree])
        self.captured = list(pvars)                               # what every (element, attribute) held at to_device()
        self.captured_val = [float(v) for v in pvars]
        self.pb = tf.ParamBlock(self.captured_val, torch.device(device))
        for i, v in enumerate(pvars):
            if isinstance(v, torch.Tensor) and getattr(v, "_is_tf_variable", False) and v.numel() == 1:
                self.pb.adopt(i, v)
        self.adopted = {i: v for i, v in self.pb.members.items()}
        self.host_tape, self.host_outs = tape, outs + [rport]
        ops, consts = tape.packed()
        dev = self.pb.block.device
        self.n_ops, self.n_out = int(ops.shape[0]), len(outs) + 1
        self.tape = torch.as_tensor(ops, device=dev).contiguous()
        self.consts = torch.as_tensor(consts if len(consts) else np.zeros(1), device=dev)
        self.outs = torch.as_tensor(np.asarray(outs + [rport], dtype=np.int32), device=dev)
        self.coef = torch.zeros(self.n_out, dtype=torch.float32, device=dev)
        self.coef64 = torch.zeros(self.n_out, dtype=torch.float64, device=dev)
        self.jac = torch.zeros((self.n_out, self.n_tree), dtype=torch.float64, device=dev)
        self.cache = EntryCache()

    def check(self):
        """Every component value must still be what to_device() captured: an adopted Variable the same object, still in the
        block; a frozen (non-Variable) value the same object or the same number -- set_resistance / `e.R = ...` afterwards
        would otherwise be silently ignored by the resident step."""
        for i, (e, n) in enumerate(self.params):
            v = e.__dict__.get(n)
            if i in self.adopted:
                if v is not self.adopted[i] or getattr(v, "_wdf_block", (None,))[0] is not self.pb:
                    raise binding.WdfHipError(f"Circuit.to_device: {type(e).__name__}.{n} was replaced after to_device(); build a new Circuit")
            elif v is not self.captured[i]:
                same = False
                try:
                    same = (not isinstance(v, torch.Tensor) or v.numel() == 1) and float(v) == self.captured_val[i]
                except (TypeError, ValueError):
                    pass
                if not same:
                    raise binding.WdfHipError(f"Circuit.to_device: {type(e).__name__}.{n} was changed after to_device() (the resident "
                                              "step holds the value it had then); build a new Circuit")
                self.captured[i] = v

    def probe(self):
        """The step's coefficients and their Jacobian from the block, on the device -- behind the optimizer updates the
        script queued since the last step (compat_tf.ParamBlock.defer), in the SAME launch."""
        L = binding.lib()
        jobs = self.pb.take_pending()
        with torch.no_grad(), torch._C.DisableTorchFunctionSubclass():
            arr = binding.adam_jobs(jobs) if jobs else None
            rc = L.wdf_ss_probe_adam(None if arr is None else ctypes.cast(arr, ctypes.c_void_p), len(jobs), binding._ptr(self.tape),
                                     self.n_ops, binding._ptr(self.consts), binding._ptr(self.pb.block), self.n_tree,
                                     binding._ptr(self.outs), self.n_out, binding._ptr(self.coef), binding._ptr(self.coef64),
                                     binding._ptr(self.jac), binding._stream())
        binding._check(rc, "wdf_ss_probe_adam")

    def host_coef(self):
        """The coefficient vector (float64 numpy, and the port resistance) at the block's lagging host mirror: what the
        time-parallel planner needs, without a synchronisation."""
        hv = tuple(self.pb.host_values()[:self.n_tree])
        if getattr(self, "_hc_key", None) != hv:                  # (the mirror moves every few dozen steps: evaluated then only)
            vals, _ = self.host_tape.evaluate(hv, self.host_outs)
            self._hc_key, self._hc_val, self.plans = hv, (vals[:-1], float(vals[-1])), {}
        return self._hc_val

    def entry(self, x, target, loss="mse", skip=0, store_output=True):
        """The buffers of one training set: per (x, target) pair and -- for the diode-root step's MSE + ESR loss -- per
        (loss, skip), so that an MSE and an ESR loop over the same data each keep their own workspace (snapshots, warm-up
        control, chunk count).  The output buffer ent["y"] is made by the first call that wants it (store_output; output()):
        an entry only ever run without the y store holds none, and calls with and without it share the entry."""
        extra = None if loss == "mse" else (loss, int(skip))
        ent = self.cache.get((x, target), extra)
        if ent is None:
            circ, dev = self.circ, self.pb.block.device
            x_tm, tgt, B, T = self._resident_pair(x, target)
            per_wave = 128 if B % 2 == 0 else 64                  # (two sequences per lane when the rows pair up)
            if loss != "mse" and circ.root_kind == "DiodePair" and circ.ns * circ.ni > 1:
                per_wave = 64                                     # (the diode-root MSE + ESR step pairs them up on the smallest tree only;
                #                                                    the linear one pairs them up on every tree, as its MSE step does)
            L_ = binding.lib()
            if circ.root_kind == "DiodePair":
                # the tangent-carried step of a diode-pair root: chunks no shorter than 64 steps, one wave per SIMD and up
                k = max(1, min(T // 64, (_NL_OCC * N_SIMD) // max(1, -(-B // per_wave))))
                ws = self._plan_nl(B, T, k, dev)
            else:
                k = max(1, min(T // 64, (_LIN_OCC * N_SIMD) // max(1, -(-B // per_wave))))
                ws_bytes = L_.wdf_ss_lin_step_ws_bytes if loss == "mse" else L_.wdf_ss_lin_step_esr_ws_bytes
                nbytes = ws_bytes(circ.ns, circ.ni, B, T, k)
                if nbytes == 0:
                    raise binding.WdfHipError(L_.wdf_last_error().decode() or "wdf_ss_lin_step_ws_bytes: unsupported tree")
                ws = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
            # results of a call: {SSE, gradients} and the loss, each call in a row of its OWN (rows are handed out from a
            # slab of _ROWS; a full slab is replaced by a fresh one and lives on for as long as anything still refers to
            # it): the loss history a script keeps (lpf.py:99 `losses.append(loss)`) and gradients read after the loop stay
            # what they were -- no copy per call, one allocation per _ROWS calls
            # (a row of the diode-root MSE + ESR step: {S, gradients}, then {mse, esr, mse + esr}; of the linear one: {0, gradients},
            #  {mse, esr, mse + esr}, then this call's sums {S, E, gP[n], gQ[n]}: the C ABI hands S back with the sums)
            width = 2 if loss == "mse" else (4 if circ.root_kind == "DiodePair" else 6 + 2 * self.pb.n)
            ent = self.cache.put((x, target), {"x": x_tm, "t": tgt, "y": None, "ws": ws,
                                       "ring": torch.zeros((_ROWS, width + self.pb.n), dtype=torch.float32, device=dev),
                                       "turn": 0, "B": B, "T": T, "k": k, "calls": 0, "watch": None, "replans": 0,
                                       "loss": loss, "skip": int(skip)},
                                 extra, nbytes=_nbytes(x_tm, tgt, tgt, ws))      # (y, where one is made, is the size of tgt)
        # this call's choice; a diode-pair root has no step without the y store and always stores
        ent["store_y"] = bool(store_output) or self.circ.root_kind == "DiodePair"
        if ent["store_y"]:
            self.output(ent)
        return ent

    def _resident_pair(self, x, target):
        """-> x time-major [T][ni][B] and target [T][B] on the block's device (made once per set), B, T"""
        dev = self.pb.block.device
        xd = x.as_subclass(torch.Tensor).to(dev).float()
        if xd.dim() == 2:
            xd = xd.unsqueeze(-1)
        B, T, ni = xd.shape
        if ni != self.circ.ni:
            raise binding.WdfHipError(f"x must be [B,T,{self.circ.ni}] (or [B,T] for one channel), got {tuple(x.shape)}")
        return xd.permute(1, 2, 0).contiguous(), target.as_subclass(torch.Tensor).to(dev).float().reshape(T, B).contiguous(), B, T

    @staticmethod
    def output(ent):
        """The entry's output buffer y [T,B], made on first use."""
        if ent["y"] is None:
            ent["y"] = torch.empty((ent["T"], ent["B"]), dtype=torch.float32, device=ent["t"].device)
        return ent["y"]

    def _plan_nl(self, B, T, k, dev, cold_floor=0):
        """Workspace of the diode-root step for k chunks, planned: cold first call, then the device steers the warm-up."""
        L_ = binding.lib()
        circ = self.circ
        nbytes = L_.wdf_ss_nl_step_ws_bytes(circ.ns, circ.ni, B, T, k)
        if nbytes == 0:
            raise binding.WdfHipError(L_.wdf_last_error().decode() or "wdf_ss_nl_step_ws_bytes: unsupported tree")
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        Lc = L_.wdf_ss_nl_step_chunk_len(T, k)
        cold = min(4096, max(self.cold_warmup(), int(cold_floor) // 16 * 16))
        warm = max(16, min(Lc // 16 * 16, 64))
        binding._check(L_.wdf_ss_nl_step_plan(binding._ptr(ws), circ.ns, circ.ni, B, T, k, cold, warm, _NL_WMIN,
                                              max(16, Lc // 16 * 16), float(NL_TOL), binding._stream()), "wdf_ss_nl_step_plan")
        return ws

    def _watch(self, ent, plan=None):
        """(plan: what makes a fresh workspace -- the step's _plan_nl, or the evaluation pass's _plan_nl_eval on its own entry.)
        Every 16th call, WITHOUT a synchronisation: look at the control block as it was 16 calls ago.  Groups that keep
        missing although the warm-up already is as long as a chunk (a circuit whose memory outlasts the chunks: every miss
        costs a sequential pass of its group) -> half as many chunks, twice the room; down to one chunk, which has no
        boundary to miss."""
        ent["calls"] += 1
        if ent["calls"] % 16:
            return
        w = ent["watch"]
        if w is None:
            w = ent["watch"] = {"buf": torch.zeros(32, dtype=torch.int32).pin_memory(), "event": None, "last": 0}
        if w["event"] is not None:
            if not w["event"].query():
                return
            raw = w["buf"].numpy()
            total, w_snap, w_max = int(raw[15]), int(raw[4]), int(raw[6])
            delta, w["last"] = total - w["last"], total
            w["event"] = None
            Lc = binding.lib().wdf_ss_nl_step_chunk_len(ent["T"], ent["k"])
            if delta >= 2 and w_snap >= min(w_max, Lc // 16 * 16) and ent["k"] > 1:
                ent["k"] = max(1, ent["k"] // 2)
                ent["ws"] = (plan or self._plan_nl)(ent["B"], ent["T"], ent["k"], ent["ws"].device, cold_floor=4 * w_snap)
                ent["watch"], ent["replans"] = None, ent["replans"] + 1
                return
        w["buf"].copy_(ent["ws"][:128].view(torch.int32), non_blocking=True)
        w["event"] = torch.cuda.Event()
        w["event"].record()

    # ---- grad=False on a diode-pair root: the loss-only evaluation pass (csrc/wdf_ss_nl_eval.h) on entries of its own
    @staticmethod
    def _nl_eval_k(T, k):
        """The chunk count the pass is called with: the chunks of wdf_ss_nl_step_chunk_len(T, k) that T really takes."""
        return -(-T // binding.lib().wdf_ss_nl_step_chunk_len(T, max(1, k)))

    def _plan_nl_eval(self, B, T, k, dev, cold_floor=0):
        """Workspace of the evaluation pass for k chunks, planned as _plan_nl plans the step's."""
        Lc = binding.lib().wdf_ss_nl_step_chunk_len(T, k)
        cold = min(4096, max(self.cold_warmup(), int(cold_floor) // 16 * 16))
        warm = max(16, min(Lc // 16 * 16, 64))
        return binding.ss_nl_eval_plan(self.circ.ns, self.circ.ni, B, T, self._nl_eval_k(T, k), cold, warm, max(16, _NL_WMIN // 16 * 16),
                                       max(16, Lc // 16 * 16), float(NL_TOL), torch.empty(0, device=dev))

    def eval_entry(self, x, target):
        """The buffers of one evaluated set: an entry of its own per (x, target) pair -- its own workspace (snapshot ring, warm-up
        control, chunk count) and result rows; the training entry of the same pair is never touched.  One entry serves both
        losses and every skip (the pass's sums are the same two); it holds no y until a call wants one."""
        ent = self.cache.get((x, target), ("eval",))
        if ent is None:
            circ, dev = self.circ, self.pb.block.device
            nl = circ.root_kind == "DiodePair"
            x_tm, tgt, B, T = self._resident_pair(x, target)
            groups = -(-B // (128 if B % 2 == 0 else 64))         # (two sequences per lane when the rows pair up, on every tree)
            k = max(1, min(T // 64, ((_NL_EVAL_OCC if nl else _LIN_EVAL_OCC) * N_SIMD) // groups))     # the training entry's chunk formula
            if nl:
                ws, own = self._plan_nl_eval(B, T, k, dev), {"calls": 0, "watch": None, "replans": 0}
            else:
                # a linear tree (csrc/wdf_ss_lin_eval.h): a zeroed workspace of the pass's own size (the ticket, the chunks'
                # zero-state ends, two partial sums per wave); its result rows are {mse, esr, mse + esr, mse by gscale}
                nbytes = binding.lib().wdf_ss_lin_eval_ws_bytes(circ.ns, circ.ni, B, T, k)
                if nbytes == 0:
                    raise binding.WdfHipError(binding.lib().wdf_last_error().decode() or "wdf_ss_lin_eval_ws_bytes: unsupported tree")
                ws, own = torch.zeros((nbytes,), dtype=torch.uint8, device=dev), {"zT": None}
            # a call's {mse, esr, mse + esr} in a row of its OWN, from a slab (entry()): a val_loss history stays what it was
            ent = self.cache.put((x, target), {"x": x_tm, "t": tgt, "y": None, "ws": ws,
                                               "ring": torch.zeros((_ROWS, 4), dtype=torch.float32, device=dev),
                                               "sums": torch.zeros(2, dtype=torch.float64, device=dev),
                                               "turn": 0, "B": B, "T": T, "k": k, **own},
                                 ("eval",), nbytes=_nbytes(x_tm, tgt, tgt, ws))
        return ent

    def evaluate(self, ent, kind, skip, store_output, z0=None, want_zT=False):
        """probe + one evaluation pass -> the loss `kind` asks for ("mse": the mean squared error, else mse + esr) past skip, a view
        into this call's own result row; the three terms {mse, esr, mse + esr} stay in ent["loss3"].  The
        probe applies the optimizer updates queued since the last step (a validation call reads the parameters AFTER them);
        the next training step's probe then finds none.  A linear tree (wdf_ss_lin_eval): kind "mse" is skip 0 with the MSE
        step's gscale = 2 / (B T) and its loss_out formula, else n = B (T - skip) and loss3[2] -- the numbers the training steps
        report; z0 [ns,B] / want_zT as in step(), the final states in ent["zT"] (one of two buffers of the eval entry's own)."""
        circ = self.circ
        self.check()
        self.probe()
        B, T = ent["B"], ent["T"]
        if ent["turn"] >= ent["ring"].shape[0]:
            ent["ring"], ent["turn"] = torch.zeros_like(ent["ring"]), 0
        if circ.root_kind != "DiodePair":
            row = ent["ring"][ent["turn"]]
            ent["turn"] += 1
            zT = None
            if want_zT and circ.ns > 0:
                bufs = ent.setdefault("zT_bufs", [torch.empty((circ.ns, B), dtype=torch.float32, device=ent["t"].device) for _ in range(2)])
                zT = bufs[0] if (z0 is None or z0.data_ptr() != bufs[0].data_ptr()) else bufs[1]
            ent["zT"] = zT
            y = self.output(ent) if store_output else None
            mse = kind == "mse"
            skip = 0 if mse else int(skip)
            at = row.data_ptr()
            rc = binding.lib().wdf_ss_lin_eval(binding._ptr(ent["x"]), binding._ptr(self.coef), circ.ns, circ.ni, binding._ptr(ent["t"]),
                                               skip, float(B * (T - skip)), ESR_EPS, 2.0 / float(B * T), binding._ptr(y),
                                               binding._ptr(ent["ws"]), binding._ptr(ent["sums"]), ctypes.c_void_p(at),
                                               ctypes.c_void_p(at + 12), B, T, ent["k"], None if z0 is None else binding._ptr(z0),
                                               None if zT is None else binding._ptr(zT), binding._stream())
            binding._check(rc, "wdf_ss_lin_eval")
            ent["loss3"] = row[:3]
            return row[3 if mse else 2]
        loss3 = ent["ring"][ent["turn"]][:3]
        ent["turn"] += 1
        y = self.output(ent) if store_output else None
        rc = binding.lib().wdf_ss_nl_eval(binding._ptr(ent["x"]), binding._ptr(self.coef), binding._ptr(self.pb.block), self.n_tree,
                                          circ.ns, circ.ni, int(circ.root.N_up), int(circ.root.N_down), binding._ptr(ent["t"]), int(skip),
                                          float(B * (T - int(skip))), ESR_EPS, binding._ptr(y), binding._ptr(ent["ws"]),
                                          binding._ptr(ent["sums"]), binding._ptr(loss3), B, T, self._nl_eval_k(T, ent["k"]),
                                          binding._stream())
        binding._check(rc, "wdf_ss_nl_eval")
        self._watch(ent, self._plan_nl_eval)
        ent["loss3"] = loss3
        return loss3[0 if kind == "mse" else 2]

    def read_eval_ctl(self, ent):
        """The evaluation entry's control block (the step's 32 words) as a dict -- synchronises."""
        return binding.ss_nl_eval_read(ent["ws"])

    def cold_warmup(self):
        """Warm-up of a chunk that starts from z = 0 (the first call on a batch): outlasts the slowest mode of the step's
        Jacobian A + Da E ca^T over the diode's slope Da in [-1, 1] (plan_ss_time_parallel's estimate), from the host mirror."""
        c, _ = self.host_coef()
        ns, ni = self.circ.ns, self.circ.ni
        A = np.asarray(c[:ns * ns]).reshape(ns, ns)
        oE = ns * ns + ns * ni
        E, ca = np.asarray(c[oE:oE + ns]), np.asarray(c[oE + ns:oE + 2 * ns])
        rho = max(float(np.max(np.abs(np.linalg.eigvals(A + sgn * np.outer(E, ca))))) for sgn in (1.0, -1.0))
        if rho <= 0.0:
            return 16
        if rho >= 1.0 - 1e-9:
            return 4096
        return int(min(4096, max(16, -(-int(math.ceil(math.log(0.01 * NL_TOL) / math.log(rho))) // 16) * 16)))

    def read_ctl(self, ent):
        """The step's control block (csrc/wdf_ss_nl_step.h, NlStepCtl) as a dict -- synchronises."""
        raw = np.zeros(32, dtype=np.int32)
        binding._check(binding.lib().wdf_ss_nl_step_read(binding._ptr(ent["ws"]), raw.ctypes.data, binding._stream()), "wdf_ss_nl_step_read")
        f = raw.view(np.float32)
        return {"call": int(raw[0]), "parity": int(raw[1]), "have_snap": int(raw[2]), "w_cur": int(raw[3]), "w_snap": int(raw[4]),
                "w_min": int(raw[5]), "w_max": int(raw[6]), "cool": int(raw[7]), "tol": float(f[8]), "n_bad": int(raw[12]),
                "max_miss": float(f[13]), "gated_groups": int(raw[14]), "total_gated": int(raw[15]), "w_used": int(raw[19])}

    def step(self, ent, z0=None, want_zT=False):
        """probe + one-pass step -> (out = {SSE, d(mean squared error)/d component value}, loss = the mean squared error): views
        of this call's own result row (never written again).  z0 [ns,B] float32 on the device: the capacitor states the call
        starts from (linear trees; None: zero); want_zT: the states it ends in are left in ent["zT"] (a buffer of its own per
        call parity, never the one z0 may be).  The MSE + ESR step of a LINEAR tree: out = {0, d(mse + esr)/d component value},
        loss = mse + esr; the call's row stays in ent["row"] = {0, g[n], mse, esr, mse + esr, S, E, gP[n], gQ[n]} (S is row[4 + n])."""
        circ = self.circ
        self.probe()
        B, T, n = ent["B"], ent["T"], self.pb.n
        if ent["turn"] >= ent["ring"].shape[0]:
            ent["ring"], ent["turn"] = torch.zeros_like(ent["ring"]), 0
        row = ent["ring"][ent["turn"]]
        ent["turn"] += 1
        out, loss = row[:1 + n], row[1 + n]
        if circ.root_kind == "DiodePair" and ent.get("loss", "mse") != "mse":
            # MSE + ESR past skip (wdf_ss_nl_step_esr): out = {S, d(mse + esr)/d component value}, loss = mse + esr; the three
            # terms stay in ent["loss3"] (a view of this call's row)
            loss3 = row[1 + n:4 + n]
            rc = binding.lib().wdf_ss_nl_step_esr(binding._ptr(ent["x"]), binding._ptr(self.coef), binding._ptr(self.pb.block),
                                                  binding._ptr(self.jac), self.n_tree, circ.ns, circ.ni, int(circ.root.N_up),
                                                  int(circ.root.N_down), binding._ptr(ent["t"]), int(ent["skip"]), ESR_EPS,
                                                  binding._ptr(ent["y"]), binding._ptr(ent["ws"]), binding._ptr(out),
                                                  binding._ptr(loss3), B, T, ent["k"], binding._stream())
            binding._check(rc, "wdf_ss_nl_step_esr")
            self._watch(ent)
            ent["loss3"] = loss3
            return out, loss3[2]
        if circ.root_kind == "DiodePair":
            rc = binding.lib().wdf_ss_nl_step_mse(binding._ptr(ent["x"]), binding._ptr(self.coef), binding._ptr(self.pb.block),
                                                  binding._ptr(self.jac), self.n_tree, circ.ns, circ.ni, int(circ.root.N_up),
                                                  int(circ.root.N_down), binding._ptr(ent["t"]), 2.0 / float(B * T),
                                                  binding._ptr(ent["y"]), binding._ptr(ent["ws"]), binding._ptr(out),
                                                  binding._ptr(loss), B, T, ent["k"], binding._stream())
            binding._check(rc, "wdf_ss_nl_step_mse")
            self._watch(ent)
            return out, loss
        zT = None
        if want_zT and circ.ns > 0:
            bufs = ent.setdefault("zT_bufs", [torch.empty((circ.ns, B), dtype=torch.float32, device=ent["t"].device) for _ in range(2)])
            zT = bufs[0] if (z0 is None or z0.data_ptr() != bufs[0].data_ptr()) else bufs[1]
        ent["zT"] = zT
        store_y = ent["store_y"]                                  # (False: the _noy twins -- no y argument, nothing stored)
        ynoy = (binding._ptr(ent["y"]),) if store_y else ()
        if ent.get("loss", "mse") != "mse":
            # MSE + ESR past skip on a linear tree (wdf_ss_lin_step_esr): the gradients land in out[1:] and {mse, esr, mse + esr} in
            # the row behind them, then this call's sums {S, E, gP, gQ} (what a data-parallel loop would all-reduce): the C ABI
            # hands S back with the sums, not in front of g, so out[0] stays 0 and S is row[4 + n] -- per call like the rest of the
            # row, never written again.  (Addresses inside the row by arithmetic: every view is microseconds of host time.)
            at = row.data_ptr()
            step = binding.lib().wdf_ss_lin_step_esr if store_y else binding.lib().wdf_ss_lin_step_esr_noy
            rc = step(binding._ptr(ent["x"]), binding._ptr(self.coef), binding._ptr(self.jac), n, circ.ns, circ.ni, binding._ptr(ent["t"]),
                      float(B * (T - ent["skip"])), ESR_EPS, int(ent["skip"]), *ynoy, binding._ptr(ent["ws"]),
                      ctypes.c_void_p(at + 4 * (4 + n)), ctypes.c_void_p(at + 4), ctypes.c_void_p(at + 4 * (1 + n)), None, B, T, ent["k"],
                      None if z0 is None else binding._ptr(z0), None if zT is None else binding._ptr(zT), binding._stream())
            binding._check(rc, "wdf_ss_lin_step_esr" if store_y else "wdf_ss_lin_step_esr_noy")
            ent["row"] = row                                      # ({0, g[n], mse, esr, mse + esr, S, E, gP[n], gQ[n]} of this call)
            return out, row[3 + n]
        step = binding.lib().wdf_ss_lin_step_mse if store_y else binding.lib().wdf_ss_lin_step_mse_noy
        rc = step(binding._ptr(ent["x"]), binding._ptr(self.coef), binding._ptr(self.jac), self.pb.n, circ.ns, circ.ni, binding._ptr(ent["t"]),
                  2.0 / float(B * T), *ynoy, binding._ptr(ent["ws"]), binding._ptr(out), binding._ptr(loss), None, B, T, ent["k"],
                  None if z0 is None else binding._ptr(z0), None if zT is None else binding._ptr(zT), binding._stream())
        binding._check(rc, "wdf_ss_lin_step_mse" if store_y else "wdf_ss_lin_step_mse_noy")
        return out, loss

    # ---- the Gauss-Newton form of the linear step (csrc/wdf_ss_lin_gn.h) on entries of its own
    def gn_entry(self, x, target):
        """The buffers of one set the Gauss-Newton step runs on: an entry of its own per (x, target) pair -- its own workspace (the
        MSE step's layout with larger partial rows) and output buffer; the MSE entry of the same pair is never touched."""
        ent = self.cache.get((x, target), ("gn",))
        if ent is None:
            circ, dev = self.circ, self.pb.block.device
            x_tm, tgt, B, T = self._resident_pair(x, target)
            # (two sequences per lane when the rows pair up, except on two capacitors with two sources: one per lane there)
            per_wave = 128 if (B % 2 == 0 and circ.ns * circ.ni != 4) else 64
            k = max(1, min(T // 64, (_LIN_OCC * N_SIMD) // max(1, -(-B // per_wave))))     # the training entry's chunk formula
            nbytes = binding.lib().wdf_ss_lin_step_gn_ws_bytes(circ.ns, circ.ni, B, T, k)
            if nbytes == 0:
                raise binding.WdfHipError(binding.lib().wdf_last_error().decode() or "wdf_ss_lin_step_gn_ws_bytes: unsupported tree")
            ws = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
            y = torch.empty((T, B), dtype=torch.float32, device=dev)
            ent = self.cache.put((x, target), {"x": x_tm, "t": tgt, "y": y, "ws": ws, "B": B, "T": T, "k": k}, ("gn",),
                                 nbytes=_nbytes(x_tm, tgt, y, ws))
        return ent

    def gn_step(self, ent, z0=None):
        """probe + the Gauss-Newton step -> out float64 [1 + n + n (n + 1) / 2] = {SSE, d(mean squared error)/d component value,
        (2/N) J^T J's upper triangle by rows} over all n values of the block: a tensor of this call's own.  z0 [ns,B] float32 on
        the device or None: a constant of the call.  The optimizer updates queued since the last step go out with the probe."""
        circ = self.circ
        self.probe()
        B, T, n = ent["B"], ent["T"], self.pb.n
        out = torch.empty((1 + n + n * (n + 1) // 2,), dtype=torch.float64, device=ent["t"].device)
        rc = binding.lib().wdf_ss_lin_step_gn(binding._ptr(ent["x"]), binding._ptr(self.coef), binding._ptr(self.jac), n, circ.ns, circ.ni,
                                              binding._ptr(ent["t"]), 2.0 / float(B * T), binding._ptr(ent["y"]), binding._ptr(ent["ws"]),
                                              binding._ptr(out), None, None, B, T, ent["k"],
                                              None if z0 is None else binding._ptr(z0), None, binding._stream())
        binding._check(rc, "wdf_ss_lin_step_gn")
        return out


class _DynResident:
    """Circuit.to_device() of a circuit that runs on the streamed-coefficient kernels (per-sample impedance / an MLP root outside
    the clipper topology, csrc/wdf_ss_dyn.h): the scalar component Variables (and a diode root's Is, nVt) become 0-dim views of one
    device block (compat_tf.ParamBlock: same objects, same constraints, same autograd leaves; tf.keras.optimizers.Adam updates
    them on the device), a DenseRootModel's kernels and biases views of one flat device vector.  _run_dyn is unchanged -- it
    only ever handed these values to device code; what goes is the host round trip per Variable and step."""

    def __init__(self, circ, device):
        own = {"Resistor": "R", "ResistiveVoltageSource": "R", "Capacitor": "C"}
        params = [(e, own[_kind(e)]) for e in circ.elements if _kind(e) in own]
        if circ.root_kind == "DiodePair":
            params += [(circ.root, "Is"), (circ.root, "nVt")]
        pvars = [e.__dict__[n] for e, n in params]
        for (e, n), v in zip(params, pvars):
            if isinstance(v, torch.Tensor) and not getattr(v, "_is_tf_variable", False) and (v.requires_grad or v.grad_fn is not None):
                raise binding.WdfHipError(f"Circuit.to_device: {type(e).__name__}.{n} is a tensor computed from other Variables -- "
                                          "keep this circuit on the host path")
            if isinstance(v, torch.Tensor) and getattr(v, "_wdf_block", None) is not None:
                raise binding.WdfHipError("Circuit.to_device: a component Variable already lives in another circuit's block")
        self.pb = tf.ParamBlock([float(v) for v in pvars], torch.device(device))
        for i, v in enumerate(pvars):
            if isinstance(v, torch.Tensor) and getattr(v, "_is_tf_variable", False) and v.numel() == 1:
                self.pb.adopt(i, v)
        self.w = None
        if circ.root_kind == "DenseRootModel":
            from . import mlp_root
            dense, _, _ = mlp_root.describe(circ.root)
            self.w = mlp_root.flat_weights(dense).detach().float().to(device).contiguous()
            o = 0
            for d in dense:
                for v in (d.kernel, d.bias):
                    n = v.numel()
                    if getattr(v, "_wdf_flat", None) is not None:
                        raise binding.WdfHipError("Circuit.to_device: this network's weights already live in another circuit's vector")
                    with torch.no_grad():
                        v.data = self.w[o:o + n].view(v.shape)
                    v._wdf_flat = (self, o, n)
                    o += n


class _ProbeFn(torch.autograd.Function):
    """(coef float32 [ncoef], rootp float32 [3] | None) of a resident tree from its parameter block, on the device
    (wdf_ss_probe); backward contracts dLoss/d coef with the probe's Jacobian -- calc_impedance's chain rule
    (tf_wdf.py:114-115,139-145,168-177) without the host."""
    _wdf_sends_pending = True        # (res.probe() carries the queued optimizer updates: compat_tf.Tensor.__torch_function__)

    @staticmethod
    def forward(ctx, res, idx, *live):
        res.probe()
        ncoef = res.n_out - 1
        coef = res.coef[:ncoef].clone()
        ctx.res, ctx.idx, ctx.ncoef = res, idx, ncoef
        ctx.save_for_backward(res.jac.clone())
        if res.circ.root_kind == "DiodePair":
            rootp = torch.cat([res.pb.block[res.n_tree:res.n_tree + 2], res.coef[ncoef:ncoef + 1]])
            return coef, rootp
        return coef, coef.new_zeros(3)

    @staticmethod
    def backward(ctx, gcoef, grootp):
        (jac,) = ctx.saved_tensors
        res = ctx.res
        g = torch.cat([gcoef, grootp[2:3]]).double() @ jac                    # [n_tree]
        if res.circ.root_kind == "DiodePair":
            g = torch.cat([g, grootp[0:2].double()])
        g = g.float()
        return (None, None) + tuple(g[i] for i in ctx.idx)


class _LinResidentMseFn(torch.autograd.Function):
    """loss = mean((y - target)^2) of a resident linear tree: the one-pass step produced d loss / d Variable with it."""
    _wdf_sends_pending = True        # (res.step() begins with res.probe(), which carries the queued optimizer updates)

    @staticmethod
    def forward(ctx, res, ent, inv_n, idx, z0, want_zT, *live):
        out, loss = res.step(ent, z0, want_zT)                   # (this call's own result row: nothing to copy)
        ctx.save_for_backward(out)
        ctx.idx = idx
        ctx.mark_non_differentiable(out)
        return loss, out

    @staticmethod
    def backward(ctx, gl, _):
        (out,) = ctx.saved_tensors
        g = gl * out
        return (None,) * 6 + tuple(g[1 + i] for i in ctx.idx)


# ------------------------------------------------------------------------------ tree walking
def _kind(e):
    return type(e).__name__


def _walk(top):
    """Post-order list of the elements under `top` (P1 before P2, children before parents)."""
    order, seen = [], set()

    def visit(e):
        if id(e) in seen:
            raise ValueError("a WDF element appears twice in the tree")
        seen.add(id(e))
        for child in (getattr(e, "P1", None), getattr(e, "P2", None)):
            if child is not None:
                visit(child)
        order.append(e)

    visit(top)
    return order


_STATE_ATTRS = ("a", "b", "z", "Vs", "R", "p1R", "p2R", "b_diff", "b_temp")


class _Saved:
    """Saves / restores the wave attributes the probe overwrites."""

    def __init__(self, elements):
        self.snap = [(e, {k: e.__dict__[k] for k in _STATE_ATTRS if k in e.__dict__}) for e in elements]

    def restore(self):
        for e, d in self.snap:
            for k in _STATE_ATTRS:
                if k in d:
                    e.__dict__[k] = d[k]
                elif k in e.__dict__ and k not in ("R",):
                    del e.__dict__[k]


def diode_pair_reflected(dp):
    """DiodePair.reflected(): recorded by the loop recorder, or -- on concrete GPU tensors --
    evaluated element-wise by the HIP kernel (no autograd; the differentiable path is Circuit)."""
    a = dp.a
    if hasattr(a, "__wdf_root__"):
        return a.__wdf_root__(dp)
    if isinstance(a, torch.Tensor) and a.is_cuda:
        R = tf.convert(dp.R, dtype=torch.float32, device=a.device).expand_as(a).contiguous()
        return binding.diode_pair(a.contiguous().float(), R, float(dp.Is), float(dp.nVt), dp.N_up, dp.N_down)
    raise binding.WdfHipError(
        "DiodePair.reflected() needs the GPU: pass CUDA tensors, or run the loop through "
        "tf_wdf.Circuit / a recorded TensorArray loop (there is no CPU fallback)")


# ------------------------------------------------------------------------------ Circuit
class Circuit:
    """The fast tier.  top: element connected to the root (e.g. the Inverter of lpf.py:28 or
    P1 of clipper_pot.py:99); root: IdealVoltageSource, DiodePair, AsymDiodePair or layers.DenseRootModel;
    probe: element whose voltage() is the output (C1 in lpf.py:44, C in clipper_pot.py:123).

    An AsymDiodePair root (two different diodes, the exact Shockley pair) runs on the diode-clipper tree probed at the
    capacitor, on kernels of its own (csrc/wdf_asym.h).  Built with any_tree=True it also terminates any tree of at most three
    capacitors and two sources, any probe, and the clipper tree under force_generic: the state-space kernels of
    csrc/wdf_statespace.h (sequential and time-parallel forward, both reverse sweeps) solve the pair by Newton in fp32 at
    every step, gradients flow to the four diode Variables and, through the port resistance and the step's matrices, to the
    components; mse / mse_esr compose the loss from the forward there, and trees of one or two capacitors have a one-pass step
    (csrc/wdf_ss_asym_step.h: _asym_tree_step; ASYM_TREE_STEP_SERVES says for which loss mse / mse_esr take it).  Off the clipper's own kernels the root takes
    solver="newton_f32" only, no per_sample_R / per_sequence_R and no to_device().  Built with streamed=True the root runs on
    the streamed-coefficient kernels instead (csrc/wdf_ss_dyn.h) on any tree of at most four capacitors and two sources:
    per_sample_R on any Resistor / ResistiveVoltageSource (a channel constant along every sequence is lowered to one row per
    sequence by itself; per_sequence_R is refused), one static row without a pot; newton_f32 only, losses composed from the
    forward, no to_device().

    Input channels: channel k of x feeds the k-th voltage source found walking the tree in
    post-order (ResistiveVoltageSource leaves), then the ideal-source root if there is one.
    per_sample_R: a ResistiveVoltageSource whose resistance is streamed from the NEXT input
    channel (clipper_pot.py:114-116: channel 0 = Vin, channel 1 = R); diode-clipper
    topology only.
    per_sequence_R: the same channel layout under an AsymDiodePair root with a Newton solver, for a pot that is constant
    along every sequence (clipper_pot.py's recordings: dataimport.py:96): top.P1, the clipper's ResistiveVoltageSource.  The
    two-different-diode kernels evaluate the port once per sequence (csrc/wdf_asym.h asym_load_seq); a channel that moves
    inside a sequence raises.  The source's own R receives no gradient: the pot is data.
    """

    def __init__(self, top, root, probe, per_sample_R=None, force_generic=False, time_parallel="auto", warm_start=True,
                 per_sequence_R=None):
        self.top, self.root, self.probe = top, root, probe
        self.time_parallel = time_parallel          # "auto" | None | engine.TpPlan
        self.warm_start = bool(warm_start)          # generic trees with a diode root: SsWarmStart when a batch is re-visited
        self.force_generic = bool(force_generic)    # tests: run the clipper tree through the generic kernel
        self.elements = _walk(top)
        if probe not in self.elements:
            raise ValueError("probe must be an element of the tree under `top`")
        self.caps = [e for e in self.elements if _kind(e) == "Capacitor"]
        self.sources = [e for e in self.elements if _kind(e) == "ResistiveVoltageSource"]
        self.root_kind = _kind(root)
        if self.root_kind not in ("IdealVoltageSource", "DiodePair", "AsymDiodePair", "DenseRootModel"):
            raise ValueError(f"unsupported root {self.root_kind}")
        self.ns = len(self.caps)
        self.ni = len(self.sources) + (1 if self.root_kind == "IdealVoltageSource" else 0)
        self.per_sample_R = per_sample_R
        if per_sample_R is not None and (per_sample_R not in self.elements or _kind(per_sample_R) not in ("ResistiveVoltageSource", "Resistor")):
            raise ValueError("per_sample_R must be a ResistiveVoltageSource or a Resistor of the tree (set_resistance: "
                             "tf_wdf.py:51-52,80-81)")
        if self.ni < 1:
            raise ValueError("the circuit has no voltage source")
        asym = self.root_kind == "AsymDiodePair"
        # AsymDiodePair(streamed=True): the streamed-coefficient kernels (csrc/wdf_ss_dyn.h, root kind ROOT_ASYM_PAIR) on any
        # tree, the clipper's included -- a pot that moves (per_sample_R on any Resistor / ResistiveVoltageSource), a fourth capacitor
        streamed = asym and bool(getattr(root, "streamed", False))
        own = self._is_clipper() and not self.force_generic and not streamed   # the two-different-diode clipper's own kernels (csrc/wdf_asym.h)
        if streamed:
            if root.mode != binding.ASYM_NEWTON_F32:
                raise binding.WdfHipError("AsymDiodePair(streamed=True) takes solver='newton_f32' only "
                                          f"(got {root.solver!r}): the streamed-coefficient kernels solve the pair in fp32")
            if per_sequence_R is not None:
                raise binding.WdfHipError("per_sequence_R is not taken under AsymDiodePair(streamed=True): pass the pot as "
                                          "per_sample_R -- a channel that is constant along every sequence is noticed and "
                                          "lowered to one coefficient row per sequence by itself")
            if self.ns > 4 or self.ni > 2:
                raise binding.WdfHipError("AsymDiodePair(streamed=True) runs on trees of at most four capacitors and two sources "
                                          f"(this one has {self.ns} and {self.ni}): the eight-slot streamed kernels' reverse "
                                          "sweep needs scratch under this root and is not built")
        if asym and not streamed and not getattr(root, "any_tree", False) and not (own and per_sample_R is None):
            raise binding.WdfHipError("an AsymDiodePair root runs on the diode-clipper tree only: top = Parallel(ResistiveVoltageSource, "
                                      "Capacitor), probe = the capacitor, no per_sample_R (a pot that is constant along every "
                                      "sequence goes in as per_sequence_R), not force_generic (csrc/wdf_asym.h); "
                                      "AsymDiodePair(..., any_tree=True) takes the generic state-space kernels on any small tree")
        # AsymDiodePair(any_tree=True) off the clipper's own kernels: the generic state-space kernels, root kind ROOT_ASYM_PAIR
        self._asym_generic = asym and not own
        self._asym_streamed = streamed
        if asym and per_sample_R is not None and not streamed:
            raise binding.WdfHipError("per_sample_R is not supported under an AsymDiodePair root: the root's kernels take static "
                                      "coefficients (a pot that is constant along every sequence goes in as per_sequence_R on "
                                      "the diode-clipper tree)")
        if self._asym_generic and not streamed:
            if root.mode != binding.ASYM_NEWTON_F32:
                raise binding.WdfHipError("an AsymDiodePair root on the generic state-space kernels takes solver='newton_f32' only "
                                          f"(got {root.solver!r}): the fp64 Newton mode and the omega closed form run on the "
                                          "diode-clipper tree's own kernels")
            if per_sequence_R is not None:
                raise binding.WdfHipError("per_sequence_R under an AsymDiodePair root belongs to the diode-clipper tree's own "
                                          "kernels (probe = the capacitor, not force_generic): the generic state-space kernels "
                                          "take static coefficients")
            if self.ns > 3 or self.ni > 2:
                raise binding.WdfHipError("an AsymDiodePair root runs on trees of at most three capacitors and two sources "
                                          f"(this one has {self.ns} and {self.ni}): with four states the chunked reverse sweep's "
                                          "sums for this root do not fit a wave's registers, so csrc/wdf_statespace.h is not "
                                          "built for it there")
        self.per_sequence_R = per_sequence_R
        if per_sequence_R is not None:
            if self.root_kind != "AsymDiodePair":
                raise binding.WdfHipError("per_sequence_R belongs to an AsymDiodePair root (one resistance per sequence: "
                                          "csrc/wdf_asym.h); every other root streams the pot per sample: per_sample_R")
            if per_sequence_R is not self.top.P1:
                raise binding.WdfHipError("per_sequence_R must be top.P1, the ResistiveVoltageSource of the clipper tree: the "
                                          f"kernels have one pot, the source's (got a {_kind(per_sequence_R)})")
            if self.root.mode == binding.ASYM_OMEGA_F32:
                raise binding.WdfHipError("per_sequence_R needs a Newton solver: the closed form (omega_f32, a model approximation "
                                          "kept for comparison) has no per-sequence pot")
        # Outside the clipper topology a per-sample impedance or a DenseRootModel root runs on the streamed-coefficient kernels
        # (csrc/wdf_ss_dyn.h) -- and so does, since round 6, ANY tree of five to eight capacitors (the static-coefficient kernels
        # of csrc/wdf_statespace.h are compiled for at most four: a larger tree hands the streamed kernels one static row)
        self._dyn = ((per_sample_R is not None or self.root_kind == "DenseRootModel") and (self.force_generic or not self._is_clipper())) \
            or self.ns > 4 or streamed                            # (a streamed two-diode root without a pot: one static row)
        if self._dyn and (self.ns > 8 or self.ni > 2):
            raise binding.WdfHipError("trees of at most eight capacitors and two sources run on the GPU kernels "
                                      f"(this one has {self.ns} and {self.ni})")

    # -- device-resident component values
    def to_device(self, device="cuda"):
        """Move the circuit's component Variables {Is, nVt, R, C} into one device-resident parameter block
        (compat_tf.ParamBlock): from here on mse() reads the values where they live, tape.gradient returns device
        scalars and tf.keras.optimizers.Adam.apply_gradients is one kernel launch -- the training loops of
        lpf.py:86-99 / clipper_pot.py:245-269 run without a host round trip per step (print / .numpy() / float() on a
        Variable still work: they copy back on demand).  Diode-clipper topology only: the generic lowering differentiates
        its float64 probe on the host and needs the Variables there.  Returns self."""
        if self.root_kind == "AsymDiodePair":
            raise binding.WdfHipError("Circuit.to_device: there is no resident training step for an AsymDiodePair root; the circuit "
                                      "trains on the host path (its forward and reverse sweep are single launches either way; "
                                      "on a generic tree the step's matrices are probed on the host)")
        binding.require_gpu()
        if any(getattr(self, a, None) is not None for a in ("_lin", "_pblock", "_tree", "_mlp", "_dynres")):
            return self
        if self._dyn:
            # (round 6) the streamed-coefficient path has no one-pass step, but nothing in it needs the component values on the
            # host either: they move into a device block (the tape interpreter, the kernels and the optimizers read them there),
            # a network root's weights into one flat device vector -- a training loop then makes no host round trip per step
            self._dynres = _DynResident(self, device)
            return self
        if self.root_kind == "DenseRootModel":
            if not self._is_clipper():
                raise binding.WdfHipError("the MLP root is supported on the diode-clipper topology (clipper_pot.py:94-101)")
            from . import mlp_root
            self._mlp = mlp_root.MlpResident(self, device)       # clipper_pot.py's model: weights in one device vector
            return self
        if self.root_kind == "IdealVoltageSource" and self.ns <= 2 and self.ni <= 2 and self.per_sample_R is None:
            # a linear tree (lpf.py, voltage_divider.py): the probed step becomes a device tape, mse() the one-pass step
            self._lin = _LinResident(self, device)
            return self
        if self.root_kind in ("IdealVoltageSource", "DiodePair") and self.per_sample_R is None and \
                not (self._is_clipper() and self.root_kind == "DiodePair"):
            # any other tree the state-space kernels run (HPFDiodeClipper.h:28-32 ...): the probe moves to the device, the
            # forward / reverse-sweep kernels stay -- __call__ no longer touches the host per step
            self._tree = _LinResident(self, device)
            return self
        if not (self._is_clipper() and self.root_kind == "DiodePair"):
            raise binding.WdfHipError("Circuit.to_device: the diode-pair clipper and linear trees (ideal-source root, at most two "
                                      "capacitors and two sources) keep their component values on the device")
        dp, vs, cap = self.root, self.top.P1, self.top.P2
        Rv = 1.0 if self.per_sample_R is not None else vs.R
        parts = [dp.Is, dp.nVt, Rv, cap.C]
        for p in parts:
            if isinstance(p, torch.Tensor) and not getattr(p, "_is_tf_variable", False) and (p.requires_grad or p.grad_fn is not None):
                raise binding.WdfHipError("Circuit.to_device: a component value is a tensor computed from other Variables; the "
                                          "resident step would freeze it -- keep this circuit on the host path")
            if isinstance(p, torch.Tensor) and getattr(p, "_wdf_block", None) is not None:
                raise binding.WdfHipError("Circuit.to_device: a component Variable already lives in another circuit's block")
        pb = tf.ParamBlock([float(p) for p in parts], torch.device(device))
        self._adopted_parts = {}
        for i, p in enumerate(parts):
            if isinstance(p, torch.Tensor) and getattr(p, "_is_tf_variable", False) and p.numel() == 1:
                pb.adopt(i, p)
                self._adopted_parts[i] = p
        self._pblock, self._res_cache = pb, EntryCache()
        return self

    def _theta(self, parts, dev):
        """{Is, nVt, R, C} as one float32[4] on the device, differentiable w.r.t. the Variables among them."""
        pb = getattr(self, "_pblock", None)
        if pb is not None:      # resident: the adopted Variables already live on the device, the rest are the block's constants
            pb.flush()
            return torch.stack([(pb.members[i] if i in pb.members else pb.block[i]).as_subclass(torch.Tensor).reshape(())
                                for i in range(4)]).to(dev)
        return torch.stack([p.as_subclass(torch.Tensor).float().reshape(()) for p in parts]).to(dev)

    def _host_RC(self, parts):
        """R and C as host numbers for the planner: the Variables themselves when they live on the host, the block's
        lagging mirror when resident (no synchronisation either way)."""
        pb = getattr(self, "_pblock", None)
        if pb is not None:
            h = pb.host_values()
            return h[2], h[3]
        return float(parts[2]), float(parts[3])

    def _z0_device(self, z0, dev, B):
        """z0 as the one-pass steps and passes take it: detached float32 [ns, B] on dev, or None."""
        if z0 is None:
            return None
        return torch.as_tensor(z0).as_subclass(torch.Tensor).detach().to(dev).float().reshape(self.ns, B).contiguous()

    def _resident_stepper(self, x, target, kind, skip, store_output):
        """What a new entry of the resident clipper holds, for training (_loss_resident) and for evaluation (_eval_resident)
        alike: x time-major, the pot channel r (or None) and the target on the block's device, and an engine.MseStep on the
        plan of engine.tuned_plan (fused: two sequences per lane).  Runs on a cache miss only."""
        from . import engine
        pb, dp, cap = self._pblock, self.root, self.top.P2
        xd = x.as_subclass(torch.Tensor).to(pb.block.device).float()
        xv, r = engine.split_channels(xd, self.per_sample_R is not None, time_major=True, anchor=x)
        tgt = target.as_subclass(torch.Tensor).to(pb.block.device).float().reshape(xv.shape).contiguous()
        host = pb.host_values()
        R_plan = host[2] if r is None else engine.resistance_max(r)
        tp = self.time_parallel
        if tp == "auto":
            tp = engine.tuned_plan(pb.block, xv, r, float(cap.FS), R_plan, host[3], n_up=dp.N_up, n_down=dp.N_down,
                                   time_major=True, R_min=None if r is None else engine.resistance_min(r), fused=True)
        T, B = xv.shape
        st = engine.MseStep(B, T, float(cap.FS), tp, pb.block.device, n_up=dp.N_up, n_down=dp.N_down, time_major=True,
                            warm=True, loss=kind, skip=int(skip), store_output=store_output)
        return st, xv, r, tgt

    def _loss_resident(self, x, target, kind="mse", skip=0, store_output=True):
        """mse() / mse_esr() on a resident circuit: inputs prepared once per (x, target) pair -- a training set and a
        validation set alternate in clipper_pot.py:245-262, each keeps its own stepper and warm-start state -- then one pass
        of the one-pass training step per call.  store_output=False: the step without the y store; the pair's entry (stepper,
        workspace, warm-start state) is the same either way, and its y buffer is made by the first call that wants it."""
        from . import engine
        pb = self._pblock
        pb.flush()                                               # (queued optimizer updates of the block go out first)
        dp_, vs_, cap_ = self.root, self.top.P1, self.top.P2
        now = [dp_.Is, dp_.nVt, (1.0 if self.per_sample_R is not None else vs_.R), cap_.C]
        for i, v in getattr(self, "_adopted_parts", {}).items():
            if now[i] is not v or getattr(v, "_wdf_block", (None,))[0] is not pb:
                raise binding.WdfHipError("Circuit.to_device: a component Variable was replaced (set_resistance?) or moved to another "
                                          "block after to_device(); build a new Circuit")
        ent = self._res_cache.get((x, target), (kind, int(skip)))
        if ent is None:
            st, xv, r, tgt = self._resident_stepper(x, target, kind, skip, store_output)
            T, B = xv.shape
            live = [(i, v) for i, v in sorted(pb.members.items()) if v.requires_grad]
            ent = self._res_cache.put((x, target), (st, xv, r, tgt, 1.0 / float(B * T) if kind == "mse" else 1.0,
                                                    [i for i, _ in live], [v for _, v in live], {id(v): i for i, v in live}),
                                      (kind, int(skip)), 3 * _nbytes(xv, r, tgt))
        st, xv, r, tgt, inv_n, idx, live = ent[:7]
        st.store_output = bool(store_output)                     # (this call's choice: step_fused makes y on first use)
        engine.LAST_TP_STATUS["status"] = st.status
        loss, out = engine._ResidentMseFn.apply(st, pb.block, xv, r, tgt, inv_n, idx, *live)
        loss = loss.as_subclass(tf.Tensor)
        # d loss / d Variable is already known: tape.gradient(loss, ...) on THIS tensor reads it (compat_tf.GradientTape)
        loss._wdf_fused = (out, ent[7])
        self.last_output = st.y if store_output else None        # (the stepper's own y [T,B], valid until the pair's next call)
        return loss

    def _loss_no_grad(self, kind, x, target, skip, z0, carry_state, store_output):
        """mse() / mse_esr() with grad=False: the loss as a detached scalar.  The resident diode-pair clipper takes the loss-only
        evaluation pass (EVAL_PASS_SERVES: DESIGN section 4), the resident MLP-root clipper its own (MLP_EVAL_PASS_SERVES), a resident
        diode-root tree with one or two states and sources its own (NL_EVAL_PASS_SERVES), a resident linear tree its own
        (LIN_EVAL_PASS_SERVES: csrc/wdf_ss_lin_eval.h, calls with z0 / carry_state included -- the pass takes the state in and hands
        it out as the step does, and its numbers are the step's bit for bit); every other circuit (and every other stateful call)
        runs the default's code and the result is detached."""
        binding.require_gpu()
        tensors = isinstance(x, torch.Tensor) and isinstance(target, torch.Tensor)
        stateful = (z0 is not None or carry_state) and self.ns > 0
        if tensors and not stateful and not self.force_generic:
            mres = getattr(self, "_mlp", None)
            if kind == "mse+esr" and mres is not None and int(x.shape[1]) % 16 == 0:
                return self._mlp_loss_no_grad(mres, x, target, skip, store_output)
            if (EVAL_PASS_SERVES and getattr(self, "_pblock", None) is not None and self._is_clipper() and self.root_kind == "DiodePair"
                    and 0 <= skip < int(x.shape[1])):
                return self._eval_resident(x, target, kind, skip, store_output)
            tree = getattr(self, "_tree", None)
            if (NL_EVAL_PASS_SERVES and tree is not None and self.root_kind == "DiodePair" and 1 <= self.ns <= 2 and 1 <= self.ni <= 2
                    and 0 <= skip < int(x.shape[1])):
                # a resident diode-root tree: the loss-only pass on an entry of its own (csrc/wdf_ss_nl_eval.h)
                with torch._C.DisableTorchFunctionSubclass():
                    ent = tree.eval_entry(x, target)
                    loss = tree.evaluate(ent, kind, int(skip), store_output)
                self.last_output = ent["y"] if store_output else None
                return loss.as_subclass(tf.Tensor)
        lin = getattr(self, "_lin", None)
        if LIN_EVAL_PASS_SERVES and lin is not None and tensors and x.dim() >= 2 and 0 <= skip < int(x.shape[1]):
            # a resident linear tree: the loss-only pass on an entry of its own (csrc/wdf_ss_lin_eval.h), stateful calls included --
            # z0 / carry_state are the pass's own z0 / zT, as they are the step's in _mse / _mse_esr_lin_step
            if carry_state and z0 is None:
                z0 = getattr(self, "last_state", None)
            if self.ns == 0:
                stateful, z0 = False, None                        # (no capacitor: nothing to carry)
            with torch._C.DisableTorchFunctionSubclass():
                ent = lin.eval_entry(x, target)
                loss = lin.evaluate(ent, kind, int(skip), store_output, self._z0_device(z0, ent["t"].device, ent["B"]), bool(stateful))
            self.last_output = ent["y"] if store_output else None
            if stateful:
                self.last_state = ent["zT"].clone()              # (ent["zT"] is one of two ping-pong buffers: kept by value)
            return loss.as_subclass(tf.Tensor)
        if kind == "mse":
            loss = self.mse(x, target, z0=z0, carry_state=carry_state, store_output=store_output)
        else:
            loss = self.mse_esr(x, target, skip, z0=z0, carry_state=carry_state, store_output=store_output)
        return loss.detach()                                     # (a new tensor: the pass's gradient is not attached to it)

    def _mlp_loss_no_grad(self, mres, x, target, skip, store_output):
        """The resident MLP-root clipper's loss without its gradient.  MLP_EVAL_PASS_SERVES: the loss-only evaluation pass
        (mlp_root.MlpEvalPass, made on first use inside the pair's entry: its own state block, the entry's tensors) -- the training
        side of the entry (its state block, st.gw, zstash, kappa, the call count and its re-plan) is not touched, so training is
        bit for bit what it is without the call, on the validated pair too.  Otherwise the step's forward and loss-sum phases,
        then the loss from the sums: no reverse sweep, st.gw untouched, the entry's call count and re-plan not advanced."""
        from . import mlp_root
        ent = mres.entry(x, target, skip)
        st = ent["st"]
        if MLP_EVAL_PASS_SERVES:
            ev = ent.get("eval")
            if ev is None:
                ev = ent["eval"] = mlp_root.MlpEvalPass.of(st)
                ent["eval_calls"] = 0
            loss3 = ev.run(store_output=store_output)
            ent["eval_calls"] += 1
            if ent["eval_calls"] == 24:                          # the controller has settled: one measured re-plan (the training entry's rule)
                ev.replan()
            self.last_output = st.y if store_output else None
            return loss3[2].clone().as_subclass(tf.Tensor)
        st._call(mlp_root.PHASE_FWD | mlp_root.PHASE_SUMS, None)
        if "eval_out" not in ent:
            ent["eval_out"] = (torch.zeros(2, dtype=torch.float32, device=st.sums.device), torch.zeros(3, dtype=torch.float32, device=st.sums.device))
        gcoef, loss3 = ent["eval_out"]
        binding.esr_coef(st.sums, st.n_global, st.eps_energy, gcoef=gcoef, loss=loss3)
        self.last_output = st.y if store_output else None
        return loss3[2].clone().as_subclass(tf.Tensor)

    def _eval_resident(self, x, target, kind, skip, store_output):
        """grad=False on a resident diode-pair clipper: one evaluation pass (engine.MseStep.eval_fused) on an entry of its own,
        keyed (kind, skip, "eval") -- its own stepper and warm-start state; the training entry of the same pair is never touched.
        The plan is the training step's (engine.tuned_plan, fused: the same two sequences per lane)."""
        from . import engine
        pb = self._pblock
        pb.flush()                                               # (queued optimizer updates of the block go out first)
        ent = self._res_cache.get((x, target), (kind, int(skip), "eval"))
        if ent is None:
            st, xv, r, tgt = self._resident_stepper(x, target, kind, skip, store_output)
            ent = self._res_cache.put((x, target), (st, xv, r, tgt), (kind, int(skip), "eval"), 3 * _nbytes(xv, r, tgt))
        st, xv, r, tgt = ent
        st.store_output = bool(store_output)                     # (this call's choice: eval_fused makes y on first use)
        engine.LAST_TP_STATUS["status"] = st.status
        loss3 = st.eval_fused(pb.block, xv, tgt, r)
        self.last_output = st.y if store_output else None
        return loss3[0 if kind == "mse" else 2].clone().as_subclass(tf.Tensor)

    def mse_esr(self, x, target, skip=0, z0=None, carry_state=False, store_output=True, grad=True):
        """The training loss of clipper_pot.py:146-156,177 on this circuit's output past `skip` samples (:232,248):
        mean((y - t)^2) + sqrt(sum((y - t)^2) / (sum(y^2) + eps) / n)  -- the scripts call esr_loss(outs, train_Y) on a
        function declared (target, predicted), so the normalising energy is the OUTPUT's.  target: [T,B] like the output.
        A resident diode-pair clipper (to_device()) evaluates loss and gradient in one pass over the data
        (wdf_clipper_step_esr_tp), and so does the clipper under an AsymDiodePair root with a Newton solver
        (wdf_clipper_asym_step_esr: forward, both loss sums and the six gradients in one sweep, with or without z0 /
        carry_state; `circ.last_output` is then the step's own y buffer, valid until the next call of the same shape, and a
        tensor of its own on stateful calls); a resident LINEAR tree (to_device() of an ideal-source root, at most two capacitors
        and two sources) likewise (wdf_ss_lin_step_esr, LIN_ESR_STEP_SERVES: z0 / carry_state are the step's own z0 / zT,
        `circ.last_output` the batch's output buffer); anything else composes it from the forward.
        z0 / carry_state: as in mse() -- the state the call starts from, or the one the previous carry_state call ended in
        (`circ.last_state`); composed from __call__(x, z0, return_state) (the resident one-pass steps start from zero state,
        which is what clipper_pot.py:110-111 does before every forward).
        store_output=False: as in mse() -- "I will not read y"; `circ.last_output` is None after the call.
        grad=False: as in mse() -- "I will not differentiate this loss" (the validation line, clipper_pot.py:262-264); a
        resident MLP-root clipper then runs its forward and the two loss sums only (no reverse sweep, no weight gradient); a
        resident linear tree has a loss-only evaluation pass of its own (csrc/wdf_ss_lin_eval.h: the step without tangents and
        Jacobian, the same bits; z0 / carry_state included), taken where LIN_EVAL_PASS_SERVES says the measurement allows it."""
        if not grad:
            return self._loss_no_grad("mse+esr", x, target, int(skip), z0, carry_state, bool(store_output))
        loss = self._mse_esr(x, target, skip, z0, carry_state, bool(store_output))
        if not store_output:
            self.last_output = None
        return loss

    def _mse_esr(self, x, target, skip, z0, carry_state, store_output):
        gx_route = self._input_grad_route(x)                     # (an x with a graph: composed from self(x), no one-pass step)
        binding.require_gpu()
        stateful = (z0 is not None or carry_state) and self.ns > 0
        if carry_state and z0 is None:                           # (once, for every branch that takes a state; the others never look at z0)
            z0 = getattr(self, "last_state", None)
        if gx_route is not None:
            if stateful:
                y, zT = self(x, z0=z0, return_state=True)
                self.last_state, self.last_output = zT.detach(), y.detach()
            else:
                y = self(x)
            o = y[int(skip):]
            t = tf.convert(target, device=o.device).reshape(y.shape)[int(skip):]
            S, E = tf.reduce_sum(tf.square(o - t)), tf.reduce_sum(tf.square(o)) + float(np.finfo(float).eps)
            n = float(o.numel())
            return S / n + tf.sqrt(S / E / n)
        if self.root_kind == "AsymDiodePair" and not self._asym_generic and self.root.mode != binding.ASYM_OMEGA_F32 \
                and 0 <= int(skip) < int(np.shape(x)[1]):
            return self._mse_esr_clipper_asym(x, target, int(skip), z0, stateful)      # the Newton solvers: the one-pass step
        if ASYM_TREE_STEP_SERVES["mse_esr"] and self._asym_step_tree(x, target, "mse_esr", skip):
            return self._asym_tree_step(x, target, "mse_esr", int(skip), z0, stateful)
        if LIN_ESR_STEP_SERVES and getattr(self, "_lin", None) is not None and isinstance(x, torch.Tensor) \
                and isinstance(target, torch.Tensor) and x.dim() >= 2 and 0 <= int(skip) < int(x.shape[1]):
            return self._mse_esr_lin_step(x, target, int(skip), z0, stateful, store_output)      # the linear step takes z0 / zT itself
        if stateful:
            y, zT = self(x, z0=z0, return_state=True)
            self.last_state, self.last_output = zT.detach(), y.detach()
            o = y[int(skip):]
            t = tf.convert(target, device=o.device).reshape(y.shape)[int(skip):]
            S, E = tf.reduce_sum(tf.square(o - t)), tf.reduce_sum(tf.square(o)) + float(np.finfo(float).eps)
            n = float(o.numel())
            return S / n + tf.sqrt(S / E / n)
        mres = getattr(self, "_mlp", None)
        if mres is not None and isinstance(x, torch.Tensor) and isinstance(target, torch.Tensor):
            from . import mlp_root
            if int(x.shape[1]) % 16 == 0:                        # (the resident step's blocks are 16 steps)
                ent = mres.entry(x, target, skip)
                live = [v for v in mres.vars if v.requires_grad]
                loss, out = mlp_root.MlpResidentFn.apply(mres, ent, *live)
                loss = loss.as_subclass(tf.Tensor)
                loss._wdf_fused = (out, {id(v): mres.spec[id(v)] for v in live})
                self.last_output = ent["st"].y
                return loss
        if (getattr(self, "_pblock", None) is not None and isinstance(x, torch.Tensor) and isinstance(target, torch.Tensor)
                and not self.force_generic):
            return self._loss_resident(x, target, "mse+esr", skip, store_output)
        # (a resident small tree under a DiodePair root has a one-pass step for this loss too -- _nl_step_tree /
        #  _mse_esr_nl_step, wdf_ss_nl_step_esr -- which this method does not take until tools/ss_nl_esr_step_bench.py has
        #  shown it faster than the composed path below at both of its shapes)
        y = self(x)
        o = y[int(skip):]
        t = tf.convert(target, device=o.device).reshape(y.shape)[int(skip):]
        S, E = tf.reduce_sum(tf.square(o - t)), tf.reduce_sum(tf.square(o)) + float(np.finfo(float).eps)
        n = float(o.numel())
        return S / n + tf.sqrt(S / E / n)

    def loss(self, x, target, skip=0, mse=1.0, esr=1.0, esr_emph=0.0, avg=0.0, coeff=0.85, n_global=None, sums_allreduce=None):
        """mse * mse_loss + esr * esr_loss + esr_emph * esr_with_emph + avg * avg_loss of clipper_pot.py:141-165 on this circuit's
        output past `skip` samples (:248: the slice first, the filter second), as one fused device stage behind the forward of
        whatever circuit this is (csrc/wdf_elementwise.h: wdf_loss_terms_sums / _coef / _grad; all sums in fp64).  With o =
        y[skip:], t = target[skip:], n = n_global (default: the kept sample count) and eps = np.finfo(float).eps:
            mse = sum((o-t)^2) / n            esr = sqrt(sum((o-t)^2) / (sum(o^2) + eps) / n)
            avg = |sum(o) - sum(t)| / n       esr_emph = esr of (f(o), f(t)),  f(v)[0] = v[0], f(v)[k] = v[k] - coeff v[k-1]
        The scripts call esr_loss(outs, train_Y) on a function declared (target, predicted), so both energies are the OUTPUT's
        (mse_esr's convention).  Weights >= 0 and not all zero, 0 <= coeff < 1; target: [T,B] like the output.
        One deviation from the reference: its pre_emphasis_filter works on axis 0 of whatever it is given, which in the script
        would be the BATCH axis of [B,T',1]; the function is never called there.  Here the filter runs along TIME, which is
        its evident purpose and what axis 0 is on this engine's [T,B] layout.

        y = self(x): the gradient reaches the Variables through the reverse sweep that forward registers, fed the stage's
        dL/dy.  Under torch.no_grad(), or when nothing requires a gradient, dL/dy is not formed and the forward keeps no
        stash (the validation pass of clipper_pot.py:258-266).  sums_allreduce: in-place SUM all-reduce of the six float64
        sums when the batch is sharded (wdf_hip.dist.allreduce_sum_), with n_global the sample count over all ranks.
        `circ.last_loss_terms` is {mse, esr, esr_emph, avg} as detached device scalars, `circ.last_output` is y: the scripts'
        history[...] lines need no second pass.  mse() and mse_esr() are untouched by this stage."""
        weights, coeff = binding.check_loss_weights((mse, esr, esr_emph, avg), coeff)
        if n_global is not None and not float(n_global) > 0.0:
            raise ValueError(f"n_global must be positive, got {n_global}")
        self._input_grad_route(x)                                # (a route without dL/dx says so before a device is asked for)
        binding.require_gpu()
        y = self(x)
        yt = y.as_subclass(torch.Tensor)
        T = int(yt.shape[0])
        if not 0 <= int(skip) < T:
            raise ValueError(f"skip must be in [0, {T}), got {skip}")
        tgt = torch.as_tensor(target).as_subclass(torch.Tensor).detach().to(yt.device).float().reshape(yt.shape).contiguous()
        n = float(n_global) if n_global is not None else float((T - int(skip)) * int(yt.shape[1]))
        want_grad = torch.is_grad_enabled() and yt.requires_grad
        loss, terms = _LossTermsFn.apply(yt, tgt, int(skip), weights, coeff, n, sums_allreduce, want_grad)
        self.last_output = yt.detach()
        self.last_loss_terms = {"mse": terms[0], "esr": terms[1], "esr_emph": terms[2], "avg": terms[3]}
        return loss.as_subclass(tf.Tensor)

    def _mse_esr_nl_step(self, lin, x, target, skip):
        """mse_esr(x, target, skip) of the resident tree `lin` as ONE pass (wdf_ss_nl_step_esr) through the MSE step's autograd
        function: the loss carries the gradient the pass produced (`_wdf_fused`), the queued optimizer updates ride in its probe
        launch, `last_output` is the step's y."""
        with torch._C.DisableTorchFunctionSubclass():
            lin.check()
            ent = lin.entry(x, target, "mse+esr", int(skip))
            live = [(i, v) for i, v in sorted(lin.pb.members.items()) if v.requires_grad]
        loss, out = _LinResidentMseFn.apply(lin, ent, 1.0, [i for i, _ in live], None, False, *[v for _, v in live])
        loss = loss.as_subclass(tf.Tensor)
        loss._wdf_fused = (out, {id(v): i for i, v in live})
        self.last_output = ent["y"]
        return loss

    def _mse_esr_lin_step(self, x, target, skip=0, z0=None, stateful=False, store_output=True):
        """mse_esr(x, target, skip) of a resident LINEAR tree as ONE pass (wdf_ss_lin_step_esr) through the MSE step's autograd
        function, factor 1.0: the loss carries the gradient the pass produced (`_wdf_fused`), the queued optimizer updates ride in
        its probe launch, `last_output` is the step's y.  z0 [ns,B] / stateful: the step's own z0 / zT, as in mse(); `last_state`
        is a clone of zT on stateful calls."""
        lin = getattr(self, "_lin", None)
        if lin is None:
            raise binding.WdfHipError("Circuit._mse_esr_lin_step: a resident linear tree only (to_device() of an ideal-source root, at "
                                      "most two capacitors and two sources)")
        if not (isinstance(x, torch.Tensor) and isinstance(target, torch.Tensor)) or not 0 <= int(skip) < int(x.shape[1]):
            raise binding.WdfHipError("Circuit._mse_esr_lin_step: tensors in and 0 <= skip < T")
        if self.ns == 0:
            stateful, z0 = False, None                            # (no capacitor: nothing to carry)
        with torch._C.DisableTorchFunctionSubclass():
            lin.check()
            ent = lin.entry(x, target, "mse+esr", int(skip), store_output)
            live = [(i, v) for i, v in sorted(lin.pb.members.items()) if v.requires_grad]
            z0d = self._z0_device(z0, ent["t"].device, ent["B"])
        loss, out = _LinResidentMseFn.apply(lin, ent, 1.0, [i for i, _ in live], z0d, bool(stateful), *[v for _, v in live])
        loss = loss.as_subclass(tf.Tensor)
        loss._wdf_fused = (out, {id(v): i for i, v in live})
        self.last_output = ent["y"]
        if stateful:
            self.last_state = ent["zT"].clone()                  # (ent["zT"] is one of two ping-pong buffers: kept by value)
        return loss

    def _asym_step_tree(self, x, target, kind="mse", skip=0):
        """Whether the one-pass step of csrc/wdf_ss_asym_step.h can serve mse(x, target) (kind="mse") or mse_esr(x, target, skip)
        (kind="mse_esr") on this circuit: an AsymDiodePair(any_tree=True) root on the generic state-space kernels, a tree the
        step is built for under this loss (one or two capacitors, one or two sources), tensors in, 0 <= skip < T."""
        if not getattr(self, "_asym_generic", False) or kind not in ("mse", "mse_esr"):
            return False
        if getattr(self, "_asym_streamed", False):                # (the streamed-coefficient kernels have no one-pass step)
            return False
        if not (isinstance(x, torch.Tensor) and isinstance(target, torch.Tensor)):
            return False
        if x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[2] != self.ni) or (x.dim() == 2 and self.ni != 1):
            return False
        if not 0 <= int(skip) < int(x.shape[1]):
            return False
        return bool(binding.ss_asym_step_built(self.ns, self.ni, kind))

    def _asym_tree_step(self, x, target, kind="mse", skip=0, z0=None, stateful=False):
        """mse(x, target) / mse_esr(x, target, skip) of a tree under AsymDiodePair(any_tree=True) as ONE pass over the data
        (wdf_ss_asym_step_mse / _esr): forward, loss and the gradient of every coefficient and of the root's five values in one
        sweep; the probe's float64 graph carries them to the components.  The chunks are plan_ss_time_parallel's (k_fwd,
        warmup, tol) or those of an explicit SsTpPlan; time_parallel=None is the sequential recursion.  z0 [ns,B] and
        stateful (z0 / carry_state was asked for): the kernel's own z0 / zT; last_output and last_state as in mse()."""
        binding.require_gpu()
        xt = x.as_subclass(torch.Tensor)
        xt = (xt if xt.is_cuda else xt.cuda()).float()
        if xt.dim() == 2:
            xt = xt.unsqueeze(-1)
        xt = xt.contiguous()
        dev, B, T = xt.device, int(xt.shape[0]), int(xt.shape[1])
        tgt = target.as_subclass(torch.Tensor).detach().to(dev).float().reshape(T, B).contiguous()
        coef64, r_port = self.matrices()
        coef = coef64.to(device=dev, dtype=torch.float32)
        dp = self.root
        rootp = torch.stack([v.as_subclass(torch.Tensor).double().reshape(()) for v in (dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down)]
                            + [r_port.double().reshape(())]).to(device=dev, dtype=torch.float32)
        tp = self.time_parallel
        if tp == "auto":
            tp = plan_ss_time_parallel(coef64, self.ns, self.ni, binding.ROOT_ASYM_PAIR, B, T)
        elif not isinstance(tp, SsTpPlan):
            tp = None
        k, W, tol = (int(tp.k_fwd), int(tp.warmup), float(tp.tol)) if (tp is not None and tp.k_fwd >= 2) else (1, 0, 1.0e-6)
        loss, y, zT = _AsymTreeStepFn.apply(coef, rootp, xt, tgt, self.ns, self.ni, kind, int(skip), self._z0_device(z0, dev, B),
                                            bool(stateful), k, W, tol)
        self.last_output = y
        if stateful:
            self.last_state = zT
        return loss.as_subclass(tf.Tensor)

    def _nl_step_tree(self, x, target, skip=0, z0=None, carry_state=False):
        """The resident tree whose one-pass MSE + ESR step (wdf_ss_nl_step_esr) can serve mse_esr(x, target, skip), or None: the
        conditions under which mse() takes the diode-root step -- to_device() made a resident tree, DiodePair root, one or
        two capacitors and sources, not force_generic, tensors in, zero initial state -- and 0 <= skip < T.  Two capacitors
        WITH two sources keep the composed path: the MSE + ESR kernels are not built for that tree (WDF_EUNSUPPORTED; both
        families of accumulators do not fit a wave's registers there)."""
        tree = getattr(self, "_tree", None)
        if tree is None or self.root_kind != "DiodePair" or not (1 <= self.ns <= 2 and 1 <= self.ni <= 2) or self.force_generic:
            return None
        if self.ns * self.ni == 4:
            return None
        if not (isinstance(x, torch.Tensor) and isinstance(target, torch.Tensor)) or z0 is not None or carry_state:
            return None
        if x.dim() < 2 or not 0 <= int(skip) < int(x.shape[1]):
            return None
        return tree

    # -- topology tests
    def mse(self, x, target, z0=None, carry_state=False, store_output=True, grad=True):
        """tf.reduce_mean(tf.square(self(x) - target)) as ONE fused evaluation where the kernels allow
        it (diode-pair clipper: forward kernel + MSE-fused reverse sweep, the gradient of every
        trainable component ready when tape.gradient asks; the clipper under an AsymDiodePair root with a Newton solver: the
        one-pass step of csrc/wdf_asym_step.h, forward, loss and six gradients in one sweep); any other circuit takes the
        plain path.  target: [T,B] like the output.

        z0 [ns,B]: the capacitor states the call starts from (default: zero, clipper_pot.py:110-111).  carry_state=True: the
        call starts from the states the PREVIOUS carry_state call on this circuit ended in (zero the first time) -- lpf.py:30-49
        never resets C1, so its epoch n starts where epoch n - 1 ended; the state handed over is a constant of the new call
        (the reference's stored tensor belongs to the previous tape).  `circ.last_state` [ns,B] is what the call ended in
        (set whenever z0 / carry_state is used; a tensor of its own that later calls leave alone); `circ.reset_state()` forgets
        it.  A resident linear tree runs this inside the one-pass step (wdf_ss_lin_step_mse's z0 / zT); every other circuit
        composes it from __call__(x, z0, return_state).  `circ.last_output` [T,B] is the call's y; on a resident tree it is the
        batch's own output buffer, valid until the next call on the same (x, target) -- clone it to keep it longer.

        store_output=False is a permission: "I will not read y" (a training loop reads the loss and the gradient,
        clipper_pot.py:245-269).  A resident diode-pair clipper and a resident linear tree then run their one-pass step
        without the y store (8 instead of 12, 12 instead of 16 B/sample); every other circuit computes exactly as with the
        default.  In every case `circ.last_output` is None after such a call.  The resident cache keeps ONE entry per
        (x, target) pair whichever way it is called -- one workspace, one warm-start state -- and allocates the pair's y buffer
        lazily, on the first call that wants it: a training set only ever run without y holds no y buffer, and a later
        storing call on the same pair gets its y.

        grad=False is a permission too: "I will not differentiate this loss" (a validation pass).  The loss that comes back is
        detached in every case (`requires_grad` False, no gradient attached).  A resident diode-pair clipper then runs the
        loss-only evaluation pass (csrc/wdf_clipper_eval.h: forward and the loss sums, no tangent, no gradient) on an entry of
        its own per (x, target) pair -- its own stepper, workspace and warm-start state; a training entry on the same pair is not
        touched; a resident linear tree has its own pass too (csrc/wdf_ss_lin_eval.h: forward and the two loss sums in the
        step's chunks, bit for bit the step's loss, y and final state, with z0 / carry_state as the step takes them; an entry of
        its own per pair; taken where LIN_EVAL_PASS_SERVES says the measurement allows it); every other circuit computes exactly
        as with the default and detaches the result.  grad=True runs the code it always ran; torch.no_grad() routes nothing."""
        if not grad:
            return self._loss_no_grad("mse", x, target, 0, z0, carry_state, bool(store_output))
        loss = self._mse(x, target, z0, carry_state, bool(store_output))
        if not store_output:
            self.last_output = None
        return loss

    def _mse(self, x, target, z0, carry_state, store_output):
        gx_route = self._input_grad_route(x)                     # (an x with a graph: composed from self(x), no one-pass step)
        binding.require_gpu()
        stateful = z0 is not None or carry_state
        if carry_state and z0 is None:
            z0 = getattr(self, "last_state", None)
        if stateful and self.ns == 0:
            stateful, z0 = False, None                            # (no capacitor: nothing to carry)
        if gx_route is not None:
            if stateful:
                y, zT = self(x, z0=z0, return_state=True)
                self.last_state, self.last_output = zT.detach(), y.detach()
            else:
                y = self(x)
            return tf.reduce_mean(tf.square(y - tf.convert(target, device=y.device).reshape(y.shape)))
        lin = getattr(self, "_lin", None)
        if lin is None and getattr(self, "_tree", None) is not None and self.root_kind == "DiodePair" and 1 <= self.ns <= 2 \
                and 1 <= self.ni <= 2 and not self.force_generic:
            lin = self._tree                                     # diode-pair root: the tangent-carried step (csrc/wdf_ss_nl_step.h)
        if stateful and lin is not None and lin is not getattr(self, "_lin", None):
            lin = None                                           # (diode-root one-pass step: zero state only -> the plain path)
        if lin is not None and isinstance(x, torch.Tensor) and isinstance(target, torch.Tensor):
            with torch._C.DisableTorchFunctionSubclass():        # (asking a tensor for its version or requires_grad must not
                lin.check()                                      #  send the queued optimizer updates: the probe carries them)
                ent = lin.entry(x, target, store_output=store_output)
                live = [(i, v) for i, v in sorted(lin.pb.members.items()) if v.requires_grad]
                z0d = self._z0_device(z0, ent["t"].device, ent["B"])      # the linear step takes the state in and hands it out
            loss, out = _LinResidentMseFn.apply(lin, ent, 1.0 / float(ent["B"] * ent["T"]), [i for i, _ in live], z0d, stateful,
                                                *[v for _, v in live])
            loss = loss.as_subclass(tf.Tensor)
            loss._wdf_fused = (out, {id(v): i for i, v in live})
            self.last_output = ent["y"]                          # the forward's y [T,B] of this call (TensorArray.stack() layout)
            if stateful:
                self.last_state = ent["zT"].clone()              # (ent["zT"] is one of two ping-pong buffers: [ns,B], kept by value)
            return loss
        if self.root_kind == "AsymDiodePair" and not self._asym_generic and self.root.mode != binding.ASYM_OMEGA_F32:
            return self._mse_clipper_asym(x, target, z0, stateful)      # the Newton solvers: the one-pass step
        if ASYM_TREE_STEP_SERVES["mse"] and self._asym_step_tree(x, target, "mse"):
            return self._asym_tree_step(x, target, "mse", 0, z0, stateful)     # any small tree under this root: its one-pass step
        if stateful:
            y, zT = self(x, z0=z0, return_state=True)
            self.last_state, self.last_output = zT.detach(), y.detach()
            return tf.reduce_mean(tf.square(y - tf.convert(target, device=y.device).reshape(y.shape)))
        if not (self._is_clipper() and self.root_kind == "DiodePair" and not self.force_generic):
            y = self(x)
            return tf.reduce_mean(tf.square(y - target))
        from . import engine
        if getattr(self, "_pblock", None) is not None and isinstance(x, torch.Tensor) and isinstance(target, torch.Tensor):
            return self._loss_resident(x, target, store_output=store_output)
        anchor = x if isinstance(x, torch.Tensor) else None
        x = torch.as_tensor(x).as_subclass(torch.Tensor)
        x = (x if x.is_cuda else x.cuda()).float()
        dp, vs, cap = self.root, self.top.P1, self.top.P2
        # a streamed pot resistance overrides the source's own R (which a recorded loop may have left symbolic)
        Rv = torch.tensor(1.0) if self.per_sample_R is not None else (vs.R if isinstance(vs.R, torch.Tensor) else torch.tensor(float(vs.R)))
        parts = [dp.Is, dp.nVt, Rv, cap.C]
        theta = self._theta(parts, x.device)
        # the sweep reads its inputs time-major: the transposed copy is made once per input tensor
        xv, r = engine.split_channels(x, self.per_sample_R is not None, time_major=True, anchor=anchor)
        tgt = torch.as_tensor(target).as_subclass(torch.Tensor).to(x.device).float().reshape(xv.shape).contiguous()
        R_host, C_host = self._host_RC(parts)
        R_plan = R_host if r is None else engine.resistance_max(r)
        tp = self.time_parallel
        if tp == "auto":
            tp = engine.tuned_plan(theta, xv, r, float(cap.FS), R_plan, C_host, n_up=dp.N_up, n_down=dp.N_down,
                                   time_major=True, R_min=None if r is None else engine.resistance_min(r), fused=True)
        loss = engine.clipper_mse(theta, xv, tgt, float(cap.FS), r=r, n_up=dp.N_up, n_down=dp.N_down, tp=tp,
                                  time_major=True)
        return loss.as_subclass(tf.Tensor)

    def _gn_parts(self):
        """The six values [Is_up, nVt_up, Is_down, nVt_down, Vs.R, C] mse_gn() differentiates against, or the refusal, by name,
        of every circuit the Gauss-Newton step (csrc/wdf_asym_gn.h) does not serve -- raised before a device is asked for."""
        def refuse(what):
            raise binding.WdfHipError(f"Circuit.mse_gn: {what} has no Gauss-Newton step: it serves the diode-clipper tree under "
                                      "AsymDiodePair with a Newton solver (csrc/wdf_asym_gn.h), stateless")
        if self.root_kind != "AsymDiodePair":
            refuse(f"a {self.root_kind} root")
        if getattr(self.root, "streamed", False):
            refuse("AsymDiodePair(streamed=True) (the streamed-coefficient kernels)")
        if self._asym_generic:
            refuse("AsymDiodePair(any_tree=True) off the clipper's own kernels (the generic state-space kernels)")
        if self.per_sequence_R is not None:
            refuse("per_sequence_R (one pot per sequence)")
        if self.root.mode == binding.ASYM_OMEGA_F32:
            refuse("the omega_f32 solver (the closed form, a model approximation)")
        dp, vs, cap = self.root, self.top.P1, self.top.P2
        return [dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down, vs.R, cap.C]

    def _gn_lin(self):
        """The resident linear tree mse_gn() runs on (csrc/wdf_ss_lin_gn.h) -- an ideal-source root, at most two capacitors and two
        sources, made resident by to_device() -- or None for every other circuit (_gn_parts names those); such a tree whose
        values still live on the host raises, naming to_device()."""
        if self.root_kind != "IdealVoltageSource" or self._dyn or self.ns > 2 or self.ni > 2 or self.per_sample_R is not None:
            return None
        lin = getattr(self, "_lin", None)
        if lin is None:
            raise binding.WdfHipError("Circuit.mse_gn: a linear tree runs its Gauss-Newton step (csrc/wdf_ss_lin_gn.h) on component "
                                      "values that live on the device: call circ.to_device() first")
        return lin

    @staticmethod
    def _gn_lin_keep(lin):
        """(index in the block, Variable) of every trainable Variable among the resident tree's component values, block order"""
        return [(i, v) for i, v in sorted(lin.adopted.items()) if isinstance(v, tf.Variable) and v.trainable]

    @property
    def gn_variables(self):
        """The rows and columns of what mse_gn() returns: the trainable Variables among [Is_up, nVt_up, Is_down, nVt_down, Vs.R, C],
        in that order (the two-different-diode clipper), or among a resident linear tree's component values, in the order of its
        parameter block (tree order)."""
        lin = self._gn_lin()
        if lin is not None:
            return [v for _, v in self._gn_lin_keep(lin)]
        return [p for p in self._gn_parts() if isinstance(p, tf.Variable) and p.trainable]

    def _mse_gn_lin(self, lin, x, target, z0, carry_state):
        """mse_gn() on a resident linear tree: probe + wdf_ss_lin_step_gn on an entry of its own per (x, target) pair."""
        if carry_state:
            raise binding.WdfHipError("Circuit.mse_gn: carry_state has no Gauss-Newton step: a rejected Levenberg-Marquardt trial would "
                                      "have moved the carried state; hand the state in as z0 (a constant of the call)")
        if not (isinstance(x, torch.Tensor) and isinstance(target, torch.Tensor)):
            raise binding.WdfHipError("Circuit.mse_gn: a resident linear tree takes x and target as tensors (the resident set is kept "
                                      "per tensor pair)")
        keep = self._gn_lin_keep(lin)
        if not keep:
            raise binding.WdfHipError("Circuit.mse_gn: no trainable Variable among the tree's component values")
        binding.require_gpu()
        with torch.no_grad(), torch._C.DisableTorchFunctionSubclass():
            lin.check()
            ent = lin.gn_entry(x, target)
            z0d = self._z0_device(z0, ent["t"].device, ent["B"]) if self.ns > 0 else None
            out = lin.gn_step(ent, z0d)
            n = lin.pb.n
            loss, g, H = out[0] / float(ent["B"] * ent["T"]), out[1:1 + n], binding.sym_from_upper(out[1 + n:], n)
            if len(keep) < n:
                idx = torch.tensor([i for i, _ in keep], device=g.device)
                g, H = g[idx], H[idx][:, idx]
        self.last_output = ent["y"].as_subclass(tf.Tensor)
        return loss, g, H

    def mse_gn(self, x, target, z0=None, carry_state=False):
        """Loss, gradient and Gauss-Newton matrix of tf.reduce_mean(tf.square(self(x) - target)) in ONE pass over the data
        (wdf_clipper_asym_step_gn: the one-pass MSE step, which holds dy_t/dtheta in registers at every sample, also sums
        its products): -> (loss, g, H), detached device tensors, loss 0-dim, g [n] the gradient and H [n,n] = (2/N) J^T J,
        symmetric, float64, over the n trainable Variables in the order of `circ.gn_variables`; rows and columns of values
        that are not trainable are dropped.  What wdf_hip.lm.LevenbergMarquardt(lambda: circ.mse_gn(x, target),
        circ.gn_variables) takes.  H is singular by construction (scaling Is_up, Is_down and C by s and R by 1/s leaves y
        unchanged): judge a fit by its loss, never by the values.  Sets `circ.last_output` (the stepper's buffer, valid until
        the next call of this shape).  Serves the clipper tree under AsymDiodePair with a Newton solver, from zero state
        (z0 and carry_state raise there), and a resident linear tree (to_device(); lpf.py, voltage_divider.py:
        wdf_ss_lin_step_gn, loss float64 too): there z0 [ns,B] is served, a constant of the call, carry_state raises (a rejected
        trial would have moved the carried state), and H is singular as well -- y depends on R C, or on R1 / R2, only.  Every
        other circuit raises, by name."""
        lin = self._gn_lin()
        if lin is not None:
            return self._mse_gn_lin(lin, x, target, z0, carry_state)
        parts = self._gn_parts()
        if z0 is not None or carry_state:
            raise binding.WdfHipError("Circuit.mse_gn: z0 / carry_state has no Gauss-Newton step: the pass starts from zero state")
        keep = [i for i, p in enumerate(parts) if isinstance(p, tf.Variable) and p.trainable]
        if not keep:
            raise binding.WdfHipError("Circuit.mse_gn: no trainable Variable among Is_up, nVt_up, Is_down, nVt_down, Vs.R, C")
        binding.require_gpu()
        from . import engine
        anchor = x if isinstance(x, torch.Tensor) else None
        x = torch.as_tensor(x).as_subclass(torch.Tensor)
        x = (x if x.is_cuda else x.cuda()).float()
        with torch.no_grad():
            theta6, xv, _, tp = self._asym_inputs(x, anchor)
        B, T = xv.shape
        tgt = torch.as_tensor(target).as_subclass(torch.Tensor).to(x.device).float().reshape(T, B).contiguous()
        loss, g, H, y = engine.clipper_asym_gn(theta6, xv, tgt, float(self.top.P2.FS), tp=tp, mode=self.root.mode)
        self.last_output = y.as_subclass(tf.Tensor)
        if len(keep) < 6:
            idx = torch.tensor(keep, device=g.device)
            g, H = g[idx], H[idx][:, idx]
        return loss, g, H

    def _input_grad_route(self, x):
        """What __call__ does with an x that carries a graph (grad mode on, x.requires_grad): None for a plain x -- nothing
        changes; "generic" for the diode-pair clipper with host-resident Variables and no resistance channel (it takes the
        generic state-space path, force_generic's); "state-space" for whatever reaches _StateSpaceFn anyway (host-resident
        trees, resident trees through _ProbeFn, AsymDiodePair(any_tree=True)): the reverse sweep is followed by the
        input-gradient pass.  Every other route has no kernel that writes dL/dx and raises, naming itself, before a device is
        asked for -- the gradient used to be dropped without a word."""
        if not (torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad):
            return None

        def refuse(route, instead):
            raise binding.WdfHipError(f"Circuit: the input carries an autograd graph (x.requires_grad), and {route} has no "
                                      f"input gradient dL/dx: {instead}, or pass x.detach() if the gradient is not wanted")

        if self._dyn:
            refuse("the streamed-coefficient route (csrc/wdf_ss_dyn.h: a per_sample_R channel, a DenseRootModel root or "
                   "AsymDiodePair(streamed=True) off the clipper's own kernels, more than four capacitors)",
                   "the static state-space kernels serve trees of at most four capacitors with fixed resistances")
        if self._is_clipper() and self.root_kind == "DiodePair" and not self.force_generic:
            if self.per_sample_R is not None:
                refuse("the diode-pair clipper with a per_sample_R channel", "a fixed source resistance takes the generic path")
            if getattr(self, "_pblock", None) is not None:
                refuse("the resident diode-pair clipper (to_device(): the one-pass step's kernels)",
                       "a clipper left on the host path takes the generic state-space kernels")
            return "generic"
        if self.root_kind == "AsymDiodePair" and not self._asym_generic:
            if self.per_sequence_R is not None:
                refuse("the two-different-diode clipper under per_sequence_R (csrc/wdf_asym.h)",
                       "AsymDiodePair(any_tree=True) with force_generic=True and a fixed resistance is served")
            refuse("the two-different-diode clipper's own kernels (csrc/wdf_asym.h)",
                   "AsymDiodePair(any_tree=True) with force_generic=True is served")
        if self.root_kind == "DenseRootModel":
            refuse("the MLP root (csrc/wdf_mlp.h)", "no route serves a network root yet")
        return "state-space"

    def reset_state(self):
        """Forget the state carried by mse(..., carry_state=True): the next such call starts from zero (Capacitor.reset,
        tf_wdf.py:117-118)."""
        self.last_state = None

    def _is_clipper(self):
        t = self.top
        return (_kind(t) == "Parallel" and _kind(t.P1) == "ResistiveVoltageSource" and _kind(t.P2) == "Capacitor"
                and self.probe is t.P2)

    # -- one probed step -> state-space matrices (float64 CPU tensors with autograd graph)
    def matrices(self):
        ns, ni = self.ns, self.ni
        K = ns + ni + 1
        eye = torch.eye(K, dtype=torch.float64)
        from . import trace
        saved = _Saved(self.elements + [self.root])
        rec, trace._current = trace._current, None      # probing is never part of a recorded loop
        plain = torch._C.DisableTorchFunctionSubclass()   # ~35 scalar / [K] torch ops: plain dispatch halves their host time
        plain.__enter__()
        try:
            for s, cap in enumerate(self.caps):
                cap.z = eye[s]
            for i, src in enumerate(self.sources):
                src.Vs = eye[ns + i]
            self.top.calc_impedance()
            up = self.top.reflected() + torch.zeros(K, dtype=torch.float64)        # broadcast scalars
            self.top.incident(eye[K - 1])
            znew = [cap.z + torch.zeros(K, dtype=torch.float64) for cap in self.caps]
            yv = (self.probe.a + self.probe.b) * 0.5 + torch.zeros(K, dtype=torch.float64)
            r_port = self.top.R
        finally:
            plain.__exit__(None, None, None)
            saved.restore()
            trace._current = rec
        up, yv = up.as_subclass(torch.Tensor), yv.as_subclass(torch.Tensor)
        Z = torch.stack([z.as_subclass(torch.Tensor) for z in znew]) if ns else torch.zeros(0, K, dtype=torch.float64)
        A, Bx, E = Z[:, :ns], Z[:, ns:ns + ni], Z[:, K - 1]
        ca, da = up[:ns], up[ns:ns + ni]
        cy, dy, fy = yv[:ns], yv[ns:ns + ni], yv[K - 1]
        if self.root_kind == "IdealVoltageSource":
            # b = -a + 2 Vs (tf_wdf.py:26-28) is linear: fold it in.  Vs is the LAST channel.
            er = torch.zeros(ni, dtype=torch.float64)
            er[ni - 1] = 1.0
            A = A - torch.outer(E, ca)
            Bx = Bx - torch.outer(E, da) + 2.0 * torch.outer(E, er)
            cy = cy - fy * ca
            dy = dy - fy * da + 2.0 * fy * er
            E, ca, da, fy = torch.zeros_like(E), torch.zeros_like(ca), torch.zeros_like(da), torch.zeros_like(fy)
        coef = torch.cat([A.reshape(-1), Bx.reshape(-1), E, ca, da, cy, dy, fy.reshape(1)])
        return coef, r_port.as_subclass(torch.Tensor) if isinstance(r_port, torch.Tensor) else torch.tensor(float(r_port))

    # -- run
    def __call__(self, x, z0=None, return_state=False):
        """x: [B,T] or [B,T,n_in] float32 CUDA tensor (batch-major, the reference's
        input[:, i, c] layout).  Returns y [T,B] (and the final capacitor states [ns,B]).
        An x that carries a graph (a trainable gain or pre-filter in front, another circuit's output) gets its gradient where
        a state-space kernel runs the tree (_input_grad_route); every other route raises."""
        gx_route = self._input_grad_route(x)
        binding.require_gpu()
        self._anchor = x if isinstance(x, torch.Tensor) else None      # the caller's object: cache key for its copies
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(x)
        x = x.as_subclass(torch.Tensor)
        if not x.is_cuda:
            x = x.cuda()
        x = x.float()
        if x.dim() == 2:
            x = x.unsqueeze(-1)
        nchan = self.ni + (1 if self.per_sample_R is not None or self.per_sequence_R is not None else 0)
        if x.dim() != 3 or x.shape[2] != nchan:
            raise binding.WdfHipError(f"x must be [B,T,{nchan}] (or [B,T] for one channel), got {tuple(x.shape)}")
        dev = x.device

        if self._dyn:
            return self._run_dyn(x, z0, return_state)
        if self._is_clipper() and self.root_kind == "DiodePair" and not self.force_generic and gx_route != "generic":
            return self._run_clipper(x, z0, return_state)
        if self.root_kind == "AsymDiodePair" and not self._asym_generic:
            return self._run_clipper_asym(x, z0, return_state)
        if self.root_kind == "DenseRootModel":
            from . import mlp_root
            return mlp_root.run_clipper_mlp(self, x, z0, return_state)

        res = getattr(self, "_tree", None) or getattr(self, "_lin", None)
        if res is not None:
            # resident component values: coefficients (and their chain rule) from the device probe, the plan from the
            # block's lagging host mirror
            res.check()
            live = [(i, v) for i, v in sorted(res.pb.members.items()) if v.requires_grad]
            coef, rootp_r = _ProbeFn.apply(res, [i for i, _ in live], *[v for _, v in live])
            c64, _ = res.host_coef()
            coef64 = torch.as_tensor(c64)
            if self.root_kind == "DiodePair":
                rootp, kind, n_up, n_down = rootp_r, binding.ROOT_DIODE_PAIR, self.root.N_up, self.root.N_down
            else:
                rootp, kind, n_up, n_down = None, binding.ROOT_NONE, 1, 1
        else:
            coef64, r_port = self.matrices()
            coef = coef64.to(device=dev, dtype=torch.float32)
            if self.root_kind == "DiodePair":
                dp = self.root
                rootp = torch.stack([dp.Is.as_subclass(torch.Tensor).double().reshape(()),
                                     dp.nVt.as_subclass(torch.Tensor).double().reshape(()),
                                     r_port.double().reshape(())]).to(device=dev, dtype=torch.float32)
                kind, n_up, n_down = binding.ROOT_DIODE_PAIR, dp.N_up, dp.N_down
            elif self.root_kind == "AsymDiodePair":
                # two different diodes on the generic kernels: the four diode Variables and the port resistance the tree shows
                dp = self.root
                rootp = torch.stack([v.as_subclass(torch.Tensor).double().reshape(()) for v in
                                     (dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down)]
                                    + [r_port.double().reshape(())]).to(device=dev, dtype=torch.float32)
                kind, n_up, n_down = binding.ROOT_ASYM_PAIR, 1, 1
            else:
                rootp, kind, n_up, n_down = None, binding.ROOT_NONE, 1, 1
        z0t = None if z0 is None else z0.as_subclass(torch.Tensor).to(dev).float().reshape(self.ns, -1).contiguous()
        tp = getattr(self, "time_parallel", None)
        if tp == "auto" and res is not None:                      # (the plan follows the host mirror: cached with it)
            pkey = (kind, int(x.shape[0]), int(x.shape[1]))
            tp = res.plans.get(pkey, "miss")
            if tp == "miss":
                tp = res.plans[pkey] = plan_ss_time_parallel(coef64, self.ns, self.ni, kind, x.shape[0], x.shape[1])
        elif tp == "auto":
            tp = plan_ss_time_parallel(coef64, self.ns, self.ni, kind, x.shape[0], x.shape[1])
        elif not isinstance(tp, SsTpPlan):
            tp = None
        warm = None
        if tp is not None and tp.k_fwd >= 2 and kind in (binding.ROOT_DIODE_PAIR, binding.ROOT_ASYM_PAIR) and self._anchor is not None \
                and self.warm_start:
            # the caller's tensor object and version name the batch: the same one again -> its chunks start warm
            ws = self.__dict__.setdefault("_ss_warm", ObjectMemo(4))
            warm = ws.get(self._anchor, tuple(x.shape))
            if warm is None:
                warm = ws.put(self._anchor, SsWarmStart(x.shape[1], x.shape[0], self.ns, tp), tuple(x.shape))
            warm.plan = tp                  # (the cold plan follows the components as they train; the warm state stays)
        y, zT = _StateSpaceFn.apply(coef, rootp, x.contiguous(), z0t, self.ns, self.ni, kind, n_up, n_down,
                                    bool(return_state), tp, warm)
        y = y.as_subclass(tf.Tensor)
        return (y, zT) if return_state else y

    def _run_dyn(self, x, z0, return_state):
        """Per-sample impedance on any small tree and / or the MLP root on any small tree (csrc/wdf_ss_dyn.h).
        The probed step is recorded once as a scalar tape over the component values (probe_tape.record: the elements' own
        calc_impedance / reflected / incident code); with a resistance channel the tape is evaluated over the whole channel
        in torch -- one coefficient row per (sample, sequence), with the autograd graph back to the static components -- which
        is set_resistance + calc_impedance every step (clipper_pot.py:116-117) hoisted out of the time loop."""
        from . import probe_tape
        dev = x.device
        B, T = int(x.shape[0]), int(x.shape[1])
        own = {"Resistor": "R", "ResistiveVoltageSource": "R", "Capacitor": "C"}
        res = getattr(self, "_dynres", None)
        if res is not None:
            res.pb.flush()                                   # (queued optimizer updates of the block go out before anything reads it)
        if getattr(self, "_dyn_tape", None) is None:
            params = [(e, own[_kind(e)]) for e in self.elements if _kind(e) in own]
            pvars = [e.__dict__[n] for e, n in params]
            tape, outs, rport = probe_tape.record(self, pvars, device_limits=False)
            self._dyn_tape = (tape, outs + [rport], params)
        tape, outs, params = self._dyn_tape
        chan = next((i for i, (e, _) in enumerate(params) if e is self.per_sample_R), -1)
        rtape = self.__dict__.get("_dyn_rtape")
        if rtape is None:
            rtape = self._dyn_rtape = binding.RowsTape(*tape.packed(), outs)
        on_device = rtape.fits(len(params)) and len(rtape.ops) <= DYN_ROWS_MAX_OPS and not x.requires_grad
        # A pot that keeps its value along every sequence (the reference's recordings: dataimport.py:96 repeats the file's
        # resistance down the whole channel, batch_data cuts sequences out of it): calc_impedance gives ONE row per sequence --
        # the tape runs over B values instead of B x T, the kernels read rows [1,n,B] and the sweep sums dL/d(row) over the
        # steps itself.  Looked at once per input tensor (one comparison pass, cached on the storage: EntryCache holds the
        # caller's tensor, so no other data -- a pot that moves -- can land at its address while the answer is kept).
        per_seq = False
        if chan >= 0 and not x.requires_grad and T > 1 and getattr(self, "per_sequence_rows", True):
            cache = self.__dict__.setdefault("_dyn_chan_const", EntryCache(max_entries=8))
            per_seq = None if self._anchor is None else cache.get(self._anchor)
            if per_seq is None:
                with torch.no_grad():
                    rch = x[:, :, self.ni]
                    per_seq = bool((rch == rch[:, :1]).all())
                if self._anchor is not None:
                    cache.put(self._anchor, per_seq)
        vals = []
        for i, (e, n) in enumerate(params):
            if i == chan:
                # the resistance channel: [T,B] for the device tape, [B,T] float64 for torch's
                if per_seq:
                    vals.append(x[:, :1, self.ni].t().contiguous() if on_device else x[:, :1, self.ni].double())
                    continue
                vals.append(x[:, :, self.ni].t().contiguous() if on_device else x[:, :, self.ni].double())
            else:
                v = e.__dict__[n]
                v = v.as_subclass(torch.Tensor) if isinstance(v, torch.Tensor) else torch.tensor(float(v))
                vals.append(v.reshape(()).to(dev) if on_device else v.double().reshape(()).to(dev))
        with torch._C.DisableTorchFunctionSubclass():
            if on_device:
                # calc_impedance of every sample in one launch (csrc/wdf_ss_dyn_rows.h); the channel's slot gets a placeholder
                r = vals[chan].float() if chan >= 0 else None
                rows = _DynRowsFn.apply(rtape, chan, r, *[v if i != chan else v.new_zeros(()) for i, v in enumerate(vals)])
            else:
                # (a tape past the device evaluator's sizes, or a channel that wants its own gradient: torch runs the tape)
                nodes = tape.evaluate_torch(vals, outs)
                if self.per_sample_R is not None:
                    Tr = 1 if per_seq else T
                    rows = torch.stack([torch.broadcast_to(v, (B, Tr)) for v in nodes], dim=0)      # [n,B,T]
                    rows = rows.permute(2, 0, 1).float().contiguous()                                # [T,n,B] ([1,n,B]: per sequence)
                else:
                    rows = torch.stack([v.reshape(()) for v in nodes]).float()                       # one static row [n]
        hidden = n_tanh = 0
        n_up = n_down = 1
        if self.root_kind == "DiodePair":
            dp = self.root
            rootvec = torch.stack([dp.Is.as_subclass(torch.Tensor).double().reshape(()),
                                   dp.nVt.as_subclass(torch.Tensor).double().reshape(())]).to(device=dev, dtype=torch.float32)
            kind, n_up, n_down = binding.ROOT_DIODE_PAIR, dp.N_up, dp.N_down
        elif self.root_kind == "AsymDiodePair":
            # two different diodes (streamed=True): the four diode Variables; the port resistance is the row's last entry
            dp = self.root
            rootvec = torch.stack([v.as_subclass(torch.Tensor).double().reshape(()) for v in
                                   (dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down)]).to(device=dev, dtype=torch.float32)
            kind = binding.ROOT_ASYM_PAIR
        elif self.root_kind == "DenseRootModel":
            from . import mlp_root
            dense, hidden, n_tanh, act = mlp_root.describe(self.root, with_activation=True)
            if act != "tanh":
                raise binding.WdfHipError("the MLP root outside the clipper topology: tanh networks (the ReLU kernels are the "
                                          "clipper's resident step)")
            rootvec = mlp_root.flat_weights(dense).float().to(dev)
            kind = binding.ROOT_MLP
        else:
            rootvec, kind = None, binding.ROOT_NONE
        z0t = None if z0 is None else z0.as_subclass(torch.Tensor).to(dev).float().reshape(self.ns, -1).contiguous()
        xs = x[:, :, :self.ni].contiguous()
        tp = self._plan_dyn(tape, outs, vals, kind, B, T, xs=xs) if self.time_parallel == "auto" else \
            (self.time_parallel if isinstance(self.time_parallel, SsTpPlan) else None)
        warm = None
        if tp is not None and self.warm_start and self.ns >= 1 and z0t is None and isinstance(getattr(self, "_anchor", None), torch.Tensor):
            # the same batch again (a training loop: lpf.py:86-99 re-runs data_in every epoch) -> its chunks start warm
            wsd = self.__dict__.setdefault("_dyn_warm", EntryCache(max_entries=4))
            warm = wsd.get(self._anchor, kind)
            if warm is None:
                warm = wsd.put(self._anchor, DynWarmStart(T, B, self.ns, tp.k_bwd, tp.warmup if tp.warmup > 0 else 64, tp.tol), kind)
        y, zT = _SsDynFn.apply(rows, rootvec, xs, z0t, self.ns, self.ni, kind, hidden, n_tanh, n_up, n_down, bool(return_state), tp, warm)
        y = y.as_subclass(tf.Tensor)
        return (y, zT[:self.ns]) if return_state else y

    def _plan_dyn(self, tape, outs, vals, kind, B, T, tol=1.0e-6, xs=None):
        """SsTpPlan for the streamed-coefficient kernels (or None: the batch fills the chip / no state).  The reverse sweep is
        exact in chunks: as many as give every SIMD ~2 waves, none shorter than 64 steps.  The forward warms a chunk up from
        z = 0: W outlasts the slowest mode of the step's Jacobian A + Da E ca^T over the root's slope Da -- [-1, 1] for a diode
        pair (passive), for a network root what its weights give over the batch's amplitude (mlp_root.slope_range: a learned
        b(a) is not bounded by 1) -- taken at BOTH ends of the resistance channel (the tape evaluated at its smallest and largest
        value -- the adaptor coefficients are monotone in one resistance); every boundary is verified on the device whatever the
        estimate.  Re-derived every 32 calls (the components train slowly; a stale W costs a re-run of the waves that missed,
        never a wrong result)."""
        ns, ni = self.ns, self.ni
        if ns < 1:
            return None
        waves = max(1, -(-B // 64))
        k_max = min(T // 64, (2 * N_SIMD) // waves)
        if k_max < 2:
            return None
        cache = self.__dict__.setdefault("_dyn_plans", {})
        key = (B, T, kind)
        hit = cache.get(key)
        if hit is not None and hit[1] < 32:
            cache[key] = (hit[0], hit[1] + 1)
            return hit[0]
        with torch.no_grad(), torch._C.DisableTorchFunctionSubclass():
            ends = [[(v if v.dim() == 0 else sel(v)).double() for v in vals] for sel in (torch.amin, torch.amax)] \
                if self.per_sample_R is not None else [[v.double() for v in vals]]
            rho = 0.0
            for pv in ends:
                c = torch.stack([v.reshape(()) for v in tape.evaluate_torch(pv, outs)]).double().cpu().numpy()
                A = c[:ns * ns].reshape(ns, ns)
                oE = ns * ns + ns * ni
                E, ca = c[oE:oE + ns], c[oE + ns:oE + 2 * ns]
                if kind == binding.ROOT_NONE:
                    slopes = (0.0,)
                elif kind == binding.ROOT_MLP:
                    from . import mlp_root
                    # the a-range the network is asked about: four times the batch's largest input (the incident wave is
                    # ca.z + da.x, both of the input's order); one read-back per re-derivation
                    a_max = 4.0 * max(float(xs.abs().max()) if xs is not None else 1.0, 0.25)
                    s_lo, s_hi = mlp_root.slope_range(mlp_root.describe(self.root, with_activation=True)[0],
                                                      [math.log(max(float(c[-1]), 1e-30))], a_max)
                    slopes = tuple(np.linspace(s_lo, s_hi, 5))          # (the radius need not peak at an end of the range)
                else:
                    slopes = (1.0, -1.0)                                # (two different diodes too: Da = 2/F - 1, F >= 1)
                rho = max(rho, max(float(np.max(np.abs(np.linalg.eigvals(A + sgn * np.outer(E, ca))))) for sgn in slopes))
        k_fwd, W = 1, 0
        if rho < 1.0 - 1e-9:
            W = 8 if rho <= 0.0 else max(8, -(-int(math.ceil(math.log(0.01 * tol) / math.log(rho))) // 8) * 8)
            k_fwd = max(1, min(k_max, T // max(W, 64)))
        plan = SsTpPlan(k_fwd, W, float(tol), k_max)
        cache[key] = (plan, 0)
        return plan

    def _asym_inputs(self, x, anchor):
        """What the three AsymDiodePair paths share: theta6, the [B,T] input, the [B] pot vector (None without per_sequence_R) and
        the plan.  With a pot the input is [B,T,2] (clipper_pot.py:68-70: channel 1 is the pot), theta6[4] is a placeholder the
        kernels ignore (vs.R gets no gradient) and the plan comes from the LARGEST pot: it forgets slowest."""
        from . import engine
        dp, vs, cap = self.root, self.top.P1, self.top.P2
        pot = self.per_sequence_R is not None
        if x.dim() == 2:
            x = x.unsqueeze(-1)
        if x.dim() != 3 or x.shape[2] != (2 if pot else 1):
            raise binding.WdfHipError(("x must be [B,T,2] (Vin, R)" if pot else "x must be [B,T,1] (or [B,T] for one channel)")
                                      + f", got {tuple(x.shape)}")
        Rv = torch.tensor(1.0) if pot else (vs.R if isinstance(vs.R, torch.Tensor) else torch.tensor(float(vs.R)))
        parts = [dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down, Rv, cap.C]
        theta6 = self._theta(parts, x.device)
        xv, r = engine.split_channels(x, pot, anchor=anchor)
        rseq = binding.r_per_sequence(r) if pot else None
        tp = self.time_parallel
        if tp == "auto":
            R_plan = engine.resistance_max(r) if pot else float(parts[4])
            tp = engine.plan_asym_time_parallel(xv.shape[0], xv.shape[1], R_plan, float(parts[5]), float(cap.FS))
        elif not isinstance(tp, engine.TpPlan):
            tp = None
        return theta6, xv, rseq, tp

    def _run_clipper_asym(self, x, z0, return_state):
        """The clipper tree under an AsymDiodePair root: one launch of the two-different-diode loop (engine.clipper_asym) in the
        root's solver mode, gradients to the four diode Variables, R and C (with per_sequence_R: to the diodes and C)."""
        from . import engine
        theta6, xv, rseq, tp = self._asym_inputs(x, getattr(self, "_anchor", None))
        z0t = None if z0 is None else torch.as_tensor(z0).as_subclass(torch.Tensor)
        y, zT = engine.clipper_asym(theta6, xv, float(self.top.P2.FS), tp=tp, mode=self.root.mode, z0=z0t, return_state=True, r=rseq)
        y = y.as_subclass(tf.Tensor)
        return (y, zT.reshape(1, -1)) if return_state else y

    def _mse_clipper_asym(self, x, target, z0, stateful):
        """mse() on the clipper tree under an AsymDiodePair root with a Newton solver: forward, loss and the six gradients in
        one pass over the data (engine.clipper_asym_mse) -- no stash, no torch loss, no reverse sweep.  State in and out as
        the composed path handles it: z0 is a constant of the call, last_state / last_output are set on stateful calls.
        With per_sequence_R the same one-pass step with one pot per sequence (wdf_clipper_asym_step_mse_rseq)."""
        from . import engine
        anchor = x if isinstance(x, torch.Tensor) else None
        x = torch.as_tensor(x).as_subclass(torch.Tensor)
        x = (x if x.is_cuda else x.cuda()).float()
        theta6, xv, rseq, tp = self._asym_inputs(x, anchor)
        B, T = xv.shape
        fs, mode = float(self.top.P2.FS), self.root.mode
        tgt = torch.as_tensor(target).as_subclass(torch.Tensor).to(x.device).float().reshape(T, B).contiguous()
        z0t = None if z0 is None else torch.as_tensor(z0).as_subclass(torch.Tensor)
        if not stateful:
            return engine.clipper_asym_mse(theta6, xv, tgt, fs, tp=tp, mode=mode, r=rseq).as_subclass(tf.Tensor)
        loss, y, zT = engine.clipper_asym_mse(theta6, xv, tgt, fs, tp=tp, mode=mode, z0=z0t, return_state=True, r=rseq)
        self.last_state, self.last_output = zT.reshape(1, -1), y.as_subclass(tf.Tensor)
        return loss.as_subclass(tf.Tensor)

    def _mse_esr_clipper_asym(self, x, target, skip, z0, stateful):
        """mse_esr() on the clipper tree under an AsymDiodePair root with a Newton solver: forward, the loss sums S and E past
        `skip` and the six gradients in one pass over the data (engine.clipper_asym_mse_esr) -- no stash, no torch
        reductions, no reverse sweep.  State in and out as _mse_clipper_asym handles it; per_sequence_R likewise
        (wdf_clipper_asym_step_esr_rseq)."""
        from . import engine
        anchor = x if isinstance(x, torch.Tensor) else None
        x = torch.as_tensor(x).as_subclass(torch.Tensor)
        x = (x if x.is_cuda else x.cuda()).float()
        theta6, xv, rseq, tp = self._asym_inputs(x, anchor)
        B, T = xv.shape
        fs, mode = float(self.top.P2.FS), self.root.mode
        tgt = torch.as_tensor(target).as_subclass(torch.Tensor).to(x.device).float().reshape(T, B).contiguous()
        z0t = None if z0 is None else torch.as_tensor(z0).as_subclass(torch.Tensor)
        if not stateful:
            loss = engine.clipper_asym_mse_esr(theta6, xv, tgt, fs, skip=skip, tp=tp, mode=mode, r=rseq)
            self.last_output = engine._ClipperAsymEsrFn.stepper(B, T, fs, tp, mode, skip, xv.device,
                                                                pot=rseq is not None).y.as_subclass(tf.Tensor)
            return loss.as_subclass(tf.Tensor)
        loss, y, zT = engine.clipper_asym_mse_esr(theta6, xv, tgt, fs, skip=skip, tp=tp, mode=mode, z0=z0t, return_state=True, r=rseq)
        self.last_state, self.last_output = zT.reshape(1, -1), y.as_subclass(tf.Tensor)
        return loss.as_subclass(tf.Tensor)

    def _run_clipper(self, x, z0, return_state):
        from . import engine
        dp, vs, cap = self.root, self.top.P1, self.top.P2
        dev = x.device
        # a streamed pot resistance overrides the source's own R (which a recorded loop may have left symbolic)
        Rv = torch.tensor(1.0) if self.per_sample_R is not None else (vs.R if isinstance(vs.R, torch.Tensor) else torch.tensor(float(vs.R)))
        parts = [dp.Is, dp.nVt, Rv, cap.C]
        theta = self._theta(parts, dev)
        xv, r = engine.split_channels(x, self.per_sample_R is not None, anchor=getattr(self, "_anchor", None))
        if z0 is not None or return_state:
            z0t = None if z0 is None else z0.as_subclass(torch.Tensor).to(dev).float().reshape(-1).contiguous()
            y, zT = engine.clipper_stateful(theta, xv, float(cap.FS), r=r, n_up=dp.N_up, n_down=dp.N_down, z0=z0t)
            y = y.as_subclass(tf.Tensor)
            return (y, zT.reshape(1, -1)) if return_state else y
        tp = self.time_parallel
        if tp == "auto":
            # component values live on the host (tiny CPU variables): planning costs no sync
            # per-sample R: the warm-up must outlast the slowest (largest-R) sequence in the batch
            R_host, C_host = self._host_RC(parts)
            R_plan = R_host if r is None else engine.resistance_max(r)
            tp = engine.tuned_plan(theta, xv, r, float(cap.FS), R_plan, C_host, n_up=dp.N_up, n_down=dp.N_down,
                                   R_min=None if r is None else engine.resistance_min(r))
        y = engine.clipper(theta, xv, float(cap.FS), r=r, n_up=dp.N_up, n_down=dp.N_down, tp=tp)
        return y.as_subclass(tf.Tensor)
