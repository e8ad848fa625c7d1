"""Autograd glue: one torch.autograd.Function per fused sequence loop.

The forward call replaces the reference's whole per-sample Python loop
(clipper_pot.py:103-127) by one HIP launch; backward replaces tape.gradient over that loop
(clipper_pot.py:246-268) by one reverse-sweep launch.  torch only carries tensors between
the two and into the loss / optimizer.
"""
import math
from collections import namedtuple

import torch

from . import binding
from .tensor_cache import ObjectMemo

# ---- time-parallel plan -------------------------------------------------------------------
# k_fwd / warmup / tol: chunks, warm-up steps and verified tolerance of the speculative forward
# (csrc/wdf_clipper.h "Time-parallel variants"); k_bwd: chunks of the exact reverse sweep.
TpPlan = namedtuple("TpPlan", ["k_fwd", "warmup", "tol", "k_bwd"])

N_SIMD = 256 * 4          # MI355X: 256 CUs x 4 SIMDs


def plan_time_parallel(B, T, R, C, fs, tol=1.0e-6, time_major=False, R_min=None):
    """Choose chunk counts from the batch shape and the circuit's memory.  R: the source
    resistance; with a per-sample resistance pass the LARGEST value present and the smallest as
    R_min: the memory |1 - 2p| grows with R above Rc = 1/(2 C fs) and with 1/R below it, so the
    slowest sequence is at one of the two ends.

    Sequential mode gives ceil(B/64) waves for 1024 SIMDs, each a dependent chain (a dependent
    VALU op completes every ~3.3 ns on gfx950 where a SIMD could issue one every ~2 ns: tools/ubench).  The
    plan aims at ~2 waves per SIMD for the forward (every extra chunk costs a warm-up) and 4-8
    for the reverse sweep (no redundancy there; 8 when x is time-major, i.e. all loads coalesced).  The forward's warm-up must outlast the circuit's
    memory: with the diode off the state contracts by (1 - 2p) per sample (p = Rc/(R+Rc),
    Rc = 1/(2 C fs)); W is the number of steps that shrinks an O(10 V) error below 1e-7
    (measured miss at the headline circuit: 3e-8 against a verified tolerance of 1e-6).  If W would make chunks more than 2x redundant, fewer chunks are used; if
    even 2 chunks do not pay, the forward stays sequential (k_fwd = 1).  The verify kernel
    still guards every run, so a bad estimate costs time, never correctness.
    """
    waves = max(1, -(-B // 64))
    Rc = 1.0 / (2.0 * float(C) * float(fs))
    rho = max(abs(1.0 - 2.0 * Rc / (float(Rv) + Rc)) for Rv in ((R,) if R_min is None else (R, R_min)))
    if rho <= 0.0:
        W = 8
    elif rho >= 1.0 - 1e-9:
        W = T
    else:
        W = int(math.ceil(math.log(1.0e-8) / math.log(rho)))
    W = max(32, -(-W // 32) * 32)
    k_fwd = max(1, min((2 * N_SIMD) // waves, T // max(W, 64)))
    if k_fwd < 2:
        k_fwd = 1
    k_bwd = max(1, min(((8 if time_major else 4) * N_SIMD) // waves, T // 64))
    return TpPlan(k_fwd, W, float(tol), k_bwd)


def plan_asym_time_parallel(B, T, R, C, fs, tol=1.0e-6):
    """TpPlan for the two-different-diode clipper (csrc/wdf_asym.h); k_fwd = 1 (sequential forward) when T is too short for
    two warmed-up chunks.  Its
    kernels are one wave per 64 sequences and chunk like the symmetric pair's: the forward at ~2 waves per SIMD (a chunk
    re-runs `warmup` steps from z = 0, so more chunks cost more), the exact reverse sweep at ~4 (no redundancy); the
    warm-up outlasts the diode-off forgetting rate 1 - 2p, the slowest the state ever forgets (a conducting diode only
    forgets faster).  At 8192 x 4096 and 45 kOhm / 4.7 nF that is 16 forward chunks warmed up over 192 steps and 32
    reverse chunks: the fastest plan measured for every mode (profiles/r07_c5_asym_sweep.jsonl).  The forward verifies
    every chunk boundary on the device and re-runs what misses: a poor plan costs time, never correctness.  The one-pass
    step (AsymMseStep) takes k_fwd, warmup and tol from the same plan and ignores k_bwd: it has no reverse chunks."""
    return plan_time_parallel(B, T, R, C, fs, tol=tol)


_R_MAX_CACHE = ObjectMemo(256)      # tensor -> (max, min)


def _r_range(r):
    lo, hi = torch.aminmax(r)
    return _R_MAX_CACHE.put(r, (float(hi), float(lo)))


def resistance_max(r):
    """max of a per-sample resistance tensor: the planner needs the slowest sequence's memory.
    One device sync, cached per tensor OBJECT and version (a training set is the same tensor every
    epoch; a fresh tensor -- even one the allocator put at a recycled address -- is looked at again)."""
    return (_R_MAX_CACHE.get(r) or _r_range(r))[0]


def resistance_min(r):
    """min of a per-sample resistance tensor (same cache entry as resistance_max)."""
    return (_R_MAX_CACHE.get(r) or _r_range(r))[1]


_SPLIT_CACHE = ObjectMemo(64)      # (x, layout) -> (xv, r)


def split_channels(x, with_r, time_major=False, anchor=None):
    """The kernels' contiguous views of a [B,T,2] script input (Vin, R: clipper_pot.py:68-70):
    xv = x[..., 0] and r = x[..., 1], as [B,T] or -- time_major -- as [T,B].  Cached per input tensor
    object, version and layout: the reference feeds the same train_X every epoch
    (clipper_pot.py:245-248), so the de-interleaving (and transposing) copies and the planner's look
    at max R happen once, not per forward."""
    xt = x.as_subclass(torch.Tensor)
    if xt.dim() == 2:
        xt = xt.unsqueeze(-1)
    # the cache hangs on the object the CALLER holds (`anchor`: the tensor as the script passed it),
    # not on the normalised views made from it, which are new objects every call
    anchor = x if anchor is None else anchor
    hit = _SPLIT_CACHE.get(anchor, bool(time_major))
    if hit is None or (with_r and hit[1] is None):
        def chan(c):
            v = xt[:, :, c]
            return v.t().contiguous() if time_major else v.contiguous()
        hit = _SPLIT_CACHE.put(anchor, (chan(0), chan(1) if with_r else None), bool(time_major))
    return hit[0], (hit[1] if with_r else None)


LAST_TP_STATUS = {"status": None}     # device status word of the most recent time-parallel forward


class _ClipperFn(torch.autograd.Function):
    """y[T,B] = clipper(theta = {Is, nVt, R, C}, x[B,T] (, r[B,T]))."""

    @staticmethod
    def forward(ctx, theta, x, r, fs, n_up, n_down, time_major, tp):
        need_grad = theta.requires_grad
        th = theta.detach().contiguous()
        if tp is not None and not time_major and tp.k_fwd > 1:
            y, zs, _, st = binding.clipper_fwd_tp(x, th, fs, tp.k_fwd, tp.warmup, tp.tol, r=r, n_up=n_up,
                                                  n_down=n_down, want_stash=need_grad)
            LAST_TP_STATUS["status"] = st
        else:
            y, zs, _ = binding.clipper_fwd(x, th, fs, r=r, n_up=n_up, n_down=n_down, want_stash=need_grad,
                                           time_major=time_major)
        ctx.tp = tp if (tp is not None and not time_major) else None
        ctx.cfg = (fs, n_up, n_down, time_major)
        ctx.has_r = r is not None
        if need_grad:
            ctx.save_for_backward(th, x, zs, *([r] if r is not None else []))
        return y

    @staticmethod
    def backward(ctx, gy):
        fs, n_up, n_down, time_major = ctx.cfg
        saved = ctx.saved_tensors
        th, x, zs = saved[0], saved[1], saved[2]
        r = saved[3] if ctx.has_r else None
        if ctx.tp is not None and ctx.tp.k_bwd > 1:
            gtheta, _ = binding.clipper_bwd_tp(x, th, fs, zs, gy.contiguous(), ctx.tp.k_bwd, r=r, n_up=n_up,
                                               n_down=n_down)
        else:
            gtheta, _ = binding.clipper_bwd(x, th, fs, zs, gy.contiguous(), r=r, n_up=n_up, n_down=n_down,
                                            time_major=time_major)
        return gtheta, None, None, None, None, None, None, None


def clipper(theta, x, fs, r=None, n_up=1, n_down=1, time_major=False, tp=None):
    """Diode-clipper sequence loop on the GPU.  theta: float32[4] = {Is, nVt, R, C} on the
    device (may require grad); x, r: [B,T] (or [T,B] when time_major).  Returns y [T,B].
    tp: a TpPlan (plan_time_parallel) to run the time-parallel kernels, None = sequential."""
    return _ClipperFn.apply(theta, x, r, float(fs), int(n_up), int(n_down), bool(time_major), tp)


class _ClipperStatefulFn(torch.autograd.Function):
    """(y[T,B], zT[B]) = clipper(theta, x (, r), z0[B]): the sequential kernels with the capacitor
    state handed in and out -- lpf.py-style loops that never call reset() carry it from one
    forward() to the next -- differentiable w.r.t. theta and z0 (gradients flow back through zT)."""

    @staticmethod
    def forward(ctx, theta, x, r, z0, fs, n_up, n_down):
        th = theta.detach().contiguous()
        z0d = None if z0 is None else z0.detach().contiguous()
        need = theta.requires_grad or (z0 is not None and z0.requires_grad)
        y, zs, zT = binding.clipper_fwd(x, th, fs, r=r, n_up=n_up, n_down=n_down, want_stash=need, z0=z0d, want_zT=True)
        ctx.cfg = (fs, n_up, n_down)
        ctx.has_r, ctx.has_z0 = r is not None, z0 is not None
        if need:
            ctx.save_for_backward(th, x, zs, *([r] if r is not None else []))
        return y, zT

    @staticmethod
    def backward(ctx, gy, gzT):
        fs, n_up, n_down = ctx.cfg
        saved = ctx.saved_tensors
        th, x, zs = saved[0], saved[1], saved[2]
        r = saved[3] if ctx.has_r else None
        T, B = zs.shape
        gy = torch.zeros((T, B), dtype=torch.float32, device=x.device) if gy is None else gy.contiguous()
        gtheta, gz0 = binding.clipper_bwd(x, th, fs, zs, gy, r=r, n_up=n_up, n_down=n_down, want_gz0=True,
                                          gzT=None if gzT is None else gzT.contiguous())
        return gtheta, None, None, (gz0 if ctx.has_z0 else None), None, None, None


def clipper_stateful(theta, x, fs, r=None, n_up=1, n_down=1, z0=None):
    """Diode-clipper loop with explicit capacitor state: -> (y [T,B], zT [B]).  z0 [B] or None (reset)."""
    return _ClipperStatefulFn.apply(theta, x, r, z0, float(fs), int(n_up), int(n_down))


class _ClipperAsymFn(torch.autograd.Function):
    """(y [T,B], zT [B]) = clipper with two different antiparallel diodes, differentiable w.r.t.
    theta6 = {Is_up, nVt_up, Is_down, nVt_down, R, C} (csrc/wdf_asym.h).  mode: Newton on the exact Shockley pair in fp64
    (default) or in fp32, or the fp32 Wright-omega closed form (a model approximation) -- each differentiates its own forward.
    The reverse sweep is the time-parallel one (no root re-solve, chunks composed exactly: wdf_clipper_asym_bwd_tp) unless tp
    says k_bwd = 0, which keeps the sequential Newton-re-solving sweep (wdf_clipper_asym_bwd; fp64 Newton mode only: the
    other modes then run the time-parallel sweep with one chunk).  z0 is a constant of the call, zT comes back detached."""

    @staticmethod
    def forward(ctx, theta6, x, fs, tol, max_iter, tp, mode, z0, rseq=None):
        th = theta6.detach().contiguous()
        # rseq: one pot per sequence (the *_rseq entry points): theta6[4] is ignored
        if tp is not None and tp.k_fwd > 1:      # time chunks, verified on the device (wdf_clipper_asym_fwd_tp)
            y, zT, zs, st = binding.clipper_asym_fwd_tp(x, th, fs, mode, tp.k_fwd, tp.warmup, tol=tol, max_iter=max_iter,
                                                        verify_tol=tp.tol, z0=z0, want_stash=True, want_zT=True, rseq=rseq)
            LAST_TP_STATUS["status"] = st
        else:
            y, zT, _, zs = binding.clipper_asym_fwd(x, th, fs, mode, tol=tol, max_iter=max_iter, z0=z0, want_stash=True,
                                                    want_zT=True, rseq=rseq)
        B, T = x.shape
        if tp is not None:
            k_bwd = int(tp.k_bwd)
        else:                                    # as many chunks as give every SIMD ~2 waves, none shorter than 64 steps
            k_bwd = max(1, min(T // 64, (2 * N_SIMD) // max(1, -(-B // 64))))
        ctx.cfg = (fs, tol, max_iter, mode, k_bwd)
        ctx.save_for_backward(th, x, zs, zT, *([rseq] if rseq is not None else []))
        ctx.mark_non_differentiable(zT)
        return y, zT

    @staticmethod
    def backward(ctx, gy, _gzT):
        fs, tol, max_iter, mode, k_bwd = ctx.cfg
        th, x, zs, zT = ctx.saved_tensors[:4]
        if len(ctx.saved_tensors) > 4:           # a pot per sequence: the time-parallel sweep (one exact chunk at the least)
            g = binding.clipper_asym_bwd_tp_rseq(x, ctx.saved_tensors[4], th, fs, mode, zs, zT, gy.contiguous(), max(1, k_bwd))
        elif k_bwd < 1 and mode == binding.ASYM_NEWTON_F64:
            g = binding.clipper_asym_bwd(x, th, fs, zs, gy.contiguous(), tol=tol, max_iter=max_iter)
        else:
            g = binding.clipper_asym_bwd_tp(x, th, fs, mode, zs, zT, gy.contiguous(), max(1, k_bwd))
        return g, None, None, None, None, None, None, None, None


def _z0_of(z0, x):
    """z0: None or the state [B] a two-different-diode call starts from -> None or that state detached, float32 and flat on x's device."""
    if z0 is None:
        return None
    z0 = z0.detach().to(device=x.device, dtype=torch.float32).reshape(-1).contiguous()
    if z0.numel() != x.shape[0]:
        raise binding.WdfHipError(f"z0 must hold one state per sequence ({x.shape[0]}), got {z0.numel()}")
    return z0


def _rseq_of(r, x):
    """r: None, a pot channel [B,T] or its [B] vector -> None or the [B] vector the *_rseq entry points take."""
    if r is None:
        return None
    if r.dim() == 2:
        r = binding.r_per_sequence(r)
    if r.dim() != 1 or r.numel() != x.shape[0]:
        raise binding.WdfHipError(f"r must hold one resistance per sequence ([{x.shape[0]}], or a [B,T] channel constant along T), "
                                  f"got {tuple(r.shape)}")
    return r.detach().to(device=x.device, dtype=torch.float32).contiguous()


def clipper_asym(theta6, x, fs, tol=1.0e-12, max_iter=50, tp=None, mode=None, z0=None, return_state=False, r=None):
    """Two-different-diode clipper loop (BASELINE config 5) with gradients to all six parameters.
    mode: binding.ASYM_NEWTON_F64 (default: the exact model in fp64), binding.ASYM_NEWTON_F32 (the exact model in fp32: the
    fast one; tol is floored at 4 FLT_EPSILON) or binding.ASYM_OMEGA_F32 (the fp32 closed form: a model approximation, kept
    for comparison).
    tp: a TpPlan (plan_asym_time_parallel with the circuit's R, C) -> the forward runs in k_fwd verified time chunks and the
    reverse sweep in k_bwd exact ones (k_bwd = 0: the sequential sweep, fp64 Newton mode; one exact chunk otherwise).
    z0 [B]: the capacitor state the loop starts from (default zero), a constant of the call: no gradient flows into it.
    return_state: -> (y, zT), zT [B] the state the loop ended in, detached.
    r: one pot resistance per sequence -- [B], or a [B,T] channel constant along T (binding.r_per_sequence) -- in place of
    theta6[4], which is then ignored and receives a zero gradient (Newton modes; plan with engine.resistance_max(r))."""
    mode = binding.ASYM_NEWTON_F64 if mode is None else int(mode)
    z0 = _z0_of(z0, x)
    if r is not None:
        y, zT = _ClipperAsymFn.apply(theta6, x, float(fs), float(tol), int(max_iter), tp, mode, z0, _rseq_of(r, x))
    else:
        y, zT = _ClipperAsymFn.apply(theta6, x, float(fs), float(tol), int(max_iter), tp, mode, z0)
    return (y, zT) if return_state else y


class AsymMseStep:
    """The MSE training step of the two-different-diode clipper in one pass over the data (csrc/wdf_asym_step.h,
    binding.clipper_asym_step_mse): forward, loss and gradient in one sweep, x [B,T] and target [T,B] read once, y written
    once, no stash, no dL/dy array, no reverse sweep.  Buffers are allocated once; step_fused() returns device tensors
    (sse[1], gtheta6[6]) -- views of self.out = {sse, dIs_up, dnVt_up, dIs_down, dnVt_down, dR, dC}, the sum of squared errors
    of THIS batch and d(mean over n_global)/dtheta6 -- and nothing synchronises.  tp: a TpPlan (plan_asym_time_parallel;
    k_bwd is ignored: the step has no reverse chunks) or None for one chunk.  mode: binding.ASYM_NEWTON_F32 (default) or
    binding.ASYM_NEWTON_F64; the closed form (a model approximation) has no one-pass step."""

    def __init__(self, B, T, fs, tp, device, mode=None, n_global=None, tol=1.0e-12, max_iter=50):
        self.mode = binding.ASYM_NEWTON_F32 if mode is None else int(mode)
        if self.mode not in (binding.ASYM_NEWTON_F32, binding.ASYM_NEWTON_F64):
            raise binding.WdfHipError(f"AsymMseStep: mode {self.mode} has no one-pass step (the Newton modes have)")
        self.B, self.T, self.fs, self.tp = int(B), int(T), float(fs), tp
        self.tol, self.max_iter = float(tol), int(max_iter)
        self.n_global = float(n_global if n_global is not None else self.B * self.T)
        self.gscale = 2.0 / self.n_global
        k, self.warmup, self.verify_tol = (tp.k_fwd, tp.warmup, tp.tol) if tp is not None else (1, 0, 1.0e-6)
        self.k = binding.asym_chunks(self.T, k)
        self.ws = torch.empty((binding.lib().wdf_clipper_asym_step_mse_ws_bytes(self.B, self.k),), dtype=torch.uint8, device=device)
        self.status = torch.zeros((4,), dtype=torch.int32, device=device)
        self.out = torch.zeros((7,), dtype=torch.float32, device=device)      # {sse, gtheta6}
        self.sse, self.gtheta = self.out[0:1], self.out[1:7]
        self.y = torch.empty((self.T, self.B), dtype=torch.float32, device=device)
        self.zT = None

    def step_fused(self, theta6, x, target, adam=None, z0=None, want_zT=False, r=None):
        """adam: a binding.Adam(6, ...) to update theta6 in the step's own last launch; otherwise the caller applies its
        optimizer to self.gtheta.  z0 [B]: the state the call starts from, a constant of it; want_zT: self.zT <- the state
        it ends in.  r [B]: one pot resistance per sequence in place of theta6[4] (dR is then exactly 0 and adam never writes
        theta6[4]; the stepper's plan must come from the largest pot).  Fills self.y, self.out, self.status."""
        kw = dict(tol=self.tol, max_iter=self.max_iter, verify_tol=self.verify_tol, y=self.y, z0=z0, want_zT=want_zT, ws=self.ws,
                  status=self.status, out7=self.out, opt=adam)
        _, self.zT, _, _ = binding.clipper_asym_step_mse(x, theta6, self.fs, self.mode, target, self.gscale, self.k, self.warmup, rseq=r,
                                                         **kw)
        return self.sse, self.gtheta


class _ClipperAsymMseFn(torch.autograd.Function):
    """mean((clipper_asym(theta6, x) - target)^2) as the one-pass step (AsymMseStep.step_fused; one stepper per shape, buffers
    reused); backward only scales the stored gradient.  keep: -> (loss, y [T,B], zT [B]), the call's own output and final
    state, detached; otherwise the loss alone (y stays in the stepper's buffer: no copy)."""
    _steppers = {}

    @staticmethod
    def forward(ctx, theta6, x, target, fs, tp, mode, z0, keep, rseq=None):
        B, T = x.shape
        key = (B, T, float(fs), tp, mode, x.device, rseq is not None)
        st = _ClipperAsymMseFn._steppers.get(key)
        if st is None:
            if len(_ClipperAsymMseFn._steppers) > 8:
                _ClipperAsymMseFn._steppers.clear()
            st = _ClipperAsymMseFn._steppers[key] = AsymMseStep(B, T, fs, tp, x.device, mode=mode)
        LAST_TP_STATUS["status"] = st.status
        st.step_fused(theta6.detach().contiguous(), x, target, z0=z0, want_zT=keep, r=rseq)
        out = st.out.clone()
        ctx.save_for_backward(out)
        if not keep:
            return out[0] / float(B * T)
        y, zT = st.y.clone(), st.zT        # (the stepper's y is overwritten by the next call of this shape)
        ctx.mark_non_differentiable(y, zT)
        return out[0] / float(B * T), y, zT

    @staticmethod
    def backward(ctx, gl, *_):
        (out,) = ctx.saved_tensors
        return gl * out[1:7], None, None, None, None, None, None, None, None


def clipper_asym_mse(theta6, x, target, fs, tp=None, mode=None, z0=None, return_state=False, r=None):
    """Scalar mean-squared error of the two-different-diode clipper's output against target [T,B], differentiable w.r.t.
    theta6 = {Is_up, nVt_up, Is_down, nVt_down, R, C} (float32[6] on the device), as ONE pass over the data
    (wdf_clipper_asym_step_mse): no stash, no torch loss temporaries, no reverse sweep.  mode: binding.ASYM_NEWTON_F32
    (default) or binding.ASYM_NEWTON_F64.  tp: a TpPlan (plan_asym_time_parallel) or None for one chunk.
    z0 [B]: the state the loop starts from, a constant of the call.
    r: one pot resistance per sequence ([B], or a [B,T] channel constant along T) in place of theta6[4], as in clipper_asym.
    -> loss, or (loss, y [T,B], zT [B]) with return_state: the call's output and final state, detached."""
    mode = binding.ASYM_NEWTON_F32 if mode is None else int(mode)
    z0 = _z0_of(z0, x)
    if r is not None:
        return _ClipperAsymMseFn.apply(theta6, x, target, float(fs), tp, mode, z0, bool(return_state), _rseq_of(r, x))
    return _ClipperAsymMseFn.apply(theta6, x, target, float(fs), tp, mode, z0, bool(return_state))


class AsymGnStep:
    """The Gauss-Newton form of AsymMseStep (csrc/wdf_asym_gn.h, binding.clipper_asym_step_gn): the same one pass over the
    data, which also sums the products of the output's tangents.  Buffers are allocated once; run() fills self.y, self.status
    and self.out = {sse, g[6], H[21]} (g the gradient of the mean over n_global, H = (2/n_global) J^T J, upper triangle) and
    nothing synchronises.  tp, mode: as AsymMseStep (the MSE step's plan: plan_asym_time_parallel)."""

    def __init__(self, B, T, fs, tp, device, mode=None, n_global=None, tol=1.0e-12, max_iter=50):
        self.mode = binding.ASYM_NEWTON_F32 if mode is None else int(mode)
        if self.mode not in (binding.ASYM_NEWTON_F32, binding.ASYM_NEWTON_F64):
            raise binding.WdfHipError(f"AsymGnStep: mode {self.mode} has no one-pass step (the Newton modes have)")
        self.B, self.T, self.fs, self.tp = int(B), int(T), float(fs), tp
        self.tol, self.max_iter = float(tol), int(max_iter)
        self.n_global = float(n_global if n_global is not None else self.B * self.T)
        self.gscale = 2.0 / self.n_global
        k, self.warmup, self.verify_tol = (tp.k_fwd, tp.warmup, tp.tol) if tp is not None else (1, 0, 1.0e-6)
        self.k = binding.asym_chunks(self.T, k)
        self.ws = torch.empty((binding.lib().wdf_clipper_asym_step_gn_ws_bytes(self.B, self.k),), dtype=torch.uint8, device=device)
        self.status = torch.zeros((4,), dtype=torch.int32, device=device)
        self.out = torch.zeros((28,), dtype=torch.float32, device=device)     # {sse, g[6], H[21]}
        self.y = torch.empty((self.T, self.B), dtype=torch.float32, device=device)

    def run(self, theta6, x, target):
        binding.clipper_asym_step_gn(x, theta6, self.fs, self.mode, target, self.gscale, self.k, self.warmup, tol=self.tol,
                                     max_iter=self.max_iter, verify_tol=self.verify_tol, y=self.y, ws=self.ws, status=self.status,
                                     out28=self.out)
        return self.out


_GN_STEPPERS = {}


def clipper_asym_gn(theta6, x, target, fs, tp=None, mode=None):
    """Loss, gradient and Gauss-Newton matrix of the two-different-diode clipper's mean squared error against target [T,B], in
    ONE pass over the data (wdf_clipper_asym_step_gn; one stepper per shape, buffers reused).  theta6 = {Is_up, nVt_up,
    Is_down, nVt_down, R, C}, float32[6] on the device.  mode: binding.ASYM_NEWTON_F32 (default) or binding.ASYM_NEWTON_F64.
    tp: a TpPlan (plan_asym_time_parallel) or None for one chunk.  Stateless: the loop starts from zero.
    -> loss (0-dim), g [6], H [6,6] symmetric, all float64 and detached, and y [T,B] -- the stepper's own buffer, overwritten
    by the next call of this shape."""
    mode = binding.ASYM_NEWTON_F32 if mode is None else int(mode)
    B, T = x.shape
    key = (B, T, float(fs), tp, mode, x.device)
    st = _GN_STEPPERS.get(key)
    if st is None:
        if len(_GN_STEPPERS) > 8:
            _GN_STEPPERS.clear()
        st = _GN_STEPPERS[key] = AsymGnStep(B, T, fs, tp, x.device, mode=mode)
    LAST_TP_STATUS["status"] = st.status
    out = st.run(theta6.detach().contiguous(), x, target).to(torch.float64)
    return out[0] / float(B * T), out[1:7], binding.gn_matrix(out[7:28]), st.y


class AsymEsrStep:
    """The MSE + ESR training step of the two-different-diode clipper in one pass over the data (csrc/wdf_asym_step.h,
    binding.clipper_asym_step_esr): loss = S/n + sqrt(S / (E + eps) / n) on the rows past `skip` (clipper_pot.py:146-156,177,
    232,248), S = sum (y - target)^2, E = sum y^2, n = n_global (default: the rows counted x B).  Buffers are allocated once;
    step_fused() returns device tensors (loss3[3] = {mse, esr, mse + esr}, gtheta6[6] = d(mse + esr)/dtheta6) and nothing
    synchronises; self.sums = {S, E, gP[6], gQ[6]} of this batch is what several ranks all-reduce (finish=False leaves loss3
    and gtheta6 alone: binding.asym_esr_finish forms them from the global sums).  tp, mode: as AsymMseStep."""

    def __init__(self, B, T, fs, tp, device, mode=None, skip=0, n_global=None, eps_energy=None, tol=1.0e-12, max_iter=50):
        self.mode = binding.ASYM_NEWTON_F32 if mode is None else int(mode)
        if self.mode not in (binding.ASYM_NEWTON_F32, binding.ASYM_NEWTON_F64):
            raise binding.WdfHipError(f"AsymEsrStep: mode {self.mode} has no one-pass step (the Newton modes have)")
        self.B, self.T, self.fs, self.tp, self.skip = int(B), int(T), float(fs), tp, int(skip)
        if not 0 <= self.skip < self.T:
            raise binding.WdfHipError(f"AsymEsrStep: skip must be in 0..T-1 = 0..{self.T - 1}, got {self.skip}")
        self.tol, self.max_iter = float(tol), int(max_iter)
        self.n_global = float(n_global if n_global is not None else self.B * (self.T - self.skip))
        self.eps_energy = float(torch.finfo(torch.float64).eps if eps_energy is None else eps_energy)
        k, self.warmup, self.verify_tol = (tp.k_fwd, tp.warmup, tp.tol) if tp is not None else (1, 0, 1.0e-6)
        self.k = binding.asym_chunks(self.T, k)
        self.ws = torch.empty((binding.lib().wdf_clipper_asym_step_esr_ws_bytes(self.B, self.k),), dtype=torch.uint8, device=device)
        self.status = torch.zeros((4,), dtype=torch.int32, device=device)
        self.sums = torch.zeros((14,), dtype=torch.float32, device=device)     # {S, E, gP[6], gQ[6]}
        self.gtheta = torch.zeros((6,), dtype=torch.float32, device=device)
        self.loss3 = torch.zeros((3,), dtype=torch.float32, device=device)     # {mse, esr, mse + esr}
        self.y = torch.empty((self.T, self.B), dtype=torch.float32, device=device)
        self.zT = None

    def step_fused(self, theta6, x, target, adam=None, z0=None, want_zT=False, finish=True, r=None):
        """adam: a binding.Adam(6, ...) to update theta6 in the step's own last launch; otherwise the caller applies its
        optimizer to self.gtheta.  z0 [B]: the state the call starts from, a constant of it; want_zT: self.zT <- the state
        it ends in.  r [B]: one pot resistance per sequence in place of theta6[4], as in AsymMseStep.step_fused.
        Fills self.y, self.sums, self.status and -- finish -- self.loss3, self.gtheta."""
        kw = dict(tol=self.tol, max_iter=self.max_iter, verify_tol=self.verify_tol, y=self.y, z0=z0, want_zT=want_zT, ws=self.ws,
                  status=self.status, sums14=self.sums, gtheta6=self.gtheta, loss3=self.loss3, finish=finish, opt=adam)
        self.zT = binding.clipper_asym_step_esr(x, theta6, self.fs, self.mode, target, self.n_global, self.eps_energy, self.skip,
                                                self.k, self.warmup, rseq=r, **kw)[1]
        return self.loss3, self.gtheta


class _ClipperAsymEsrFn(torch.autograd.Function):
    """MSE + ESR of clipper_asym(theta6, x) against target past `skip` as the one-pass step (AsymEsrStep.step_fused; one
    stepper per shape, buffers reused); backward only scales the stored gradient.  keep: -> (loss, y [T,B], zT [B]), the
    call's own output and final state, detached; otherwise the loss alone (y stays in the stepper's buffer: no copy)."""
    _steppers = {}

    @staticmethod
    def stepper(B, T, fs, tp, mode, skip, device, pot=False):
        key = (B, T, float(fs), tp, mode, int(skip), device, bool(pot))
        st = _ClipperAsymEsrFn._steppers.get(key)
        if st is None:
            if len(_ClipperAsymEsrFn._steppers) > 8:
                _ClipperAsymEsrFn._steppers.clear()
            st = _ClipperAsymEsrFn._steppers[key] = AsymEsrStep(B, T, fs, tp, device, mode=mode, skip=skip)
        return st

    @staticmethod
    def forward(ctx, theta6, x, target, fs, skip, tp, mode, z0, keep, rseq=None):
        B, T = x.shape
        st = _ClipperAsymEsrFn.stepper(B, T, fs, tp, mode, skip, x.device, pot=rseq is not None)
        LAST_TP_STATUS["status"] = st.status
        st.step_fused(theta6.detach().contiguous(), x, target, z0=z0, want_zT=keep, r=rseq)
        ctx.save_for_backward(st.gtheta.clone())
        loss = st.loss3[2].clone()
        if not keep:
            return loss
        y, zT = st.y.clone(), st.zT        # (the stepper's y is overwritten by the next call of this shape)
        ctx.mark_non_differentiable(y, zT)
        return loss, y, zT

    @staticmethod
    def backward(ctx, gl, *_):
        (g,) = ctx.saved_tensors
        return gl * g, None, None, None, None, None, None, None, None, None


def clipper_asym_mse_esr(theta6, x, target, fs, skip=0, tp=None, mode=None, z0=None, return_state=False, r=None):
    """The scripts' training loss (clipper_pot.py:146-156,177: mean((y - t)^2) + sqrt(sum((y - t)^2) / (sum(y^2) + eps) / n)
    on the rows past `skip`) of the two-different-diode clipper's output against target [T,B], differentiable w.r.t.
    theta6 = {Is_up, nVt_up, Is_down, nVt_down, R, C} (float32[6] on the device), as ONE pass over the data
    (wdf_clipper_asym_step_esr): no stash, no torch reductions, no reverse sweep.  mode: binding.ASYM_NEWTON_F32
    (default) or binding.ASYM_NEWTON_F64.  tp: a TpPlan (plan_asym_time_parallel) or None for one chunk.
    z0 [B]: the state the loop starts from, a constant of the call.
    r: one pot resistance per sequence ([B], or a [B,T] channel constant along T) in place of theta6[4], as in clipper_asym.
    -> loss, or (loss, y [T,B], zT [B]) with return_state: the call's output and final state, detached."""
    mode = binding.ASYM_NEWTON_F32 if mode is None else int(mode)
    z0 = _z0_of(z0, x)
    if r is not None:
        return _ClipperAsymEsrFn.apply(theta6, x, target, float(fs), int(skip), tp, mode, z0, bool(return_state), _rseq_of(r, x))
    return _ClipperAsymEsrFn.apply(theta6, x, target, float(fs), int(skip), tp, mode, z0, bool(return_state))


class MseStep:
    """Fused training step for the mean-squared-error loss (lpf.py:78, clipper_pot.py:176):
    forward, loss and reverse sweep in two kernel launches + three tiny ones, all buffers
    preallocated.  step() returns device tensors (sse[1], gtheta[4]): the sum of squared errors
    over THIS batch and d(mean over n_global)/d{Is, nVt, R, C}; nothing synchronises.

    time_major: x (and r) are [T,B] -- the layout an engine keeps its training inputs resident
    in (one transpose when the dataset is loaded; the reference trains on the same train_X
    for all 501 epochs, clipper_pot.py:245-248), giving fully coalesced loads."""

    def __init__(self, B, T, fs, tp, device, n_up=1, n_down=1, n_global=None, time_major=False, loss="mse",
                 skip=0, sums_allreduce=None, warm=False, max_warm_tiles=16, store_output=True):
        """loss: "mse" (mean over n_global samples) or "mse+esr", the training loss of
        clipper_pot.py:177 evaluated past `skip` samples (:232,248; n_global then counts the samples
        past skip over all ranks).  sums_allreduce: in-place SUM all-reduce for the two float64 loss
        sums when the batch is sharded (wdf_hip.dist.allreduce_sum_).
        warm: this stepper always sees the SAME resident x (a training set re-visited every epoch,
        clipper_pot.py:245-269): keep the forward's warm-start state between calls
        (binding.TpWarmState; call reset_warm() if x changes).
        store_output=False: a training-only stepper -- step_fused runs the one-pass step without the y store (8 B/sample
        instead of 12) and allocates no y (self.y stays None), single-rank and with sums_allreduce; forward() / backward() /
        step(), the two-kernel path that needs y and the stash, raise WdfHipError."""
        if loss not in ("mse", "mse+esr"):
            raise binding.WdfHipError(f"unknown loss {loss!r}")
        if loss == "mse" and skip:
            raise binding.WdfHipError("skip is only meaningful with loss='mse+esr'")
        self.B, self.T, self.fs, self.tp = B, T, float(fs), tp
        self.n_up, self.n_down, self.time_major = n_up, n_down, bool(time_major)
        self.loss_kind, self.skip, self.sums_allreduce = loss, int(skip), sums_allreduce
        self.store_output = bool(store_output)
        self.n_global = float(n_global if n_global is not None else B * (T - self.skip))
        self.gscale = 2.0 / self.n_global
        if loss == "mse+esr":
            self.ws_l = torch.empty((binding.lib().wdf_loss_sums_ws_bytes(),), dtype=torch.uint8, device=device)
            self.sums = torch.zeros((2,), dtype=torch.float64, device=device)
            self.gcoef = torch.zeros((2,), dtype=torch.float32, device=device)
            self.loss = torch.zeros((3,), dtype=torch.float32, device=device)      # mse, esr, mse + esr
            self.sums10 = torch.zeros((10,), dtype=torch.float32, device=device)   # one-pass step: {S, E, gP[4], gQ[4]}
        L = binding.lib()
        kf, kb = (tp.k_fwd, tp.k_bwd) if tp is not None else (1, 1)
        self.ws_f = torch.empty((max(16, L.wdf_clipper_fwd_tp_ws_bytes(B, kf)),), dtype=torch.uint8, device=device)
        self.ws_b = binding.bwd_tp_workspace(B, kb, device)
        self.status = torch.zeros((4,), dtype=torch.int32, device=device)
        # one fused buffer [sse, dIs, dnVt, dR, dC]: it is also the all-reduce payload
        self.out = torch.zeros((5,), dtype=torch.float32, device=device)
        self.sse, self.gtheta = self.out[0:1], self.out[1:5]
        self.y = self.zs = self.zT = None
        self.ws_s, self.ws_s_k = None, None          # workspace of step_fused (made on first use)
        self.ws_e, self.ws_e_k = None, None          # workspace of eval_fused (its own, made on first use)
        self.sums_eval = self.loss_eval = None       # eval_fused: {S, E} (float64, the all-reduce payload), {mse, esr, mse + esr}
        self.warm = None
        if warm and tp is not None and tp.k_fwd > 1:
            self.warm = binding.TpWarmState(B, T, tp.k_fwd, max(max_warm_tiles, -(-tp.warmup // binding.warm_unit())), device)

    def reset_warm(self):
        if self.warm is not None:
            self.warm.reset()

    def _needs_output(self, what):
        if not self.store_output:
            raise binding.WdfHipError(f"MseStep.{what}: made with store_output=False (no y, no stash): only step_fused runs")

    def forward(self, theta, x, r=None):
        self._needs_output("forward")
        tp = self.tp
        if tp is not None and tp.k_fwd > 1:
            self.y, self.zs, self.zT, _ = binding.clipper_fwd_tp(
                x, theta, self.fs, tp.k_fwd, tp.warmup, tp.tol, r=r, n_up=self.n_up, n_down=self.n_down,
                want_zT=True, ws=self.ws_f, status=self.status, time_major=self.time_major, state=self.warm)
        else:
            self.y, self.zs, self.zT = binding.clipper_fwd(x, theta, self.fs, r=r, n_up=self.n_up,
                                                           n_down=self.n_down, want_zT=True,
                                                           time_major=self.time_major)
        return self.y

    def backward(self, theta, x, target, r=None, adam=None):
        """adam: a binding.Adam(4, ...) to update theta in the sweep's own last kernel (single rank,
        MSE loss); otherwise the caller applies its optimizer to self.gtheta afterwards."""
        self._needs_output("backward")
        kb = self.tp.k_bwd if self.tp is not None else 1
        if adam is not None and self.loss_kind == "mse":
            binding.clipper_bwd_mse_tp_adam(x, theta, self.fs, self.zs, self.zT, target, self.gscale, kb, adam, r=r,
                                            n_up=self.n_up, n_down=self.n_down, gtheta=self.gtheta, sse=self.sse,
                                            ws=self.ws_b, time_major=self.time_major)
            return self.sse, self.gtheta
        if self.loss_kind == "mse+esr":
            # loss sums over this rank's y (one streaming pass), made global, then the two
            # coefficients of dL/dy = ga (y - t) + gb y; the sweep itself is the MSE one
            binding.loss_sums(self.y, target, self.skip, sums=self.sums, ws=self.ws_l)
            if self.sums_allreduce is not None:
                self.sums_allreduce(self.sums)
            binding.esr_coef(self.sums, self.n_global, float(torch.finfo(torch.float64).eps), self.gcoef, self.loss)
            binding.clipper_bwd_esr_tp(x, theta, self.fs, self.zs, self.zT, target, self.gcoef, self.skip, kb, r=r,
                                       n_up=self.n_up, n_down=self.n_down, gtheta=self.gtheta, sse=self.sse,
                                       ws=self.ws_b, time_major=self.time_major)
            return self.sse, self.gtheta
        binding.clipper_bwd_mse_tp(x, theta, self.fs, self.zs, self.zT, target, self.gscale, kb, r=r,
                                   n_up=self.n_up, n_down=self.n_down, gtheta=self.gtheta, sse=self.sse,
                                   ws=self.ws_b, time_major=self.time_major)
        return self.sse, self.gtheta

    def step(self, theta, x, target, r=None):
        self._needs_output("step")
        self.forward(theta, x, r)
        return self.backward(theta, x, target, r)

    def step_fused(self, theta, x, target, r=None, adam=None):
        """The same step in ONE pass over the data (csrc/wdf_clipper_fused.h): forward, loss and gradient with x and target
        read once and y written once -- no state stash, one root solve per sample, the gradient carried forward as the
        state's tangent.  Chunking / verification / warm start as forward(); fills self.y, self.sse, self.gtheta (for
        "mse+esr" also self.loss = {mse, esr, mse + esr}) and, with `adam` on a single rank, updates theta in the same launch.
        (store_output=False: y is neither written nor allocated, self.y is None.)
        With sums_allreduce set (sharded batch, "mse+esr") the ten sums are all-reduced between the pass and its finish."""
        tp = self.tp
        k = tp.k_fwd if tp is not None else 1
        if self.ws_s is None or self.ws_s_k != k:
            self.ws_s, self.ws_s_k = binding.step_mse_workspace(self.B, binding.lib().wdf_clipper_tp_chunks(self.T, k), x.device), k
            self.y = self.zs = self.zT = None
        if self.store_output and self.y is None:                 # (made by the first call that wants it)
            self.y = torch.empty((self.T, self.B), dtype=torch.float32, device=x.device)
        y = self.y if self.store_output else None
        W, tol = (tp.warmup, tp.tol) if tp is not None else (0, 1.0e-6)
        if self.loss_kind == "mse":
            binding.clipper_step_mse_tp(x, theta, self.fs, target, self.gscale, k, W, tol=tol, r=r, n_up=self.n_up,
                                        n_down=self.n_down, y=y, ws=self.ws_s, status=self.status, state=self.warm,
                                        gtheta=self.gtheta, sse=self.sse, opt=adam, time_major=self.time_major,
                                        store_y=self.store_output)
            return self.sse, self.gtheta
        eps = float(torch.finfo(torch.float64).eps)
        local = self.sums_allreduce is None
        binding.clipper_step_esr_tp(x, theta, self.fs, target, self.n_global, eps, self.skip, k, W, tol=tol, r=r, n_up=self.n_up,
                                    n_down=self.n_down, y=y, ws=self.ws_s, status=self.status, state=self.warm,
                                    sums10=self.sums10, gtheta=self.gtheta, loss3=self.loss, finish=local,
                                    opt=adam if local else None, time_major=self.time_major, store_y=self.store_output)
        if not local:
            self.sums_allreduce(self.sums10)
            binding.esr_finish(self.sums10, self.n_global, eps, gtheta=self.gtheta, loss3=self.loss)
        self.sse.copy_(self.sums10[0:1])
        return self.sse, self.gtheta


    def eval_fused(self, theta, x, target, r=None):
        """The loss WITHOUT its gradient in one pass over the data (csrc/wdf_clipper_eval.h, binding.clipper_eval_tp): forward and
        the two loss sums, no tangent, no records -- a validation pass.  Chunking / verification / warm start as step_fused;
        honours store_output (False: no y, self.y stays None) and sums_allreduce (the two float64 sums are all-reduced, then
        binding.esr_coef).  Fills self.loss_eval = {mse, esr, mse + esr} (for "mse": skip = 0 and n = n_global, the loss is
        loss_eval[0]) and self.y; self.gtheta and self.sse are not touched.  -> self.loss_eval."""
        tp = self.tp
        k = tp.k_fwd if tp is not None else 1
        if self.ws_e is None or self.ws_e_k != k:
            self.ws_e, self.ws_e_k = binding.eval_workspace(self.B, binding.lib().wdf_clipper_tp_chunks(self.T, k), x.device), k
            self.sums_eval = torch.zeros((2,), dtype=torch.float64, device=x.device)
            self.loss_eval = torch.zeros((3,), dtype=torch.float32, device=x.device)
        if self.store_output and self.y is None:                 # (made by the first call that wants it)
            self.y = torch.empty((self.T, self.B), dtype=torch.float32, device=x.device)
        W, tol = (tp.warmup, tp.tol) if tp is not None else (0, 1.0e-6)
        eps = float(torch.finfo(torch.float64).eps)
        binding.clipper_eval_tp(x, theta, self.fs, target, self.n_global, eps, self.skip, k, W, tol=tol, r=r, n_up=self.n_up,
                                n_down=self.n_down, y=self.y if self.store_output else None, store_y=self.store_output, ws=self.ws_e,
                                status=self.status, state=self.warm, sums=self.sums_eval, loss3=self.loss_eval,
                                time_major=self.time_major)
        if self.sums_allreduce is not None:
            self.sums_allreduce(self.sums_eval)
            binding.esr_coef(self.sums_eval, self.n_global, eps, loss=self.loss_eval)
        return self.loss_eval


def autotune_time_parallel(theta, x, target, fs, plan, time_major=False, n_up=1, n_down=1, reps=7, r=None):
    """Refine a TpPlan by timing a few candidates on the actual batch (HIP events on the launch
    stream, a handful of launches each): the chunk counts, and the warm-up -- the planned W
    assumes a 10 V error at the chunk start; on real data the diodes clamp the state to ~1 V, so
    W - 32 is tried too and kept only if the verify kernel reports a miss 8x below the tolerance
    (every run is still verified, so a drifting circuit costs a repair, never a wrong result)."""
    B, T = (x.shape[1], x.shape[0]) if time_major else x.shape
    if plan is None:
        return plan

    def timed(fn):
        """median of `reps` single-call timings (a mean lets one slow launch flip the plan)"""
        fn()
        e0, e1 = binding.Event(), binding.Event()
        ts = []
        for _ in range(reps):
            e0.record()
            fn()
            e1.record()
            ts.append(e0.elapsed_ms(e1))
        return sorted(ts)[len(ts) // 2]

    best_f, best_b = plan.k_fwd, plan.k_bwd
    if plan.k_fwd > 1:
        cands = sorted({k for k in (plan.k_fwd // 2, plan.k_fwd, plan.k_fwd * 2) if 2 <= k <= T // max(plan.warmup // 2, 64)})
        times = {}
        for k in cands:
            st = MseStep(B, T, fs, plan._replace(k_fwd=k), x.device, n_up=n_up, n_down=n_down, time_major=time_major)
            times[k] = timed(lambda: st.forward(theta, x, r))
        best_f = _pick(times, plan.k_fwd)
        t_now = times[best_f]
        for _ in range(8):                                  # shorter warm-ups, 32 steps at a time, while they pay
            if plan.warmup < 96:
                break
            shorter = plan._replace(k_fwd=best_f, warmup=plan.warmup - 32)
            st = MseStep(B, T, fs, shorter, x.device, n_up=n_up, n_down=n_down, time_major=time_major)
            t_short = timed(lambda: st.forward(theta, x, r))
            stat = binding.tp_status(st.status)
            if not (stat["n_bad"] == 0 and stat["max_miss"] <= plan.tol / 8.0 and t_short < 0.98 * t_now):
                break
            plan, t_now = shorter, t_short
    st = MseStep(B, T, fs, plan._replace(k_fwd=best_f), x.device, n_up=n_up, n_down=n_down, time_major=time_major)
    st.forward(theta, x, r)
    times = {}
    for k in sorted({k for k in (plan.k_bwd // 2, plan.k_bwd, plan.k_bwd * 2) if 1 <= k <= max(1, T // 32)}):
        st.tp = plan._replace(k_fwd=best_f, k_bwd=k)
        st.ws_b = binding.bwd_tp_workspace(B, k, x.device)
        times[k] = timed(lambda: st.backward(theta, x, target, r))
    # reverse sweep: among the candidates within 2 % of the fastest take the fewest chunks (less
    # combine work and workspace; also keeps the choice stable from run to run)
    t_best = min(times.values())
    best_b = min(k for k, t in times.items() if t <= 1.02 * t_best)
    return plan._replace(k_fwd=best_f, k_bwd=best_b)


def autotune_fused(theta, x, target, fs, plan, time_major=False, n_up=1, n_down=1, reps=7, r=None, warm=True):
    """The chunk count of the one-pass step (MseStep.step_fused), by timing the planned count, half and double
    on the actual batch (median of single-launch timings of the warm-started step, as the training loop will run it)."""
    if plan is None:
        return plan
    B, T = (x.shape[1], x.shape[0]) if time_major else x.shape

    def timed(fn):
        for _ in range(8):                   # past the cold call and the warm-start controller's descent (one tile per call)
            fn()
        e0, e1 = binding.Event(), binding.Event()
        ts = []
        for _ in range(reps):
            e0.record()
            fn()
            e1.record()
            ts.append(e0.elapsed_ms(e1))
        return sorted(ts)[len(ts) // 2]

    # plan_time_parallel counts one sequence per lane (two waves per SIMD at k_fwd chunks); with an even batch the one-pass
    # step runs two per lane, i.e. half the waves: the planned count is doubled to keep two waves per SIMD
    k_cap = T // max(plan.warmup // 2, 64)
    planned = plan.k_fwd * 2 if (B % 2 == 0 and not binding.ONE_SEQUENCE_PER_LANE and plan.k_fwd * 2 <= k_cap) else plan.k_fwd
    cands = {k for k in (max(1, planned // 2), planned, planned * 2) if k == 1 or k <= k_cap}
    if warm:
        # Round 6: a stepper that keeps its warm-start state pays the cold warm-up ONCE, then runs 0-16 warm-up steps per chunk
        # -- so its chunk count is not bounded by the cold warm-up's redundancy but by the chip: enough chunks for two waves
        # on every SIMD, down to 32-step chunks (a few thousand sequences: the per-rank share of a strong-scaling run).  The
        # step's tail no longer grows with the chunk count on one wave (clipper_fused_finish_kernel: 8 waves per tile).
        per_tile = 128 if (B % 2 == 0 and not binding.ONE_SEQUENCE_PER_LANE) else 64
        fill = (2 * N_SIMD) // max(1, -(-B // per_tile))
        for k in (fill // 2, fill):
            k = min(k, T // 32)
            if k >= 2 and k > max(cands):
                cands.add(int(binding.lib().wdf_clipper_tp_chunks(T, k)))
    times = {}
    for k in sorted(cands):
        st = MseStep(B, T, fs, plan._replace(k_fwd=k), x.device, n_up=n_up, n_down=n_down, time_major=time_major, warm=warm)
        times[k] = timed(lambda: st.step_fused(theta, x, target, r))
        if binding.tp_status(st.status)["n_bad"]:
            del times[k]                     # a chunking whose speculation fails on this data is not a candidate
    return plan._replace(k_fwd=_pick(times, planned)) if times else plan


class _ClipperMseFn(torch.autograd.Function):
    """mean((clipper(theta, x) - target)^2) as the one-pass training step (MseStep.step_fused: forward, loss
    and gradient in one kernel, one stepper per shape, buffers reused); backward only scales the stored
    gradient -- no y-sized loss temporaries, no dL/dy array, no state stash."""
    _steppers = {}

    @staticmethod
    def forward(ctx, theta, x, r, target, fs, n_up, n_down, tp, time_major):
        B, T = (x.shape[1], x.shape[0]) if time_major else x.shape
        key = (B, T, float(fs), n_up, n_down, tp, x.device, time_major)
        st = _ClipperMseFn._steppers.get(key)
        if st is None:
            if len(_ClipperMseFn._steppers) > 8:
                _ClipperMseFn._steppers.clear()
            st = _ClipperMseFn._steppers[key] = MseStep(B, T, fs, tp, x.device, n_up=n_up, n_down=n_down,
                                                        time_major=time_major)
        th = theta.detach().contiguous()
        LAST_TP_STATUS["status"] = st.status
        if not theta.requires_grad:          # validation / no_grad losses: forward + one streaming pass for the sum
            st.forward(th, x, r)
            d = st.y - target
            return torch.sum(d * d) / float(B * T)
        sse, g = st.step_fused(th, x, target, r)      # forward, loss and gradient in one pass over the data
        ctx.save_for_backward(g.clone())
        return sse[0] / float(B * T)

    @staticmethod
    def backward(ctx, gl):
        (g,) = ctx.saved_tensors
        return gl * g, None, None, None, None, None, None, None, None     # (never reached when theta needs no grad)


class _ResidentMseFn(torch.autograd.Function):
    """_ClipperMseFn for component values resident in a parameter block (lowering.Circuit.to_device): the one-pass step
    reads theta straight from the block; the Variables that own its entries are the differentiable inputs, each handed
    its entry of the gradient as a device scalar.  One stepper per (x, target) pair, with the warm-start state the
    repeated visits of a training set allow."""

    @staticmethod
    def forward(ctx, st, block, x, r, target, inv_n, idx, *live):
        st.step_fused(block, x, target, r)
        # {sse | mse + esr, gtheta[4]} of THIS call (a validation pass may run before backward)
        out = st.out.clone() if st.loss_kind == "mse" else torch.cat((st.loss[2:3], st.gtheta))
        ctx.save_for_backward(out)
        ctx.idx = idx
        ctx.mark_non_differentiable(out)
        return out[0] * inv_n, out            # (out: what GradientTape.gradient hands out directly, compat_tf)

    @staticmethod
    def backward(ctx, gl, _):
        (out,) = ctx.saved_tensors
        g = gl * out
        return (None,) * 7 + tuple(g[1 + i] for i in ctx.idx)


def clipper_mse(theta, x, target, fs, r=None, n_up=1, n_down=1, tp=None, time_major=False):
    """Scalar mean-squared error of the clipper output against target [T,B], differentiable w.r.t.
    theta = {Is, nVt, R, C} (float32[4] on the device); the fused path of lpf.py:87-90-style loops.
    time_major: x (and r) are [T,B]."""
    if tp is None:
        tp = TpPlan(1, 32, 1.0e-6, 1)
    return _ClipperMseFn.apply(theta, x, r, target, float(fs), int(n_up), int(n_down), tp, bool(time_major))


_TUNED = {}      # (B, T, n_up, n_down, per-sample R?, R, C to 2 digits, fs, device, layout, consumer) -> TpPlan


def tuned_plan(theta, x, r, fs, R_plan, C, n_up=1, n_down=1, min_samples=1 << 22, time_major=False, R_min=None, fused=False):
    """plan_time_parallel, refined once per (shape, circuit) by timing candidates on the batch when it is large enough for
    the ~0.1 s of set-up to pay (>= 4 M samples); later calls with the same shape and (to two digits) the same R and C
    reuse the result.  fused: the consumer is the one-pass training step (clipper_mse) -- its chunk count is what is
    tuned (autotune_fused); otherwise the forward / reverse-sweep pair (autotune_time_parallel).
    The key is built from values the caller holds on the HOST (R_plan, C: floats); theta is a device tensor and is only
    handed to the kernels on a miss -- a hit costs no device-to-host copy, no synchronisation.  The diode's own
    parameters are not part of the key: they do not enter the warm-up estimate, training moves them slowly, and every
    forward is verified whatever the plan."""
    B, T = (x.shape[1], x.shape[0]) if time_major else x.shape
    plan = plan_time_parallel(B, T, R_plan, C, fs, time_major=time_major, R_min=R_min)
    if B * T < min_samples or plan.k_fwd < 2:
        return plan
    key = (B, T, n_up, n_down, r is not None, f"{R_plan:.1e}", f"{C:.1e}", float(fs), str(x.device), time_major, bool(fused))
    hit = _TUNED.get(key)
    if hit is None:
        if len(_TUNED) > 32:
            _TUNED.clear()
        with torch.no_grad():
            zero_target = torch.zeros((T, B), dtype=torch.float32, device=x.device)
            tune = autotune_fused if fused else autotune_time_parallel
            hit = _TUNED[key] = tune(theta.detach(), x, zero_target, fs, plan, time_major=time_major,
                                     n_up=n_up, n_down=n_down, reps=5, r=r)
    return hit


def _pick(times, planned):
    """The fastest candidate, but the planned one unless another is at least 3 % faster (timing
    noise should not flip the plan between runs)."""
    best = min(times, key=times.get)
    if planned in times and times[best] > 0.97 * times[planned]:
        return planned
    return best
