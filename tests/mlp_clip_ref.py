"""The reference of the MLP-root clipper kernels (csrc/wdf_mlp.h, wdf_mlp_row.h, wdf_mlp_tp.h, wdf_mlp_mfma.h), plain torch on the
CPU, for tests/test_mlp_clip_ref_cpu.py and tests/test_gpu_mlp_clip_kernels.py.  It imports no project code (unpack, mlp and
weight_count come from tests/mlp_step_ref.py, which imports none either).

The recursion restated DIRECTLY -- no chunks, no rows, no matrix-core layout -- from the scripts (clipper_pot.py:103-127,
tf_wdf.py:168-192):

    per sample:  G1 = 1/R[n] ;  G2 = 2 C fs ;  p = G1/(G1 + G2) ;  lr = log(1/(G1 + G2))
    a  = z - p (z - x)
    z' = -p (z - x) - MLP(a, lr) + e          (e = 0: the slot the root's wave b_root = -MLP goes through)
    y  = (z' + z)/2 ,  z_0 = z0 or 0

forward():  y, zstash (row t = the state BEFORE step t), zT.
sweep():    for a GIVEN stash and L = sum gy . y, per step  a, lr, kappa = dz'/dz in closed form (-p - (1 - p) dMLP/da) and
            gb = dL/de  from the adjoint recurrence written out,
                gb[T-1] = gy[T-1]/2 ;  gb[t] = gy[t]/2 + gy[t+1]/2 + kappa[t+1] gb[t+1] ,
            and gw, dL/dR (static R only), dL/dC by autograd of  sum_t gb[t] z'_t(z_t held at the stash; w, R, C)  -- every
            parameter enters L through the z'_t alone, so this IS dL/dtheta once gb is dL/dz'_t.
recursion_autograd():  the same gradients, gb and kappa by autograd THROUGH the recursion (tests/test_mlp_clip_ref_cpu.py pins
            sweep() on it to 1e-12).
dtype=torch.float32 runs every operation of the recursion and of the sweep in float32: the fp32 floor of a comparison.

Also here, ONE list, so that the CPU file asserts its conditions on exactly what the GPU file runs: the cases (architecture, B, T,
static or per-sample R, z0, seeds, weight scale) of the GPU file's sections, the bounds, and the inputs of the mlp_eval test.
"""
import collections
import functools

import numpy as np
import torch

from mlp_step_ref import mlp, sweeps, unpack, varying_pot, weight_count

FS = 48000.0
C_CLIPPER = float(np.float32(4.7e-9))                             # (the kernels hold {R, C} in float32)
R_STATIC = float(np.float32(20.0e3))
ARCHS = [(4, 3), (8, 3), (16, 3), (4, 4), (8, 4), (4, 5), (8, 5)]   # (width, tanh layers): all that csrc/wdf_capi_mlp.hip builds

# ------------------------------------------------------------------------------------------------------------ bounds
Y_BOUND = 5e-6            # y, zstash, zT: x max(1, max |z_ref|)                    (tests/test_gpu_mlp_root.py, the g3 test)
G_REL, G_ABS = 1e-4, 1e-5  # a gradient component: G_REL |ref| + G_ABS max |ref|     (the same test)
FLOOR_FACTOR = 8.0        # kappa, gb, ain, lrin, mlp_eval: x the case's float32 floor (see floor())
TP_TOL = 1e-6             # the time-parallel forward's arrival tolerance (its default); a repaired result may sit 2 tol off
SATURATED = 0.995         # |tanh| above this (|pre-activation| > 3) counts as saturated


def grad_bound(ref):
    """per component: G_REL |ref| + G_ABS max |ref| (the vector's own largest entry)."""
    ref = np.atleast_1d(np.asarray(ref, dtype=np.float64))
    return G_REL * np.abs(ref) + G_ABS * np.max(np.abs(ref))


def grad_ratio(got, ref):
    """largest |got - ref| / bound over the components."""
    got, ref = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(ref, dtype=np.float64))
    b = grad_bound(ref)
    return float(np.max(np.abs(got - ref) / np.where(b > 0.0, b, np.finfo(float).tiny)))


def floor(ref32, ref64):
    """The float32 floor of one quantity of one case: max |ref32 - ref64| of the reference itself -- but never less than half an ulp
    of the quantity's largest value, 2^-24 max |ref64|: a result that is STORED in float32 cannot be closer than that, and on a case
    of one or two samples the float32 run can land on the float64 value by luck."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    return max(float(np.max(np.abs(np.asarray(ref32, dtype=np.float64) - ref64))), 2.0 ** -24 * float(np.max(np.abs(ref64))))


# --------------------------------------------------------------------------------------------------------- the recursion
class Result:
    pass


def _coeffs(R, C, fs):
    G1 = 1.0 / R
    G2 = 2.0 * C * fs
    return G1 / (G1 + G2), torch.log(1.0 / (G1 + G2))


def _tensors(x, R, w, z0, dtype):
    x = torch.as_tensor(np.asarray(x, dtype=np.float64)).to(dtype)
    B, T = x.shape
    static = np.ndim(R) == 0
    Rt = torch.as_tensor(np.asarray(R, dtype=np.float64)).to(dtype)
    assert static or tuple(Rt.shape) == (B, T)
    wt = torch.as_tensor(np.asarray(w, dtype=np.float64)).to(dtype).clone()
    z = torch.zeros(B, dtype=dtype) if z0 is None else torch.as_tensor(np.asarray(z0, dtype=np.float64)).to(dtype)
    assert tuple(z.shape) == (B,)
    return x, Rt, wt, z, static


def forward(x, R, w, H, NL, z0=None, C=C_CLIPPER, fs=FS, dtype=torch.float64):
    """x [B,T]; R a number (static) or [B,T]; w flat -> Result: y [T,B], zstash [T,B], zT [B] (float64 numpy)."""
    x, Rt, wt, z, static = _tensors(x, R, w, z0, dtype)
    B, T = x.shape
    with torch.no_grad():
        layers = unpack(wt, H, NL)
        p_all, lr_all = _coeffs(Rt, torch.tensor(C, dtype=dtype), fs)
        if static:
            p_all, lr_all = p_all.expand(B, T), lr_all.expand(B, T)
        ys, zs = [], []
        for t in range(T):
            bt = -p_all[:, t] * (z - x[:, t])
            m, _ = mlp(layers, z + bt, lr_all[:, t], "tanh")
            zn = bt - m
            zs.append(z)
            ys.append(0.5 * (zn + z))
            z = zn
    res = Result()
    res.y, res.zstash, res.zT = torch.stack(ys).double().numpy(), torch.stack(zs).double().numpy(), z.double().numpy()
    return res


def sweep(x, R, w, H, NL, zstash, gy, C=C_CLIPPER, fs=FS, dtype=torch.float64):
    """The reverse sweep at a GIVEN stash [T,B] -> Result: a, lr, kappa, gb [T,B]; gw [count]; gR (None under per-sample R), gC;
    sat [NL]: per tanh layer the fraction of (step, unit) pairs with |tanh| > SATURATED; sat_live: the same without the units that
    are saturated on every step (dead units of a trained network: constants, whatever the input)."""
    x, Rt, wt, _, static = _tensors(x, R, w, None, dtype)
    B, T = x.shape
    zs = torch.as_tensor(np.asarray(zstash, dtype=np.float64)).to(dtype)
    g = torch.as_tensor(np.asarray(gy, dtype=np.float64)).to(dtype)
    assert tuple(zs.shape) == (T, B) and tuple(g.shape) == (T, B)
    wt.requires_grad_(True)
    Ct = torch.tensor(C, dtype=dtype, requires_grad=True)
    if static:
        Rt.requires_grad_(True)
    layers = unpack(wt, H, NL)
    p, lr = _coeffs(Rt, Ct, fs)
    p, lr = (p.expand(T, B), lr.expand(T, B)) if static else (p.T, lr.T)                  # [T,B]
    bt = -p * (zs - x.T)
    a = zs + bt
    m, da = mlp(layers, a.reshape(-1), lr.reshape(-1), "tanh")
    zn = bt - m.reshape(T, B)
    with torch.no_grad():
        kap = -p - (1.0 - p) * da.reshape(T, B)                   # dz'/dz: da/dz = 1 - p
        gb = torch.zeros_like(kap)
        gb[T - 1] = 0.5 * g[T - 1]
        for t in range(T - 2, -1, -1):
            gb[t] = 0.5 * g[t] + (0.5 * g[t + 1] + kap[t + 1] * gb[t + 1])
        h, sat, sat_live = torch.stack([a.reshape(-1), lr.reshape(-1)], dim=1), [], []
        for k, b in layers[:-1]:
            h = torch.tanh(h @ k + b)
            u = (h.abs() > SATURATED).double().mean(dim=0)            # per unit: the fraction of steps it is saturated on
            sat.append(float(u.mean()))
            sat_live.append(float((u * (u < 1.0)).mean()))            # ... leaving out units that are saturated on EVERY step
    grads = torch.autograd.grad((gb * zn).sum(), [wt, Ct] + ([Rt] if static else []))
    res = Result()
    res.a, res.lr = a.detach().double().numpy(), lr.detach().double().numpy()
    res.kappa, res.gb = kap.double().numpy(), gb.double().numpy()
    res.gw, res.gC = grads[0].double().numpy(), float(grads[1])
    res.gR = float(grads[2]) if static else None
    res.sat, res.sat_live = sat, sat_live
    return res


def run(x, R, w, H, NL, gy, z0=None, C=C_CLIPPER, fs=FS, dtype=torch.float64):
    """forward(), then sweep() at its own stash: one Result with everything."""
    f = forward(x, R, w, H, NL, z0=z0, C=C, fs=fs, dtype=dtype)
    s = sweep(x, R, w, H, NL, f.zstash, gy, C=C, fs=fs, dtype=dtype)
    s.y, s.zstash, s.zT = f.y, f.zstash, f.zT
    return s


def recursion_autograd(x, R, w, H, NL, gy, z0=None, C=C_CLIPPER, fs=FS):
    """float64 autograd THROUGH the recursion, L = sum gy . y -> Result: y, gw, gR | None, gC, gb = dL/de [T,B] (e: a zero added to
    every z'), kappa [T,B] = d z'_t / d z_t (autograd of one step at the recursion's own states) and a [T,B]."""
    dtype = torch.float64
    x, Rt, wt, z, static = _tensors(x, R, w, z0, dtype)
    B, T = x.shape
    g = torch.as_tensor(np.asarray(gy, dtype=np.float64))
    wt.requires_grad_(True)
    Ct = torch.tensor(C, dtype=dtype, requires_grad=True)
    if static:
        Rt.requires_grad_(True)
    e = torch.zeros((T, B), dtype=dtype, requires_grad=True)
    layers = unpack(wt, H, NL)
    p_all, lr_all = _coeffs(Rt, Ct, fs)
    if static:
        p_all, lr_all = p_all.expand(B, T), lr_all.expand(B, T)
    ys, kap, av = [], [], []
    for t in range(T):
        zl = z.detach().clone().requires_grad_(True)              # one step on its own, for d z'/d z
        btl = -p_all[:, t].detach() * (zl - x[:, t])
        ml, _ = mlp([(k.detach(), b.detach()) for k, b in layers], zl + btl, lr_all[:, t].detach(), "tanh")
        kap.append(torch.autograd.grad((btl - ml).sum(), zl)[0])
        bt = -p_all[:, t] * (z - x[:, t])
        a = z + bt
        m, _ = mlp(layers, a, lr_all[:, t], "tanh")
        zn = bt - m + e[t]
        ys.append(0.5 * (zn + z))
        av.append(a.detach())
        z = zn
    y = torch.stack(ys)
    grads = torch.autograd.grad((g * y).sum(), [wt, Ct, e] + ([Rt] if static else []))
    res = Result()
    res.y, res.a, res.kappa = y.detach().numpy(), torch.stack(av).numpy(), torch.stack(kap).numpy()
    res.gw, res.gC, res.gb = grads[0].numpy(), float(grads[1]), grads[2].numpy()
    res.gR = float(grads[3]) if static else None
    return res


def mlp_out(w, H, NL, a, lr, dtype=torch.float64):
    """MLP(a, lr) over flat samples -> float64 numpy."""
    with torch.no_grad():
        wt = torch.as_tensor(np.asarray(w, dtype=np.float64)).to(dtype)
        out, _ = mlp(unpack(wt, H, NL), torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype),
                     torch.as_tensor(np.asarray(lr, dtype=np.float64)).to(dtype), "tanh")
    return out.double().numpy()


def warmup_from_kappa(kappa, tol):
    """The warm-up a chunk needs wherever it starts: the smallest W such that over EVERY window of W steps of every sequence the
    product of |kappa| is below tol/4, rounded up to 16 (None: no window of the sequence gets there)."""
    lk = np.log(np.maximum(np.abs(np.asarray(kappa, dtype=np.float64)), 1e-300))             # [T,B]
    T = lk.shape[0]
    cs = np.concatenate([np.zeros((1, lk.shape[1])), np.cumsum(lk, axis=0)])
    want = np.log(tol / 4.0)
    for W in range(1, T + 1):
        if np.all(cs[W:] - cs[:-W] < want):
            return -(-W // 16) * 16
    return None


# ----------------------------------------------------------------------------------------------- what the GPU module runs
# A case: section(s) it serves, architecture, shape, R mode, z0, the seeds of input / weights / gy, the weight scale, or the name of
# a committed trained network (`net`: the test files load it with workload.reference_mlp_weights) and `pot`: how R [B,T] is made
# ("varying": mlp_step_ref.varying_pot between 8 and 60 kOhm, no two neighbouring steps alike; "dataset": the four contiguous
# blocks of workload.dataset_resistance_batch, restated here).
Case = collections.namedtuple("Case", "sec H NL B T dyn z0 seed scale net pot")

# seeded normal weights x scale, the log R row x 0.1 (as mlp_step_ref.synthetic_mlp); seed and scale chosen so that the conditions of
# tests/test_mlp_clip_ref_cpu.py hold on every case: (seed, scale) per architecture
SYNTH = {(4, 3): (79, 1.0), (8, 3): (86, 0.6), (16, 3): (46, 0.5), (4, 4): (44, 1.0), (8, 4): (144, 0.6), (4, 5): (143, 0.8),
         (8, 5): (47, 0.75)}

AB_SHAPES = [(1, 1, False), (3, 15, False), (4, 16, False), (5, 17, False), (17, 33, False), (66, 130, True)]   # (B, T, z0 != 0)
C_ARCHS = [(4, 4), (8, 3), (16, 3)]
# kScanChunk = 128 steps per scan chunk, an 8-step unrolled body and a step-by-step tail: 127 / 128 the last single scans, 129 a second
# chunk of one step, 131 one of three steps (the only length here at which the chunked scan's TAIL carries an adjoint from one step
# to the next), 136 a second chunk of exactly one unrolled body, 257 three chunks
C_T = [7, 8, 9, 127, 128, 129, 131, 136, 257]
C_B = [3, 66]
D_SHAPES = [(5, 100, False), (17, 257, True), (66, 130, False)]
D_TRAINED = ["2x16", "2x8"]


def c_chunk_counts(T):
    """1, 2 and one larger than T/16 (the library cuts it to whole blocks of 16 steps)."""
    return [1, 2, T // 16 + 2]


def _cases():
    out = []
    for H, NL in ARCHS:
        seed, scale = SYNTH[(H, NL)]
        for dyn in (False, True):
            for B, T, z0 in AB_SHAPES:
                out.append(Case("AB", H, NL, B, T, dyn, z0, seed, scale, None, "varying"))
    for H, NL in C_ARCHS:
        seed, scale = SYNTH[(H, NL)]
        for B in C_B:
            for T in C_T:
                for dyn in (False, True):
                    out.append(Case("C", H, NL, B, T, dyn, False, seed, scale, None, "varying"))
    for H, NL in C_ARCHS:
        seed, scale = SYNTH[(H, NL)]
        for B, T, z0 in D_SHAPES:
            for dyn in (False, True):
                out.append(Case("D", H, NL, B, T, dyn, z0, seed, scale, None, "varying"))
    for net in D_TRAINED:
        for B, T, z0 in D_SHAPES:
            out.append(Case("Dt", 16 if net == "2x16" else 8, 3, B, T, True, z0, 6, 0.0, net, "dataset"))
    return out


CASES = _cases()


def cases(sec):
    return [c for c in CASES if c.sec == sec]


def case_id(c):
    return (f"{c.sec} {c.NL - 1}x{c.H}{'' if c.net is None else ' trained ' + c.net} B={c.B} T={c.T} "
            f"{'R[B,T]' if c.dyn else 'static R'}{' z0' if c.z0 else ''}")


def synthetic_mlp(H, NL, seed, scale):
    rng = np.random.default_rng(seed)
    w = scale * rng.standard_normal(weight_count(H, NL))
    w[H:2 * H] *= 0.1                                             # kernel_0[1][:]: the log R row (log R is about -7.6)
    return w.astype(np.float32)


def dataset_pot(B, T, grid=(10.0e3, 25.2e3, 75.0e3, 99.1e3)):
    g = np.asarray(grid, dtype=np.float64)
    idx = np.minimum((np.arange(B) * len(g)) // max(B, 1), len(g) - 1)
    return np.ascontiguousarray(np.repeat(g[idx][:, None], T, axis=1), dtype=np.float32)


Inputs = collections.namedtuple("Inputs", "x R w z0 gy")


def inputs(c, trained=None):
    """The float32 inputs of a case: x [B,T], R (a number | [B,T]), w, z0 [B] | None, gy [T,B].  trained: name -> (w, H, NL) for the
    cases that name a committed network."""
    # (the trained roots forget slowest at small signals, diodes off: |kappa| 0.95 .. 0.998; their cases run at the larger amplitude)
    x = sweeps(c.B, c.T, seed=100 + c.seed + c.B + c.T, amp=0.6 if c.net is None else 1.0)
    if c.dyn:
        R = dataset_pot(c.B, c.T) if c.pot == "dataset" else varying_pot(c.B, c.T, lo=8.0e3, hi=60.0e3, seed=c.seed + c.T)
    else:
        R = R_STATIC
    if c.net is None:
        w = synthetic_mlp(c.H, c.NL, c.seed, c.scale)
    else:
        w, H, NL = trained(c.net)
        assert (H, NL) == (c.H, c.NL)
        w = np.asarray(w, dtype=np.float32)
    rng = np.random.default_rng(7000 + c.seed + 13 * c.B + c.T)
    z0 = rng.uniform(-0.2, 0.2, c.B).astype(np.float32) if c.z0 else None
    gy = ((0.5 + rng.standard_normal((c.T, c.B))) / (c.B * c.T)).astype(np.float32)
    return Inputs(x, R, w, z0, gy)


_trained = {}


def set_trained_loader(fn):
    """the test files hand in workload.reference_mlp_weights (this module imports no project code)"""
    _trained["fn"] = fn


@functools.lru_cache(maxsize=None)
def ref(c):
    """float64: forward + sweep at its own stash."""
    i = inputs(c, _trained.get("fn"))
    return run(i.x, i.R, i.w, c.H, c.NL, i.gy, z0=i.z0)


@functools.lru_cache(maxsize=None)
def ref32(c):
    """the same, every operation in float32 (own forward, own stash): the floor of the forward's outputs and of a kappa that a forward
    kernel computes at its own states."""
    i = inputs(c, _trained.get("fn"))
    return run(i.x, i.R, i.w, c.H, c.NL, i.gy, z0=i.z0, dtype=torch.float32)


def stash32(c):
    """the float64 stash rounded to float32: what the reverse-sweep tests feed the kernels."""
    return ref(c).zstash.astype(np.float32)


@functools.lru_cache(maxsize=None)
def sweep_at_stash32(c, dtype=torch.float64):
    """sweep() at stash32(c): in float64 what a reverse-sweep kernel fed that stash should return; in float32 its floor."""
    i = inputs(c, _trained.get("fn"))
    return sweep(i.x, i.R, i.w, c.H, c.NL, stash32(c), i.gy, dtype=dtype)


# mlp_eval: S samples, a in [-20, 20] (the first layer saturates from |a| of a few volts on: where tanh_fast has to clamp), every
# eighth sample within +-0.5 V, lr over the pot's range
EVAL_S = [1, 63, 64, 65, 131072 + 65]


def eval_inputs(S, seed=5):
    rng = np.random.default_rng(seed + S)
    a = rng.uniform(-20.0, 20.0, S)
    a[::8] = rng.uniform(-0.5, 0.5, a[::8].size)
    if S > 2:
        a[1], a[2] = 20.0, -20.0
    lr = np.log(1.0 / (1.0 / rng.uniform(8.0e3, 100.0e3, S) + 2.0 * C_CLIPPER * FS))
    return a.astype(np.float32), lr.astype(np.float32)


@functools.lru_cache(maxsize=None)
def kappa_slope(c, h=1.0e-4):
    """max |d kappa / d z| along the case's trajectory (central difference of the closed form in the stash): how far a state that is
    off by d moves kappa -- what a forward that was REPAIRED to tol may add to its stored kappa."""
    i = inputs(c, _trained.get("fn"))
    zs = ref(c).zstash
    kp = sweep(i.x, i.R, i.w, c.H, c.NL, zs + h, i.gy).kappa
    km = sweep(i.x, i.R, i.w, c.H, c.NL, zs - h, i.gy).kappa
    return float(np.max(np.abs(kp - km)) / (2.0 * h))
