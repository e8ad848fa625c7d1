"""The reference of the resident training step of the MLP-root pot clipper (csrc/wdf_mlp_step.h: wdf_clipper_mlp_step), plain torch on
the CPU, for tests/test_mlp_step_ref_cpu.py and tests/test_gpu_mlp_step_edges.py.  It imports no project code.

One training step restated DIRECTLY -- no chunks, no warm-ups, no block maps, no matrix-core layout -- from the scripts
(clipper_pot.py:103-127,141-177, tf_wdf.py:168-192):

    per sample:  G1 = 1/R[n] ;  G2 = 2 C fs ;  p = G1/(G1 + G2) ;  lr = log(1/(G1 + G2))
    a  = z - p (z - x)
    z' = -p (z - x) - MLP(a, lr)
    y  = (z' + z)/2 ,  z_0 = 0
    MLP: 2 -> H -> ... -> H -> 1 (NL hidden layers, tanh or relu), flat weights = kernel[in][out] then bias[out] per layer
    past `skip`:  S = sum (y - t)^2 ;  E = sum y^2 + eps ;  mse = S/n ;  esr = sqrt(S/E/n) ;  loss = mse + esr     (n = n_global)

The gradient of every weight is autograd's.  With a pair of GLOBAL sums (the two sums after an all-reduce over data-parallel ranks)
the loss's two coefficients  dLoss/dy = ga (y - t) + gb y,  ga = 2/n + 1/(esr E n),  gb = -esr/E  are constants taken from those
sums, and the gradient is autograd's of  ga/2 S_local + gb/2 E_local  -- this rank's share of the whole batch's gradient.

Also here: kappa = dz'/dz per step in closed form (checked against autograd on the CPU), a float64 Adam (the tf.keras 2.5 rule, no
clipping), the slope range of a network's root, and -- one list, so that the CPU file can assert the conditions on exactly what the
GPU module runs -- the inputs, pots, targets and synthetic networks of the GPU module.
"""
import numpy as np
import torch

EPS = float(np.finfo(float).eps)                                  # what the scripts' esr_loss adds to the energy
FS = 48000.0
C_CLIPPER = float(np.float32(4.7e-9))                             # (the step holds {R, C} in float32)


def weight_count(H, NL):
    return 3 * H + (NL - 1) * (H * H + H) + H + 1


def unpack(w, H, NL):
    """flat [count] -> [(kernel [in, out], bias [out])] of the NL + 1 dense layers (views: autograd flows to w)."""
    sizes = [2] + [H] * NL + [1]
    out, o = [], 0
    for ni, no in zip(sizes[:-1], sizes[1:]):
        k = w[o:o + ni * no].reshape(ni, no)
        o += ni * no
        out.append((k, w[o:o + no]))
        o += no
    assert o == w.numel() == weight_count(H, NL)
    return out


def _act(h, act):
    return torch.tanh(h) if act == "tanh" else torch.relu(h)


def _dact(h_out, act):
    """the activation's derivative from its output"""
    return 1.0 - h_out * h_out if act == "tanh" else (h_out > 0).to(h_out.dtype)


def mlp(layers, a, lr, act):
    """MLP(a, lr) for vectors a, lr [B] -> (out [B], d out / d a [B], detached, closed form)."""
    h = torch.stack([a, lr], dim=1)
    outs = []
    for i, (k, b) in enumerate(layers):
        h = h @ k + b
        if i + 1 < len(layers):
            h = _act(h, act)
            outs.append(h)
    with torch.no_grad():
        d = layers[0][0][0].detach().unsqueeze(0) * _dact(outs[0].detach(), act)          # d h_0 / d a  [B, H]
        for (k, _), ho in zip(layers[1:-1], outs[1:]):
            d = (d @ k.detach()) * _dact(ho.detach(), act)
        da = (d @ layers[-1][0].detach())[:, 0]
    return h[:, 0], da


class Result:
    pass


def run(x, R, w, H, NL, act, target, skip, C=C_CLIPPER, fs=FS, n_global=None, eps=EPS, global_sums=None, dtype=torch.float64,
        grad=True):
    """x [B,T]; R: a number (static) or [B,T]; w flat [count]; target [T,B].  -> Result: y, kappa [T,B], S, E (before eps; this
    batch's own), mse, esr, loss (of the global sums where given), ga, gb, gw [count] (grad=True), all float64 numpy / floats.
    dtype=torch.float32 runs every operation of the recursion and of the loss in float32 (the fp32 floor of a comparison)."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float64)).to(dtype)
    B, T = x.shape
    tgt = torch.as_tensor(np.asarray(target, dtype=np.float64)).to(dtype)
    assert tgt.shape == (T, B) and 0 <= skip < T
    Rt = torch.as_tensor(np.broadcast_to(np.asarray(R, dtype=np.float64), (B, T)).copy()).to(dtype)
    wt = torch.as_tensor(np.asarray(w, dtype=np.float64)).to(dtype).clone().requires_grad_(grad)
    layers = unpack(wt, H, NL)
    G1 = 1.0 / Rt
    G2 = 2.0 * C * fs
    p_all = G1 / (G1 + G2)
    lr_all = torch.log(1.0 / (G1 + G2))
    z = torch.zeros(B, dtype=dtype)
    ys, kap = [], []
    for t in range(T):
        p, lr = p_all[:, t], lr_all[:, t]
        bt = -p * (z - x[:, t])
        a = z + bt
        m, da = mlp(layers, a, lr, act)
        zn = bt - m
        ys.append(0.5 * (zn + z))
        kap.append(-p - (1.0 - p) * da)                          # dz'/dz = -p - MLP'(a) da/dz, da/dz = 1 - p
        z = zn
    y = torch.stack(ys)                                           # [T,B]
    o, tt = y[skip:], tgt[skip:]
    S, E = ((o - tt) ** 2).sum(), (o ** 2).sum()
    n = float(B * (T - skip)) if n_global is None else float(n_global)
    res = Result()
    res.y, res.kappa = y.detach().double().numpy(), torch.stack(kap).double().numpy()
    res.S, res.E, res.n = float(S.detach()), float(E.detach()), n
    Sg, Eg = (res.S, res.E) if global_sums is None else (float(global_sums[0]), float(global_sums[1]))
    res.mse = Sg / n
    res.esr = float(np.sqrt(Sg / (Eg + eps) / n))
    res.loss = res.mse + res.esr
    res.ga = 2.0 / n + 1.0 / (res.esr * (Eg + eps) * n)
    res.gb = -res.esr / (Eg + eps)
    if grad:
        if global_sums is None:
            loss = S / n + torch.sqrt(S / (E + eps) / n)          # the loss itself (clipper_pot.py:177)
        else:
            loss = 0.5 * res.ga * S + 0.5 * res.gb * E            # the coefficients are constants: they came over the wire
        (g,) = torch.autograd.grad(loss, wt)
        res.gw = g.double().numpy()
    return res


def slope_range(w, H, NL, act, log_r, a_max, n=513):
    """(min, max) of d(-MLP)/da over a in [-a_max, a_max] at the given log R values, float64 autograd."""
    wt = torch.as_tensor(np.asarray(w, dtype=np.float64))
    layers = unpack(wt, H, NL)
    lo, hi = float("inf"), float("-inf")
    for lr in log_r:
        a = torch.linspace(-float(a_max), float(a_max), int(n), dtype=torch.float64, requires_grad=True)
        out, _ = mlp(layers, a, torch.full_like(a, float(lr)), act)
        (g,) = torch.autograd.grad(-out.sum(), a)
        lo, hi = min(lo, float(g.min())), max(hi, float(g.max()))
    return lo, hi


class Adam64:
    """tf.keras.optimizers.Adam (2.5: no amsgrad, no clipping), float64, per-parameter learning rates:
        m = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g^2 ;  lr_t = lr sqrt(1 - b2^t)/(1 - b1^t) ;  w -= lr_t m/(sqrt(v) + eps)"""

    def __init__(self, n, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        self.lr = np.broadcast_to(np.asarray(lr, dtype=np.float64), (n,)).copy()
        self.b1, self.b2, self.eps = float(beta_1), float(beta_2), float(epsilon)
        self.m, self.v, self.step = np.zeros(n), np.zeros(n), 0

    def apply(self, w, g):
        """-> the updated copy of w (float64); the moments advance."""
        g = np.asarray(g, dtype=np.float64)
        self.step += 1
        self.m = self.b1 * self.m + (1.0 - self.b1) * g
        self.v = self.b2 * self.v + (1.0 - self.b2) * g * g
        lr_t = self.lr * np.sqrt(1.0 - self.b2 ** self.step) / (1.0 - self.b1 ** self.step)
        return np.asarray(w, dtype=np.float64) - lr_t * self.m / (np.sqrt(self.v) + self.eps)


# ---------------------------------------------------------------------------------------- what the GPU module runs
def sweeps(B, T, seed=4, amp=0.6, fs=FS):
    """[B,T] float32: exponential sine sweeps 100 Hz -> 10 kHz, amplitude amp U(0.1, 5) V, random start phase."""
    rng = np.random.default_rng(seed)
    A = amp * rng.uniform(0.1, 5.0, B)
    ph = rng.uniform(0.0, 2.0 * np.pi, B)
    t = np.arange(T, dtype=np.float64) / fs
    k = np.log(100.0)
    inst = 2.0 * np.pi * 100.0 * (T / fs) / k * (np.exp(t / (T / fs) * k) - 1.0)
    return np.ascontiguousarray(A[:, None] * np.sin(inst[None, :] + ph[:, None]), dtype=np.float32)


def targets(x):
    """[T,B] float32: a soft clipper of the input, delayed by one sample -- something a clipper can be trained towards, with a
    residual far above rounding."""
    xd = np.concatenate([np.zeros_like(x[:, :1]), x[:, :-1]], axis=1).astype(np.float64)
    return np.ascontiguousarray((0.45 * np.tanh(1.3 * (0.6 * x + 0.4 * xd))).T, dtype=np.float32)


def varying_pot(B, T, lo=5.0e3, hi=12.0e3, seed=9):
    """[B,T] float32 in [lo + 0.25 span, lo + 0.95 span]: per sequence a level, a slow ramp over the sequence and a jump between two
    values from one sample to the next -- no two neighbouring steps of a sequence share a pot value."""
    rng = np.random.default_rng(seed)
    u, v, j = rng.uniform(0, 1, (3, B, 1))
    t = np.arange(T, dtype=np.float64)[None, :]
    span = hi - lo
    r = lo + span * (0.25 + 0.3 * u + 0.2 * v * t / max(T - 1, 1) + 0.2 * (0.25 + 0.75 * j) * (t % 2))
    return np.ascontiguousarray(r, dtype=np.float32)


def constant_pot(B, T, values):
    """[B,T] float32: sequence b at values[b] (a list of B values, or one value for all)."""
    v = np.broadcast_to(np.asarray(values, dtype=np.float64).reshape(-1), (B,)) if np.ndim(values) else np.full(B, float(values))
    return np.ascontiguousarray(np.repeat(v[:, None], T, axis=1), dtype=np.float32)


# Networks for the architectures without committed weights: seeded normal weights times `scale`, biases included; the first layer's
# log R row is scaled by 0.1 (log R is about -7.6: at full scale it would saturate every unit of layer 0).  Seed and scale are
# chosen in tests/test_mlp_step_ref_cpu.py's conditions (max |kappa| <= 0.97 over the GPU module's inputs, slope range >= 0.2 wide).
SYNTH = {
    # (H, NL, act): (seed, scale)
    (4, 3, "relu"): (11, 0.7), (4, 4, "tanh"): (112, 0.6), (4, 4, "relu"): (13, 0.7), (4, 5, "relu"): (214, 0.5),
    (8, 3, "relu"): (121, 0.6), (8, 4, "tanh"): (22, 0.7), (8, 4, "relu"): (23, 0.5), (8, 5, "relu"): (224, 0.5),
    (16, 3, "relu"): (231, 0.3), (16, 4, "tanh"): (32, 0.4), (16, 4, "relu"): (233, 0.4),
    (16, 5, "tanh"): (34, 0.3), (16, 5, "relu"): (35, 0.4),
}
COMMITTED = {(4, 3): "2x4", (8, 3): "2x8", (16, 3): "2x16_pre", (4, 5): "4x4", (8, 5): "4x8"}     # tanh networks with committed weights


def synthetic_mlp(H, NL, act):
    """float32 flat weights of the synthetic network of (H, NL, act)."""
    seed, scale = SYNTH[(H, NL, act)]
    rng = np.random.default_rng(seed)
    w = scale * rng.standard_normal(weight_count(H, NL))
    w[H:2 * H] *= 0.1                                             # kernel_0[1][:]: the log R row
    return w.astype(np.float32)


A_SHAPE = dict(B=21, T=256, skip=37, n_items=6, wgrad_chunks=3)    # test A of the GPU module
A_ARCHS = [(H, NL, act) for H in (4, 8, 16) for NL in (3, 4, 5) for act in ("tanh", "relu")]
A_STATIC_R = 8.0e3
