"""The circuits and data the tests of the two-different-diode root on the streamed-coefficient kernels share
(tf_wdf.AsymDiodePair(..., streamed=True): csrc/wdf_ss_dyn.h, root kind WDF_ROOT_ASYM_PAIR): each case builds the tf_wdf
circuit, names its trainable Variables in the order of the reference's parameter vector -- the pot's own entry left out: the
channel replaces it, so it has no gradient -- and gives the same tree to tests/asym_pot_tree_ref.py.

x and gy are ss_asym_cases.data's (x = standard_normal * 1.2, gy = standard_normal / (B T)); the pot is
tests/test_gpu_ss_dyn.py's pot_channel (a log-uniform level per sequence with a slow sine on top), or one value per sequence
from a grid.  CASES[name]["seed"]: the first seed for which every component of the reference gradient keeps
|sum of terms| >= 0.03 sum |terms| (one term per sequence); found on the CPU with find_seed(), asserted where used.
"""
import numpy as np

import asym_pot_tree_ref as pref
import ss_asym_cases as base

FS = base.FS
BALANCE = base.BALANCE
f32 = base.f32


def pot_channel(B, T, lo, hi, seed):
    """a slowly moving pot per sequence: log-uniform level, a slow sine on top (every sample its own resistance)"""
    rng = np.random.default_rng(seed)
    level = np.exp(rng.uniform(np.log(lo), np.log(hi), B))
    wob = 1.0 + 0.3 * np.sin(2 * np.pi * np.arange(T)[None, :] / rng.uniform(200, 900, B)[:, None] + rng.uniform(0, 6, B)[:, None])
    return (level[:, None] * wob).astype(np.float32)


def pot_grid(B, T):
    """one value per sequence, constant along it (the reference's recordings: dataimport.py:96)"""
    return np.repeat(np.array([300.0, 1.0e3, 2.5e3, 5.0e3], dtype=np.float32)[np.arange(B) % 4][:, None], T, axis=1)


# name -> tree, shape (B, T, ni), pot_index into theta (None: static), the pot channel, the seed
CASES = {
    "hpf_vs": dict(tree="hpf", shape=(70, 300, 1), pot=1, chan=lambda B, T: pot_channel(B, T, 300.0, 5.0e3, 1), seed=1),
    "hpf_r": dict(tree="hpf", shape=(70, 300, 1), pot=0, chan=lambda B, T: pot_channel(B, T, 5.0e3, 80.0e3, 2), seed=0),
    "hpf_vs_seq": dict(tree="hpf", shape=(70, 300, 1), pot=1, chan=pot_grid, seed=0),
    "two_state_vs2": dict(tree="two_state", shape=(70, 300, 2), pot=3, chan=lambda B, T: pot_channel(B, T, 2.0e3, 40.0e3, 3), seed=4),
    "four_state_small": dict(tree="four_state", shape=(5, 131, 1), pot=None, chan=None, seed=0),
    "four_state": dict(tree="four_state", shape=(70, 300, 1), pot=None, chan=None, seed=1),
    # chunks beyond one state (tests/test_gpu_ss_dyn_chunks_state.py): 70 x 131 -- one full and one ragged wave; four chunks of
    # 8-step units are 40, 40, 40 and 11 steps, the last one ragged and no whole unit
    "two_state_vs2_c": dict(tree="two_state", shape=(70, 131, 2), pot=3, chan=lambda B, T: pot_channel(B, T, 2.0e3, 40.0e3, 3), seed=0),
    "three_state_c": dict(tree="three_state", shape=(70, 131, 1), pot=None, chan=None, seed=4),
    "three_state_r1": dict(tree="three_state", shape=(70, 131, 1), pot=2, chan=lambda B, T: pot_channel(B, T, 2.0e3, 20.0e3, 4), seed=1),
    "four_state_c": dict(tree="four_state", shape=(70, 131, 1), pot=None, chan=None, seed=1),
    "four_state_vs": dict(tree="four_state", shape=(70, 131, 1), pot=0, chan=lambda B, T: pot_channel(B, T, 300.0, 5.0e3, 1), seed=1),
    "four_state_vs_seq": dict(tree="four_state", shape=(70, 131, 1), pot=0, chan=pot_grid, seed=1),
}


def _root(W, top, **kw):
    kw.setdefault("streamed", True)
    return W.AsymDiodePair(top, base.DIODES[0], base.DIODES[2], nDiodes_up=1.906, nDiodes_down=1.4, trainable=True, **kw)


def _diode_vars(dp):
    return [dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down]


def hpf(W, pot_on=None, time_parallel=None, root_kw=None, **kw):
    """HPFDiodeClipper.h:28-32: Parallel(R, Series(Vs, C)), probed at R.  theta = [R, Vs.R, C, diodes]; pot_on: None | "R" | "Vs"."""
    R = W.Resistor(33.0e3, True)
    Vs = W.ResistiveVoltageSource(1.0e3, trainable=True)
    C = W.Capacitor(22.0e-9, FS, True)
    top = W.Parallel(R, W.Series(Vs, C))
    dp = _root(W, top, **(root_kw or {}))
    pot = {"R": R, "Vs": Vs, None: None}[pot_on]
    params = [v for e, v in ((R, R.R), (Vs, Vs.R), (C, C.C)) if e is not pot] + _diode_vars(dp)
    return W.Circuit(top, dp, R, per_sample_R=pot, time_parallel=time_parallel, **kw), params


def two_state(W, pot_on=None, time_parallel=None, root_kw=None, **kw):
    """ss_asym_cases.two_state.  theta = [Vs1.R, C1, R1, Vs2.R, C2, diodes]; pot_on: None | "Vs2"."""
    Vs1 = W.ResistiveVoltageSource(22.0e3, trainable=True)
    C1 = W.Capacitor(4.7e-9, FS, trainable=True)
    R1 = W.Resistor(3.3e3, True)
    Vs2 = W.ResistiveVoltageSource(10.0e3, trainable=True)
    C2 = W.Capacitor(10.0e-9, FS, trainable=True)
    top = W.Series(W.Parallel(Vs1, C1), W.Parallel(W.Series(R1, Vs2), C2))
    dp = _root(W, top, **(root_kw or {}))
    pot = {"Vs2": Vs2, None: None}[pot_on]
    params = [v for e, v in ((Vs1, Vs1.R), (C1, C1.C), (R1, R1.R), (Vs2, Vs2.R), (C2, C2.C)) if e is not pot] + _diode_vars(dp)
    return W.Circuit(top, dp, C2, per_sample_R=pot, time_parallel=time_parallel, **kw), params


def three_state(W, pot_on=None, time_parallel=None, **kw):
    """ss_asym_cases.three_state's tree.  theta = [Vs.R, R0, R1, C0, C1, C2, diodes]; pot_on: None | "R1"."""
    Vs = W.ResistiveVoltageSource(1.0e3, trainable=True)
    Rs = [W.Resistor(v, True) for v in (33.0e3, 6.8e3)]
    Cs = [W.Capacitor(v, FS, True) for v in (47.0e-9, 22.0e-9, 10.0e-9)]
    top = W.Parallel(Cs[2], W.Series(Rs[1], W.Parallel(Cs[1], W.Series(W.Series(Vs, Cs[0]), Rs[0]))))
    dp = _root(W, top)
    pot = {"R1": Rs[1], None: None}[pot_on]
    params = [v for e, v in [(Vs, Vs.R)] + [(e, e.R) for e in Rs] + [(e, e.C) for e in Cs] if e is not pot] + _diode_vars(dp)
    return W.Circuit(top, dp, Cs[2], per_sample_R=pot, time_parallel=time_parallel, **kw), params


def four_state(W, pot_on=None, time_parallel=None, **kw):
    """ss_asym_cases.four_state_top: four capacitors, what any_tree=True refuses.  theta = [Vs.R, R0, R1, R2, C0..C3, diodes];
    pot_on: None | "Vs"."""
    top, probe = base.four_state_top(W)
    s1 = top.P2                               # Series(R2, Parallel(C2, Series(R1, Parallel(C1, Series(Series(Vs, C0), R0)))))
    p2 = s1.P2
    s2 = p2.P2
    p3 = s2.P2
    inner = p3.P2
    Vs, C0, R0 = inner.P1.P1, inner.P1.P2, inner.P2
    dp = _root(W, top)
    pot = {"Vs": Vs, None: None}[pot_on]
    params = ([] if pot is Vs else [Vs.R]) + [R0.R, s2.P1.R, s1.P1.R, C0.C, p3.P1.C, p2.P1.C, top.P1.C] + _diode_vars(dp)
    return W.Circuit(top, dp, probe, per_sample_R=pot, time_parallel=time_parallel, **kw), params


def four_state_ref():
    c3 = ("C", 7)
    inner = ("S", ("S", ("V", 0, 0), ("C", 4)), ("R", 1))
    tree = ("P", c3, ("S", ("R", 3), ("P", ("C", 6), ("S", ("R", 2), ("P", ("C", 5), inner)))))
    return tree, c3, f32([1.0e3, 33.0e3, 6.8e3, 15.0e3, 47.0e-9, 22.0e-9, 10.0e-9, 4.7e-9] + base.DIODES)


BUILD = {"hpf": hpf, "two_state": two_state, "three_state": three_state, "four_state": four_state}
REFS = {"hpf": base.hpf_ref, "two_state": base.two_state_ref, "three_state": base.three_state_ref, "four_state": four_state_ref}
POT_NAME = {("hpf", 0): "R", ("hpf", 1): "Vs", ("two_state", 3): "Vs2", ("three_state", 2): "R1", ("four_state", 0): "Vs"}


def build(W, name, time_parallel=None, **kw):
    c = CASES[name]
    return BUILD[c["tree"]](W, POT_NAME.get((c["tree"], c["pot"])), time_parallel, **kw)


def data(name, seed=None):
    """x [B,T] or [B,T,ni] float32, gy [T,B] float32, r [B,T] float32 | None of a case."""
    c = CASES[name]
    B, T, _ = c["shape"]
    x, gy = base.data("hpf", c["seed"] if seed is None else seed, c["shape"])
    return x, gy, (None if c["chan"] is None else c["chan"](B, T))


def with_pot(x, r):
    """[B,T,ni+1]: the voltage channels, then the pot's (clipper_pot.py:68-70)."""
    if r is None:
        return x
    x3 = x if x.ndim == 3 else x[:, :, None]
    return np.concatenate([x3, r[:, :, None]], axis=2).astype(np.float32)


def forward_of(oracle, name, x, r):
    """theta -> y [T,B] of the case's reference tree under the exact two-diode root, and theta."""
    c = CASES[name]
    tree, probe, theta = REFS[c["tree"]]()
    nd = theta.size - 4
    r64 = None if r is None else r.astype(np.float64)
    return (lambda th: pref.tree_fwd_pot(tree, probe, th, FS, x, c["pot"], r64, pref.asym_root_elementwise(oracle, th, nd))), theta


def reference(oracle, name, seed=None):
    """-> dict(x, gy, r, y, grad, balance, theta) of a case at its seed; grad / balance over every parameter but the pot's."""
    x, gy, r = data(name, seed)
    f, theta = forward_of(oracle, name, x.astype(np.float64), r)
    g, bal = pref.grad_and_balance(f, theta, gy, CASES[name]["pot"])
    out = {"x": x, "gy": gy, "y": f(theta), "grad": g, "balance": bal, "theta": theta}
    if r is not None:
        out["r"] = r
    return out


def find_seed(oracle, name, limit=64):
    for seed in range(limit):
        if np.all(reference(oracle, name, seed)["balance"] >= BALANCE):
            return seed
    raise RuntimeError(f"{name}: no seed below {limit} keeps every gradient component's terms from cancelling")
