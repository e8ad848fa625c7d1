"""The circuits the tests of the two-different-diode root on generic trees share: each case builds the tf_wdf circuit, names
its trainable Variables in the order of the reference's parameter vector, and gives the same tree to tests/asym_tree_ref.py.
Parameter vectors end in the four diode values {Is_up, nVt_up, Is_down, nVt_down} (tests/test_gpu_asym.py's THETA6); the
reference is evaluated at the float32-rounded values, the ones the kernels see.

SEED[case]: the first seed of np.random.default_rng (x = standard_normal * 1.2, gy = standard_normal / (B T), in that order)
for which every component of the reference gradient satisfies |sum of terms| >= 0.03 sum |terms| (one term per sequence:
asym_tree_ref.grad_and_balance) -- a relative bound on a component means something only there.  Found on the CPU with find_seed(); the tests assert the condition.
"""
import numpy as np

import asym_tree_ref as ref

FS = 48000
DIODES = [4.352e-9, 25.85e-3 * 1.906, 2.0e-6, 25.85e-3 * 1.4]
BALANCE = 0.03
SHAPES = {"hpf": (70, 300, 1), "two_state": (70, 300, 2), "three_state": (5, 131, 1), "clipper": (70, 300, 1)}
SEED = {"hpf": 0, "two_state": 9, "three_state": 0, "clipper": 1}


def f32(v):
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def _root(W, top, **kw):
    return W.AsymDiodePair(top, DIODES[0], DIODES[2], nDiodes_up=1.906, nDiodes_down=1.4, trainable=True, **kw)


def _diode_vars(dp):
    return [dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down]


def hpf(W, time_parallel=None, any_tree=True, **kw):
    """HPFDiodeClipper.h:28-32: Parallel(R, Series(Vs, C)), probed at R.  theta = [R, Vs.R, C, diodes]."""
    R = W.Resistor(33.0e3, True)
    Vs = W.ResistiveVoltageSource(1.0e3, trainable=True)
    C = W.Capacitor(22.0e-9, FS, True)
    top = W.Parallel(R, W.Series(Vs, C))
    dp = _root(W, top, any_tree=any_tree)
    return W.Circuit(top, dp, R, time_parallel=time_parallel, **kw), [R.R, Vs.R, C.C] + _diode_vars(dp)


def hpf_ref():
    r = ("R", 0)
    return ("P", r, ("S", ("V", 1, 0), ("C", 2))), r, f32([33.0e3, 1.0e3, 22.0e-9] + DIODES)


def two_state(W, time_parallel=None, **kw):
    """tests/test_gpu_circuit.py's _two_state_clipper: two capacitors, two sources.  theta = [Vs1.R, C1, R1, Vs2.R, C2, diodes]."""
    Vs1 = W.ResistiveVoltageSource(22.0e3, trainable=True)
    C1 = W.Capacitor(4.7e-9, FS, trainable=True)
    R1 = W.Resistor(3.3e3, True)
    Vs2 = W.ResistiveVoltageSource(10.0e3, trainable=True)
    C2 = W.Capacitor(10.0e-9, FS, trainable=True)
    top = W.Series(W.Parallel(Vs1, C1), W.Parallel(W.Series(R1, Vs2), C2))
    dp = _root(W, top, any_tree=True)
    return W.Circuit(top, dp, C2, time_parallel=time_parallel, **kw), [Vs1.R, C1.C, R1.R, Vs2.R, C2.C] + _diode_vars(dp)


def two_state_ref():
    c2 = ("C", 4)
    tree = ("S", ("P", ("V", 0, 0), ("C", 1)), ("P", ("S", ("R", 2), ("V", 3, 1)), c2))
    return tree, c2, f32([22.0e3, 4.7e-9, 3.3e3, 10.0e3, 10.0e-9] + DIODES)


def three_state(W, time_parallel=None, **kw):
    """The tone-shaping network of test_four_state_two_stage_trees_vs_oracle less its last shelving section:
    Parallel(C2, Series(R1, Parallel(C1, Series(Series(Vs, C0), R0)))), probed at C2.  theta = [Vs.R, R0, R1, C0, C1, C2, diodes]."""
    Vs = W.ResistiveVoltageSource(1.0e3, trainable=True)
    Rs = [W.Resistor(v, True) for v in (33.0e3, 6.8e3)]
    Cs = [W.Capacitor(v, FS, True) for v in (47.0e-9, 22.0e-9, 10.0e-9)]
    top = W.Parallel(Cs[2], W.Series(Rs[1], W.Parallel(Cs[1], W.Series(W.Series(Vs, Cs[0]), Rs[0]))))
    dp = _root(W, top, any_tree=True)
    return (W.Circuit(top, dp, Cs[2], time_parallel=time_parallel, **kw),
            [Vs.R] + [e.R for e in Rs] + [e.C for e in Cs] + _diode_vars(dp))


def three_state_ref():
    c2 = ("C", 5)
    tree = ("P", c2, ("S", ("R", 2), ("P", ("C", 4), ("S", ("S", ("V", 0, 0), ("C", 3)), ("R", 1)))))
    return tree, c2, f32([1.0e3, 33.0e3, 6.8e3, 47.0e-9, 22.0e-9, 10.0e-9] + DIODES)


def four_state_top(W):
    """test_four_state_two_stage_trees_vs_oracle's diode-root tree (four capacitors): refused under this root."""
    Vs = W.ResistiveVoltageSource(1.0e3, trainable=True)
    R2 = [W.Resistor(v, True) for v in (33.0e3, 6.8e3, 15.0e3)]
    C2 = [W.Capacitor(v, FS, True) for v in (47.0e-9, 22.0e-9, 10.0e-9, 4.7e-9)]
    inner = W.Series(W.Series(Vs, C2[0]), R2[0])
    return W.Parallel(C2[3], W.Series(R2[2], W.Parallel(C2[2], W.Series(R2[1], W.Parallel(C2[1], inner))))), C2[3]


def clipper(W, time_parallel=None, any_tree=True, **kw):
    """The diode-clipper tree Parallel(Vs, C), probed at C (45 kOhm, 4.7 nF: THETA6).  theta = [Vs.R, C, diodes]."""
    Vs = W.ResistiveVoltageSource(45.0e3, trainable=True)
    C = W.Capacitor(4.7e-9, FS, trainable=True)
    top = W.Parallel(Vs, C)
    dp = _root(W, top, any_tree=any_tree)
    return W.Circuit(top, dp, C, time_parallel=time_parallel, **kw), [Vs.R, C.C] + _diode_vars(dp)


def clipper_ref():
    c = ("C", 1)
    return ("P", ("V", 0, 0), c), c, f32([45.0e3, 4.7e-9] + DIODES)


REFS = {"hpf": hpf_ref, "two_state": two_state_ref, "three_state": three_state_ref, "clipper": clipper_ref}


def data(case, seed=None, shape=None):
    """x [B,T] or [B,T,2] float32 and gy [T,B] float32 of a case."""
    B, T, ni = shape or SHAPES[case]
    rng = np.random.default_rng(SEED[case] if seed is None else seed)
    x = (rng.standard_normal((B, T, ni)) * 1.2).astype(np.float32)
    gy = (rng.standard_normal((T, B)) / (B * T)).astype(np.float32)
    return (x[:, :, 0] if ni == 1 else x), gy


def forward_of(oracle, case, x):
    """theta -> y [T,B] of the case's reference tree under the exact two-diode root."""
    tree, probe, theta = REFS[case]()
    nd = theta.size - 4
    if case == "clipper":       # the oracle's own loop for this tree (theta6 = diodes, R, C)
        return (lambda th: oracle.clipper_asym_fwd(np.concatenate([th[2:], th[:2]]), float(FS), x)), theta
    return (lambda th: ref.tree_fwd(tree, probe, th, FS, x, ref.asym_root_of(oracle, th, nd))), theta


def reference(oracle, case, seed=None):
    """-> dict(x, gy, y, grad, balance) of a case at its seed: y and the finite-difference gradient of sum(y gy), fp64."""
    x, gy = data(case, seed)
    f, theta = forward_of(oracle, case, x.astype(np.float64))
    g, bal = ref.grad_and_balance(f, theta, gy)
    return {"x": x, "gy": gy, "y": f(theta), "grad": g, "balance": bal, "theta": theta}


def find_seed(oracle, case, limit=64):
    for seed in range(limit):
        if np.all(reference(oracle, case, seed)["balance"] >= BALANCE):
            return seed
    raise RuntimeError(f"{case}: no seed below {limit} keeps every gradient component's terms from cancelling")
