"""The circuits, data and fp64 references the tests of the one-pass step under the two-different-diode root share
(csrc/wdf_ss_asym_step.h): tests/ss_asym_cases.py's four trees and three more, so that (ns, ni) = (1,2) and (2,1) are covered
and a two-state tree contracts (the planner speculates for `a`, `b` and `hpf2`; `two_state` reaches |eigenvalue| >= 1).

Data of every case: x = default_rng(0).standard_normal((B, T, ni)) * 1.2; the target is the reference's y at the teacher values
theta * (1 + 0.12 (-1)^k), rounded to float32.  Reference: the fp64 NumPy tree of tests/asym_tree_ref.py under
oracle.asym_root at the float32-rounded parameters; gradients are central differences (h = 1e-5 relative) of the loss itself.
Balance: per gradient component |sum of terms| / sum |terms| with one term per sequence; the tests assert >= BALANCE.
"""
import numpy as np

import asym_tree_ref as ref
import ss_asym_cases as cases

FS = cases.FS
DIODES = cases.DIODES
BALANCE = cases.BALANCE
EPS = float(np.finfo(float).eps)
H = 1.0e-5
SHAPES = {"hpf": (70, 300, 1), "hpf2": (70, 300, 2), "a": (70, 300, 1), "b": (70, 300, 2), "two_state": (70, 300, 2),
          "three_state": (5, 131, 1), "clipper": (70, 300, 1)}
NS_NI = {"hpf": (1, 1), "hpf2": (1, 2), "a": (2, 1), "b": (2, 2), "two_state": (2, 2), "three_state": (3, 1), "clipper": (1, 1)}
ALL = tuple(SHAPES)


def hpf2(W, time_parallel=None, **kw):
    """Parallel(R, Series(Series(Vs, Vs2), C)), probed at R: ns 1, ni 2.  theta = [R, Vs.R, Vs2.R, C, diodes]."""
    R = W.Resistor(33.0e3, True)
    Vs = W.ResistiveVoltageSource(1.0e3, trainable=True)
    Vs2 = W.ResistiveVoltageSource(2.2e3, trainable=True)
    C = W.Capacitor(22.0e-9, FS, True)
    top = W.Parallel(R, W.Series(W.Series(Vs, Vs2), C))
    dp = cases._root(W, top, any_tree=True)
    return W.Circuit(top, dp, R, time_parallel=time_parallel, **kw), [R.R, Vs.R, Vs2.R, C.C] + cases._diode_vars(dp)


def hpf2_ref():
    r = ("R", 0)
    return ("P", r, ("S", ("S", ("V", 1, 0), ("V", 2, 1)), ("C", 3))), r, cases.f32([33.0e3, 1.0e3, 2.2e3, 22.0e-9] + DIODES)


def a(W, time_parallel=None, **kw):
    """Parallel(R, Series(Vs, Series(C1, Parallel(R2, C2)))), probed at R: ns 2, ni 1.  theta = [R, Vs.R, C1, R2, C2, diodes]."""
    R = W.Resistor(33.0e3, True)
    Vs = W.ResistiveVoltageSource(1.0e3, trainable=True)
    C1 = W.Capacitor(22.0e-9, FS, True)
    R2 = W.Resistor(4.7e3, True)
    C2 = W.Capacitor(10.0e-9, FS, True)
    top = W.Parallel(R, W.Series(Vs, W.Series(C1, W.Parallel(R2, C2))))
    dp = cases._root(W, top, any_tree=True)
    return W.Circuit(top, dp, R, time_parallel=time_parallel, **kw), [R.R, Vs.R, C1.C, R2.R, C2.C] + cases._diode_vars(dp)


def a_ref():
    r = ("R", 0)
    tree = ("P", r, ("S", ("V", 1, 0), ("S", ("C", 2), ("P", ("R", 3), ("C", 4)))))
    return tree, r, cases.f32([33.0e3, 1.0e3, 22.0e-9, 4.7e3, 10.0e-9] + DIODES)


def b(W, time_parallel=None, **kw):
    """Parallel(R, Series(Series(Vs, C1), Parallel(Vs2, C2))), probed at R: ns 2, ni 2.  theta = [R, Vs.R, C1, Vs2.R, C2, diodes]."""
    R = W.Resistor(33.0e3, True)
    Vs = W.ResistiveVoltageSource(1.0e3, trainable=True)
    C1 = W.Capacitor(22.0e-9, FS, True)
    Vs2 = W.ResistiveVoltageSource(4.7e3, trainable=True)
    C2 = W.Capacitor(10.0e-9, FS, True)
    top = W.Parallel(R, W.Series(W.Series(Vs, C1), W.Parallel(Vs2, C2)))
    dp = cases._root(W, top, any_tree=True)
    return W.Circuit(top, dp, R, time_parallel=time_parallel, **kw), [R.R, Vs.R, C1.C, Vs2.R, C2.C] + cases._diode_vars(dp)


def b_ref():
    r = ("R", 0)
    tree = ("P", r, ("S", ("S", ("V", 1, 0), ("C", 2)), ("P", ("V", 3, 1), ("C", 4))))
    return tree, r, cases.f32([33.0e3, 1.0e3, 22.0e-9, 4.7e3, 10.0e-9] + DIODES)


def _clipper(W, time_parallel=None, **kw):
    return cases.clipper(W, time_parallel, force_generic=True, **kw)


BUILD = {"hpf": cases.hpf, "hpf2": hpf2, "a": a, "b": b, "two_state": cases.two_state, "three_state": cases.three_state,
         "clipper": _clipper}
REFS = dict(cases.REFS, hpf2=hpf2_ref, a=a_ref, b=b_ref)


def data_x(case, shape=None):
    B, T, ni = shape or SHAPES[case]
    x = (np.random.default_rng(0).standard_normal((B, T, ni)) * 1.2).astype(np.float32)
    return x[:, :, 0] if ni == 1 else x


def forward_of(oracle, case, x):
    tree, probe, theta = REFS[case]()
    nd = theta.size - 4
    if case == "clipper":
        return (lambda th: oracle.clipper_asym_fwd(np.concatenate([th[2:], th[:2]]), float(FS), x)), theta
    return (lambda th: ref.tree_fwd(tree, probe, th, FS, x, ref.asym_root_of(oracle, th, nd))), theta


def sums_of(y, target, skip):
    """S = sum (y - t)^2 and E = sum y^2 over the rows past skip, per sequence -> [B], [B] (fp64)."""
    o, t = y[skip:], target[skip:]
    return ((o - t) ** 2).sum(axis=0), (o ** 2).sum(axis=0)


def loss_of(S, E, n, kind):
    """The loss from the global sums: "mse": S / n; "mse_esr": S / n + sqrt(S / (E + eps) / n)."""
    return S / n if kind == "mse" else S / n + np.sqrt(S / (E + EPS) / n)


class Reference:
    """x, target (float32) and, in fp64, y and y at theta (1 +- h) per component: every loss, gradient and balance of a case at
    a shape comes from these 2 n + 2 forwards, computed once."""

    def __init__(self, oracle, case, shape=None):
        self.case, self.shape = case, shape or SHAPES[case]
        self.x = data_x(case, self.shape)
        f, theta = forward_of(oracle, case, self.x.astype(np.float64))
        self.theta = theta
        teacher = theta * (1.0 + 0.12 * (-1.0) ** np.arange(theta.size))
        self.target = f(teacher).astype(np.float32)
        self.y = f(theta)
        self.yp, self.ym, self.d = [], [], []
        for k in range(theta.size):
            tp, tm = theta.copy(), theta.copy()
            tp[k] *= 1.0 + H
            tm[k] *= 1.0 - H
            self.yp.append(f(tp))
            self.ym.append(f(tm))
            self.d.append(tp[k] - tm[k])
        for v in [self.x, self.target, self.y, self.theta] + self.yp + self.ym:
            v.setflags(write=False)

    def n(self, skip=0):
        B, T, _ = self.shape
        return float(B * (T - skip))

    def sums(self, skip=0):
        S, E = sums_of(self.y, self.target.astype(np.float64), skip)
        return float(S.sum()), float(E.sum())

    def loss(self, kind, skip=0):
        S, E = self.sums(skip)
        return loss_of(S, E, self.n(skip), kind)

    def residual(self):
        """e = y - target of the reference [T,B] (fp64): the MSE's weight is 2 e / n."""
        return self.y - self.target.astype(np.float64)

    def abs_sensitivity(self):
        """sum over every sample of |dy/dtheta_k| (central differences) -> [n]: an error dy in y that enters a weight of the MSE
        moves gradient component k by at most (2 / n) max |dy| times this."""
        return np.array([np.abs((yp - ym) / d).sum() for yp, ym, d in zip(self.yp, self.ym, self.d)])

    def grad_and_balance(self, kind, skip=0):
        """Central differences of the loss itself -> grad [n]; the balance of its per-sequence terms [n]."""
        t64, n = self.target.astype(np.float64), self.n(skip)
        S, E = self.sums(skip)
        E += EPS
        esr = np.sqrt(S / E / n)
        ga, gb = (2.0 / n, 0.0) if kind == "mse" else (2.0 / n + 1.0 / (esr * E * n), -esr / E)
        g, bal = [], []
        for yp, ym, d in zip(self.yp, self.ym, self.d):
            Sp, Ep = sums_of(yp, t64, skip)
            Sm, Em = sums_of(ym, t64, skip)
            g.append((loss_of(Sp.sum(), Ep.sum(), n, kind) - loss_of(Sm.sum(), Em.sum(), n, kind)) / d)
            terms = (ga * 0.5 * (Sp - Sm) + gb * 0.5 * (Ep - Em)) / d          # one per sequence
            bal.append(abs(terms.sum()) / np.abs(terms).sum())
        return np.array(g), np.array(bal)
