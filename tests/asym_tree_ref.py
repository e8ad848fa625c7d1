"""A small fp64 NumPy WDF tree interpreter with a pluggable root: the reference of the tests of the two-different-diode
root on generic trees (the oracle has the scalar exact root, oracle.asym_root, and no tree interpreter for it).

A tree is nested tuples over indices into a parameter vector theta:
    ("R", k)            resistor, R = theta[k]                                 b = 0
    ("V", k, chan)      resistive voltage source, R = theta[k]                  b = x[:, t, chan]
    ("C", k)            capacitor, C = theta[k], port resistance 1/(2 C fs)     b = z, z <- a
    ("S", p1, p2)       series adaptor          ("P", p1, p2)   parallel adaptor
with the reflected / incident rules of lib/tf_wdf.py (Series :157-176, Parallel :179-202, Capacitor :120-142).  The root is
b = root(a, R_port) on [B] vectors; one Python loop over T, vectorised over B.  The probe is one of the tree's own tuples
(matched by identity), y = (a + b) / 2 there.
"""
import numpy as np


class _Node:
    def __init__(self, spec):
        self.spec, self.kind = spec, spec[0]
        self.kids = [_Node(s) for s in spec[1:]] if self.kind in "SP" else []
        self.a = self.b = 0.0

    def walk(self):
        for k in self.kids:
            yield from k.walk()
        yield self

    def impedance(self, theta, fs):
        if self.kind in "RV":
            self.R = theta[self.spec[1]]
        elif self.kind == "C":
            self.R = 1.0 / (theta[self.spec[1]] * (2.0 * fs))
        else:
            p1, p2 = self.kids
            p1.impedance(theta, fs)
            p2.impedance(theta, fs)
            if self.kind == "S":
                self.R = p1.R + p2.R
                self.p1R = p1.R / self.R
            else:
                G1, G2 = 1.0 / p1.R, 1.0 / p2.R
                G = G1 + G2
                self.R = 1.0 / G
                self.p1R = G1 / G

    def reflected(self, xt):
        if self.kind == "R":
            self.b = np.zeros(xt.shape[0])
        elif self.kind == "V":
            self.b = xt[:, self.spec[2]]
        elif self.kind == "C":
            self.b = self.z
        elif self.kind == "S":
            self.b = -(self.kids[0].reflected(xt) + self.kids[1].reflected(xt))
        else:
            b1, b2 = self.kids[0].reflected(xt), self.kids[1].reflected(xt)
            self.b_diff = b2 - b1
            self.b_temp = -self.p1R * self.b_diff
            self.b = b2 + self.b_temp
        return self.b

    def incident(self, x):
        if self.kind == "C":
            self.z = x
        elif self.kind == "S":
            p1, p2 = self.kids
            b1 = p1.b - self.p1R * (x + p1.b + p2.b)
            p1.incident(b1)
            p2.incident(-(x + b1))
        elif self.kind == "P":
            b2 = x + self.b_temp
            self.kids[0].incident(self.b_diff + b2)
            self.kids[1].incident(b2)
        self.a = x


def tree_fwd(tree, probe, theta, fs, x, root):
    """x [B,T] or [B,T,n_in] -> y [T,B] (fp64).  root(a [B], R_port) -> b [B]."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    B, T, _ = x.shape
    theta = np.asarray(theta, dtype=np.float64)
    top = _Node(tree)
    nodes = list(top.walk())
    pn = [n for n in nodes if n.spec is probe]
    assert len(pn) == 1, "probe must be one of the tree's own tuples"
    for n in nodes:
        if n.kind == "C":
            n.z = np.zeros(B)
    top.impedance(theta, float(fs))
    y = np.empty((T, B))
    for t in range(T):
        up = top.reflected(x[:, t, :])
        top.incident(root(up, top.R))
        y[t] = (pn[0].a + pn[0].b) * 0.5
    return y


def asym_root_of(oracle, theta, k):
    """The exact two-diode root with {Is_up, nVt_up, Is_down, nVt_down} = theta[k:k+4]."""
    Is1, V1, Is2, V2 = (float(v) for v in theta[k:k + 4])
    return lambda a, R: oracle.asym_root(a, float(R), Is1, V1, Is2, V2)


def central(f, theta, h):
    """d f / d theta[k] for every k by central differences with relative step h -> array [n, *f.shape]."""
    theta = np.asarray(theta, dtype=np.float64)
    out = []
    for k in range(theta.size):
        tp, tm = theta.copy(), theta.copy()
        tp[k] *= 1.0 + h
        tm[k] *= 1.0 - h
        out.append((f(tp) - f(tm)) / (tp[k] - tm[k]))
    return np.array(out)


def grad_and_balance(f, theta, gy, h=1.0e-5):
    """dL/dtheta for L = sum(y gy) by central differences, and per component |sum of terms| / sum |terms| with one term per
    SEQUENCE, term_b = sum_t gy[t,b] dy[t,b]/dtheta: a relative bound on a component means something only where its terms do
    not cancel.  (One term per time sample cannot serve: gy is zero-mean noise, so B T = 21000 such terms cancel to
    ~1/sqrt(B T) = 0.007 of their absolute sum whatever the seed -- measured 0.005 .. 0.03 over seeds 0..63 on the HPF tree.)
    -> grad [n], balance [n]."""
    terms = (central(f, theta, h) * np.asarray(gy, dtype=np.float64)[None]).sum(axis=1)       # [n, B]
    g = terms.sum(axis=1)
    return g, np.abs(g) / np.abs(terms).sum(axis=1)
