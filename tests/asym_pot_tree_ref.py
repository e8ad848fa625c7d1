"""tests/asym_tree_ref.py's fp64 NumPy tree with a resistance that MOVES: one of the tree's resistances is taken from a channel
r [B,T] instead of the parameter vector, and the impedances are propagated again at every step -- the reference's
set_resistance + calc_impedance every step (clipper_pot.py:116-117).  The root is the oracle's exact two-diode root, called
per element: with a pot the port resistance is a [B] vector, and oracle.asym_root takes a scalar one.

Gradients and the cancellation measure are asym_tree_ref.grad_and_balance's (central differences, h = 1e-5, one term per
sequence), taken over every parameter but the pot's own: the channel replaces it, so it has no derivative.
"""
import numpy as np

import asym_tree_ref as ref


def asym_root_elementwise(oracle, theta, k):
    """root(a [B], R scalar or [B]) -> b [B] with {Is_up, nVt_up, Is_down, nVt_down} = theta[k:k+4]."""
    Is1, V1, Is2, V2 = (float(v) for v in theta[k:k + 4])
    f = oracle.lib().oracle_asym_root_f64

    def root(a, R):
        Rv = np.broadcast_to(np.asarray(R, dtype=np.float64), a.shape)
        return np.array([f(float(ai), float(Ri), Is1, V1, Is2, V2) for ai, Ri in zip(a, Rv)])
    return root


def tree_fwd_pot(tree, probe, theta, fs, x, pot_index, r, root):
    """x [B,T] or [B,T,n_in], r [B,T] (None: no pot, the static tree) -> y [T,B] (fp64); theta[pot_index] is not read."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    B, T, _ = x.shape
    th = [float(v) for v in np.asarray(theta, dtype=np.float64)]
    top = ref._Node(tree)
    nodes = list(top.walk())
    pn = [n for n in nodes if n.spec is probe]
    assert len(pn) == 1, "probe must be one of the tree's own tuples"
    for n in nodes:
        if n.kind == "C":
            n.z = np.zeros(B)
    if r is None:
        top.impedance(th, float(fs))
    else:
        r = np.asarray(r, dtype=np.float64)
        assert r.shape == (B, T)
    y = np.empty((T, B))
    for t in range(T):
        if r is not None:
            th[pot_index] = r[:, t]
            top.impedance(th, float(fs))
        up = top.reflected(x[:, t, :])
        top.incident(root(up, top.R))
        y[t] = (pn[0].a + pn[0].b) * 0.5
    return y


def grad_and_balance(f, theta, gy, pot_index=None, h=1.0e-5):
    """asym_tree_ref.grad_and_balance over every parameter but theta[pot_index] -> grad [n - 1], balance [n - 1] (n without a pot),
    in the order of theta with the pot's entry left out."""
    theta = np.asarray(theta, dtype=np.float64)
    if pot_index is None:
        return ref.grad_and_balance(f, theta, gy, h)
    keep = [k for k in range(theta.size) if k != pot_index]

    def g(sub):
        full = theta.copy()
        full[keep] = sub
        return f(full)
    return ref.grad_and_balance(g, theta[keep], gy, h)
