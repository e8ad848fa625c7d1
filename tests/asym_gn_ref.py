"""numpy, float64: what the Gauss-Newton step of the two-different-diode clipper (csrc/wdf_asym_gn.h) is checked against.

    fd_jacobian     J [T*B, 6] = dy/dtheta6 by central differences of the oracle's exact fp64 forward (relative step 1e-6)
    gn_reference    loss = mean e^2, g = (2/n) J^T e, H = (2/n) J^T J at the fp32-rounded parameters
    lm_reference    a Levenberg-Marquardt loop on those (Marquardt's scaling, lambda 1e-3, x4 up, /3 down), written out on its own
    chunk_* / walk  the record algebra of the kernels on synthetic data: what a chunk accumulates and how the finish walk
                    composes the records
The data, the parameter sets and the teacher are tests/test_gpu_asym_step.py's.  References are computed once per (set, shape,
seed, step) and shared; nobody writes into them.
"""
import numpy as np

FS = 48000.0
VT = 25.85e-3
TEACHER = 1.25
THETA6 = np.array([4.352e-9, VT * 1.906, 2.0e-6, VT * 1.4, 45.0e3, 4.7e-9])
SETS = {
    "theta6": THETA6,
    "swapped": THETA6[[2, 3, 0, 1, 4, 5]],
    "leaky_low_R": np.array([1.0e-4, VT * 1.0, 4.352e-9, VT * 1.906, 10.0e3, 4.7e-9]),
    "schottky_big_R": np.array([1.0e-5, VT * 1.05, 1.0e-12, VT * 1.2, 99.1e3, 1.0e-9]),
}
NAMES = list(SETS)
GAUGE = np.array([1.0, 0.0, 1.0, 0.0, -1.0, 1.0])      # v = theta o GAUGE: (Is_up, Is_down, C) -> s (...), R -> R / s leaves y unchanged
TRI = [(q, r) for q in range(6) for r in range(q, 6)]  # out28[7:28]


def r32(theta):
    return np.asarray(theta).astype(np.float32).astype(np.float64)


def teacher_target(oracle, theta, x):
    """the oracle's forward at the teacher's parameters, as the fp32 array the device reads"""
    return oracle.clipper_asym_fwd(r32(theta) * TEACHER, FS, x.astype(np.float64)).astype(np.float32)


def fd_jacobian(oracle, t64, x, step=1e-6):
    """J [T*B, 6]: central differences of the oracle's forward, relative step `step`"""
    x64 = np.asarray(x, dtype=np.float64)
    cols = []
    for i in range(6):
        h = step * t64[i]
        tp, tm = t64.copy(), t64.copy()
        tp[i] += h
        tm[i] -= h
        cols.append(((oracle.clipper_asym_fwd(tp, FS, x64) - oracle.clipper_asym_fwd(tm, FS, x64)) / (2 * h)).reshape(-1))
    return np.stack(cols, axis=1)


def gn_at(oracle, t64, x, target, step=1e-6):
    """-> loss, g [6], H [6,6] at t64 (used as it is: no rounding)"""
    e = (oracle.clipper_asym_fwd(t64, FS, np.asarray(x, dtype=np.float64)) - np.asarray(target, dtype=np.float64)).reshape(-1)
    J = fd_jacobian(oracle, t64, x, step)
    n = e.size
    return float(e @ e) / n, (2.0 / n) * (J.T @ e), (2.0 / n) * (J.T @ J)


_CACHE = {}


def workload_case(oracle, name, B, T, seed):
    """-> x [B,T] float32, target [T,B] float32 (the teacher's output), both read-only"""
    key = ("case", name, B, T, seed)
    if key not in _CACHE:
        from wdf_hip import workload
        x = workload.sweep_batch(B, T, seed=seed)
        tg = teacher_target(oracle, SETS[name], x)
        x.setflags(write=False)
        tg.setflags(write=False)
        _CACHE[key] = (x, tg)
    return _CACHE[key]


def gn_reference(oracle, name, B, T, seed, step=1e-6):
    """loss, g, H of set `name` at its fp32-rounded parameters on workload_case(name, B, T, seed); cached, read-only"""
    key = ("gn", name, B, T, seed, step)
    if key not in _CACHE:
        x, tg = workload_case(oracle, name, B, T, seed)
        loss, g, H = gn_at(oracle, r32(SETS[name]), x, tg, step)
        g.setflags(write=False)
        H.setflags(write=False)
        _CACHE[key] = (loss, g, H)
    return _CACHE[key]


def scale(H):
    """sqrt(H_qq H_rr) [6,6]: the scale every bound on H is relative to"""
    d = np.sqrt(np.diag(H))
    return np.outer(d, d)


def gauge_residual(H, theta):
    """(v^T H v, sum |v_q v_r| sqrt(H_qq H_rr)) for the gauge direction v = theta o GAUGE"""
    v = np.asarray(theta, dtype=np.float64) * GAUGE
    return float(v @ H @ v), float(np.abs(np.outer(v, v)).ravel() @ scale(H).ravel())


def lm_reference(evaluate, theta0, max_evaluations, lam=1e-3, up=4.0, down=3.0):
    """Levenberg-Marquardt in float64 on evaluate(theta) -> (loss, g, H): Marquardt's scaling D = sqrt(diag H), one evaluation
    per trial, a trial with a non-positive value rejected unevaluated.  -> (theta, [(evaluations so far, loss)] per evaluation
    that was accepted, the first entry the start's)."""
    theta = np.array(theta0, dtype=np.float64)
    loss, g, H = evaluate(theta)
    n_eval, path = 1, [(1, loss)]
    while n_eval < max_evaluations:
        d = np.sqrt(np.diag(H))
        delta = np.linalg.solve(H / np.outer(d, d) + lam * np.eye(len(d)), -g / d) / d
        trial = theta + delta
        if np.all(trial > 0.0):
            lt, gt, Ht = evaluate(trial)
            n_eval += 1
            if lt < loss:
                theta, loss, g, H = trial, lt, gt, Ht
                lam /= down
                path.append((n_eval, loss))
                continue
        lam *= up
        if lam > 1e30:
            break
    return theta, path


def evaluations_to_reach(path, ratio):
    """the number of evaluations after which the loss is <= ratio x the start's, or None"""
    for n, loss in path:
        if loss <= ratio * path[0][1]:
            return n
    return None


# ---- the record algebra on synthetic data: tau' = kappa tau + c, dy = (tau' + tau) / 2 ------------------------------------------
def unsplit(kappa, c, e):
    """the whole series in one go from tau = 0 -> G [6] = sum e dy, H [6,6] = sum dy dy^T"""
    tau, G, H = np.zeros(6), np.zeros(6), np.zeros((6, 6))
    for t in range(len(kappa)):
        new = kappa[t] * tau + c[t]
        dy = 0.5 * (new + tau)
        G += e[t] * dy
        H += np.outer(dy, dy)
        tau = new
    return G, H


def chunk_record(kappa, c, e):
    """what one chunk accumulates from ZERO entering tangent: {P, A, q[6], beta[6], M2, N[6], H0[6,6]} (csrc/wdf_asym_gn.h)"""
    tau, m = np.zeros(6), 1.0
    A, beta, M2, N, H0 = 0.0, np.zeros(6), 0.0, np.zeros(6), np.zeros((6, 6))
    for t in range(len(kappa)):
        new, m_new = kappa[t] * tau + c[t], kappa[t] * m
        u, w = 0.5 * (new + tau), 0.5 * (m_new + m)
        A += e[t] * w
        beta += e[t] * u
        M2 += w * w
        N += w * u
        H0 += np.outer(u, u)
        tau, m = new, m_new
    return dict(P=m, A=A, q=tau, beta=beta, M2=M2, N=N, H0=H0)


def walk(records):
    """the finish kernel's walk over a sequence's records, first to last, tau = 0 entering the first -> G [6], H [6,6]"""
    tau, G, H = np.zeros(6), np.zeros(6), np.zeros((6, 6))
    for r in records:
        G += r["A"] * tau + r["beta"]
        H += r["M2"] * np.outer(tau, tau) + np.outer(tau, r["N"]) + np.outer(r["N"], tau) + r["H0"]
        tau = r["P"] * tau + r["q"]
    return G, H


def chunked(kappa, c, e, n_chunks):
    bounds = np.linspace(0, len(kappa), n_chunks + 1).astype(int)
    return walk([chunk_record(kappa[a:b], c[a:b], e[a:b]) for a, b in zip(bounds[:-1], bounds[1:])])
