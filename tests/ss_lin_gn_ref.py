"""The reference of the linear trees' Gauss-Newton step (csrc/wdf_ss_lin_gn.h: wdf_ss_lin_step_gn), numpy only, for
tests/test_ss_lin_gn_cpu.py, tests/test_gpu_ss_lin_gn_kernel.py and tests/test_gpu_circuit_lin_gn.py.

ss_lin_ref.run() restates the step's recursion directly and returns the weighted sums; this module restates the same recursion
and keeps the per-row tangents of the output themselves,

    d[t, r, b] = dy[t, b] / d coefficient_r ,   r over {A, Bx, cy, dy} in the kernel's order (ss_lin_ref.rows)
               = cy . S_{A_ij}  |  cy . S_{Bx_ij}  |  z_s  |  x_i

in float64, or with every product and state in float32 (the rounding floor the kernel is judged against); sums over rows and
sequences are float64 in both, as in ss_lin_ref.  From d:

    Hc   = sum d d^T                    [kG, kG]   the Gauss-Newton matrix in coefficient space (before gscale)
    magH = sum |d| |d|^T                [kG, kG]   what an entry's rounding error scales with
    H    = gscale J^T Hc J              [P, P]     J = jac[rows]: the chain rule to the component values

Also here: the cases of the GPU kernel module (one list, so that the CPU file measures the reference's own fp32-against-fp64
distance over exactly the cases the GPU bound is used on), the two fits of the Circuit module, and the reference composed with
probe_tape's host evaluation of a circuit's probed step.
"""
import functools

import numpy as np

import ss_lin_ref as R


class Result:
    pass


def tangents(ns, ni, coef, x, z0=None, dtype=np.float64):
    """x [T,ni,B], coef [>= ncoef], z0 [ns,B] | None -> y [T,B], d [T,kG,B], zT [ns,B] (dtype)."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    c = np.asarray(coef).astype(dt)
    T, _, B = x.shape
    o = R.offsets(ns, ni)
    A = c[o["A"]:o["A"] + ns * ns].reshape(ns, ns)
    Bx = c[o["B"]:o["B"] + ns * ni].reshape(ns, ni)
    cy, dy = c[o["cy"]:o["cy"] + ns], c[o["dy"]:o["dy"] + ni]
    nA, nB, G = ns * ns, ns * ni, R.kg(ns, ni)
    z = np.zeros((ns, B), dt) if z0 is None else np.asarray(z0).astype(dt).reshape(ns, B).copy()
    SA, SB = np.zeros((nA, ns, B), dt), np.zeros((nB, ns, B), dt)
    y = np.empty((T, B), dt)
    d = np.empty((T, G, B), dt)
    for t in range(T):
        xt = x[t]
        yv = np.zeros(B, dt)
        for i in range(ni):
            yv = yv + dy[i] * xt[i]
        for s in range(ns):
            yv = yv + cy[s] * z[s]
        y[t] = yv
        dA, dB = np.zeros((nA, B), dt), np.zeros((nB, B), dt)
        for s in range(ns):
            dA = dA + cy[s] * SA[:, s]
            dB = dB + cy[s] * SB[:, s]
        d[t, :nA], d[t, nA:nA + nB] = dA, dB
        d[t, nA + nB:nA + nB + ns], d[t, nA + nB + ns:] = z, xt
        injA, injB = np.zeros((nA, ns, B), dt), np.zeros((nB, ns, B), dt)
        for i in range(ns):
            for j in range(ns):
                injA[i * ns + j, i] = z[j]
            for j in range(ni):
                injB[i * ni + j, i] = xt[j]
        for q in range(ns):
            injA = injA + A[None, :, q, None] * SA[:, q:q + 1]
            injB = injB + A[None, :, q, None] * SB[:, q:q + 1]
        SA, SB = injA, injB
        zn = np.zeros((ns, B), dt)
        for i in range(ni):
            zn = zn + Bx[:, i:i + 1] * xt[i][None]
        for q in range(ns):
            zn = zn + A[:, q:q + 1] * z[q][None]
        z = zn
    return y, d, z


def run(ns, ni, coef, x, target, gscale, z0=None, dtype=np.float64):
    """-> y, d, zT (dtype); sse, g [kG] = gscale sum e d, Hc, magH [kG,kG] (float64 sums of dtype products)."""
    dt = np.dtype(dtype).type
    r = Result()
    r.y, r.d, r.zT = tangents(ns, ni, coef, x, z0, dtype)
    e = r.y - np.asarray(target).astype(dt)
    r.sse = float((e * e).astype(np.float64).sum())
    gs = dt(np.float32(gscale))
    r.g = ((gs * e)[:, None, :] * r.d).astype(np.float64).sum(axis=(0, 2))
    G = r.d.shape[1]
    r.Hc, r.magH = np.zeros((G, G)), np.zeros((G, G))
    for i in range(G):
        for j in range(i, G):
            p = (r.d[:, i] * r.d[:, j]).astype(np.float64)        # (the product in dtype, the sum in float64)
            r.Hc[i, j] = r.Hc[j, i] = p.sum()
            r.magH[i, j] = r.magH[j, i] = np.abs(p).sum()
    return r


def upper(M):
    """the upper triangle of a square matrix by rows: the layout of hcoef and of out[1 + P:]"""
    return M[np.triu_indices(M.shape[0])]


def chain(ns, ni, Hc, jac, gscale):
    """H = gscale J^T Hc J with J = jac[rows] (float64; gscale as the kernel holds it, a float32)"""
    J = np.asarray(jac, np.float64)[R.rows(ns, ni)]
    return float(np.float32(gscale)) * (J.T @ Hc @ J)


def chain_bound(ns, ni, magH, jac, b_h, gscale):
    """sum_ij b_h magH_ij |J_iq| |J_jr| (times gscale): what H_qr may be off by when every Hc_ij is within b_h magH_ij"""
    J = np.abs(np.asarray(jac, np.float64)[R.rows(ns, ni)])
    return float(np.float32(gscale)) * b_h * (J.T @ magH @ J)


# ---- the cases of tests/test_gpu_ss_lin_gn_kernel.py -----------------------------------------------------------------------------
SHAPES = [(1, 40, 1), (65, 100, 4), (130, 257, 3), (2, 33, 2)]     # (B, T, n_chunks): dead lanes, a second wave with one live lane
#                                                                    (B = 65: one per lane; 130: two per lane, a third wave of
#                                                                    two lanes on (2,2)), both lane widths, a ragged last chunk
MISALIGNED = (1, 1, "plain", 64, 100, False)                       # at 4 chunks, x / target / y one float into their storage
STATE_TREES = [(1, 1), (2, 2)]                                     # z0 and zT at B in {65, 130}, T = 257 in 3 chunks
STATE_BATCHES = [65, 130]
LONG_WALK = (2, 1, "plain", 65, 2048, False)                       # 64 chunks
SLOW = [((1, 1, "slow", 130, 2048, False), 8), ((2, 1, "slow", 65, 2048, False), 64)]
PARAMS = [1, 2, 15]                                                # on (2,2) B = 130, T = 257: 15 gives 120 entries of H
PARAMS_CASE = (2, 2, "plain", 130, 257, False)


def gpu_case_keys():
    keys = [(ns, ni, "plain", B, T, False) for ns, ni in R.TREES for B, T, _ in SHAPES]
    keys += [MISALIGNED]
    keys += [(ns, ni, "plain", B, 257, True) for ns, ni in STATE_TREES for B in STATE_BATCHES]
    keys += [LONG_WALK] + [k for k, _ in SLOW] + [PARAMS_CASE]
    return list(dict.fromkeys(keys))


@functools.lru_cache(maxsize=None)
def ref(key, dtype_name="float64"):
    """the reference of a case (ss_lin_ref.case's inputs), computed once per process and left unchanged"""
    c = R.case(*key)
    return run(c.ns, c.ni, c.coef, c.x, c.target, c.gscale, z0=c.z0, dtype=np.dtype(dtype_name))


def h_distance(key):
    """max |Hc32 - Hc64| / magH of the float32 restatement on one case"""
    r64, r32 = ref(key), ref(key, "float32")
    assert np.all(r64.magH > 0)
    return float(np.max(np.abs(r32.Hc - r64.Hc) / r64.magH))


# B_H: the bound on hcoef_ij / magH_ij.  FLOOR is max h_distance over gpu_case_keys(), measured by
# tests/test_ss_lin_gn_cpu.py::test_the_float32_restatement_stays_under_the_floor (which asserts it): 5.64e-7 at (1,2) B = 2,
# T = 33 (66 rows: nothing averages out), written down here rounded up.  8 x that allows for fused against separate roundings
# and one affine map per chunk boundary; the kernel adds 32 addends in fp32 before it goes to double: at most 32 x 2^-24.
FLOOR = 5.7e-7
B_H = 8 * FLOOR + 32 * 2.0 ** -24                                  # = 6.5e-6


# ---- a circuit's probed step (lib/wdf_hip/probe_tape.py) composed with the reference -----------------------------------------------
def circuit_gn(tape, outs, ns, ni, values, x_tm, target, z0=None):
    """tape.evaluate (float64 coefficients and their Jacobian at `values`) -> loss = mean squared error, g [P], H [P,P] =
    (2/N) J^T J and y, all float64.  outs: the coefficient nodes, then the port resistance's (ignored by the step)."""
    coef, jac = tape.evaluate([float(v) for v in values], outs)
    T, _, B = np.asarray(x_tm).shape
    gscale = 2.0 / (B * T)
    y, d, _ = tangents(ns, ni, coef, x_tm, z0)
    e = y - np.asarray(target, np.float64)
    J = jac[R.rows(ns, ni)]
    dth = np.einsum("tgb,gp->tpb", d, J)                          # dy/d component value at every row
    g = gscale * np.einsum("tb,tpb->p", e, dth)
    H = gscale * np.einsum("tpb,tqb->pq", dth, dth)
    return float((e * e).sum() / (B * T)), g, H, y


FS = 48000
# lpf.py's tree and start (R = 1000, C = 1 uF) towards a teacher at another R C; voltage_divider.py's towards another R1 / R2.
# values in the order of the resident block (tree order)
LPF = dict(start=(1000.0, 1.0e-6), teacher=(2700.0, 2.2e-6), B=4, T=1280)
DIVIDER = dict(start=(2000.0, 100.0), teacher=(1000.0, 3300.0), B=4, T=256)


def fit_input(B, T, seed):
    """[T,1,B] float32: a few sines of different frequency per sequence plus noise, as x_tm"""
    rng = np.random.default_rng([B, T, seed])
    t = np.arange(T)[:, None] / FS
    f = rng.uniform(50.0, 2000.0, (1, B))
    x = np.sin(2 * np.pi * f * t) + 0.5 * np.sin(2 * np.pi * 3.7 * f * t + 1.0) + 0.05 * rng.standard_normal((T, B))
    return x[:, None, :].astype(np.float32)


def build_lpf(W, values=None, trainable=(True, True)):
    """lpf.py:20-28's tree -> (Circuit, [R1.R, C1.C]): the order of the resident block"""
    v = LPF["start"] if values is None else values
    Vs, R1, C1 = W.IdealVoltageSource(), W.Resistor(v[0], trainable[0]), W.Capacitor(v[1], FS, trainable[1])
    return W.Circuit(W.Inverter(W.Series(R1, C1)), Vs, C1), [R1.R, C1.C]


def build_divider(W, values=None):
    """voltage_divider.py:19-27's tree (no capacitor) -> (Circuit, [R1.R, R2.R])"""
    v = DIVIDER["start"] if values is None else values
    Vs, R1, R2 = W.IdealVoltageSource(), W.Resistor(v[0], True), W.Resistor(v[1], True)
    return W.Circuit(W.Inverter(W.Series(R1, R2)), Vs, R1), [R1.R, R2.R]


FITS = {"lpf": (LPF, build_lpf), "divider": (DIVIDER, build_divider)}


@functools.lru_cache(maxsize=None)
def fit_data(which):
    """-> (x_tm [T,1,B] float32, target [T,B] float32: the float64 reference at the teacher's values, rounded once)"""
    import tf_wdf as W
    from wdf_hip import probe_tape
    spec, build = FITS[which]
    circ, pvars = build(W)
    tape, outs, rport = probe_tape.record(circ, pvars)
    x = fit_input(spec["B"], spec["T"], 1)
    y = circuit_gn(tape, list(outs) + [rport], circ.ns, circ.ni, spec["teacher"], x, np.zeros((spec["T"], spec["B"])))[3]
    return x, y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference_fit(which):
    """LevenbergMarquardt on the float64 reference composed with the probe tape's host evaluation, float64 Variables under the
    elements' own constraints -> ([(evaluations, loss)], the starting loss)"""
    import tf_wdf as W
    from wdf_hip import probe_tape
    spec, build = FITS[which]
    circ, pvars = build(W)
    tape, outs, rport = probe_tape.record(circ, pvars)
    outs = list(outs) + [rport]
    x, target = fit_data(which)
    vs = [W.tf.Variable(v, dtype=W.tf.float64, trainable=True, constraint=p.constraint) for v, p in zip(spec["start"], pvars)]
    return lm_path(lambda: circuit_gn(tape, outs, circ.ns, circ.ni, [float(v) for v in vs], x, target)[:3], vs, 40)


def lm_path(evaluate, variables, n_max, **kw):
    """wdf_hip.lm.LevenbergMarquardt on evaluate() -> [(evaluations, loss)] after every step, the starting loss"""
    from wdf_hip import lm
    opt = lm.LevenbergMarquardt(evaluate, variables, **kw)
    path = []
    while opt.evaluations < n_max:
        loss = opt.step()
        path.append((opt.evaluations, loss))
        if loss <= 1e-12 * opt.start_loss:
            break
    return path, opt.start_loss


def evaluations_to_reach(path, start, ratio):
    for n, loss in path:
        if loss <= ratio * start:
            return n
    return None
