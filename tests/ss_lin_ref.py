"""The reference of the linear one-pass step (csrc/wdf_ss_step.h: wdf_ss_lin_step_mse) and of its device probe (ss_probe_kernel),
numpy only, for tests/test_ss_lin_ref_cpu.py and tests/test_gpu_ss_lin_step_kernel.py.

The step is restated DIRECTLY -- no chunks, no affine map, no partial sums: with coef in SSCoef order (csrc/wdf_statespace.h:45-48;
E, ca, da, fy unused)

    z' = A z + Bx x ;  y = cy . z + dy . x ;  e = y - target ;  g = gscale e
    S_{A_ij}' = A S_{A_ij} + e_i z_j ;  S_{Bx_ij}' = A S_{Bx_ij} + e_i x_j            (the tangents dz/dc, from 0)
    dLoss/dA_ij = sum g cy . S_{A_ij} ;  dLoss/dBx_ij = sum g cy . S_{Bx_ij} ;  dLoss/dcy_s = sum g z_s ;  dLoss/ddy_i = sum g x_i

run() steps it in float64, or with every product and state in float32 (the rounding floor the kernel is judged against); sums over
samples and sequences are float64 in both.  Beside every gradient entry it returns mag_i = sum |g| |addend|: what the entry's rounding
error scales with (|g_i| / mag_i goes down to 0.001 on these cases, so a relative bound on g_i itself would mean nothing).

Also here: the coefficient families and the cases of the GPU module (one list, so that the CPU file can assert the reference's own
fp32-against-fp64 caps over exactly the cases the GPU bounds are used on), the builder of random probe tapes and the tape's
evaluation with a magnitude pass.
"""
import functools

import numpy as np

OP_CONST, OP_PARAM, OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_NEG, OP_RECIP = range(8)          # lib/wdf_hip/probe_tape.py


# ---- layout ------------------------------------------------------------------------------------------------------------------
def ncoef(ns, ni):
    return ns * ns + ns * ni + ns + ns + ni + ns + ni + 1


def offsets(ns, ni):
    """SSCoef<NS, NI>: A, Bx, E, ca, da, cy, dy, fy"""
    oA, oB = 0, ns * ns
    oE = oB + ns * ni
    oCa = oE + ns
    oDa = oCa + ns
    oCy = oDa + ni
    oDy = oCy + ns
    return dict(A=oA, B=oB, E=oE, ca=oCa, da=oDa, cy=oCy, dy=oDy, fy=oDy + ni)


def kg(ns, ni):
    return ns * ns + ns * ni + ns + ni


def rows(ns, ni):
    """the coefficient (SSCoef index) of every gradient entry, in the kernel's order {A, Bx, cy, dy}"""
    o = offsets(ns, ni)
    return ([o["A"] + i for i in range(ns * ns)] + [o["B"] + i for i in range(ns * ni)] + [o["cy"] + i for i in range(ns)]
            + [o["dy"] + i for i in range(ni)])


# ---- the recursion -----------------------------------------------------------------------------------------------------------
class Result:
    pass


def run(ns, ni, coef, x, target, gscale, z0=None, dtype=np.float64, grads=True):
    """x [T,ni,B], target [T,B], coef [>= ncoef], z0 [ns,B] | None (a constant of the call: the tangents start at 0): float32 inputs.
    -> y [T,B] (dtype), sse, zT [ns,B], g [kG] and mag [kG] (float64)."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    target = np.asarray(target).astype(dt)
    c = np.asarray(coef).astype(dt)
    T, _, B = x.shape
    assert x.shape[1] == ni and target.shape == (T, B) and c.size >= ncoef(ns, ni)
    o = offsets(ns, ni)
    A = c[o["A"]:o["A"] + ns * ns].reshape(ns, ns)
    Bx = c[o["B"]:o["B"] + ns * ni].reshape(ns, ni)
    cy, dy = c[o["cy"]:o["cy"] + ns], c[o["dy"]:o["dy"] + ni]
    gs = dt(np.float32(gscale))
    nA, nB, G = ns * ns, ns * ni, kg(ns, ni)
    z = np.zeros((ns, B), dt) if z0 is None else np.asarray(z0).astype(dt).reshape(ns, B).copy()
    SA, SB = np.zeros((nA, ns, B), dt), np.zeros((nB, ns, B), dt)
    y = np.empty((T, B), dt)
    esq = np.empty((T, B), dt)
    add = np.empty((T, G, B), dt) if grads else None
    for t in range(T):
        xt = x[t]
        yv = np.zeros(B, dt)
        for i in range(ni):
            yv = yv + dy[i] * xt[i]
        for s in range(ns):
            yv = yv + cy[s] * z[s]
        e = yv - target[t]
        y[t], esq[t] = yv, e * e
        if grads:
            g = gs * e
            dA, dB = np.zeros((nA, B), dt), np.zeros((nB, B), dt)
            for s in range(ns):
                dA = dA + cy[s] * SA[:, s]
                dB = dB + cy[s] * SB[:, s]
            a = add[t]
            a[:nA], a[nA:nA + nB] = g * dA, g * dB
            a[nA + nB:nA + nB + ns], a[nA + nB + ns:] = g * z, g * xt
            injA, injB = np.zeros((nA, ns, B), dt), np.zeros((nB, ns, B), dt)
            for i in range(ns):
                for j in range(ns):
                    injA[i * ns + j, i] = z[j]                    # S_{A_ij}' = A S + e_i z_j
                for j in range(ni):
                    injB[i * ni + j, i] = xt[j]                   # S_{Bx_ij}' = A S + e_i x_j
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
    r = Result()
    r.y, r.zT, r.sse = y, z, float(esq.astype(np.float64).sum())
    if grads:
        a64 = add.astype(np.float64)
        r.g, r.mag = a64.sum(axis=(0, 2)), np.abs(a64).sum(axis=(0, 2))
    return r


def loss_of(ns, ni, coef, x, target, gscale, z0=None):
    """gscale / 2 x the sum of squared errors, float64, at float64 coefficients (what central differences step)"""
    return 0.5 * gscale * run(ns, ni, coef, x, target, gscale, z0=z0, grads=False).sse


# ---- coefficient families ----------------------------------------------------------------------------------------------------
FAMILIES = ("plain", "slow", "neg", "fast", "complex")
POLES = {1: {"plain": (0.98,), "slow": (0.9995,), "neg": (-0.98,), "fast": (0.3,)},
         2: {"plain": (0.98, 0.6), "slow": (0.9995, 0.9), "neg": (-0.98, 0.5), "fast": (0.3, -0.2)}}
Q = np.array([[1.0, 0.4], [-0.3, 1.0]])


def families(ns):
    return ("plain",) if ns == 0 else (FAMILIES[:4] if ns == 1 else FAMILIES)


def coefs(ns, ni, family, rng):
    """float32 [ncoef + 1] (the last entry stands for the probe's port resistance: jac has a row for it, the step ignores it):
    A with the family's poles, Bx uniform in [-1, 1] scaled by 1 - max |pole| (|y| stays O(1)), cy, dy uniform in [-1, 1]."""
    c = np.zeros(ncoef(ns, ni) + 1)
    o = offsets(ns, ni)
    if ns == 1:
        A = np.array([[POLES[1][family][0]]])
        rho = abs(A[0, 0])
    elif ns == 2 and family == "complex":
        A = 0.97 * np.array([[np.cos(0.3), -np.sin(0.3)], [np.sin(0.3), np.cos(0.3)]])
        rho = 0.97
    elif ns == 2:
        lam = POLES[2][family]
        A = Q @ np.diag(lam) @ np.linalg.inv(Q)
        rho = max(abs(v) for v in lam)
    if ns:
        c[o["A"]:o["A"] + ns * ns] = A.reshape(-1)
        c[o["B"]:o["B"] + ns * ni] = (1.0 - rho) * rng.uniform(-1.0, 1.0, ns * ni)
        c[o["cy"]:o["cy"] + ns] = rng.uniform(-1.0, 1.0, ns)
    c[o["dy"]:o["dy"] + ni] = rng.uniform(-1.0, 1.0, ni)
    c[-1] = 1.0e3
    return c.astype(np.float32)


# ---- cases -------------------------------------------------------------------------------------------------------------------
# the offset's amplitude.  At 1.0 the state of a slow pole carries so much of y that the float32 restatement itself leaves the
# 4e-7 cap of tests/test_ss_lin_ref_cpu.py (9.6e-7 on (1,1) slow B = 130: 1 / (1 - 0.9995^2) = 1000 steps of rounding add up in z)
OFFSET = 0.3


class Case:
    """Inputs of one call (float32, from a fixed seed) and its references: ref() in float64, ref(np.float32) the float32 restatement."""

    def __init__(self, ns, ni, family, B, T, z0=False, seed=0):
        self.key = (ns, ni, family, B, T, bool(z0), seed)
        self.ns, self.ni, self.family, self.B, self.T = ns, ni, family, B, T
        rng = np.random.default_rng([ns, ni, FAMILIES.index(family), B, T, int(z0), seed])
        self.coef = coefs(ns, ni, family, rng)
        # white noise on an offset of its own per sequence and channel: a slow pole has something to remember
        self.x = (rng.standard_normal((T, ni, B)) + OFFSET * rng.uniform(-1.0, 1.0, (1, ni, B))).astype(np.float32)
        self.z0 = rng.standard_normal((ns, B)).astype(np.float32) if (z0 and ns) else None
        self.gscale = 2.0 / (B * T)
        y = run(ns, ni, self.coef, self.x, np.zeros((T, B), np.float32), 0.0, z0=self.z0, grads=False).y
        # (no gradient entry a sum of pure noise)
        self.target = (0.8 * y + 0.1 * np.max(np.abs(y)) * rng.standard_normal((T, B))).astype(np.float32)
        self._ref = {}

    def ref(self, dtype=np.float64):
        k = np.dtype(dtype).name
        if k not in self._ref:
            self._ref[k] = run(self.ns, self.ni, self.coef, self.x, self.target, self.gscale, z0=self.z0, dtype=dtype)
        return self._ref[k]

    def part(self, t0, t1, z0):
        """the steps t0..t1 of this case as a call of their own, from the states z0 [ns,B] (float32)"""
        c = object.__new__(Case)
        c.key = self.key + (t0, t1)
        c.ns, c.ni, c.family, c.B, c.T = self.ns, self.ni, self.family, self.B, t1 - t0
        c.coef, c.x, c.target = self.coef, self.x[t0:t1], self.target[t0:t1]
        c.z0 = z0
        c.gscale, c._ref = 2.0 / (c.B * c.T), {}
        return c

    def __repr__(self):
        ns, ni, fam, B, T, z0 = self.key[:6]
        return f"({ns},{ni}) {fam} B={B} T={T}" + (" z0" if z0 else "") + (f" [{self.key[7]}:{self.key[8]}]" if len(self.key) > 7 else "")


@functools.lru_cache(maxsize=None)
def case(ns, ni, family, B, T, z0=False, seed=0):
    return Case(ns, ni, family, B, T, z0, seed)


TREES = [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2)]
# section A: (B, T, n_chunks); odd B: one sequence per lane, even B: two
SHAPES_A = [(1, 40, 1), (65, 100, 4), (129, 257, 3), (2, 33, 2), (126, 100, 4), (130, 257, 3)]
MISALIGNED_A = [(1, 1), (2, 2)]                                   # at (64, 100, 4)
# section B
TREES_B = [(1, 1), (2, 1), (2, 2)]
GEOM_B = [(32, 1), (33, 2), (64, 2), (65, 3), (100, 8), (1000, 5), (2048, 64)]
BATCHES = [65, 130]
# section C: ns in {1, 2}, (T, n_chunks) = (257, 3); D: (B, 200, 4), `slow` at T = 2048 with n_chunks in {1, 8, 64}
TREES_C = [(1, 1), (2, 2)]
TREES_D = [(1, 1), (1, 2), (2, 1), (2, 2)]
SLOW_CHUNKS = [1, 8, 64]
PARAMS_E = [1, 2, 15]


def gpu_case_keys():
    """every (ns, ni, family, B, T, z0) the GPU module runs the step on, once each"""
    keys = []
    for ns, ni in TREES:
        keys += [(ns, ni, "plain", B, T, False) for B, T, _ in SHAPES_A]
    for ns, ni in MISALIGNED_A:
        keys += [(ns, ni, "plain", 64, 100, False), (ns, ni, "plain", 64, 100, True)]
    for ns, ni in TREES_B:
        keys += [(ns, ni, "plain", B, T, False) for B in BATCHES for T, _ in GEOM_B]
    for ns, ni in TREES_C:
        for B in BATCHES:
            keys += [(ns, ni, "plain", B, 257, False)]
    keys += [(0, 1, "plain", 65, 257, False)]
    for ns, ni in TREES_D:
        for fam in families(ns):
            keys += [(ns, ni, fam, B, 2048 if fam == "slow" else 200, False) for B in BATCHES]
    keys += [(2, 2, "plain", 130, 257, False)]                    # section E
    return list(dict.fromkeys(keys))


@functools.lru_cache(maxsize=None)
def carried(ns, ni, B, T=257):
    """section C: 2 T steps from a random z0 as two calls of T; the second starts from the float64 states the first one's
    reference ends in, so that the two references together ARE the run over the 2 T inputs (asserted on the CPU)"""
    whole = case(ns, ni, "plain", B, 2 * T, True)
    first = whole.part(0, T, whole.z0)
    return whole, first, whole.part(T, 2 * T, first.ref().zT)


def gpu_cases():
    """every call the GPU module compares with a reference: the cases of gpu_case_keys() and section C's halves"""
    cs = [case(*k) for k in gpu_case_keys()]
    for ns, ni in TREES_C:
        for B in BATCHES:
            cs += list(carried(ns, ni, B)[1:])
    return cs


# ---- the probe ---------------------------------------------------------------------------------------------------------------
def _node(i, op, a, b, consts, params, val, tan, vm, tm):
    """node i of a tape into the four arrays: value, tangents, and the same recurrences on absolute values"""
    dt = val.dtype.type
    tan[i], tm[i] = 0, 0
    if op == OP_CONST:
        val[i] = dt(consts[a])
        vm[i] = abs(val[i])
    elif op == OP_PARAM:
        val[i] = dt(params[a])
        vm[i] = abs(val[i])
        tan[i, a] = tm[i, a] = dt(1.0)
    elif op in (OP_ADD, OP_SUB):
        sg = dt(1.0) if op == OP_ADD else dt(-1.0)
        val[i], tan[i] = val[a] + sg * val[b], tan[a] + sg * tan[b]
        vm[i], tm[i] = vm[a] + vm[b], tm[a] + tm[b]
    elif op == OP_MUL:
        val[i], tan[i] = val[a] * val[b], tan[a] * val[b] + val[a] * tan[b]
        vm[i], tm[i] = vm[a] * vm[b], tm[a] * vm[b] + vm[a] * tm[b]
    elif op == OP_DIV:
        q = val[a] / val[b]
        val[i], tan[i] = q, (tan[a] - q * tan[b]) / val[b]
        qm = vm[a] / vm[b]
        vm[i], tm[i] = qm, (tm[a] + qm * tm[b]) / vm[b]
    elif op == OP_NEG:
        val[i], tan[i], vm[i], tm[i] = -val[a], -tan[a], vm[a], tm[a]
    elif op == OP_RECIP:
        r = dt(1.0) / val[a]
        val[i], tan[i] = r, -r * r * tan[a]
        rm = dt(1.0) / vm[a]
        vm[i], tm[i] = rm, rm * rm * tm[a]


def evaluate_mag(ops, consts, params, outs, dtype=np.float64):
    """probe_tape.Tape.evaluate with a magnitude pass: the same recurrences on absolute values.
    -> val [n_out], jac [n_out, P], vmag [n_out], tmag [n_out, P]: a rounding of relative size u anywhere moves val by at most
    (its count) u vmag and jac by (its count) u tmag -- the divisors are leaves, so no magnitude is divided by a computed value."""
    dt = np.dtype(dtype).type
    P, n = len(params), len(ops)
    val, vm = np.zeros(n, dt), np.zeros(n, dt)
    tan, tm = np.zeros((n, P), dt), np.zeros((n, P), dt)
    for i, (op, a, b) in enumerate(ops):
        _node(i, op, a, b, consts, params, val, tan, vm, tm)
    o = np.asarray(outs, dtype=np.int64)
    return val[o], tan[o], vm[o], tm[o]


def random_tape(n_ops, P, seed, n_consts=8):
    """A tape of n_ops operations in the manner of tests/test_gpu_ss_dyn.py::test_rows_at_the_largest_tape_the_device_takes: PARAM
    and CONST leaves first, then ADD / SUB / MUL / NEG on earlier nodes and DIV / RECIP whose divisor is a leaf.  A drawn operation
    whose magnitude at `params` leaves [1e-3, 1e3] (value) or 1e6 (tangents) is drawn again, so that nothing overflows however long
    the tape.  -> ops [n_ops][3] (lists), consts float64, params float32 [P] (values in 0.7..1.3)."""
    rng = np.random.default_rng([n_ops, P, seed])
    params = rng.uniform(0.7, 1.3, P).astype(np.float32)
    consts = rng.uniform(0.5, 1.5, n_consts)
    if n_ops == 1:
        return [[OP_PARAM, 0, 0]], consts, params
    n_leaf_p = min(P, max(1, n_ops // 2))
    n_leaf_c = min(n_consts, 1 + P // 2, max(0, n_ops // 2 - n_leaf_p))        # (few parameters: few constants to dilute them)
    ops = [[OP_PARAM, p, 0] for p in range(n_leaf_p)] + [[OP_CONST, j, 0] for j in range(n_leaf_c)]
    n_leaf = len(ops)
    val, vm = np.zeros(n_ops), np.zeros(n_ops)
    tan, tm = np.zeros((n_ops, P)), np.zeros((n_ops, P))
    for i, (op, a, b) in enumerate(ops):
        _node(i, op, a, b, consts, params, val, tan, vm, tm)
    while len(ops) < n_ops:
        i = len(ops)
        for _ in range(64):
            a, b, lf = int(rng.integers(0, i)), int(rng.integers(0, i)), int(rng.integers(0, n_leaf))
            cand = [[OP_ADD, a, b], [OP_SUB, a, b], [OP_MUL, a, b], [OP_NEG, a, 0], [OP_DIV, a, lf], [OP_RECIP, lf, 0]][int(rng.integers(0, 6))]
            _node(i, *cand, consts, params, val, tan, vm, tm)
            if 1e-3 <= vm[i] <= 1e3 and tm[i].max() <= 1e6:
                break
        else:
            cand = [OP_NEG, int(rng.integers(0, n_leaf)), 0]
            _node(i, *cand, consts, params, val, tan, vm, tm)
        ops.append(cand)
    return ops, consts, params
