"""The reference of the input gradient dL/dx of the static state-space kernels (csrc/wdf_statespace.h: ss_bwd_gx_kernel), numpy only,
for tests/test_ss_gx_ref_cpu.py, tests/test_gpu_ss_gx.py and tests/test_gpu_circuit_input_grad.py.  It stands on
tests/ss_static_ref.py and changes nothing there: run(...) gives the forward (zs, a, b), Da and the coefficients' split; this file
repeats the adjoint walk of run() for L = sum(y gy) and keeps what falls out of it one line before the update (lam = dL/dz', the
adjoint of the state AFTER step t, 0 behind the last step):

    gb = fy g + E . lam ;  ga = gb Da
    gx[t][i] = dy[i] g + da[i] ga + sum_s Bx[s][i] lam[s]
    lam <- ca ga + cy g + A^T lam

gx is [T,ni,B], time-major as the kernel writes it.  Beside it stands mag [T,ni,B]: the SAME walk on absolute values (|coef|, |g|,
|Da|) -- an upper bound of the sum of |addend| behind every entry, what the entry's rounding error scales with.  An entry of gx can
cancel to nothing while its addends do not, so errors are measured against the channel's magnitude, mag's maximum over t and b
(channel_mag), with ss_static_ref's own bounds: G_NL under a root, g_lin(ns + ni + 2) on linear trees (an entry is the sum of
ns + 2 float32 products, and gb behind it of ns + 1: at most ns + ni + 2 addends summed in float32 before anything is rounded again;
the adjoint's own error is what the float32 mode's cap, eight times over, is there for).

walk(dtype=np.float32) is the float32 mode, built the way run(dtype=np.float32) is: the adjoint, every product and every per-step
value rounded to float32 (Da is the float32 run's: the float64 root's slope at the float32 a, rounded), every sum float64.

Cases: the GPU module's, from ss_static_ref's generators.  case(...) takes ss_static_ref.case's seed unless the float32 mode of gx
misses an eighth of the cap there (half of that on calls of fewer than FEW steps, seed_of's rule); then the next seed that keeps it.
The cap never changes.
"""
import functools

import numpy as np

import ss_static_ref as R


class Gx:
    pass


def walk(ns, ni, coef, res, gy, dtype=np.float64):
    """res: ss_static_ref.run(..., gy=gy, dtype=dtype)'s Result (its Da [T,B]); gy [T,B] -> Gx with gx, mag [T,ni,B], lam0 [ns,B]
    (the adjoint in front of the first step: run()'s gz0)"""
    dt = np.dtype(dtype).type
    c = R.split(coef, ns, ni, dt)
    m = {k: np.abs(R.f64(v)) for k, v in c.items()}
    gy = np.asarray(gy).astype(dt)
    Da = np.asarray(res.Da).astype(dt)
    T, B = gy.shape
    gx, mag = np.empty((T, ni, B), dt), np.empty((T, ni, B))
    lam, lam_m = np.zeros((ns, B), dt), np.zeros((ns, B))
    for t in range(T - 1, -1, -1):
        g = gy[t]
        gb = (R.f64(c["fy"] * g) + R.mv(c["E"][None], lam)[0]).astype(dt)
        ga = gb * Da[t]
        gx[t] = (R.f64(c["dy"][:, None] * g) + R.f64(c["da"][:, None] * ga) + R.mv(c["Bx"].T, lam)).astype(dt)
        lam = (R.f64(c["ca"][:, None] * ga) + R.f64(c["cy"][:, None] * g) + R.mv(c["A"].T, lam)).astype(dt)
        # the same walk on absolute values, float64
        gm = np.abs(R.f64(g))
        gbm = m["fy"] * gm + R.mv(m["E"][None], lam_m)[0]
        gam = gbm * np.abs(R.f64(Da[t]))
        mag[t] = m["dy"][:, None] * gm + m["da"][:, None] * gam + R.mv(m["Bx"].T, lam_m)
        lam_m = m["ca"][:, None] * gam + m["cy"][:, None] * gm + R.mv(m["A"].T, lam_m)
    r = Gx()
    r.gx, r.mag, r.lam0 = gx, mag, lam
    return r


def channel_mag(mag):
    """[ni]: the channel's magnitude, mag's maximum over t and b"""
    return np.max(mag, axis=(0, 2))


def cap(c):
    """the bound of gx against the float64 reference on case c, per unit of channel magnitude: ss_static_ref's own"""
    return R.g_lin(c.ns + c.ni + 2) if c.linear else R.G_NL


def cap32(c):
    """what the float32 mode has to stay within: CAP32 on linear trees, an eighth of G_NL under a root"""
    return R.CAP32 if c.linear else R.G_NL / 8


def ref(c, dtype=np.float64):
    """Gx of ss_static_ref.Case c (cached on the case)"""
    k = "gx " + np.dtype(dtype).name
    if k not in c._ref:
        c._ref[k] = walk(c.ns, c.ni, c.coef, c.ref(dtype), c.gy, dtype)
    return c._ref[k]


def float32_figure(c):
    """the float32 mode of gx against float64 on case c, over cap32 x the channel's magnitude"""
    r64, r32 = ref(c), ref(c, np.float32)
    err = np.max(np.abs(R.f64(r32.gx) - r64.gx), axis=(0, 2))
    return R.ratio(err, cap32(c) * channel_mag(r64.mag))


@functools.lru_cache(maxsize=None)
def case(ns, ni, root, family, B, T):
    first = R.seed_of(ns, ni, root, family, B, T)
    want = 0.5 if (root != "none" and B * T < R.FEW) else 1.0
    for seed in range(first, first + 64):
        c = R.case(ns, ni, root, family, B, T) if seed == first else R.Case(ns, ni, root, family, B, T, seed)
        if float32_figure(c) <= want:
            return c
    raise AssertionError(f"no seed keeps the float32 mode of gx within its cap: {(ns, ni, root, family, B, T)}")


# ---- what tests/test_gpu_ss_gx.py runs -------------------------------------------------------------------------------------------
GX_FAMILIES = ("plain", "fast")


def seq_keys():
    """the sequential form: every tree and every root it is built for, the "plain" family at SHAPES_A"""
    return [(ns, ni, root, "plain", B, T) for ns, ni in R.TREES for root in R.ROOTS if R.built(ns, root) for B, T in R.SHAPES_A]


def chunk_keys():
    """the chunked form: (ns, ni, root, family, B, T, n_chunks) at GEOM_C, both families"""
    return [(ns, ni, root, fam, B, T, K) for ns, ni in R.TREES1 for root in R.ROOTS if R.built(ns, root) for fam in GX_FAMILIES
            for B, T, K in R.GEOM_C]


def gpu_case_keys():
    return list(dict.fromkeys(seq_keys() + [k[:6] for k in chunk_keys()]))
