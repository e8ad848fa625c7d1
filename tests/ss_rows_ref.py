"""The recursion csrc/wdf_ss_dyn.h states, over coefficient ROWS, in NumPy float64 -- the reference for what the streamed
kernels do with the rows they are handed, the state they start from and the state they leave:

    a = ca.z + da.x ;  b = root(a, R_port) ;  z' = A z + Bx x + E b ;  y = cy.z + dy.x + fy b

rows in the kernels' layout, A[ns][ns] | Bx[ns][ni] | E[ns] | ca[ns] | da[ni] | cy[ns] | dy[ni] | fy | R_port, as [n] (one static
row), [1,n,B] (a row per sequence) or [T,n,B] (a row per sample); x [B,T,ni]; z0 [ns,B] (None: zero) -> y [T,B], zT [ns,B].

Roots (root(a [B], R [B]) -> b [B]): none (b = 0: kDynRootNone, the ideal source folded into the rows), the symmetric diode
pair through oracle.diode_pair, the two different diodes through the oracle's exact root per element.  dL/dz0 of
L = sum(y gy): central differences, h = 1e-5, state s of ALL sequences moved at once (the sequences are independent, so 2 ns
evaluations give the whole [ns,B])."""
import numpy as np


def row_len(ns, ni):
    return ns * ns + ns * ni + 3 * ns + 2 * ni + 2


def split_rows(rows, ns, ni, B, T):
    """rows [n] | [1,n,B] | [T,n,B] -> dict of float64 arrays with a leading time axis of 1 or T and a trailing B."""
    r = np.asarray(rows, dtype=np.float64)
    n = row_len(ns, ni)
    if r.shape == (n,):
        r = np.broadcast_to(r[None, :, None], (1, n, B))
    assert r.shape in ((1, n, B), (T, n, B)), (r.shape, (T, n, B))
    Tr = r.shape[0]
    o = 0
    out = {}
    for name, shape in (("A", (ns, ns)), ("Bx", (ns, ni)), ("E", (ns,)), ("ca", (ns,)), ("da", (ni,)), ("cy", (ns,)), ("dy", (ni,)),
                        ("fy", ()), ("rp", ())):
        k = int(np.prod(shape, dtype=np.int64))
        out[name] = r[:, o:o + k, :].reshape((Tr,) + shape + (B,))
        o += k
    assert o == n
    return out


def rows_of(circ, r=None):
    """The float64 rows of a tf_wdf.Circuit from its own probe tape (lib/wdf_hip/probe_tape.py: the elements' calc_impedance /
    reflected / incident code recorded once) at the component values the circuit holds; r [B,T]: the channel of
    circ.per_sample_R -> rows [T,n,B]; without a pot -> one row [n]."""
    import torch
    from wdf_hip import lowering, probe_tape
    own = {"Resistor": "R", "ResistiveVoltageSource": "R", "Capacitor": "C"}
    els = [(e, own[lowering._kind(e)]) for e in circ.elements if lowering._kind(e) in own]
    tape, outs, rport = probe_tape.record(circ, [e.__dict__[n] for e, n in els], device_limits=False)
    vals = [torch.tensor(float(e.__dict__[n]), dtype=torch.float64) for e, n in els]
    chan = next((i for i, (e, _) in enumerate(els) if e is circ.per_sample_R), -1)
    assert (chan >= 0) == (r is not None)
    if chan < 0:
        return np.array([float(v) for v in tape.evaluate_torch(vals, outs + [rport])])
    r = torch.as_tensor(np.asarray(r, dtype=np.float64))
    vals[chan] = r
    rows = torch.stack([torch.broadcast_to(v, r.shape) for v in tape.evaluate_torch(vals, outs + [rport])], dim=0)    # [n,B,T]
    return rows.permute(2, 0, 1).contiguous().numpy()


def root_none(a, R):
    return np.zeros_like(a)


def root_diode(oracle, Is, nVt, n_up=1, n_down=1):
    """the symmetric pair {Is, nVt} with n_up / n_down diodes in series, per element (the port resistance moves with the pot)"""
    Is, nVt = float(Is), float(nVt)

    def root(a, R):
        return np.array([oracle.diode_pair(float(ai), float(Ri), Is, nVt, 1.0, int(n_up), int(n_down))[0] for ai, Ri in zip(a, R)])
    return root


def root_asym(oracle, rootp):
    """two different diodes, rootp = {Is_up, nVt_up, Is_down, nVt_down}: asym_pot_tree_ref.asym_root_elementwise's call"""
    Is1, V1, Is2, V2 = (float(v) for v in rootp)
    f = oracle.lib().oracle_asym_root_f64

    def root(a, R):
        return np.array([f(float(ai), float(Ri), Is1, V1, Is2, V2) for ai, Ri in zip(a, R)])
    return root


def run(rows, x, ns, ni, root=root_none, z0=None):
    """-> y [T,B], zT [ns,B] (float64)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    B, T, _ = x.shape
    assert x.shape[2] == ni
    c = split_rows(rows, ns, ni, B, T)
    per = c["fy"].shape[0] == T and T > 1
    z = np.zeros((ns, B)) if z0 is None else np.array(z0, dtype=np.float64).reshape(ns, B)
    y = np.empty((T, B))
    for t in range(T):
        k = t if per else 0
        xt = x[:, t, :].T                                                  # [ni,B]
        a = np.sum(c["ca"][k] * z, axis=0) + np.sum(c["da"][k] * xt, axis=0)
        b = root(a, c["rp"][k])
        y[t] = np.sum(c["cy"][k] * z, axis=0) + np.sum(c["dy"][k] * xt, axis=0) + c["fy"][k] * b
        z = np.einsum("ijb,jb->ib", c["A"][k], z) + np.einsum("ijb,jb->ib", c["Bx"][k], xt) + c["E"][k] * b
    return y, z


def time_slice(rows, t0, t1):
    """the rows of steps [t0, t1): per-sample rows are cut, rows constant in time stay"""
    r = np.asarray(rows)
    return r[t0:t1] if (r.ndim == 3 and r.shape[0] > 1) else r


def grad_z0(rows, x, ns, ni, root, z0, gy, h=1.0e-5):
    """dL/dz0 [ns,B] of L = sum(y gy) by central differences."""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    z0 = np.zeros((ns, B)) if z0 is None else np.array(z0, dtype=np.float64).reshape(ns, B)
    gy = np.asarray(gy, dtype=np.float64)
    g = np.empty((ns, B))
    for s in range(ns):
        zp, zm = z0.copy(), z0.copy()
        zp[s] += h
        zm[s] -= h
        yp, ym = run(rows, x, ns, ni, root, zp)[0], run(rows, x, ns, ni, root, zm)[0]
        g[s] = np.sum((yp - ym) * gy, axis=0) / (2.0 * h)
    return g
