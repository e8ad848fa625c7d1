"""CPU: tests/ss_static_ref.py -- the reference tests/test_gpu_ss_static_kernels.py judges the static state-space kernels against --
pinned before anything is compared with it:

  * the vectorised symmetric pair against oracle.diode_pair, both diode counts, a = 0 and both signs;
  * the recursion and its adjoint against oracle.tree_fwd / tree_grad on the RC lowpass and the two-capacitor clipper of
    tests/test_gpu_circuit.py, the coefficients taken from the circuit's own lowering (its probe tape, evaluated in
    float64) and the gradient chained to the component values through its Jacobian;
  * every gcoef, groot and gz0 entry against central differences of the float64 recursion, one small case per (ns, root);
  * the float32 mode against float64 over gpu_cases(): the caps the GPU bounds rest on (an eighth of Y_REF on y, the stash and zT;
    CAP32 mag_i on a linear tree's gradients; an eighth of G_NL mag_i under a root), and under a root both diode regimes on REGIME
    of the steps (asserted on the cases of 1000 steps and more: a call of one or seven steps cannot show both, and draws its
    inputs from the same distribution on the same coefficients).
"""
import numpy as np
import pytest

import ss_static_ref as R

FS = 48000


ratio = R.ratio


@pytest.mark.parametrize("n_up,n_down", [(1, 1), (2, 3)])
def test_vectorised_pair_is_the_oracles(oracle, n_up, n_down):
    a = np.concatenate([np.linspace(-4.0, 4.0, 81), [0.0, 1e-9, -1e-9, 1e-3, -1e-3]])
    for Rp in (1.0e3, 7.3e3, 45.0e3):
        want = oracle.diode_pair(a, Rp, R.PAIR[0], R.PAIR[1], 1.0, n_up, n_down)
        got = R.pair_b(a, R.PAIR[0], R.PAIR[1], Rp, n_up, n_down)
        assert np.max(np.abs(got - want)) <= 1e-13 * 4.0


def _lowered(circ, params):
    """The circuit's own lowering -- its probe tape (lib/wdf_hip/probe_tape.py: the elements' calc_impedance / reflected / incident
    code recorded once), evaluated in float64 at the values the Variables hold -> coef [ncoef] and R_port, torch tensors on a graph,
    and the leaves in the order of params (the Variables themselves hold float32: Circuit.matrices() starts from those roundings)."""
    import torch
    from wdf_hip import lowering, probe_tape
    own = {"Resistor": "R", "ResistiveVoltageSource": "R", "Capacitor": "C"}
    els = [(e, own[lowering._kind(e)]) for e in circ.elements if lowering._kind(e) in own]
    tape, outs, rport = probe_tape.record(circ, [e.__dict__[n] for e, n in els], device_limits=False)
    vals = [torch.tensor(float(e.__dict__[n]), dtype=torch.float64, requires_grad=True) for e, n in els]
    out = tape.evaluate_torch(vals, outs + [rport])
    leaves = [next(v for v, (e, n) in zip(vals, els) if e.__dict__[n] is p) for p in params]
    return torch.stack([o + 0.0 * vals[0] for o in out[:-1]]), out[-1], leaves


def _chain(coef, rport, leaves, g, groot_R):
    """dL/d component value from dL/dcoef and dL/dR_port through the lowering's own graph"""
    import torch
    out = []
    for p in leaves:
        d = torch.autograd.grad(coef, p, grad_outputs=torch.as_tensor(g), retain_graph=True, allow_unused=True)[0]
        v = 0.0 if d is None else float(d)
        if groot_R is not None:
            d = torch.autograd.grad(rport, p, retain_graph=True, allow_unused=True)[0]
            v += 0.0 if d is None else groot_R * float(d)
        out.append(v)
    return np.array(out)


def test_rc_lowpass_against_the_oracle(oracle):
    import tf_wdf as W
    Vs, R1, C1 = W.IdealVoltageSource(), W.Resistor(1000, True), W.Capacitor(1.0e-6, FS, True)
    circ = W.Circuit(W.Inverter(W.Series(R1, C1)), Vs, C1)
    assert (circ.ns, circ.ni) == (1, 1)
    coef, rport, leaves = _lowered(circ, [R1.R, C1.C])
    rng = np.random.default_rng(3)
    B, T = 4, 200
    x, gy = rng.standard_normal((B, T)), rng.standard_normal((T, B)) / (B * T)
    oc = oracle.rc_lowpass_circuit(FS)
    theta = np.array([float(R1.R), float(C1.C)])
    r = R.run(1, 1, coef.detach().numpy(), x, R.Root("none"), gy=gy)
    yref = oracle.tree_fwd(oc, theta, x)
    assert np.max(np.abs(r.y - yref)) <= 1e-12 * max(1.0, np.max(np.abs(yref)))
    gref = oracle.tree_grad(oc, theta, x, gy)
    got = _chain(coef, rport, leaves, r.g, None)
    assert np.max(np.abs(got - gref) / np.abs(gref)) <= 1e-9, (got, gref)


def test_two_state_clipper_against_the_oracle(oracle):
    import tf_wdf as W
    O = oracle
    Vs1, C1 = W.ResistiveVoltageSource(22.0e3, trainable=True), W.Capacitor(4.7e-9, FS, trainable=True)
    R1, Vs2, C2 = W.Resistor(3.3e3, True), W.ResistiveVoltageSource(10.0e3, trainable=True), W.Capacitor(10.0e-9, FS, trainable=True)
    top = W.Series(W.Parallel(Vs1, C1), W.Parallel(W.Series(R1, Vs2), C2))
    dp = W.DiodePair(top, 4.352e-9, Vt=0.0493, trainable=True)
    circ = W.Circuit(top, dp, C2)
    assert (circ.ns, circ.ni) == (2, 2)
    params = [Vs1.R, C1.C, R1.R, Vs2.R, C2.C]
    coef, rport, leaves = _lowered(circ, params)
    nodes = [(O.NODE_RES_VSOURCE, -1, -1, 0, 0, -1), (O.NODE_CAPACITOR, -1, -1, 1, -1, -1), (O.NODE_PARALLEL, 0, 1, -1, -1, -1),
             (O.NODE_RESISTOR, -1, -1, 2, -1, -1), (O.NODE_RES_VSOURCE, -1, -1, 3, 1, -1), (O.NODE_SERIES, 3, 4, -1, -1, -1),
             (O.NODE_CAPACITOR, -1, -1, 4, -1, -1), (O.NODE_PARALLEL, 5, 6, -1, -1, -1), (O.NODE_SERIES, 2, 7, -1, -1, -1)]
    oc = O.Circuit(nodes, top=8, probe=6, n_in=2, root_kind=O.ROOT_DIODE_PAIR, fs=FS, p_is=5, p_nvt=6)
    Is, nVt = float(dp.Is), float(dp.nVt)
    theta = np.array([float(p) for p in params] + [Is, nVt])
    rng = np.random.default_rng(5)
    B, T = 5, 200
    x = rng.standard_normal((B, T, 2)) * np.array([1.5, 0.7])
    gy = rng.standard_normal((T, B)) / (B * T)
    root = R.Root("pair11", p=np.array([Is, nVt, float(rport)]))
    r = R.run(2, 2, coef.detach().numpy(), x, root, gy=gy)
    yref = O.tree_fwd(oc, theta, x)
    assert np.max(np.abs(r.y - yref)) <= 1e-11 * max(1.0, np.max(np.abs(yref)))
    gref = O.tree_grad(oc, theta, x, gy)
    got = np.concatenate([_chain(coef, rport, leaves, r.g, float(r.groot[2])), r.groot[:2]])
    # (Da and the root's partials are central differences: 1e-9 relative, not the complex step's 1e-15)
    assert np.max(np.abs(got - gref) / np.abs(gref)) <= 1e-6, (got, gref)


SMALL = [(ns, root) for ns in range(5) for root in R.ROOTS if R.built(ns, root)]


@pytest.mark.parametrize("ns,root", SMALL, ids=[f"ns{a}-{b}" for a, b in SMALL])
def test_adjoint_against_central_differences_of_the_recursion(oracle, ns, root):
    """every gcoef, groot and gz0 entry, judged against mag_i.  1e-7: the quotients' own noise (an entry whose mag_i is a hundredth of
    the loss: 1e-16 of the loss over a step of 1e-6 is 1e-8 of it); a wrong or transposed index is a difference of order 1"""
    ni = 1 + ns % 2
    c = R.Case(ns, ni, root, "plain", 3, 24, seed=1)
    ref = c.ref()
    gy = c.gy.astype(np.float64)
    c64 = c.coef.astype(np.float64)

    def loss(coef=c64, z0=c.z0, rootp=None):
        return float(np.sum(R.run(ns, ni, coef, c.x, c.root, z0=z0, rootp=rootp).y * gy))

    worst = 0.0
    for i in range(c64.size):
        h = 1e-5 * max(abs(c64[i]), 0.1)
        cp, cm = c64.copy(), c64.copy()
        cp[i] += h
        cm[i] -= h
        fd = (loss(cp) - loss(cm)) / (2.0 * h)
        worst = max(worst, ratio(abs(fd - ref.g[i]), ref.mag[i]))
    for j in range(c.root.nr):                            # (four points, steps of 1e-3 p: see Root.partials)
        p0 = c.root.p.astype(np.float64)
        h, d = 1e-3 * p0[j], []
        for k in (1.0, 2.0):
            pp, pm = p0.copy(), p0.copy()
            pp[j] += k * h
            pm[j] -= k * h
            d.append(loss(rootp=pp) - loss(rootp=pm))
        fd = (8.0 * d[0] - d[1]) / (12.0 * h)
        worst = max(worst, ratio(abs(fd - ref.groot[j]), ref.groot_mag[j]))
    for s in range(ns):
        h = 1e-6
        zp, zm = c.z0.astype(np.float64), c.z0.astype(np.float64)
        zp[s] += h
        zm[s] -= h
        yp, ym = (R.run(ns, ni, c64, c.x, c.root, z0=z).y for z in (zp, zm))
        fd = np.sum((yp - ym) * gy, axis=0) / (2.0 * h)                     # (the sequences are independent)
        worst = max(worst, ratio(np.abs(fd - ref.gz0[s]), ref.gz0_mag[s]))
        assert ratio(np.abs(ref.gz0_tangent[s] - ref.gz0[s]), ref.gz0_mag[s]) <= 1e-12
    print(f"FIG cpu | {c} | adjoint - central differences = {worst:.2e} mag")
    assert worst <= 1e-7, worst


def test_one_list_of_cases():
    keys = R.gpu_case_keys()
    assert len(keys) == len(set(keys)) and len(keys) > 400
    for root in R.ROOTS:
        for ns in range(5):
            for ni in (1, 2):
                assert ((ns, ni, root, "plain", 65, 43) in keys) == R.built(ns, root)
    for ns, ni in R.TREES1:
        for fam in R.families(ns):
            assert (ns, ni, "none", fam, 65, 257) in keys


@pytest.mark.parametrize("ns,ni", R.TREES, ids=[f"ns{a}-ni{b}" for a, b in R.TREES])
def test_float32_mode_stays_within_the_caps_over_the_gpu_cases(oracle, ns, ni):
    """the conditions the GPU module's bounds rest on, over exactly its cases; prints the worst of each"""
    worst = {}

    def note(k, v, c):
        if v > worst.get(k, (-1.0, None))[0]:
            worst[k] = (v, repr(c))

    for key in R.gpu_case_keys():
        if key[:2] != (ns, ni):
            continue
        c = R.case(*key)
        assert np.all(c.coef != 0.0) and c.coef.dtype == np.float32
        r64 = c.ref()
        for k, v in R.float32_figures(c).items():
            note(k, v, c)
        if ns:
            assert ratio(np.abs(r64.gz0_tangent - r64.gz0), r64.gz0_row_mag[:, None]) <= 1e-11
        if not c.linear and c.B * c.T >= 1000:
            lo, hi = R.regimes(r64.Da)
            assert lo >= R.REGIME and hi >= R.REGIME, (repr(c), lo, hi)
        if c.linear:                                  # (a linear tree has no wave into a root: the dead entries are exactly 0)
            o = R.offsets(ns, ni)
            dead = list(range(o["E"], o["da"] + ni)) + [o["fy"]]
            assert np.all(r64.g[dead] == 0.0) and np.all(r64.mag[dead] == 0.0)
    print(f"FIG cpu | ({ns},{ni}) float32 mode / cap | " + "  ".join(f"{k}={v:.3f} [{w}]" for k, (v, w) in worst.items()))
    assert all(v <= 1.0 for v, _ in worst.values()), worst
