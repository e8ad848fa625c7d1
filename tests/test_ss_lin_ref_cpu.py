"""CPU: the reference of the linear one-pass step's kernel-level GPU tests (tests/ss_lin_ref.py) has to be right before anything
is compared with it: against the oracle's tree interpreter, against central differences of its own loss, the caps on its own
fp32-against-fp64 distance that the GPU bounds rest on (over exactly the GPU module's cases), the chunk geometry those cases are
named for, the random probe tapes, and what the two new binding wrappers refuse without a GPU."""
import os

import numpy as np
import pytest

import ss_lin_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 48000


@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


# ---- against the oracle ------------------------------------------------------------------------------------------------------
def _lpf(W):
    Vs, R1, C1 = W.IdealVoltageSource(), W.Resistor(1000.0, True), W.Capacitor(1.0e-6, FS, True)
    return W.Circuit(W.Inverter(W.Series(R1, C1)), Vs, C1), [R1.R, C1.C]


def _ladder(W):
    """tests/test_gpu_ss_step.py's (2,2) tree: a resistive source inside the ladder and the ideal-source root"""
    Ra = W.Resistor(1.0e3, True)
    Vr = W.ResistiveVoltageSource(2.2e3, trainable=True)
    Ca, Cb = W.Capacitor(1.0e-7, FS, True), W.Capacitor(2.2e-7, FS, True)
    top = W.Inverter(W.Series(Ra, W.Parallel(Ca, W.Series(Vr, Cb))))
    return W.Circuit(top, W.IdealVoltageSource(), Cb), [Ra.R, Vr.R, Ca.C, Cb.C]


def _oracle_circuit(O, which):
    if which == "lpf":
        return O.rc_lowpass_circuit(float(FS))
    R_, C_, V_, S_, P_, I_ = O.NODE_RESISTOR, O.NODE_CAPACITOR, O.NODE_RES_VSOURCE, O.NODE_SERIES, O.NODE_PARALLEL, O.NODE_INVERTER
    nodes = [(R_, -1, -1, 0, -1, -1), (C_, -1, -1, 2, -1, -1), (V_, -1, -1, 1, 0, -1), (C_, -1, -1, 3, -1, -1), (S_, 2, 3, -1, -1, -1),
             (P_, 1, 4, -1, -1, -1), (S_, 0, 5, -1, -1, -1), (I_, 6, -1, -1, -1, -1)]
    return O.Circuit(nodes, top=7, probe=3, n_in=2, root_kind=O.ROOT_IDEAL_VSOURCE, fs=FS, root_vin=1)


@pytest.mark.parametrize("which", ["lpf", "ladder"])
def test_reference_against_the_oracle_tree_interpreter(oracle, which):
    """y against oracle.tree_fwd and the coefficient gradients, contracted with the host tape's Jacobian, against oracle.tree_grad
    (complex step).  Coefficients: Circuit.matrices() on the host -- which does part of its arithmetic in the Variables' float32
    (2e-6 relative, tests/test_probe_tape_cpu.py), and a pole's error counts 1 / (1 - |pole|) = 48-fold in y: 1e-4 of max |y|.  The
    same with the tape's own float64 coefficients, which carry no such error: 1e-9."""
    import tf_wdf as W
    from wdf_hip import probe_tape
    O = oracle
    circ, params = (_lpf if which == "lpf" else _ladder)(W)
    ns, ni = circ.ns, circ.ni
    assert (ns, ni) == ((1, 1) if which == "lpf" else (2, 2))
    B, T = 5, 300
    rng = np.random.default_rng(3)
    x = rng.standard_normal((B, T, ni)).astype(np.float32)
    tgt = (0.3 * rng.standard_normal((T, B))).astype(np.float32)
    theta = np.array([float(p) for p in params], dtype=np.float32).astype(np.float64)
    oc = _oracle_circuit(O, which)
    x64 = x.astype(np.float64)
    yref = O.tree_fwd(oc, theta, x64 if ni > 1 else x64[:, :, 0])
    gscale = 2.0 / (B * T)
    gy = float(np.float32(gscale)) * (yref - tgt)
    gref = O.tree_grad(oc, theta, x64 if ni > 1 else x64[:, :, 0], gy)
    tape, outs, rport = probe_tape.record(circ, params)
    val, jac = tape.evaluate(theta, outs + [rport])
    coef_m = circ.matrices()[0].detach().numpy()
    x_tm = np.ascontiguousarray(x.transpose(1, 2, 0))
    rows = R.rows(ns, ni)
    for name, coef, tol_y, tol_g in (("matrices()", coef_m, 1e-4, 1e-3), ("tape", val[:-1], 1e-9, 1e-7)):
        r = R.run(ns, ni, coef, x_tm, tgt, gscale)
        e_y = float(np.max(np.abs(r.y - yref)) / np.max(np.abs(yref)))
        got = r.g @ jac[rows]
        scale = np.abs(r.g) @ np.abs(jac[rows])
        e_g = float(np.max(np.abs(got - gref) / scale))
        print(f"{which} {name}: |y - oracle| / max|y| {e_y:.2e}, gradients / sum |g_i J_ip| {e_g:.2e}")
        assert e_y <= tol_y and e_g <= tol_g


# ---- against central differences ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns,ni", R.TREES)
@pytest.mark.parametrize("z0", [False, True])
def test_reference_gradients_against_central_differences_of_its_own_loss(ns, ni, z0):
    """every family, fp64, step 1e-6: the truncation term is h^2 / 6 x the third derivative (at most ~T^3 of the loss's scale at
    T = 60: 1e-8 of mag), the rounding term 1e-16 / h: the entries agree within 1e-6 of mag_i."""
    for fam in R.families(ns):
        c = R.case(ns, ni, fam, 3, 60, z0)
        ref = c.ref()
        rows = R.rows(ns, ni)
        c64 = c.coef.astype(np.float64)
        for i, row in enumerate(rows):
            h = 1e-6
            cp, cm = c64.copy(), c64.copy()
            cp[row] += h
            cm[row] -= h
            fd = (R.loss_of(ns, ni, cp, c.x, c.target, float(np.float32(c.gscale)), c.z0)
                  - R.loss_of(ns, ni, cm, c.x, c.target, float(np.float32(c.gscale)), c.z0)) / (2 * h)
            assert abs(ref.g[i] - fd) <= 1e-6 * ref.mag[i], (fam, i, ref.g[i], fd, ref.mag[i])


def test_two_calls_with_the_state_handed_over_are_the_run_over_both_halves():
    """section C's references: the first half from z0, the second from the float64 states the first ends in -- y and the final
    states of the run over all 2 T steps; and the sums add up (the SSE; not the gradients: the hand-over is a constant)."""
    for ns, ni in R.TREES_C:
        whole, first, second = R.carried(ns, ni, 65)
        w, a, b = whole.ref(), first.ref(), second.ref()
        assert np.max(np.abs(np.concatenate([a.y, b.y]) - w.y)) <= 1e-13 and np.max(np.abs(b.zT - w.zT)) <= 1e-13
        assert abs(a.sse + b.sse - w.sse) <= 1e-12 * w.sse
        assert np.max(np.abs(whole.z0)) > 1.0 and np.any(np.abs(a.g + b.g - 2.0 * w.g) > 1e-3 * w.mag)


# ---- the caps the GPU bounds rest on -----------------------------------------------------------------------------------------
CAP_Y, CAP_G, CAP_SSE = 4e-7, 2e-7, 2e-7


def test_fp32_restatement_stays_within_the_caps_on_every_gpu_case():
    """The same recursion with every product and state in float32 against the float64 one, over every call the GPU module
    compares: y within 4e-7 max |y|, every gradient entry within 2e-7 mag_i, the SSE within 2e-7 relative.  The GPU bounds are 8 x
    these (plus the kernel's 32-addend fp32 sums), so a case over a cap would make its GPU bound mean nothing.  The final states,
    where the GPU module asks for them (T = 257 and section C's halves), like y."""
    worst = [0.0, 0.0, 0.0, 0.0]
    for c in R.gpu_cases():
        r64, r32 = c.ref(), c.ref(np.float32)
        f_y = float(np.max(np.abs(r32.y.astype(np.float64) - r64.y)) / np.max(np.abs(r64.y)))
        f_g = float(np.max(np.abs(r32.g - r64.g) / r64.mag))
        f_s = abs(r32.sse - r64.sse) / r64.sse
        f_z = float(np.max(np.abs(r32.zT.astype(np.float64) - r64.zT)) / max(1.0, np.max(np.abs(r64.zT)))) if (c.ns and c.T == 257) else 0.0
        worst = [max(a, b) for a, b in zip(worst, (f_y, f_g, f_s, f_z))]
        assert f_y <= CAP_Y and f_g <= CAP_G and f_s <= CAP_SSE and f_z <= CAP_Y, (c, f_y, f_g, f_s, f_z)
        assert np.all(r64.mag > 0) and np.max(np.abs(r64.y)) < 50.0, c
    print(f"fp32 against fp64, worst over {len(R.gpu_cases())} cases: y {worst[0]:.2e}, g / mag {worst[1]:.2e}, sse {worst[2]:.2e}, "
          f"zT {worst[3]:.2e}")


def test_the_cases_cover_every_instantiation_and_family():
    keys = R.gpu_case_keys()
    assert {(k[0], k[1], k[3] % 2) for k in keys if (k[3], k[4]) in {(b, t) for b, t, _ in R.SHAPES_A}} == \
        {(ns, ni, w) for ns, ni in R.TREES for w in (0, 1)}                                      # 12: {ns} x {ni} x {one, two per lane}
    assert {k[2] for k in keys if k[:2] == (2, 2)} == set(R.FAMILIES)
    for fam in R.FAMILIES:
        for ns in (1, 2):
            if fam in R.families(ns):
                A = R.coefs(ns, 1, fam, np.random.default_rng(0))[:ns * ns].reshape(ns, ns).astype(np.float64)
                lam = np.linalg.eigvals(A)
                want = R.POLES[ns][fam] if fam != "complex" else None
                if want:
                    assert np.allclose(sorted(lam.real), sorted(want), atol=2e-7) and np.max(np.abs(lam.imag)) < 1e-6
                else:
                    assert np.allclose(np.abs(lam), 0.97, atol=1e-6) and np.allclose(np.abs(np.angle(lam)), 0.3, atol=1e-6)


# ---- chunk geometry ----------------------------------------------------------------------------------------------------------
def test_chunk_geometry_of_the_gpu_cases(lib):
    from wdf_hip import binding
    for (T, n), want in {(33, 2): (32, 2), (65, 3): (32, 3), (100, 8): (32, 4), (1000, 5): (224, 5), (2048, 64): (32, 64), (32, 1): (32, 1),
                         (64, 2): (32, 2), (40, 1): (64, 1), (100, 4): (32, 4), (257, 3): (96, 3), (200, 4): (64, 4), (2048, 8): (256, 8),
                         (2048, 1): (2048, 1)}.items():
        assert binding.chunk_geom(T, n, 32) == want, (T, n)
    ws = lib.wdf_ss_lin_step_ws_bytes
    assert ws(3, 1, 64, 64, 1) == 0 and ws(1, 0, 64, 64, 1) == 0 and ws(1, 1, 0, 64, 1) == 0 and ws(1, 1, 64, 64, 0) == 0
    assert ws(1, 1, 64, 0, 1) == 0 and ws(1, 3, 64, 64, 1) == 0 and ws(-1, 1, 64, 64, 1) == 0
    # sized by the chunks the launch runs with (K = 4 at T = 100), not by the count asked for
    assert ws(2, 2, 130, 100, 8) == ws(2, 2, 130, 100, 4) > ws(2, 2, 130, 100, 3)
    for ns, ni in R.TREES:
        for B, T, n in [(1, 40, 1), (65, 100, 4), (130, 2048, 64)]:
            K = binding.chunk_geom(T, n, 32)[1]
            d, g = ns * (1 + ns * ns + ns * ni), R.kg(ns, ni)
            assert ws(ns, ni, B, T, n) == 512 + K * d * B * 4 + -(-B // 64) * K * (g + 1) * 8, (ns, ni, B, T, n)


# ---- the probe's tapes -------------------------------------------------------------------------------------------------------
PROBE_TAPES = [(n_ops, P) for n_ops in (1, 128, 129, 384) for P in (1, 15)]


@pytest.mark.parametrize("n_ops,P", PROBE_TAPES)
def test_random_tapes_are_well_formed_and_the_magnitudes_bound_the_rounding(n_ops, P):
    """The builder's tapes pass the binding's checks and the library's own evaluation agrees with the magnitude pass's; every
    value is finite; and the fp64 evaluation stays within a QUARTER of the GPU bound 64 n_ops 2^-53 (vmag, tmag) of the same
    recurrences in extended precision -- the kernel does the same operations in fp64, so half the bound is left over."""
    from wdf_hip import binding, probe_tape
    ops, consts, params = R.random_tape(n_ops, P, seed=0)
    assert len(ops) == n_ops and params.dtype == np.float32 and len(params) == P
    binding._probe_tape(ops, consts, np.arange(n_ops), P)
    outs = np.arange(n_ops)
    val, jac, vm, tm = R.evaluate_mag(ops, consts, params, outs)
    tape = probe_tape.Tape()
    tape.ops, tape.consts = [tuple(o) for o in ops], list(consts)
    v2, j2 = tape.evaluate(params.astype(np.float64), outs)
    assert np.array_equal(val, v2) and np.array_equal(jac, j2)
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(jac)) and np.all(np.abs(val) <= vm) and np.all(np.abs(jac) <= tm)
    if n_ops > 1:
        kinds = {o[0] for o in ops}
        assert kinds == set(range(8)) if n_ops >= 128 else True
        assert np.count_nonzero(tm.sum(axis=1)) > n_ops // 2          # (most nodes depend on a parameter)
    if np.finfo(np.longdouble).eps < 2.0 ** -60:
        vx, jx, _, _ = R.evaluate_mag(ops, consts, params, outs, dtype=np.longdouble)
        bound = 0.25 * 64 * n_ops * 2.0 ** -53
        assert np.all(np.abs(val - vx) <= bound * vm) and np.all(np.abs(jac - jx) <= bound * tm)


def test_ss_probe_refuses_a_tape_that_reads_outside_itself():
    from wdf_hip import binding
    good = [[R.OP_PARAM, 0, 0], [R.OP_CONST, 0, 0], [R.OP_MUL, 0, 1], [R.OP_RECIP, 2, 0]]
    binding._probe_tape(good, [1.5], [3, 0], 1)
    for ops, consts, outs, P in [
            ([[R.OP_PARAM, 0, 0], [R.OP_ADD, 0, 1]], [1.0], [1], 1),                # names itself
            ([[R.OP_PARAM, 0, 0], [R.OP_NEG, 2, 0], [R.OP_CONST, 0, 0]], [1.0], [1], 1),   # names a later operation
            ([[R.OP_PARAM, 0, 0], [R.OP_SUB, 0, -1]], [1.0], [1], 1),
            ([[R.OP_PARAM, 1, 0]], [1.0], [0], 1),                                  # a parameter outside the block
            ([[R.OP_CONST, 1, 0]], [1.0], [0], 1),                                  # a constant outside consts
            ([[R.OP_CONST, 0, 0]], [], [0], 1),
            ([[8, 0, 0]], [1.0], [0], 1),                                           # no such operation
            (good, [1.5], [4], 1), (good, [1.5], [-1], 1), (good, [1.5], [], 1),    # outputs
            (good, [1.5], [0], 16), (good, [1.5], [0], 0),
            ([[R.OP_PARAM, 0, 0]] * 385, [1.5], [0], 1), ([], [1.5], [0], 1)]:
        with pytest.raises(binding.WdfHipError):
            binding._probe_tape(ops, consts, outs, P)
