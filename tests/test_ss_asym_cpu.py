"""CPU: the two-different-diode root on generic trees (root kind WDF_ROOT_ASYM_PAIR of the state-space kernels,
tf_wdf.AsymDiodePair(..., any_tree=True)) as far as it can be checked without a GPU: the fp64 NumPy reference the GPU tests
compare against (tests/asym_tree_ref.py) pinned to the oracle, the finite differences through it, the trees Circuit accepts
and refuses under this root, the planner, and the C ABI's argument checks (through ctypes; validation fails before any
pointer is dereferenced)."""
import ctypes as C
import os

import numpy as np
import pytest

import asym_tree_ref as ref
import ss_asym_cases as cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = cases.FS


@pytest.fixture(scope="module")
def lib():
    from wdf_hip import binding
    if not os.path.exists(binding.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "differentiable-wdfs_amd", "csrc")])
    return binding.lib()


# ---- the reference ---------------------------------------------------------------------------------------------------
def test_reference_tree_reproduces_the_oracle_interpreter_on_the_hpf_tree(oracle):
    """HPFDiodeClipper.h:28-32's tree with the 2-up / 3-down symmetric pair: the NumPy tree with root = oracle.diode_pair against
    oracle.tree_fwd."""
    O = oracle
    x = (np.random.default_rng(12).standard_normal((40, 300)) * 1.2).astype(np.float32).astype(np.float64)
    nodes = [(O.NODE_RESISTOR, -1, -1, 0, -1, -1), (O.NODE_RES_VSOURCE, -1, -1, 1, 0, -1),
             (O.NODE_CAPACITOR, -1, -1, 2, -1, -1), (O.NODE_SERIES, 1, 2, -1, -1, -1), (O.NODE_PARALLEL, 0, 3, -1, -1, -1)]
    oc = O.Circuit(nodes, top=4, probe=0, n_in=1, root_kind=O.ROOT_DIODE_PAIR, fs=FS, p_is=3, p_nvt=4, n_up=2, n_down=3)
    theta = cases.f32([33.0e3, 1.0e3, 22.0e-9, 4.352e-9, 25.85e-3 * 1.906])
    tree, probe, _ = cases.hpf_ref()
    y = ref.tree_fwd(tree, probe, theta, FS, x, lambda a, R: O.diode_pair(a, float(R), theta[3], theta[4], 1.0, 2, 3))
    d = float(np.max(np.abs(y - O.tree_fwd(oc, theta, x))))
    print("max |tree_fwd - oracle.tree_fwd| =", d)
    assert d <= 1e-12


def test_reference_tree_reproduces_the_oracle_two_diode_clipper(oracle):
    """The clipper tree with root = oracle.asym_root against oracle.clipper_asym_fwd."""
    x = (np.random.default_rng(5).standard_normal((40, 300)) * 1.2).astype(np.float32).astype(np.float64)
    tree, probe, theta = cases.clipper_ref()
    y = ref.tree_fwd(tree, probe, theta, FS, x, ref.asym_root_of(oracle, theta, 2))
    d = float(np.max(np.abs(y - oracle.clipper_asym_fwd(np.concatenate([theta[2:], theta[:2]]), float(FS), x))))
    print("max |tree_fwd - oracle.clipper_asym_fwd| =", d)
    assert d <= 1e-12


def test_finite_differences_through_the_reference_are_stable(oracle):
    """Central differences of sum(y gy) on the HPF tree under the two-diode root: relative steps 1e-4 and 1e-5 agree within 1e-6
    relative for all seven parameters."""
    x, gy = cases.data("hpf", shape=(20, 200, 1))
    f, theta = cases.forward_of(oracle, "hpf", x.astype(np.float64))
    g4 = (ref.central(f, theta, 1.0e-4) * gy[None]).reshape(theta.size, -1).sum(axis=1)
    g5 = (ref.central(f, theta, 1.0e-5) * gy[None]).reshape(theta.size, -1).sum(axis=1)
    d = np.abs(g4 - g5) / np.abs(g5)
    print("relative difference between the two steps:", d)
    assert np.all(d <= 1e-6)


def test_the_committed_seeds_are_the_first_whose_gradient_terms_do_not_cancel(oracle):
    """ss_asym_cases.SEED on the smallest case (the others are asserted where their references are computed, on the GPU side)."""
    assert cases.find_seed(oracle, "three_state") == cases.SEED["three_state"]
    assert cases.find_seed(oracle, "clipper") == cases.SEED["clipper"]


# ---- Circuit ---------------------------------------------------------------------------------------------------------
def test_any_tree_builds_on_the_hpf_tree_and_the_default_still_refuses():
    import tf_wdf as W
    from wdf_hip.binding import WdfHipError
    circ, params = cases.hpf(W)
    assert circ.root_kind == "AsymDiodePair" and (circ.ns, circ.ni) == (1, 1) and circ._asym_generic and len(params) == 7
    with pytest.raises(WdfHipError, match="clipper"):
        cases.hpf(W, any_tree=False)
    assert W.AsymDiodePair(circ.top, 1e-9, 1e-8).any_tree is False


def test_the_clipper_tree_keeps_its_own_kernels_unless_forced():
    import tf_wdf as W
    assert not cases.clipper(W)[0]._asym_generic
    assert cases.clipper(W, force_generic=True)[0]._asym_generic
    assert cases.two_state(W)[0]._asym_generic and cases.three_state(W)[0]._asym_generic


def test_refusals_under_any_tree():
    import tf_wdf as W
    from wdf_hip.binding import WdfHipError

    def hpf(solver="newton_f32", **kw):
        R, Vs, Cp = W.Resistor(33.0e3), W.ResistiveVoltageSource(1.0e3), W.Capacitor(22.0e-9, FS)
        top = W.Parallel(R, W.Series(Vs, Cp))
        kw = {k: {"Vs": Vs, "R": R}.get(v, v) for k, v in kw.items()}
        return W.Circuit(top, W.AsymDiodePair(top, 4.352e-9, 2.0e-6, solver=solver, any_tree=True), R, **kw)

    for solver in ("newton_f64", "omega_f32"):
        with pytest.raises(WdfHipError, match="newton_f32"):
            hpf(solver)
    with pytest.raises(WdfHipError, match="per_sample_R is not supported under an AsymDiodePair root"):
        hpf(per_sample_R="Vs")
    with pytest.raises(WdfHipError, match="per_sequence_R under an AsymDiodePair root belongs to the diode-clipper"):
        hpf(per_sequence_R="Vs")
    with pytest.raises(WdfHipError, match="resident"):
        hpf().to_device()
    # the clipper tree through the generic kernels: the same limits
    with pytest.raises(WdfHipError, match="newton_f32"):
        Vs, Cp = W.ResistiveVoltageSource(45.0e3), W.Capacitor(4.7e-9, FS)
        P1 = W.Parallel(Vs, Cp)
        W.Circuit(P1, W.AsymDiodePair(P1, 4.352e-9, 2.0e-6, solver="newton_f64", any_tree=True), Cp, force_generic=True)
    with pytest.raises(WdfHipError, match="per_sequence_R"):
        Vs, Cp = W.ResistiveVoltageSource(45.0e3), W.Capacitor(4.7e-9, FS)
        P1 = W.Parallel(Vs, Cp)
        W.Circuit(P1, W.AsymDiodePair(P1, 4.352e-9, 2.0e-6, any_tree=True), Cp, force_generic=True, per_sequence_R=Vs)
    # four capacitors: the chunked reverse sweep for this root is not built there
    top, probe = cases.four_state_top(W)
    with pytest.raises(WdfHipError, match="at most three capacitors and two sources"):
        W.Circuit(top, W.AsymDiodePair(top, 4.352e-9, 2.0e-6, any_tree=True), probe)
    # three sources
    vs = [W.ResistiveVoltageSource(1.0e3 * (k + 1)) for k in range(3)]
    Cp = W.Capacitor(22.0e-9, FS)
    top = W.Parallel(Cp, W.Series(vs[0], W.Series(vs[1], vs[2])))
    with pytest.raises(WdfHipError, match="at most three capacitors and two sources"):
        W.Circuit(top, W.AsymDiodePair(top, 4.352e-9, 2.0e-6, any_tree=True), Cp)


def test_planner_treats_the_root_like_the_symmetric_pair():
    import tf_wdf as W
    from wdf_hip import binding as wb, lowering
    assert wb.ROOT_ASYM_PAIR == 4
    circ, _ = cases.hpf(W)
    coef64, r_port = circ.matrices()
    plan = lowering.plan_ss_time_parallel(coef64, 1, 1, wb.ROOT_ASYM_PAIR, 200, 2048)
    assert plan is not None and plan.k_fwd >= 2 and plan.k_bwd >= 2
    assert plan == lowering.plan_ss_time_parallel(coef64, 1, 1, wb.ROOT_DIODE_PAIR, 200, 2048)
    assert float(r_port) == pytest.approx(1.0 / (1.0 / 33.0e3 + 1.0 / (1.0e3 + 1.0 / (2.0 * 22.0e-9 * FS))), rel=1e-6)


# ---- C ABI -----------------------------------------------------------------------------------------------------------
def test_header_names_the_root_kind_and_the_new_entry_point():
    hdr = open(os.path.join(REPO, "include", "wdf_hip.h")).read()
    assert "WDF_ROOT_ASYM_PAIR = 4" in hdr and "int wdf_ss_fwd_tp_root(" in hdr


def test_entry_points_check_the_root_kinds_arguments(lib):
    one = C.c_void_p(16)   # never dereferenced
    EINVAL, EUNSUPPORTED = -1, -3
    assert lib.wdf_ss_fwd(one, one, None, 1, 1, 4, 1, 1, one, None, None, None, 4, 8, 0, None) == EINVAL
    assert b"Is_up, nVt_up, Is_down, nVt_down, R_port" in lib.wdf_last_error()
    assert lib.wdf_ss_bwd(one, one, None, 1, 1, 4, 1, 1, one, one, one, one, one, None, 4, 8, 0, None) == EINVAL
    assert b"rootp" in lib.wdf_last_error()
    assert lib.wdf_ss_bwd(one, one, one, 1, 1, 4, 1, 1, one, one, one, one, None, None, 4, 8, 0, None) == EINVAL
    assert b"null groot" in lib.wdf_last_error()
    assert lib.wdf_ss_bwd_tp(one, one, one, 1, 1, 4, 1, 1, one, one, one, one, None, None, 4, 64, 1, None) == EINVAL
    assert b"null groot" in lib.wdf_last_error()
    assert lib.wdf_ss_fwd(one, one, one, 1, 1, 5, 1, 1, one, None, None, None, 4, 8, 0, None) == EINVAL
    assert b"unknown root kind 5" in lib.wdf_last_error()
    # four states under this root: no kernel is built
    for f, args in ((lib.wdf_ss_fwd, (one, one, one, 4, 1, 4, 1, 1, one, None, None, None, 4, 8, 0, None)),
                    (lib.wdf_ss_bwd, (one, one, one, 4, 1, 4, 1, 1, one, one, one, one, one, None, 4, 8, 0, None)),
                    (lib.wdf_ss_bwd_tp, (one, one, one, 4, 1, 4, 1, 1, one, one, one, one, one, None, 4, 64, 1, None)),
                    (lib.wdf_ss_fwd_tp_root, (one, one, one, 4, 1, 4, 1, 1, one, None, None, None, 4, 64, 1, 8, 1e-6, None, one, one, None))):
        assert f(*args) == EUNSUPPORTED
        assert b"at most 3 states" in lib.wdf_last_error()
    # the speculating forward takes the two nonlinear roots only; its old name is the symmetric pair's
    assert lib.wdf_ss_fwd_tp_root(one, one, one, 1, 1, 0, 1, 1, one, None, None, None, 4, 64, 1, 8, 1e-6, None, one, one, None) == EINVAL
    assert b"root kind 0" in lib.wdf_last_error()
    assert lib.wdf_ss_fwd_tp_root(one, one, None, 1, 1, 4, 1, 1, one, None, None, None, 4, 64, 1, 8, 1e-6, None, one, one, None) == EINVAL
    assert b"Is_up" in lib.wdf_last_error()
    assert lib.wdf_ss_fwd_tp(one, one, None, 1, 1, 1, 1, one, None, None, None, 4, 64, 1, 8, 1e-6, None, one, one, None) == EINVAL
    assert b"{Is, nVt, R_port}" in lib.wdf_last_error()


def test_reverse_sweep_workspaces_hold_five_root_sums(lib):
    for ns, ni in ((0, 1), (1, 1), (2, 2), (4, 2)):
        kn = lib.wdf_ss_ncoef(ns, ni)
        assert lib.wdf_ss_bwd_ws_bytes(ns, ni, 130) == 3 * (kn + 5) * 8
        if ns:
            rec = ns * ns + ns + (kn + 5) * (ns + 1)
            assert lib.wdf_ss_bwd_tp_ws_bytes(ns, ni, 130, 4) == 3 * (kn + 5) * 8 + 4 * rec * 130 * 4
