"""GPU: the diode-root one-pass step (csrc/wdf_ss_nl_step.h: wdf_ss_nl_step_mse through Circuit.mse, wdf_ss_nl_step_esr through
Circuit._nl_step_tree + Circuit._mse_esr_nl_step) where tests/test_gpu_ss_nl_step.py and tests/test_gpu_ss_nl_esr_step.py do not
take it:

  A  two states WITH two sources (ns = ni = 2) on the MSE step, both lane widths, cold and from the snapshots;
  B  the sequential repair branch of the finish kernel on every instantiation (one sequence per lane, the (2,1), (1,2) and
     (2,2) trees, MSE + ESR), and the call after it, which starts from the snapshots the repair rewrote;
  C  a call in which the first group needs no repair and the others do (the launch's last wave adds both kinds of partial);
  D  the root tiers of ss_nl_step_kernel (LEAN / FAST / general) on either side of both tier boundaries;
  E  edge shapes of the MSE + ESR step (one chunk, T < 8, skip = T - 1, skip in the last blocks, more than 64 chunks);
  F  the (2,1) and (1,2) trees of the two existing files at their shapes, against the oracle instead of the host-probe path.

Reference, everywhere: the fp64 oracle's tree interpreter.  y = oracle.tree_fwd, the loss formed from it in numpy fp64 (the
mean squared error as oracle_hpf does; S, E, mse, esr, ga, gb as esr_terms / oracle_esr do), gradients = oracle.tree_grad
(complex step) with dLoss/dy formed from the oracle's own y.  No other path of this library is compared with.

Bounds (not derived from what the step gives; the rows are the ones the two existing files hold for this arithmetic):
  one capacitor, cold or repaired (the sequential recursion itself):  y 3e-6, S and E 1e-5, loss 2e-6 (MSE) / 1e-5 (each of
      mse, esr, mse + esr), gradients 3e-4 relative;
  the (2,1), (1,2), (2,2) trees, and every call that starts from snapshots:  y 4e-6, loss 1e-5, gradients 5e-4.
  S and E where section B and E ask for them on a larger tree: 1e-5, tests/test_gpu_ss_nl_esr_step.py's bound for the two sums.
A relative gradient error means something only where the oracle's component is not a small difference of large terms: section
E asserts |g_k| >= 3 % of sum |dLoss/dy . dy/dtheta_k| (a per-term fp32 error of 1e-5 stays below the 3e-4 bound), S > 0, E > 0.

Every check prints a line `FIG <section> | <case> | y=... loss=... grad=...` before it asserts (run with -s).

Measured on an MI355X (worst figure of each section): NOT MEASURED YET.  The module has been collected and its oracle side run
on the CPU (the silent group's y is exactly 0; the tier values land at -7.55, -7.45, -5.5, -4.05, -3.95 to 1e-7; the edge
shapes' seeds are the first at which no oracle gradient component cancels below 3 %); it has not run on a GPU.  Whoever runs it
first: take the worst `FIG` figure of each section from the output of `pytest -s`, put them here and in DESIGN.md's section on
this step, and treat a case over its bound as a finding (the bounds are not to be adjusted to the figures).
"""
import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_ss_nl_step import FS, THETA, cuda, hpf, oracle_hpf, rel  # noqa: E402
from test_gpu_ss_nl_step import one_call as mse_call  # noqa: E402
from test_gpu_ss_nl_esr_step import _ORACLE, _two_sources, _two_states, entry_of, esr_step, esr_terms, hpf_oracle, oracle_esr  # noqa: E402,F401
from test_gpu_ss_nl_esr_step import one_call as esr_call  # noqa: E402

COLD_11 = dict(y=3e-6, mse=2e-6, sums=1e-5, terms=1e-5, grad=3e-4)      # one capacitor: cold, or the sequential recursion
WIDER = dict(y=4e-6, mse=1e-5, sums=1e-5, terms=1e-5, grad=5e-4)        # larger trees; calls that start from snapshots


@pytest.fixture
def wdf():
    import tf_wdf
    return tf_wdf


@pytest.fixture(autouse=True)
def _oracle(oracle):
    _ORACLE["o"] = oracle                                        # (oracle_esr of tests/test_gpu_ss_nl_esr_step.py reads it there)


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """What this file's circuits cached goes back to the device when the file is done (as tests/test_gpu_ss_nl_esr_step.py
    does: tests/test_gpu_cache_identity.py relies on the caching allocator handing a freed block straight back)."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- the trees: the library's circuit, and the same program for the oracle's interpreter -----------------------------------
def _two_states_two_sources(wdf, n_up=1, n_down=1):
    """tests/test_gpu_circuit.py's (2,2) tree: Series(Parallel(Vs1, C1), Parallel(Series(R1, Vs2), C2)) + diode pair, y = v(C2)"""
    Vs1 = wdf.ResistiveVoltageSource(22.0e3, trainable=True)
    C1 = wdf.Capacitor(4.7e-9, FS, trainable=True)
    R1 = wdf.Resistor(3.3e3, True)
    Vs2 = wdf.ResistiveVoltageSource(10.0e3, trainable=True)
    C2 = wdf.Capacitor(10.0e-9, FS, trainable=True)
    top = wdf.Series(wdf.Parallel(Vs1, C1), wdf.Parallel(wdf.Series(R1, Vs2), C2))
    dp = wdf.DiodePair(top, 4.352e-9, Vt=0.0493, N_up=n_up, N_down=n_down, trainable=True)
    return wdf.Circuit(top, dp, C2), [Vs1.R, C1.C, R1.R, Vs2.R, C2.C, dp.Is, dp.nVt]


def build_tree(wdf, tree, n_up=1, n_down=1):
    """-> the resident circuit, its trainable values in the order of the oracle's theta"""
    if tree == (1, 1):
        circ, params = hpf(wdf, n_up, n_down)
    elif tree == (2, 2):
        circ, params = _two_states_two_sources(wdf, n_up, n_down)
    else:
        assert n_up == n_down == 1
        circ, params = (_two_states if tree == (2, 1) else _two_sources)(wdf)
    assert (circ.ns, circ.ni) == tree
    circ.to_device()
    assert circ._tree is not None
    return circ, params


def oracle_circuit(O, tree, n_up=1, n_down=1):
    def leaf(kind, param, vin=-1):
        return (kind, -1, -1, param, vin, -1)

    def join(kind, c0, c1):
        return (kind, c0, c1, -1, -1, -1)

    R, C, V, S, P = O.NODE_RESISTOR, O.NODE_CAPACITOR, O.NODE_RES_VSOURCE, O.NODE_SERIES, O.NODE_PARALLEL
    kw = dict(root_kind=O.ROOT_DIODE_PAIR, fs=FS, n_up=n_up, n_down=n_down)
    if tree == (1, 1):
        return hpf_oracle(O, n_up, n_down)
    if tree == (2, 1):      # _two_states: Parallel(Series(Ra, Ca), Series(Vr, Cb)), y = v(Ra); theta = [Ra, Rvr, Ca, Cb, Is, nVt]
        nodes = [leaf(R, 0), leaf(C, 2), join(S, 0, 1), leaf(V, 1, 0), leaf(C, 3), join(S, 3, 4), join(P, 2, 5)]
        return O.Circuit(nodes, top=6, probe=0, n_in=1, p_is=4, p_nvt=5, **kw)
    if tree == (1, 2):      # _two_sources: Parallel(Series(Va, Ca), Vb), y = v(Ca); theta = [Rva, Rvb, Ca, Is, nVt]
        nodes = [leaf(V, 0, 0), leaf(C, 2), join(S, 0, 1), leaf(V, 1, 1), join(P, 2, 3)]
        return O.Circuit(nodes, top=4, probe=1, n_in=2, p_is=3, p_nvt=4, **kw)
    # (2,2): theta = [Rs1, C1, R1, Rs2, C2, Is, nVt] (test_two_capacitor_two_source_tree_vs_oracle's node list)
    nodes = [leaf(V, 0, 0), leaf(C, 1), join(P, 0, 1), leaf(R, 2), leaf(V, 3, 1), join(S, 3, 4), leaf(C, 4), join(P, 5, 6), join(S, 2, 7)]
    return O.Circuit(nodes, top=8, probe=6, n_in=2, p_is=5, p_nvt=6, **kw)


def theta_of(params):
    """the values the device holds (fp32), as the oracle's fp64 theta"""
    return np.array([float(p) for p in params], dtype=np.float32).astype(np.float64)


def data(tree, B, T, seed, amp=1.2):
    rng = np.random.default_rng(seed)
    shape = (B, T, 2) if tree[1] == 2 else (B, T)
    x = (rng.standard_normal(shape) * (np.array([1.5, 0.7]) if tree == (2, 2) else amp)).astype(np.float32)
    tgt = (0.3 * rng.standard_normal((T, B))).astype(np.float32)
    return x, tgt


class Ref:
    """The oracle at one (tree, theta, x, target): y once; the MSE and MSE + ESR references formed from it on demand."""

    def __init__(self, tree, theta, x, tgt, n_up=1, n_down=1):
        self.O = _ORACLE["o"]
        self.tree, self.theta, self.x, self.tgt, self.n = tree, theta, x, tgt, (n_up, n_down)
        self.oc = oracle_circuit(self.O, tree, n_up, n_down)
        self.x64, self.t64 = x.astype(np.float64), tgt.astype(np.float64)
        self.y = self.O.tree_fwd(self.oc, theta, self.x64)
        self._mse, self._esr = None, {}

    def mse(self):
        """-> y, the mean squared error, its gradient (oracle_hpf's construction; oracle_hpf itself on the one-capacitor tree)"""
        if self._mse is None:
            if self.tree == (1, 1):
                self._mse = oracle_hpf(self.O, self.theta, self.x, self.tgt, *self.n)
            else:
                e = self.y - self.t64
                self._mse = (self.y, float(np.mean(e * e)), self.O.tree_grad(self.oc, self.theta, self.x64, 2.0 * e / e.size))
        return self._mse

    def gy_esr(self, skip):
        S, E, l3, (ga, gb) = esr_terms(self.y, self.tgt, skip)
        gy = ga * (self.y - self.t64) + gb * self.y
        gy[:skip] = 0.0
        return gy

    def esr(self, skip):
        """-> y, S, E, {mse, esr, mse + esr}, the gradient (oracle_esr's construction; oracle_esr itself on the one-capacitor tree)"""
        if skip not in self._esr:
            if self.tree == (1, 1):
                self._esr[skip] = oracle_esr(self.theta, self.x, self.tgt, *self.n, skip, y=self.y)
            else:
                S, E, l3, _ = esr_terms(self.y, self.tgt, skip)
                self._esr[skip] = (self.y, S, E, l3, self.O.tree_grad(self.oc, self.theta, self.x64, self.gy_esr(skip)))
        return self._esr[skip]

    def weight_of_the_gradients(self, gy):
        """|g_k| / sum |gy . dy/dtheta_k| per component: 1 when no term cancels"""
        dys = [self.O.tree_dtheta(self.oc, self.theta, k, self.x64)[1] for k in range(len(self.theta))]
        return np.array([abs(np.sum(gy * d)) / np.sum(np.abs(gy * d)) for d in dys])


def mse_entry(circ):
    ents = [e for e in circ._tree.cache.values() if e.get("loss", "mse") == "mse"]
    assert len(ents) == 1
    return ents[0]


def chunks_of(ent):
    """the chunk count the launches run with (ent["k"] is what was asked for)"""
    from wdf_hip import binding
    return binding.chunk_geom(ent["T"], ent["k"], 32)[1]


def groups_of(tree, B, esr):
    pair = B % 2 == 0 and (not esr or tree == (1, 1))             # two sequences per lane (wdf_capi_ss_step.hip, nl_step_launch)
    return -(-B // (128 if pair else 64))


def set_ctl(ent, field, value):
    from wdf_hip import binding
    binding._check(binding.lib().wdf_ss_nl_step_set(binding._ptr(ent["ws"]), field, float(value), binding._stream()), "set")


def check_mse(section, case, got, ref, bound):
    loss, g, y = got
    yref, lref, gref = ref.mse()
    e_y, e_l, e_g = float(np.max(np.abs(y - yref))), abs(loss - lref) / lref, rel(g, gref)
    print(f"FIG {section} | {case} | y={e_y:.2e} loss={e_l:.2e} grad={e_g:.2e} | loss {loss:.7e} / {lref:.7e}; per component {np.abs(g - gref) / np.abs(gref)}")
    assert e_y < bound["y"], (case, e_y)
    assert e_l < bound["mse"], (case, e_l)
    assert e_g < bound["grad"], (case, e_g)


def check_esr(section, case, got, ref, skip, bound, sums=True):
    loss, g, y, S, E, l3 = got
    yref, Sr, Er, l3r, gref = ref.esr(skip)
    e_y, e_S, e_E, e_l, e_g = float(np.max(np.abs(y - yref))), rel(S, Sr), rel(E, Er), rel(l3, l3r), rel(g, gref)
    e_l = max(e_l, abs(float(loss) - l3r[2]) / l3r[2])
    print(f"FIG {section} | {case} | y={e_y:.2e} S={e_S:.2e} E={e_E:.2e} loss={e_l:.2e} grad={e_g:.2e} | terms {l3} / {l3r}; "
          f"per component {np.abs(g - gref) / np.abs(gref)}")
    assert e_y < bound["y"], (case, e_y)
    if sums:
        assert e_S < bound["sums"] and e_E < bound["sums"], (case, e_S, e_E)
    assert e_l < bound["terms"], (case, e_l)
    assert e_g < bound["grad"], (case, e_g)


# ---- A: ns = ni = 2 on the MSE step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_up,n_down", [(1, 1), (2, 3)])
@pytest.mark.parametrize("B", [130, 67])
def test_two_states_two_sources_against_the_oracle(wdf, B, n_up, n_down):
    """16 tangents of two components and a 2 x 2 Psi: B = 130 two sequences per lane (two groups, a padded tail), B = 67 one
    (two groups); T = 1001: eleven chunks of 96 steps, a tail that is no multiple of 8.  Cold, then twice from the snapshots."""
    tree, T = (2, 2), 1001
    x, tgt = data(tree, B, T, 2200 + B)
    circ, params = build_tree(wdf, tree, n_up, n_down)
    xd, td = cuda(x), cuda(tgt)
    assert circ._nl_step_tree(xd, td, 50) is None                 # MSE + ESR keeps the composed path (tests/test_ss_nl_esr_step_cpu.py)
    ref = Ref(tree, theta_of(params), x, tgt, n_up, n_down)
    for call in range(3):
        got = mse_call(wdf, circ, params, xd, td)
        ent = mse_entry(circ)
        ctl = circ._tree.read_ctl(ent)
        print(f"call {call}: chunks {chunks_of(ent)}; {ctl}")
        assert chunks_of(ent) >= 4
        assert ctl["call"] == call + 1 and (call == 0 or ctl["have_snap"] == 1)
        check_mse("A", f"(2,2) B {B} N {n_up}/{n_down} call {call}", got, ref, WIDER)
        assert ctl["gated_groups"] == 0


# ---- B: the repair on every instantiation ---------------------------------------------------------------------------------
REPAIRS = [((1, 1), 131, None), ((2, 1), 130, None), ((2, 1), 131, None), ((1, 2), 130, None), ((1, 2), 131, None),
           ((2, 2), 130, None), ((2, 2), 131, None), ((1, 1), 131, 50), ((2, 1), 130, 50), ((1, 2), 131, 50)]


@pytest.mark.parametrize("tree,B,skip", REPAIRS, ids=[f"{t[0]}{t[1]}-B{b}-{'mse' if s is None else 'esr'}" for t, b, s in REPAIRS])
def test_the_repair_on_every_instantiation(wdf, tree, B, skip):
    """A cold call; a call under a tolerance nothing meets (every group's finishing wave runs its sequences again from t = 0);
    the tolerance back, and a call from the snapshots the repair wrote.  skip None: the MSE step, else MSE + ESR.  The (2,2)
    tree with N_up != N_down, the others with the symmetric pair (the repair is the general evaluation under either flag)."""
    from wdf_hip import lowering
    T = 1001
    esr = skip is not None
    n = (2, 3) if tree == (2, 2) else (1, 1)
    x, tgt = data(tree, B, T, 3300 + 10 * tree[0] + tree[1] + B)
    circ, params = build_tree(wdf, tree, *n)
    xd, td = cuda(x), cuda(tgt)
    ref = Ref(tree, theta_of(params), x, tgt, *n)
    groups = groups_of(tree, B, esr)
    exact = COLD_11 if tree == (1, 1) else WIDER

    def call(case, bound):
        if esr:
            got = esr_call(wdf, circ, params, xd, td, skip)
            ent = entry_of(circ, skip)
            ctl = circ._tree.read_ctl(ent)
            print(f"{case}: chunks {chunks_of(ent)}; {ctl}")
            check_esr("B", f"{tree} B {B} esr {case}", got, ref, skip, bound)
        else:
            got = mse_call(wdf, circ, params, xd, td)
            ent = mse_entry(circ)
            ctl = circ._tree.read_ctl(ent)
            print(f"{case}: chunks {chunks_of(ent)}; {ctl}")
            check_mse("B", f"{tree} B {B} mse {case}", got, ref, bound)
        return ent, ctl

    ent, ctl = call("cold", exact)
    assert chunks_of(ent) > 1
    set_ctl(ent, 8, -1.0)
    ent, ctl = call("repaired", exact)
    assert ctl["gated_groups"] == groups and ctl["n_bad"] > 0
    set_ctl(ent, 8, lowering.NL_TOL)
    ent, ctl = call("after", WIDER)
    assert ctl["gated_groups"] == 0 and ctl["n_bad"] == 0


# ---- C: some groups repaired, others not -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_up,n_down", [(1, 1), (2, 3)])
@pytest.mark.parametrize("B", [256, 129])
@pytest.mark.parametrize("skip", [None, 50])
def test_some_groups_repaired_and_others_not(wdf, skip, B, n_up, n_down):
    """The one-capacitor clipper, cold, with the cold warm-up set to 0: every chunk starts from z = 0 at its own first sample.
    The first group's input is identically zero, so its states ARE zero (sign(0) = 0 at the root: zero in, zero out) and its
    boundaries miss by exactly 0; the other groups miss by the size of their state and are re-run.  The launch's last wave
    adds the unrepaired group's walk + chunk sums and the repaired groups' sequential sums.  B = 256: two sequences per lane,
    two groups; B = 129: one per lane, three groups, the last with a single live lane."""
    tree, T = (1, 1), 1000
    esr = skip is not None
    groups = groups_of(tree, B, esr)
    silent = B // groups if B % 2 == 0 else 64
    assert (groups, silent) == {256: (2, 128), 129: (3, 64)}[B]
    x, tgt = data(tree, B, T, 4400 + B)
    x[:silent] = 0.0
    circ, params = build_tree(wdf, tree, n_up, n_down)
    xd, td = cuda(x), cuda(tgt)
    ref = Ref(tree, theta_of(params), x, tgt, n_up, n_down)
    assert np.all(ref.y[:, :silent] == 0.0) and np.min(np.max(np.abs(ref.y[:, silent:]), axis=0)) > 1e-3
    ent = circ._tree.entry(xd, td, "mse+esr", skip) if esr else circ._tree.entry(xd, td)
    assert chunks_of(ent) > 1
    set_ctl(ent, 3, 0)
    if esr:
        got = esr_call(wdf, circ, params, xd, td, skip)
        assert entry_of(circ, skip) is ent
    else:
        got = mse_call(wdf, circ, params, xd, td)
        assert mse_entry(circ) is ent
    ctl = circ._tree.read_ctl(ent)
    print(f"chunks {chunks_of(ent)}; {ctl}")
    assert np.all(got[2][:, :silent] == 0.0)
    if esr:
        check_esr("C", f"B {B} N {n_up}/{n_down} esr", got, ref, skip, COLD_11)
    else:
        check_mse("C", f"B {B} N {n_up}/{n_down} mse", got, ref, COLD_11)
    assert ctl["w_used"] == 0 and ctl["call"] == 1
    assert ctl["gated_groups"] == groups - 1 and ctl["n_bad"] > 0


# ---- D: the root tiers of ss_nl_step_kernel ----------------------------------------------------------------------------------
def port_resistance(theta):
    """what the root of hpf() sees: R parallel to (Rs in series with the capacitor's 1 / (2 fs C))"""
    s = theta[1] + 1.0 / (2.0 * FS * theta[2])
    return theta[0] * s / (theta[0] + s)


def tier_theta(l0, n):
    """THETA with Is such that log(Rp Is / nVt) - log N = l0 (before Is is rounded to fp32)"""
    th = THETA.copy()
    th[3] = np.float64(np.float32(np.exp(l0 + np.log(n)) * th[4] / port_resistance(th)))
    return th


def tier_of(l0):
    """ss_nl_step_kernel's choice for a symmetric pair"""
    return "lean" if -80.0 <= l0 <= -7.5 else ("fast" if l0 <= -4.0 else "general")


TIERS = [(-7.55, "lean"), (-7.45, "fast"), (-5.5, "fast"), (-4.05, "fast"), (-3.95, "general")]


@pytest.mark.parametrize("B,n,l0,tier", [(130, n, l0, t) for n in (1, 2) for l0, t in TIERS] + [(67, 1, -5.5, "fast")])
def test_root_tiers_against_the_oracle(wdf, B, n, l0, tier):
    """LEAN for L - log N in [-80, -7.5], FAST up to -4, the general evaluation above: 0.05 on either side of both boundaries
    (where the series truncations of a tier are at their worst) and the middle of FAST, whose SYM && FAST arithmetic in nl_step
    (the cubic series of omega_1 / (1 + omega_1); Da, DL, DV through copysign and (a != 0)) no other test runs.  MSE cold and
    from the snapshots, MSE + ESR with skip = 50.  B = 130: two sequences per lane; B = 67: one."""
    tree, T, skip = (1, 1), 1500, 50
    theta = tier_theta(l0, n)
    circ, params = hpf(wdf, n, n, theta=theta)
    circ.to_device()
    assert np.array_equal(theta_of(params), theta)
    rp = float(circ._tree.host_coef()[1])
    assert abs(rp - port_resistance(theta)) < 1e-6 * rp
    got_l0 = float(np.log(rp * theta[3] / theta[4]) - np.log(float(n)))
    print(f"Rp {rp:.3f}, Is {theta[3]:.4e}: L - log N = {got_l0:.5f} ({tier})")
    assert abs(got_l0 - l0) < 1e-3 and tier_of(got_l0) == tier
    x, tgt = data(tree, B, T, 5500 + B)
    xd, td = cuda(x), cuda(tgt)
    ref = Ref(tree, theta, x, tgt, n, n)
    for call in range(2):
        got = mse_call(wdf, circ, params, xd, td)
        ctl = circ._tree.read_ctl(mse_entry(circ))
        check_mse("D", f"l0 {l0} ({tier}) N {n} B {B} mse call {call}", got, ref, COLD_11 if call == 0 else WIDER)
        assert ctl["gated_groups"] == 0
    got = esr_call(wdf, circ, params, xd, td, skip)
    check_esr("D", f"l0 {l0} ({tier}) N {n} B {B} esr", got, ref, skip, COLD_11)
    assert chunks_of(entry_of(circ, skip)) >= 4 and chunks_of(mse_entry(circ)) >= 4


# ---- E: edge shapes of the MSE + ESR step ------------------------------------------------------------------------------------
# (seeds: the first of 6600 + 7 B + T, 7001, 7002, ... at which no component of the oracle's gradient cancels below 3 %)
EDGES = [((1, 1), 1, 40, 0, (2, 3), 6647),          # one chunk shorter than 64 steps
         ((1, 1), 1, 7, 6, (1, 1), 6614),           # T < 8, skip = T - 1, n = 1
         ((1, 1), 2, 7, 6, (1, 1), 6621),           # the same with the pair kernel at B = WD
         ((1, 1), 67, 1001, 999, (1, 1), 7001),     # skip in the last blocks of the last chunk
         ((1, 1), 6, 6145, 6100, (2, 3), 12787),    # 65 chunks of 96 steps, the last one a single sample
         ((1, 1), 3, 6145, 6100, (2, 3), 12766),    # the same with one sequence per lane
         ((2, 1), 3, 6145, 50, (1, 1), 7001)]       # LOSS = 1, NS = 2: the finish reads the chunks' sums without the early fetch


def assert_the_gradients_mean_something(ref, gy, S, E):
    w = ref.weight_of_the_gradients(gy)
    print(f"oracle: S {S:.4e}, E {E:.4e}, |g| / sum |terms| per component {w}")
    assert S > 0.0 and E > 0.0
    assert np.all(w >= 0.03), w


@pytest.mark.parametrize("tree,B,T,skip,n,seed", EDGES, ids=[f"{t[0]}{t[1]}-B{b}-T{T}-skip{s}-N{n[0]}{n[1]}" for t, b, T, s, n, _ in EDGES])
def test_esr_edge_shapes_against_the_oracle(wdf, tree, B, T, skip, n, seed):
    """test_first_call_against_the_oracle of tests/test_gpu_ss_nl_esr_step.py (every B there is even, every T >= 1500) at the
    shapes where an index or a count can go wrong."""
    x, tgt = data(tree, B, T, seed)
    circ, params = build_tree(wdf, tree, *n)
    ref = Ref(tree, theta_of(params), x, tgt, *n)
    _, Sr, Er, _, _ = ref.esr(skip)
    assert_the_gradients_mean_something(ref, ref.gy_esr(skip), Sr, Er)
    got = esr_call(wdf, circ, params, cuda(x), cuda(tgt), skip)
    ent = entry_of(circ, skip)
    K = chunks_of(ent)
    print(f"chunks {K} (asked for {ent['k']}); {circ._tree.read_ctl(ent)}")
    if T == 6145:
        assert K == 65 and K > 64
    elif T < 64:
        assert K == 1
    check_esr("E", f"{tree} B {B} T {T} skip {skip} N {n[0]}/{n[1]}", got, ref, skip, COLD_11 if tree == (1, 1) else WIDER)


def test_mse_with_more_than_64_chunks_and_one_sequence_per_lane(wdf):
    """(3, 6145) on the MSE step with the symmetric pair: 65 chunks, lane k and lane k + 64 of the finish read the chunks' sums."""
    tree, B, T, n = (1, 1), 3, 6145, (1, 1)
    x, tgt = data(tree, B, T, 7002)
    circ, params = build_tree(wdf, tree, *n)
    ref = Ref(tree, theta_of(params), x, tgt, *n)
    e = ref.y - ref.t64
    assert_the_gradients_mean_something(ref, 2.0 * e / e.size, float(np.sum(e * e)), float(np.sum(ref.y ** 2)))
    got = mse_call(wdf, circ, params, cuda(x), cuda(tgt))
    ent = mse_entry(circ)
    print(f"chunks {chunks_of(ent)} (asked for {ent['k']}); {circ._tree.read_ctl(ent)}")
    assert chunks_of(ent) == 65
    check_mse("E", f"{tree} B {B} T {T} mse", got, ref, COLD_11)


# ---- F: the larger trees of the two existing files, against the oracle ----------------------------------------------------------
LARGER = [((2, 1), 96, 3000, 6, 1.5, None), ((1, 2), 192, 2048, 16, 1.2, None), ((2, 1), 96, 3000, 6, 1.2, 50), ((1, 2), 192, 2048, 16, 1.2, 50)]


@pytest.mark.parametrize("tree,B,T,seed,amp,skip", LARGER, ids=[f"{t[0]}{t[1]}-{'mse' if s is None else 'esr'}" for t, _, _, _, _, s in LARGER])
def test_larger_trees_against_the_oracle(wdf, tree, B, T, seed, amp, skip):
    """test_two_state_diode_tree_against_the_host_probe_path, test_one_state_two_sources_diode_tree_against_the_host_probe_path
    (MSE) and test_larger_trees_against_the_host_probe_path (MSE + ESR, skip = 50) at their shapes, seeds and amplitudes: cold,
    then twice from the snapshots, against the fp64 oracle."""
    x, tgt = data(tree, B, T, seed, amp)
    circ, params = build_tree(wdf, tree)
    xd, td = cuda(x), cuda(tgt)
    ref = Ref(tree, theta_of(params), x, tgt)
    for call in range(3):
        if skip is None:
            got = mse_call(wdf, circ, params, xd, td)
            ctl = circ._tree.read_ctl(mse_entry(circ))
            check_mse("F", f"{tree} mse call {call}", got, ref, WIDER)
        else:
            got = esr_call(wdf, circ, params, xd, td, skip)
            ctl = circ._tree.read_ctl(entry_of(circ, skip))
            check_esr("F", f"{tree} esr call {call}", got, ref, skip, WIDER, sums=False)
        assert ctl["gated_groups"] == 0
