"""GPU: the streamed-coefficient kernels (csrc/wdf_ss_dyn.h) in time chunks with MORE THAN ONE state, and the state they carry.

1-3: under the two-different-diode root the chunked forward (wdf_ss_dyn_fwd_tp: verified chunks, gated re-run) and the three
launches of the chunked sweep (wdf_ss_dyn_bwd_tp: MODE 1, ss_dyn_bwd_combine_kernel, MODE 2) on trees of two, three and four
capacitors, one and two sources, static rows (the double accumulators), rows per sequence and rows per sample (the emitting pass)
at 70 x 131: one full and one ragged wave, four chunks of 40, 40, 40 and 11 steps.  With one state the chunk map is a scalar: a
transposed rec[j][s], a wrong hom update or a wrong stride in the seven-float rpart record cannot show there.
4-6: z0, zT and gz0 -- through Circuit.__call__(x, z0=..., return_state=True) and at the binding, for the ideal-source root,
the symmetric pair, the two different diodes and the network root -- and what the binding refuses before any launch.

References: the fp64 tree of tests/asym_pot_tree_ref.py (central differences for the gradients; every component keeps
|sum of terms| >= 0.03 sum |terms|: asserted) and the row-level fp64 recursion of tests/ss_rows_ref.py on the float32-rounded rows,
pinned to the tree in tests/test_ss_dyn_chunks_state_cpu.py.  Bounds (the project's own for these kernels) and the worst value
measured on an MI355X over this module:

    against the fp64 reference   y, zT                         3e-6 V           6.9e-7 V (the HPF tree under DiodePair, carried;
                                                                                the two-diode cases: y 2.1e-7, zT 8.8e-8)
                                 every live gradient component 3e-4 relative    3.7e-6 (four_state_vs_seq, four chunks)
                                 gz0, per state row            3e-4 of the row's largest reference entry    3.7e-7
    chunked against sequential   y, zT                         2e-6 V           0: the same bits everywhere (see below)
                                 gradients                     2e-5 relative    3.8e-6 (four states, the planner's 16 chunks)
                                 gz0, per state row            2e-5 relative    2.5e-7

New with this module (never measured before): gz0 for any root, and every figure of the chunked sweep and the chunked forward
with more than one state under the two-diode root.  The chunked forward gives the sequential run's bits in all of these runs:
with an eight-step warm-up the waves miss and are re-run by the sequential kernel, and where the warm-up suffices (two states,
256 steps) the chunk arrives at the boundary with a float32 miss of exactly 0.  A split run carried through zT -> z0 is
bit-equal to the unsplit one under every root, sequentially and in chunks.
"""
import numpy as np
import pytest

import ss_asym_cases as base
import ss_dyn_asym_cases as cases
import ss_rows_ref as rref
from test_gpu_ss_dyn_asym import check_against_reference, cuda, rel, run

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NEW_CASES = ["two_state_vs2_c", "three_state_c", "three_state_r1", "four_state_c", "four_state_vs", "four_state_vs_seq"]
Y_REF, G_REF, Y_PATH, G_PATH = 3e-6, 3e-4, 2e-6, 2e-5
SPLIT = 57


@pytest.fixture(scope="module")
def wdf():
    import tf_wdf
    from wdf_hip import binding
    binding.require_gpu()
    return tf_wdf


@pytest.fixture(scope="module")
def reference(oracle):
    """case -> its reference (computed once per case, shared, never written to)."""
    memo = {}

    def get(name):
        if name not in memo:
            r = cases.reference(oracle, name)
            for v in r.values():
                v.setflags(write=False)
            memo[name] = r
        return memo[name]
    return get


def tt(y):
    return y.as_subclass(torch.Tensor).detach()


def sweep_spy(monkeypatch):
    """-> the list every binding.ss_dyn_bwd_tp call appends (requested chunks, chunks cut, ns) to"""
    from wdf_hip import binding as wb
    seen, real = [], wb.ss_dyn_bwd_tp

    def spy(x, rows, ns, ni, zstash, gy, n_chunks, *a, **kw):
        seen.append((int(n_chunks), wb.dyn_chunks(int(x.shape[1]), n_chunks), int(ns)))
        return real(x, rows, ns, ni, zstash, gy, n_chunks, *a, **kw)
    monkeypatch.setattr(wb, "ss_dyn_bwd_tp", spy)
    return seen


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NEW_CASES)
def test_chunked_sweep_with_more_than_one_state_vs_reference(wdf, reference, monkeypatch, name):
    """A sequential forward and the sweep in four chunks (MODE 1 / combine / MODE 2) against the fp64 tree: y and every live
    gradient; then 9 chunks of 16 steps (what 16 asked-for chunks are cut to) and 17 of 8 against the sequential sweep."""
    from wdf_hip import lowering
    r = reference(name)
    seen = sweep_spy(monkeypatch)
    circ, params = cases.build(wdf, name, lowering.SsTpPlan(1, 0, 1.0e-6, 4))
    ns = {"two_state": 2, "three_state": 3, "four_state": 4}[cases.CASES[name]["tree"]]
    assert (circ.ns, circ.ni) == (ns, cases.CASES[name]["shape"][2])
    xin, y4, g4 = check_against_reference(wdf, circ, params, r, f"{name}, sweep in 4 chunks")
    assert circ.time_parallel.k_bwd == 4 and circ.time_parallel.k_fwd == 1 and seen == [(4, 4, ns)], (circ.time_parallel, seen)
    if cases.CASES[name]["pot"] is not None:                          # rows per sample: the emitting pass; per sequence: the sums
        assert list(circ._dyn_chan_const.values()) == [name.endswith("_seq")]
    gy = cuda(r["gy"])
    seq, p_seq = cases.build(wdf, name, None)
    y_seq, g_seq = run(wdf, seq, p_seq, xin, gy)
    assert len(seen) == 1                                             # (the sequential sweep is not the chunked entry point)
    dy, dg = float((tt(y4) - y_seq).abs().max()), rel(g4, g_seq)
    print(f"{name}: 4 chunks against sequential: max |dy| = {dy:.3g}; gradients {np.array2string(dg, precision=3)}")
    assert dy <= Y_PATH and np.all(dg <= G_PATH), (g4, g_seq)
    for k, cut in ((16, 9), (17, 17)):
        del seen[:]
        tp, p_tp = cases.build(wdf, name, lowering.SsTpPlan(1, 0, 1.0e-6, k))
        y_tp, g_tp = run(wdf, tp, p_tp, xin, gy)
        dy, dg = float((y_tp - y_seq).abs().max()), rel(g_tp, g_seq)
        print(f"{name}: {cut} chunks against sequential: max |dy| = {dy:.3g}; gradients {np.array2string(dg, precision=3)}")
        assert seen == [(k, cut, ns)], seen
        assert dy <= Y_PATH and g_tp.shape == g_seq.shape and np.all(dg <= G_PATH), (g_tp, g_seq)


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_state_vs2_c", "four_state_vs"])
def test_chunked_forward_with_more_than_one_state(wdf, oracle, reference, name):
    """Four chunks that warm up for eight steps from z = 0 -- eight steps cannot forget these capacitors: whatever the device's
    verdict, y and the gradients are the sequential run's.  Where the fp64 rows recursion says a wave arrives at a boundary
    further than tol (plus 6e-6 V: twice the bound on a state's own fp32 error) from the true state, that wave was re-run."""
    from wdf_hip import lowering, binding as wb
    r = reference(name)
    B, T, ni = cases.CASES[name]["shape"]
    xin, gy = cuda(cases.with_pot(r["x"], r["r"])), cuda(r["gy"])
    seq, p_seq = cases.build(wdf, name, None)
    y_seq, g_seq = run(wdf, seq, p_seq, xin, gy)
    plan = lowering.SsTpPlan(4, 8, 1.0e-6, 4)
    lowering.LAST_SS_TP_STATUS["status"] = None
    circ, params = cases.build(wdf, name, plan)
    y_tp, g_tp = run(wdf, circ, params, xin, gy)
    st = wb.ss_tp_status(lowering.LAST_SS_TP_STATUS["status"])
    assert lowering.LAST_SS_TP_STATUS["chunks_used"] == 4 and lowering.LAST_SS_TP_STATUS["warmup_used"] == 8
    dy, dg = float((y_tp - y_seq).abs().max()), rel(g_tp, g_seq)
    # the boundaries in fp64: the true state at 40, 80, 120 and the one eight steps from zero arrive with
    rows = rref.rows_of(seq, r["r"])
    x64 = r["x"].astype(np.float64).reshape(B, T, ni)
    root = rref.root_asym(oracle, r["theta"][-4:])
    L, _ = wb.chunk_geom(T, plan.k_fwd, 8)
    miss, z = np.zeros(B), None
    for t0 in range(L, T, L):
        _, z = rref.run(rref.time_slice(rows, t0 - L, t0), x64[:, t0 - L:t0], circ.ns, ni, root, z0=z)
        _, zw = rref.run(rref.time_slice(rows, t0 - plan.warmup, t0), x64[:, t0 - plan.warmup:t0], circ.ns, ni, root)
        miss = np.maximum(miss, np.max(np.abs(zw - z), axis=0))
    waves = [float(np.max(miss[w:w + 64])) for w in range(0, B, 64)]
    must = sum(m > plan.tol + 6e-6 for m in waves)
    print(f"{name}: verdict {st}; fp64 boundary miss per wave {np.array2string(np.array(waves), precision=3)} V -> at least {must} "
          f"waves re-run; max |y_tp - y_seq| = {dy:.3g}; gradients {np.array2string(dg, precision=3)}")
    assert L == 40 and dy <= Y_PATH and np.all(dg <= G_PATH), (g_tp, g_seq)
    if must:
        assert st["gated_waves"] >= must and st["n_bad"] >= 1, st


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree,pot_on", [("two_state", "Vs2"), ("four_state", None)])
def test_the_planners_own_plan_on_trees_with_more_than_one_state(wdf, tree, pot_on):
    """time_parallel="auto" at 70 x 1024 against the sequential kernels: the exact chunked sweep, and the forward in verified chunks
    where the plan speculates -- then with a clean verdict."""
    from wdf_hip import binding as wb, lowering
    B, T = 70, 1024
    ni = 2 if tree == "two_state" else 1
    x, gy = base.data("hpf", B + T, (B, T, ni))
    xin, gy = cuda(cases.with_pot(x, cases.pot_channel(B, T, 2.0e3, 40.0e3, 3) if pot_on else None)), cuda(gy)

    def one(tp):
        circ, params = cases.BUILD[tree](wdf, pot_on, tp)
        lowering.LAST_SS_TP_STATUS["status"] = None
        y, g = run(wdf, circ, params, xin, gy)
        st = lowering.LAST_SS_TP_STATUS["status"]
        return circ, y, g, (None if st is None else wb.ss_tp_status(st))

    _, y_seq, g_seq, st_seq = one(None)
    circ, y_tp, g_tp, st_tp = one("auto")
    plan = next(iter(circ._dyn_plans.values()))[0]
    assert st_seq is None and plan.k_bwd >= 2 and circ.ns >= 2, plan
    if st_tp is not None:
        assert st_tp["n_bad"] == 0, (st_tp, plan)
    dy, dg = float((y_tp - y_seq).abs().max()), rel(g_tp, g_seq)
    print(f"{tree}: plan {plan}; verdict {st_tp}; max |y_tp - y_seq| = {dy:.3g}; gradients {np.array2string(dg, precision=3)}")
    assert dy <= Y_PATH
    assert g_tp.shape == g_seq.shape and np.all(dg <= G_PATH), (g_tp, g_seq)


def test_verified_forward_that_holds_with_two_states(wdf, oracle):
    """The planner does not speculate on these trees (with the diodes off a capacitor keeps its charge: the step's Jacobian
    has a mode at 1), but driven at 1.2 V the two-state tree forgets: in fp64 the state 256 steps from zero is within 1e-10 V of
    the true one at t = 512.  Two chunks with that warm-up: where the reference's miss is below a hundredth of tol the device's
    verdict is clean, no wave is re-run, and y is the chunk kernels' own -- against the sequential run."""
    from wdf_hip import binding as wb, lowering
    B, T, ni = 70, 1024, 2
    plan = lowering.SsTpPlan(2, 256, 1.0e-6, 16)
    x, gy = base.data("hpf", B + T, (B, T, ni))
    r = cases.pot_channel(B, T, 2.0e3, 40.0e3, 3)
    xin, gy = cuda(cases.with_pot(x, r)), cuda(gy)
    seq, p_seq = cases.two_state(wdf, "Vs2", None)
    y_seq, g_seq = run(wdf, seq, p_seq, xin, gy)
    lowering.LAST_SS_TP_STATUS["status"] = None
    circ, params = cases.two_state(wdf, "Vs2", plan)
    y_tp, g_tp = run(wdf, circ, params, xin, gy)
    st = wb.ss_tp_status(lowering.LAST_SS_TP_STATUS["status"])
    rows, x64 = rref.rows_of(seq, r), x.astype(np.float64)
    root = rref.root_asym(oracle, base.f32(base.DIODES))
    t0 = wb.chunk_geom(T, plan.k_fwd, 8)[0]
    _, z = rref.run(rref.time_slice(rows, 0, t0), x64[:, :t0], 2, ni, root)
    _, zw = rref.run(rref.time_slice(rows, t0 - plan.warmup, t0), x64[:, t0 - plan.warmup:t0], 2, ni, root)
    miss = float(np.max(np.abs(zw - z)))
    dy, dg = float((y_tp - y_seq).abs().max()), rel(g_tp, g_seq)
    print(f"two_state, {plan}: fp64 boundary miss {miss:.3g} V; verdict {st}; max |y_tp - y_seq| = {dy:.3g}; "
          f"gradients {np.array2string(dg, precision=3)}")
    assert t0 == 512 and lowering.LAST_SS_TP_STATUS["chunks_used"] == 2
    if miss <= 0.01 * plan.tol:
        assert st["n_bad"] == 0 and st["gated_waves"] == 0 and st["max_miss"] <= plan.tol, st
    assert dy <= Y_PATH and np.all(dg <= G_PATH), (g_tp, g_seq)


# 4 ---------------------------------------------------------------------------------------------------------------------
def split_and_whole(make, xin, what, y_ref=None):
    """circ(x[:, :57]) then circ(x[:, 57:], z0 = the state the first call left) against circ(x): sequentially -- the same fp32
    arithmetic per step from the same state, so the same bits -- and in three verified chunks per call (warm-up 8; z0 starts
    every chunk whose warm-up reaches t = 0, the last chunk and the gated re-run write zT), within the path bounds."""
    from wdf_hip import lowering
    whole = make(None)
    y, zT = whole(xin, return_state=True)
    y, zT = tt(y).clone(), tt(zT).clone()
    assert tuple(zT.shape) == (whole.ns, xin.shape[0]) and float(zT.abs().max()) > 1e-3
    if y_ref is not None:
        d = float(np.max(np.abs(y.cpu().numpy() - y_ref)))
        print(f"{what}: unsplit: max |y - ref| = {d:.3g}")
        assert d <= Y_REF
    for tp in (None, lowering.SsTpPlan(3, 8, 1.0e-6, 3)):
        circ = make(tp)
        taken = []
        for part, z_in in ((xin[:, :SPLIT], None), (xin[:, SPLIT:], "carried")):
            lowering.LAST_SS_TP_STATUS.update(status=None, chunks_used=None, warmup_used=None)
            out = circ(part, z0=(None if z_in is None else taken[-1][1]), return_state=True)
            taken.append(out)
            if tp is None:                                            # which forward ran: the sequential one leaves no verdict
                assert lowering.LAST_SS_TP_STATUS["status"] is None
            else:
                assert lowering.LAST_SS_TP_STATUS["status"] is not None
                assert (lowering.LAST_SS_TP_STATUS["chunks_used"], lowering.LAST_SS_TP_STATUS["warmup_used"]) == (3, 8)
        (y1, z1), (y2, z2) = taken
        y12, z2 = torch.cat([tt(y1), tt(y2)]), tt(z2)
        dy, dz = float((y12 - y).abs().max()), float((z2 - zT).abs().max())
        print(f"{what}, {'sequential' if tp is None else 'three chunks'}: split at {SPLIT} against unsplit: max |dy| = {dy:.3g}, "
              f"max |dzT| = {dz:.3g}")
        assert tuple(y12.shape) == tuple(y.shape) and tuple(z2.shape) == tuple(zT.shape)
        if tp is None:
            assert torch.equal(y12, y) and torch.equal(z2, zT)
        assert dy <= Y_PATH and dz <= Y_PATH
        if y_ref is not None:
            d = float(np.max(np.abs(y12.cpu().numpy() - y_ref)))
            print(f"{what}: split: max |y - ref| = {d:.3g}")
            assert d <= Y_REF


@pytest.mark.parametrize("name", ["two_state_vs2_c", "four_state_c"])
def test_carried_state_through_circuit_two_diode_root(wdf, reference, name):
    r = reference(name)
    xin = cuda(cases.with_pot(r["x"], r.get("r")))
    split_and_whole(lambda tp: cases.build(wdf, name, tp)[0], xin, name, r["y"])


def test_carried_state_through_circuit_diode_pair_with_a_pot(wdf, oracle):
    from test_gpu_ss_dyn import build_hpf, hpf_oracle, pot_channel
    B, T = 70, 131
    vals = [33.0e3, 1.0e3, 22.0e-9, 4.352e-9, 25.85e-3 * 1.906]
    rng = np.random.default_rng(B + T)
    x = (1.5 * rng.standard_normal((B, T))).astype(np.float32)
    xr = np.stack([x, pot_channel(B, T, 300.0, 5.0e3, 1)], axis=-1)
    y_ref = oracle.tree_fwd(hpf_oracle(oracle, "diode", "Vs"), np.array(vals, dtype=np.float32).astype(np.float64), xr.astype(np.float64))

    def make(tp):
        circ = build_hpf(wdf, "diode", "Vs", vals)[0]
        circ.time_parallel = tp
        return circ
    split_and_whole(make, cuda(xr), "HPF tree, DiodePair, pot on Vs", y_ref)


def test_carried_state_through_circuit_network_root(wdf, golden):
    """test_three_state_tree_with_a_pot_and_an_mlp_root's circuit at 40 x 131 (ten blocks of four sequences), path against path."""
    from layers import DenseRootModel
    from test_gpu_ss_dyn import FS, _net, pot_channel
    js, _, _ = _net(golden, "2x8")
    B, T = 40, 131
    rng = np.random.default_rng(33)
    x = (0.8 * rng.standard_normal((B, T))).astype(np.float32)
    xr = np.stack([x, pot_channel(B, T, 2.0e3, 50.0e3, 6)], axis=-1)

    def make(tp):
        Vs = wdf.ResistiveVoltageSource(2.2e3, trainable=True)
        R1, Rp = wdf.Resistor(15.0e3, True), wdf.Resistor(10.0e3, True)
        C0, C1, C2 = wdf.Capacitor(47.0e-9, FS, True), wdf.Capacitor(10.0e-9, FS, True), wdf.Capacitor(22.0e-9, FS, True)
        top = wdf.Parallel(wdf.Series(Rp, C2), wdf.Series(wdf.Series(Vs, C0), wdf.Parallel(R1, C1)))
        circ = wdf.Circuit(top, DenseRootModel(js), C2, per_sample_R=Rp, time_parallel=tp)
        assert (circ.ns, circ.ni) == (3, 1)
        return circ
    split_and_whole(make, cuda(xr), "three states, pot, network root")


# 5 ---------------------------------------------------------------------------------------------------------------------
def _rc_lowpass(wdf, pot):
    R1, C1 = wdf.Resistor(1000.0, True), wdf.Capacitor(1.0e-6, 48000.0, True)
    return wdf.Circuit(wdf.Inverter(wdf.Series(R1, C1)), wdf.IdealVoltageSource(), C1, per_sample_R=R1 if pot else None)


def binding_setup(wdf, oracle, root, shape):
    """-> rows float32 (numpy), ns, ni, root kind, rootp | None, (n_up, n_down), the reference's root.  `shape`: "70x40" (two
    states, two sources, a row per sample; the ideal-source root: the RC low-pass, a row per sample), "65x24" (four states, one
    static row; the RC low-pass: its static row), "1x1" (as 70x40)."""
    from wdf_hip import binding as wb
    B, T = (int(v) for v in shape.split("x"))
    static = shape == "65x24"
    if root == "none":
        circ = _rc_lowpass(wdf, not static)
        r = None if static else cases.pot_channel(B, T, 300.0, 3.0e3, 9)
    elif static:
        circ, r = cases.four_state(wdf)[0], None
    else:
        circ, r = cases.two_state(wdf, "Vs2")[0], cases.pot_channel(B, T, 2.0e3, 40.0e3, 3)
    rows = rref.rows_of(circ, r).astype(np.float32)
    if root == "none":
        return rows, circ.ns, circ.ni, wb.ROOT_NONE, None, (1, 1), rref.root_none
    if root == "diode":
        rootp = base.f32([4.352e-9, 25.85e-3 * 1.906])
        nud = (1, 2) if static else (1, 1)
        return rows, circ.ns, circ.ni, wb.ROOT_DIODE_PAIR, rootp, nud, rref.root_diode(oracle, rootp[0], rootp[1], *nud)
    rootp = base.f32(base.DIODES)
    return rows, circ.ns, circ.ni, wb.ROOT_ASYM_PAIR, rootp, (1, 1), rref.root_asym(oracle, rootp)


def draw(B, T, ns, ni, k):
    """x [B,T,ni], z0 [ns,B] in +-0.2 V, gy [T,B] (float32) of draw k"""
    rng = np.random.default_rng(B + T + ns + k)
    x = (1.2 * rng.standard_normal((B, T, ni))).astype(np.float32)
    z0 = rng.uniform(-0.2, 0.2, (ns, B)).astype(np.float32)
    return x, z0, (rng.standard_normal((T, B)) / (B * T)).astype(np.float32)


def one_step_balance(rows, ns, ni, ref_root, x, z0, gy, h=1.0e-6):
    """T = 1: |t1 + t2| / (|t1| + |t2|) per entry of dL/dz0 = gy cy + gy fy Da ca (fp64; Da by central differences) -> [ns,B]"""
    c = rref.split_rows(rows, ns, ni, x.shape[0], 1)
    xt = x[:, 0, :].T.astype(np.float64)
    a = np.sum(c["ca"][0] * z0, axis=0) + np.sum(c["da"][0] * xt, axis=0)
    Da = (ref_root(a + h, c["rp"][0]) - ref_root(a - h, c["rp"][0])) / (2.0 * h)
    t1, t2 = c["cy"][0] * gy[0], c["ca"][0] * (c["fy"][0] * gy[0] * Da)
    return np.abs(t1 + t2) / (np.abs(t1) + np.abs(t2))


@pytest.mark.parametrize("shape", ["70x40", "65x24", "1x1"])
@pytest.mark.parametrize("root", ["none", "diode", "asym"])
def test_z0_zT_and_gz0_at_the_binding(wdf, oracle, root, shape):
    """wdf_ss_dyn_fwd / _bwd from a random z0 in +-0.2 V against the rows recursion in fp64 on the same float32 rows: y, zT and
    gz0 (central differences); then wdf_ss_dyn_fwd_tp (three chunks, warm-up 8) and wdf_ss_dyn_bwd_tp (three chunks) against them.
    65 x 24: a second wave with one live lane; 1 x 1: one chunk, whatever is asked for."""
    from wdf_hip import binding as wb
    B, T = (int(v) for v in shape.split("x"))
    rows, ns, ni, kind, rootp, (n_up, n_down), ref_root = binding_setup(wdf, oracle, root, shape)
    assert (ns, ni) == ((1, 1) if root == "none" else (4, 1) if shape == "65x24" else (2, 2))
    assert rows.shape == ((rref.row_len(ns, ni),) if shape == "65x24" else (T, rref.row_len(ns, ni), B))
    x, z0, gy = draw(B, T, ns, ni, 0)
    if T == 1:
        # one step: dL/dz0[s] = gy (cy[s] + fy Da ca[s]), and with the diodes off (Da -> 1) the two terms of a state the probe
        # does not see directly cancel -- a row of ONE entry is then a zero of the tree, not a number to hold a kernel to.  The
        # project's rule for such data (tests/ss_asym_cases.py): the first draw whose reference terms keep
        # |sum| >= 0.03 sum |terms|.  On the reference alone.
        k = next((k for k in range(64) if np.all(one_step_balance(rows, ns, ni, ref_root, *draw(B, T, ns, ni, k)) >= cases.BALANCE)), None)
        assert k is not None, f"{root} {shape}: none of 64 draws keeps the two terms of every dL/dz0 entry from cancelling"
        print(f"{root} {shape}: draw {k}")
        x, z0, gy = draw(B, T, ns, ni, k)
    y_ref, zT_ref = rref.run(rows, x, ns, ni, ref_root, z0)
    g_ref = rref.grad_z0(rows, x, ns, ni, ref_root, z0, gy)
    kw = dict(root_kind=kind, rootp=None if rootp is None else cuda(rootp), n_up=n_up, n_down=n_down)
    xd, rd, zd, gd = cuda(x), cuda(rows), cuda(z0), cuda(gy)
    y, zs, zT = wb.ss_dyn_fwd(xd, rd, ns, ni, z0=zd, want_zT=True, **kw)
    _, _, gz0 = wb.ss_dyn_bwd(xd, rd, ns, ni, zs, gd, want_gz0=True, **kw)
    assert tuple(y.shape) == (T, B) and tuple(zT.shape) == (ns, B) and tuple(gz0.shape) == (ns, B) and tuple(zs.shape) == (T, ns, B)
    assert torch.equal(zs[0], zd)                                      # the stash holds the state every step STARTS from
    scale = np.max(np.abs(g_ref), axis=1, keepdims=True)
    dy, dz = float(np.max(np.abs(y.cpu().numpy() - y_ref))), float(np.max(np.abs(zT.cpu().numpy() - zT_ref)))
    dg = np.max(np.abs(gz0.cpu().numpy() - g_ref) / scale, axis=1)
    print(f"{root} {shape}: max |y - ref| = {dy:.3g}, max |zT - ref| = {dz:.3g}; gz0 per state row (of the row's largest) "
          f"{np.array2string(dg, precision=3)}")
    assert np.all(scale > 0.0) and dy <= Y_REF and dz <= Y_REF and np.all(dg <= G_REF)
    # the chunked entry points against the sequential ones
    y3, zs3, zT3, st = wb.ss_dyn_fwd_tp(xd, rd, ns, ni, 3, 8, 1.0e-6, z0=zd, want_zT=True, **kw)
    _, _, gz3 = wb.ss_dyn_bwd_tp(xd, rd, ns, ni, zs, gd, 3, want_gz0=True, **kw)
    dy, dz = float((y3 - y).abs().max()), float((zT3 - zT).abs().max())
    dg = ((gz3 - gz0).abs().amax(dim=1) / gz0.abs().amax(dim=1)).cpu().numpy()
    ds = float((zs3 - zs).abs().max())
    print(f"{root} {shape}: {wb.dyn_chunks(T, 3)} chunks against sequential: verdict {wb.ss_tp_status(st)}; max |dy| = {dy:.3g}, "
          f"max |dzT| = {dz:.3g}, max |dstash| = {ds:.3g}; gz0 per state row {np.array2string(dg, precision=3)}")
    assert wb.dyn_chunks(T, 3) == (1 if T == 1 else 3)
    assert dy <= Y_PATH and dz <= Y_PATH and ds <= Y_PATH and np.all(dg <= G_PATH)


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_binding_refuses_arrays_the_kernels_would_read_out_of_bounds(wdf):
    """z0 that is not [ns,B], zstash that is not [T,ns,B], gy that is not [T,B], rootp shorter than the root kind reads: every
    streamed entry point raises from the binding's own check (its message), so no such call reaches the C ABI or a kernel."""
    from wdf_hip import binding as wb
    B, T, ns, ni = 6, 16, 2, 1
    n = wb.lib().wdf_ss_dyn_row_len(ns, ni)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    x, rows, zs, gy = z(B, T, ni), z(n), z(T, ns, B), z(T, B)
    asym, pair = dict(root_kind=wb.ROOT_ASYM_PAIR), dict(root_kind=wb.ROOT_DIODE_PAIR)
    p4, p2 = z(4) + 1.0, z(2) + 1.0
    fwds = [lambda **kw: wb.ss_dyn_fwd(x, rows, ns, ni, **kw), lambda **kw: wb.ss_dyn_fwd_tp(x, rows, ns, ni, 2, 8, **kw)]
    bwds = [lambda zs_, gy_, **kw: wb.ss_dyn_bwd(x, rows, ns, ni, zs_, gy_, **kw),
            lambda zs_, gy_, **kw: wb.ss_dyn_bwd_tp(x, rows, ns, ni, zs_, gy_, 2, **kw)]
    for f in fwds:
        for bad in (z(ns + 1, B), z(ns, B + 1), z(ns, B - 1), z(ns * B), z(B, ns), z(1, ns, B)):
            with pytest.raises(wb.WdfHipError, match=r"z0 must be \[ns,B\]"):
                f(z0=bad, rootp=p4, **asym)
        for bad, kw in ((z(1) + 1.0, pair), (p2, asym), (z(3) + 1.0, asym), (z(1) + 1.0, asym)):
            with pytest.raises(wb.WdfHipError, match="rootp must hold"):
                f(rootp=bad, **kw)
    for f in bwds:
        for bad in (z(T - 1, ns, B), z(T, ns + 1, B), z(T, ns, B + 1), z(T, ns - 1, B), z(T * ns * B), z(ns, T, B)):
            with pytest.raises(wb.WdfHipError, match=r"zstash must be \[T,ns,B\]"):
                f(bad, gy, rootp=p4, **asym)
        with pytest.raises(wb.WdfHipError, match=r"zstash must be \[T,ns,B\]"):
            f(None, gy, rootp=p4, **asym)
        for bad in (z(B, T), z(T - 1, B), z(T, B + 1), z(T * B), z(T, B, 1)):
            with pytest.raises(wb.WdfHipError, match=r"gy must be \[T,B\]"):
                f(zs, bad, rootp=p4, **asym)
        for bad, kw in ((z(1) + 1.0, pair), (p2, asym), (z(3) + 1.0, asym)):
            with pytest.raises(wb.WdfHipError, match="rootp must hold"):
                f(zs, gy, rootp=bad, **kw)
