"""GPU: the one-pass MSE + ESR training step of small trees with a DIODE-PAIR root (wdf_ss_nl_step_esr, csrc/wdf_ss_nl_step.h)
through Circuit.to_device() + the resident tree's step (Circuit._nl_step_tree / Circuit._mse_esr_nl_step; Circuit.mse_esr
itself keeps the composed path until the step is measured faster): HPFDiodeClipper.h:28-32's circuit as tests/test_gpu_ss_nl_step.py
builds it.

Reference: the fp64 oracle.  y = oracle.tree_fwd; S = sum e^2, E = sum y^2, mse = S / n, esr = sqrt(S / (E + eps) / n) over the rows
skip..T-1 in numpy fp64 (eps = np.finfo(float).eps, n = B (T - skip)); gradients = oracle.tree_grad with gy = ga e + gb y formed
from the oracle's own y (ga = 2/n + 1/(esr (E + eps) n), gb = -esr / (E + eps)), zero before skip.

Bounds.  y 3e-6 and gradients 3e-4 relative: test_first_call_against_the_oracle's (tests/test_gpu_ss_nl_step.py) -- the
per-step arithmetic is the same and the loss coefficients are formed in fp64.  S and E 1e-5 relative to the oracle's sums:
tests/test_gpu_asym_esr_step.py's bound for the same two sums.  The three loss terms 1e-5: mse = S / n inherits S's bound, esr =
sqrt(S / E / n) half the sum of the two.  The step reports S (out[0]) and {mse, esr, mse + esr} and does NOT hand out E: the E
compared here is S / (esr^2 n) - eps, so sum y^2 is covered only through the esr term (three roundings to float: 2e-7) and
through the gradient, whose gb = -esr / (E + eps) multiplies the whole Q family.  Training loop, two-state and two-source trees:
the bounds of the MSE step's tests of the same name (y 4e-6, loss 1e-5, gradients 5e-4).  Step against the composed path
(the same resident circuit built with force_generic: device probe, forward, torch's reductions, reverse sweep): loss 1e-6,
gradients 3e-4.

Every test prints its figures before it asserts (run with -s)."""
import functools
import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_ss_nl_step import FS, THETA, cuda, hpf, rel  # noqa: E402

EPS = float(np.finfo(float).eps)
_ORACLE = {}


@pytest.fixture
def wdf():
    import tf_wdf
    return tf_wdf


@pytest.fixture(autouse=True)
def _oracle(oracle):
    _ORACLE["o"] = oracle


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """What this file's circuits cached goes back to the device when the file is done (as tests/test_gpu_asym_esr_step.py
    does: tests/test_gpu_cache_identity.py relies on the caching allocator handing a freed block straight back)."""
    yield
    inputs.cache_clear()
    oracle_fwd.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def hpf_oracle(O, n_up, n_down):
    nodes = [(O.NODE_RESISTOR, -1, -1, 0, -1, -1), (O.NODE_RES_VSOURCE, -1, -1, 1, 0, -1),
             (O.NODE_CAPACITOR, -1, -1, 2, -1, -1), (O.NODE_SERIES, 1, 2, -1, -1, -1), (O.NODE_PARALLEL, 0, 3, -1, -1, -1)]
    return O.Circuit(nodes, top=4, probe=0, n_in=1, root_kind=O.ROOT_DIODE_PAIR, fs=FS, p_is=3, p_nvt=4, n_up=n_up, n_down=n_down)


def esr_terms(y, tgt, skip):
    """fp64: S, E, (mse, esr, mse + esr), (ga, gb) over the rows skip..T-1 of y, tgt [T,B]"""
    o, t = y[skip:].astype(np.float64), tgt[skip:].astype(np.float64)
    S, E, n = float(np.sum((o - t) ** 2)), float(np.sum(o ** 2)), float(o.size)
    mse, esr = S / n, float(np.sqrt(S / (E + EPS) / n))
    return S, E, np.array([mse, esr, mse + esr]), (2.0 / n + 1.0 / (esr * (E + EPS) * n), -esr / (E + EPS))


def oracle_esr(theta, x, tgt, n_up, n_down, skip, y=None):
    """-> y [T,B], S, E, the three loss terms, the gradient w.r.t. {R, Rs, C, Is, nVt}: fp64"""
    O = _ORACLE["o"]
    oc = hpf_oracle(O, n_up, n_down)
    x64 = x.astype(np.float64)
    if y is None:
        y = O.tree_fwd(oc, theta, x64)
    S, E, l3, (ga, gb) = esr_terms(y, tgt, skip)
    gy = ga * (y - tgt.astype(np.float64)) + gb * y
    gy[:skip] = 0.0
    return y, S, E, l3, O.tree_grad(oc, theta, x64, gy)


@functools.lru_cache(maxsize=None)
def inputs(B, T, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T)) * 1.2).astype(np.float32)
    tgt = (0.3 * rng.standard_normal((T, B))).astype(np.float32)
    x.setflags(write=False)
    tgt.setflags(write=False)
    return x, tgt


@functools.lru_cache(maxsize=None)
def oracle_fwd(B, T, seed, n_up, n_down):
    """the oracle's y at THETA: once per input and diode pair, shared by the skips, never modified"""
    O = _ORACLE["o"]
    x, _ = inputs(B, T, seed)
    y = O.tree_fwd(hpf_oracle(O, n_up, n_down), THETA, x.astype(np.float64))
    y.setflags(write=False)
    return y


def entry_of(circ, skip):
    ents = [e for e in circ._tree.cache.values() if e.get("loss") == "mse+esr" and e["skip"] == skip]
    assert len(ents) == 1
    return ents[0]


def esr_step(circ, x, tgt, skip):
    """the one-pass step on the resident tree, under the conditions of Circuit._nl_step_tree"""
    lin = circ._nl_step_tree(x, tgt, skip)
    assert lin is not None and lin is circ._tree
    return circ._mse_esr_nl_step(lin, x, tgt, skip)


def one_call(wdf, circ, params, x, tgt, skip):
    """-> loss (tensor), gradients, y, S, E (read back from S and esr), the three loss terms"""
    tf = wdf.tf
    with tf.GradientTape() as tape:
        loss = esr_step(circ, x, tgt, skip)
    assert getattr(loss, "_wdf_fused", None) is not None        # (the gradient the pass produced rides on the loss)
    grads = tape.gradient(loss, params)
    g = np.array([float(v) for v in grads])
    ent = entry_of(circ, skip)
    l3 = ent["loss3"].detach().cpu().numpy().astype(np.float64)
    S = float(loss._wdf_fused[0][0])
    n = float(ent["B"] * (ent["T"] - skip))
    E = S / (l3[1] ** 2 * n) - EPS
    return loss, g, circ.last_output.detach().cpu().numpy(), S, E, l3


def composed_call(wdf, build, x, tgt, skip):
    """the path Circuit.mse_esr takes: the same resident circuit with force_generic composes the loss from the device probe, the
    forward, torch's reductions and the reverse sweep"""
    tf = wdf.tf
    ref, pr = build()
    ref.force_generic = True
    ref.to_device()
    assert ref._tree is not None and ref._nl_step_tree(x, tgt, skip) is None
    with tf.GradientTape() as tape:
        l0 = ref.mse_esr(x, tgt, skip=skip)
    g0 = np.array([float(v) for v in tape.gradient(l0, pr)])
    assert getattr(l0, "_wdf_fused", None) is None
    return float(l0), g0


@pytest.mark.parametrize("n_up,n_down", [(1, 1), (2, 1)])
@pytest.mark.parametrize("skip", [0, 50, 700])
def test_first_call_against_the_oracle(wdf, skip, n_up, n_down):
    """B = 130: two groups at two sequences per lane, a padded tail; T = 1500: no multiple of 8, a ragged last chunk; skip 50
    inside an 8-step block, 700 in a later chunk; (1, 1) the SYM instantiation, (2, 1) the general one."""
    B, T = 130, 1500
    x, tgt = inputs(B, T, 1630)
    circ, params = hpf(wdf, n_up, n_down)
    circ.to_device()
    loss, g, y, S, E, l3 = one_call(wdf, circ, params, cuda(x), cuda(tgt), skip)
    ent = entry_of(circ, skip)
    yref, Sr, Er, l3r, gref = oracle_esr(THETA, x, tgt, n_up, n_down, skip, y=oracle_fwd(B, T, 1630, n_up, n_down))
    ctl = circ._tree.read_ctl(ent)
    print(f"skip {skip} N {n_up}/{n_down}: chunks {ent['k']}, |y - oracle| {np.max(np.abs(y - yref)):.2e}, S {rel(S, Sr):.2e}, E {rel(E, Er):.2e}, "
          f"loss terms {l3} / {l3r}: {rel(l3, l3r):.2e}, gradients {np.abs(g - gref) / np.abs(gref)} (max {rel(g, gref):.2e}); {ctl}")
    assert ent["k"] >= 4
    assert np.max(np.abs(y - yref)) < 3e-6
    assert rel(S, Sr) < 1e-5 and rel(E, Er) < 1e-5
    assert rel(l3, l3r) < 1e-5 and abs(float(loss) - l3r[2]) < 1e-5 * l3r[2]
    assert rel(g, gref) < 3e-4


def test_against_the_composed_path(wdf):
    B, T, skip = 130, 1500, 50
    x, tgt = inputs(B, T, 1630)
    xd, td = cuda(x), cuda(tgt)
    circ, params = hpf(wdf)
    circ.to_device()
    loss, g, y, _, _, l3 = one_call(wdf, circ, params, xd, td, skip)
    l0, g0 = composed_call(wdf, lambda: hpf(wdf), xd, td, skip)
    print(f"step {float(loss):.7e} / composed {l0:.7e}: {abs(float(loss) - l0) / l0:.2e}; gradients {rel(g, g0):.2e}")
    assert abs(float(loss) - l0) <= 1e-6 * l0
    assert rel(g, g0) < 3e-4
    # the loss carries the gradient the pass produced, and tape.gradient returns it
    fused = getattr(loss, "_wdf_fused", None)
    assert fused is not None
    out, index = fused
    assert sorted(index.values()) == list(range(5))
    assert np.array_equal(g.astype(np.float32), np.array([float(out[1 + index[id(p)]]) for p in params], dtype=np.float32))


def test_skip_semantics(wdf):
    B, T = 130, 1500
    x, tgt = inputs(B, T, 1630)
    xd, td = cuda(x), cuda(tgt)
    circ, params = hpf(wdf)
    circ.to_device()
    ys = {}
    for skip in (0, 50, 700):
        loss, _, ys[skip], _, _, l3 = one_call(wdf, circ, params, xd, td, skip)
        if skip == 0:
            mse0 = float(entry_of(circ, 0)["loss3"][0])
    m = float(circ.mse(xd, td))
    print(f"skip 0: mse term {mse0:.7e}, circ.mse {m:.7e}: {abs(mse0 - m) / m:.2e}; y differs over the skips by "
          f"{max(float(np.max(np.abs(ys[s] - ys[0]))) for s in ys):.1e}")
    assert abs(mse0 - m) <= 1e-6 * m
    assert np.array_equal(ys[0], ys[50]) and np.array_equal(ys[0], ys[700])      # y does not know about skip
    assert len(circ._tree.cache) == 4                                            # three ESR entries and the MSE one: nothing shared


def test_missed_boundaries_are_repaired_sequentially(wdf, monkeypatch):
    """A tolerance no prediction can meet (test_missed_boundaries_are_repaired_sequentially of the MSE step): every group's
    finishing wave runs its sequences again from t = 0, both families of sums and skip included -- against the one-chunk plan,
    which has no boundary."""
    from wdf_hip import binding, lowering
    B, T, skip = 200, 2048, 50
    x, tgt = inputs(B, T, 8)
    xd, td = cuda(x), cuda(tgt)
    circ, params = hpf(wdf)
    circ.to_device()
    one_call(wdf, circ, params, xd, td, skip)
    ent = entry_of(circ, skip)
    assert ent["k"] > 1
    binding._check(binding.lib().wdf_ss_nl_step_set(binding._ptr(ent["ws"]), 8, -1.0, binding._stream()), "set")
    loss, g, y, S, E, l3 = one_call(wdf, circ, params, xd, td, skip)
    ctl = circ._tree.read_ctl(ent)
    monkeypatch.setattr(lowering, "N_SIMD", 1)
    one, p1 = hpf(wdf)
    one.to_device()
    loss1, g1, y1, S1, E1, l31 = one_call(wdf, one, p1, xd, td, skip)
    assert entry_of(one, skip)["k"] == 1
    print(f"{ctl}; vs one chunk: |dy| {np.max(np.abs(y - y1)):.2e}, S {rel(S, S1):.2e}, E {rel(E, E1):.2e}, loss terms {rel(l3, l31):.2e}, "
          f"gradients {rel(g, g1):.2e}")
    assert ctl["gated_groups"] == 2 and ctl["n_bad"] > 0              # 200 sequences, two per lane: two groups
    assert np.max(np.abs(y - y1)) < 3e-6
    assert rel(S, S1) < 1e-5 and rel(E, E1) < 1e-5 and rel(l3, l31) < 1e-5
    assert rel(g, g1) < 3e-4


def test_training_loop_against_the_oracle_every_step(wdf):
    """clipper_pot.py's loss in lpf.py:86-99's loop on the HPF clipper, five optimizers, skip = 50: every step's output, loss and
    gradients against the oracle AT THE PARAMETERS OF THAT STEP; warm calls; the optimizers' updates ride in the next probe."""
    tf = wdf.tf
    B, T, skip = 128, 4096, 50
    x, _ = inputs(B, T, 3)
    ref, _ = hpf(wdf)
    tgt = (ref(cuda(x)) * 0.8).as_subclass(torch.Tensor).detach().cpu().numpy()
    circ, params = hpf(wdf)
    circ.to_device()
    pb = circ._tree.pb
    opts = [tf.keras.optimizers.Adam(learning_rate=1.0e-3 * float(p)) for p in params]
    xd, td = cuda(x), cuda(tgt)
    worst_y = worst_g = worst_l = 0.0
    used, gated = [], 0
    for step in range(12):
        with tf.GradientTape() as tape:
            loss = esr_step(circ, xd, td, skip)
        grads = tape.gradient(loss, params)
        assert len(pb.pending) == 0                                # (the step's probe launch took the queued updates along)
        theta = np.array([float(p) for p in params], dtype=np.float32).astype(np.float64)
        g = np.array([float(v) for v in grads])
        y = circ.last_output.detach().cpu().numpy()
        ent = entry_of(circ, skip)
        ctl = circ._tree.read_ctl(ent)
        used.append(ctl["w_used"])
        gated += ctl["gated_groups"]
        assert ctl["call"] == step + 1 and (step == 0 or ctl["have_snap"] == 1)
        yref, _, _, l3r, gref = oracle_esr(theta, x, tgt, 2, 3, skip)
        worst_y = max(worst_y, float(np.max(np.abs(y - yref))))
        worst_g = max(worst_g, rel(g, gref))
        worst_l = max(worst_l, abs(float(loss) - l3r[2]) / l3r[2])
        for o, gr, p in zip(opts, grads, params):
            o.apply_gradients([(gr, p)])
        # three launches per step: the five updates are queued, not launched -- the next call's probe carries them
        assert len(pb.pending) == 5
    print(f"warm-ups used {used}; groups repaired {gated}; worst |y - oracle| {worst_y:.2e}, loss {worst_l:.2e}, gradients {worst_g:.2e}")
    assert worst_y < 4e-6 and worst_g < 5e-4 and worst_l < 1e-5
    assert used[0] >= 256 and max(used[2:]) <= 128
    assert gated == 0
    pb.flush()


def _two_states(wdf):
    Ra = wdf.Resistor(4.7e3, True)
    Vr = wdf.ResistiveVoltageSource(1.0e3, trainable=True)
    Ca, Cb = wdf.Capacitor(4.7e-8, FS, True), wdf.Capacitor(2.2e-8, FS, True)
    top = wdf.Parallel(wdf.Series(Ra, Ca), wdf.Series(Vr, Cb))
    dp = wdf.DiodePair(top, 2.52e-9, Vt=25.85e-3, nDiodes=1.752, trainable=True)
    return wdf.Circuit(top, dp, Ra), [Ra.R, Vr.R, Ca.C, Cb.C, dp.Is, dp.nVt]


def _two_sources(wdf):
    Va = wdf.ResistiveVoltageSource(1.0e3, trainable=True)
    Vb = wdf.ResistiveVoltageSource(4.7e3, trainable=True)
    Ca = wdf.Capacitor(2.2e-8, FS, True)
    top = wdf.Parallel(wdf.Series(Va, Ca), Vb)
    dp = wdf.DiodePair(top, 2.52e-9, Vt=25.85e-3, nDiodes=1.752, trainable=True)
    return wdf.Circuit(top, dp, Ca), [Va.R, Vb.R, Ca.C, dp.Is, dp.nVt]


@pytest.mark.parametrize("build,shape,B,T,seed", [(_two_states, (2, 1), 96, 3000, 6), (_two_sources, (1, 2), 192, 2048, 16)])
def test_larger_trees_against_the_host_probe_path(wdf, build, shape, B, T, seed):
    """The trees of test_two_state_diode_tree_against_the_host_probe_path (ns = 2) and
    test_one_state_two_sources_diode_tree_against_the_host_probe_path (ni = 2), skip = 50: cold, then twice from the snapshots."""
    skip = 50
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T) + ((2,) if shape[1] == 2 else ())) * 1.2).astype(np.float32)
    tgt = (0.3 * rng.standard_normal((T, B))).astype(np.float32)
    xd, td = cuda(x), cuda(tgt)
    ref, pr = build(wdf)
    assert (ref.ns, ref.ni) == shape
    tf = wdf.tf
    with tf.GradientTape() as tape:
        l0 = ref.mse_esr(xd, td, skip=skip)
    g0 = np.array([float(v) for v in tape.gradient(l0, pr)])
    y0 = ref(xd).as_subclass(torch.Tensor).detach().cpu().numpy()
    circ, p = build(wdf)
    circ.to_device()
    for call in range(3):
        l1, g1, y1, _, _, _ = one_call(wdf, circ, p, xd, td, skip)
        ctl = circ._tree.read_ctl(entry_of(circ, skip))
        e_y = float(np.max(np.abs(y1 - y0)))
        print(f"{shape} call {call}: loss {float(l0):.6e} / {float(l1):.6e}; |y - host path| {e_y:.2e}; gradients {rel(g1, g0):.2e}; {ctl}")
        assert e_y < 4e-6 and abs(float(l1) - float(l0)) < 1e-5 * float(l0) and rel(g1, g0) < 5e-4
