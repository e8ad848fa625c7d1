"""GPU: the input gradient at Circuit level, (B, T) = (70, 300), with the builders of tests/test_gpu_circuit.py: the RC low-pass of
lpf.py under the ideal source, the HPF tree of HPFDiodeClipper.h:28-32 under DiodePair (2 up, 3 down), and the diode clipper
Parallel(Vs, C) under DiodePair with host-resident Variables -- which, for an x that carries a graph, takes the generic
state-space route.  At this shape the planner cuts the reverse sweep in 4 chunks, so every gradient here comes out of the chunked
form of the input-gradient pass.

References: tests/ss_gx_ref.py in float64 on the coefficients `circ.matrices()` gives, rounded to float32 as the kernels get them.
x.grad: within ss_static_ref's caps (G_NL under a root, g_lin(ns + ni + 2) on the linear tree) times the channel's magnitude.
The gain's gradient dL/dg = sum(gx x): the same cap per entry, summed over |x|, plus the float32 tree sum of torch's own backward
of g * x (64 x 2^-24 of sum |gx x|: 21000 addends, a tree of depth 15 and the rounding of its leaves).
The cascade RC low-pass -> transpose -> HPF tree: the first stage's dL/dR and dL/dC against the float64 chain that uses none of
the new code -- ss_gx_ref for the second stage, its gx as the first stage's gy in ss_static_ref.run, matrices()' autograd from
the coefficients to the components.  That bound cannot be derived without the chain's own sums of |addend|, so it is measured on
one MI355X against the chain, doubled (the reductions are fixed-order: the factor absorbs box-to-box differences in the compiler's
fp contraction only), and never above 1e-4: GRAD_MEASURED / GRAD_BOUND, the convention of tests/test_gpu_circuit_loss.py.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ss_gx_ref as G                                  # noqa: E402
import ss_static_ref as R                              # noqa: E402
import test_gpu_circuit as tgc                         # noqa: E402  (the circuits' builders)

B, T = 70, 300
ULP32 = 2.0 ** -23
# Worst relative difference of the first stage's component gradients in the cascade against the float64 chain, measured on one
# MI355X (the test prints it): {dL/dR, dL/dC}.
GRAD_MEASURED = {"R": 0.0, "C": 1.093e-7}
GRAD_BOUND = {k: 2.0 * max(v, ULP32) for k, v in GRAD_MEASURED.items()}
assert all(v <= 1e-4 for v in GRAD_BOUND.values())


@pytest.fixture(scope="module")
def wdf():
    import tf_wdf
    from wdf_hip import binding
    binding.require_gpu()
    return tf_wdf


def build(wdf, case):
    """-> circuit, its trainable Variables, the reference's root name"""
    if case == "lpf":
        Vs, R1, C1, I1 = tgc.build_lpf(wdf)
        return wdf.Circuit(I1, Vs, C1), [R1.R, C1.C], "none"
    if case == "clipper":
        from wdf_hip import workload
        Vs, Cap, P1, dp = tgc.build_clipper(wdf, workload.clipper_theta())
        return wdf.Circuit(P1, dp, Cap), [dp.Is, dp.nVt, Vs.R, Cap.C], "pair11"
    circ, tv = tgc._hpf_clipper(wdf, "auto")
    return circ, tv, "pair23"


def kernel_inputs(circ, root_name):
    """the coefficients and root values the kernels get: matrices() in float64, rounded to float32 -> coef32, ss_static_ref.Root"""
    coef64, r_port = circ.matrices()
    coef32 = coef64.detach().numpy().astype(np.float32)
    if root_name == "none":
        return coef32, R.Root("none")
    dp = circ.root
    p = np.array([float(dp.Is), float(dp.nVt), float(r_port)], dtype=np.float64).astype(np.float32)
    return coef32, R.Root(root_name, p=p)


_X = {}


def x_of(scale=1.2):
    if scale not in _X:
        _X[scale] = tgc.cuda(np.random.default_rng(0).standard_normal((B, T)) * scale)
    return _X[scale]


def gy_for(y):
    """dL/dy of an MSE against a target near y (ss_static_ref.Case's), as a device tensor [T,B]"""
    yn = y.detach().as_subclass(torch.Tensor).cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(1)
    return tgc.cuda((0.2 * yn + 0.1 * max(np.max(np.abs(yn)), 1e-3) * rng.standard_normal(yn.shape)) * (2.0 / yn.size))


def reference(circ, root_name, x, gy):
    """float64 -> Gx (gx, mag [T,ni,B]) and the bound per unit of channel magnitude"""
    coef32, root = kernel_inputs(circ, root_name)
    xn, gyn = x.detach().cpu().numpy(), gy.cpu().numpy()
    res = R.run(circ.ns, circ.ni, coef32, xn, root, gy=gyn)
    g = G.walk(circ.ns, circ.ni, coef32, res, gyn)
    return g, (R.g_lin(circ.ns + circ.ni + 2) if root_name == "none" else R.G_NL), res


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lpf", "hpf", "clipper"])
def test_x_grad_exists_and_matches_the_reference(wdf, case):
    from wdf_hip import lowering
    circ, tv, root_name = build(wdf, case)
    x = x_of().clone().requires_grad_(True)
    before = lowering._StateSpaceFn.launches["gx"]
    y = circ(x).as_subclass(torch.Tensor)
    gy = gy_for(y)
    (y * gy).sum().backward()
    assert x.grad is not None, "the input gradient was dropped"
    assert lowering._StateSpaceFn.launches["gx"] == before + 1
    assert tuple(x.grad.shape) == (B, T) and bool(torch.all(torch.isfinite(x.grad)))
    g, cap, _ = reference(circ, root_name, x, gy)
    err = np.max(np.abs(x.grad.cpu().numpy().astype(np.float64).T - g.gx[:, 0, :]))
    bound = cap * G.channel_mag(g.mag)[0]
    print(f"{case}: max |x.grad - reference| {err:.3e}, bound {bound:.3e} ({err / bound:.3f} of it); max |gx| {np.max(np.abs(g.gx)):.3e}")
    assert err <= bound
    assert np.max(np.abs(g.gx)) > 100.0 * bound                                # (the check can tell a gradient from none)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["lpf", "hpf"])
def test_trainable_input_gain(wdf, case):
    tf = wdf.tf
    circ, tv, root_name = build(wdf, case)
    x = x_of()
    gain = tf.Variable(0.8, trainable=True)
    with tf.GradientTape() as tape:
        xin = gain.as_subclass(torch.Tensor).to(x.device) * x
        y = circ(xin)
        gy = gy_for(y)
        loss = tf.reduce_sum(y * gy)
    dg = tape.gradient(loss, [gain])[0]
    assert dg is not None, "tape.gradient gave the upstream Variable nothing"
    g, cap, _ = reference(circ, root_name, xin, gy)
    xn = x.cpu().numpy().astype(np.float64).T                                  # [T,B]
    terms = g.gx[:, 0, :] * xn
    want = float(terms.sum())
    bound = cap * G.channel_mag(g.mag)[0] * float(np.abs(xn).sum()) + 64.0 * 2.0 ** -24 * float(np.abs(terms).sum())
    print(f"{case}: dL/dg {float(dg)!r} want {want!r} |diff| {abs(float(dg) - want):.3e} bound {bound:.3e}")
    assert abs(float(dg) - want) <= bound
    assert abs(want) > 10.0 * bound


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def cascade(wdf):
    a, tva, _ = build(wdf, "lpf")
    b, tvb, _ = build(wdf, "hpf")
    return a, tva, b, tvb


def run_cascade(a, b, x):
    return b(a(x).as_subclass(torch.Tensor).T)


_TARGET = {}


def cascade_target(wdf):
    if "t" not in _TARGET:
        a, tva, b, tvb = cascade(wdf)
        for k, v in enumerate(tva + tvb):
            v.assign(float(v) * (1.0 + 0.12 * (-1.0) ** k))
        with torch.no_grad():
            _TARGET["t"] = run_cascade(a, b, x_of()).as_subclass(torch.Tensor).detach().clone()
    return _TARGET["t"]


def test_cascade_first_stage_gradients_against_the_float64_chain(wdf):
    tf = wdf.tf
    x, target = x_of(), cascade_target(wdf)
    a, tva, b, tvb = cascade(wdf)
    with tf.GradientTape() as tape:
        y = run_cascade(a, b, x)
        loss = tf.reduce_mean(tf.square(y - target))
    grads = tape.gradient(loss, tva)
    assert all(g is not None for g in grads), "the first stage stands still: tape.gradient gave its Variables nothing"
    got = np.array([float(g) for g in grads])
    # the chain in float64, none of the new code: stage A forward, stage B forward and ss_gx_ref, stage A's sweep with gx as its gy
    coefA, rootA = kernel_inputs(a, "none")
    coefB, rootB = kernel_inputs(b, "pair23")
    xn, tn = x.cpu().numpy(), target.cpu().numpy().astype(np.float64)
    yA = R.run(a.ns, a.ni, coefA, xn, rootA).y                                 # [T,B] float64
    fB = R.run(b.ns, b.ni, coefB, yA.T, rootB)
    gyB = 2.0 * (fB.y - tn) / tn.size
    rB = R.run(b.ns, b.ni, coefB, yA.T, rootB, gy=gyB)
    gxB = G.walk(b.ns, b.ni, coefB, rB, gyB).gx[:, 0, :]                       # [T,B]: dL/d(stage A's y)
    rA = R.run(a.ns, a.ni, coefA, xn, rootA, gy=gxB)
    coef64, _ = a.matrices()
    want = tf.GradientTape().gradient((coef64 * torch.as_tensor(rA.g)).sum(), tva)
    want = np.array([float(w) for w in want])
    rel = np.abs(got - want) / np.abs(want)
    print(f"cascade: first stage dL/d{{R, C}} {got} chain {want} relative difference {rel}")
    assert np.all(np.isfinite(got)) and np.all(want != 0.0)
    assert rel[0] <= GRAD_BOUND["R"] and rel[1] <= GRAD_BOUND["C"], (rel, GRAD_BOUND)


def test_one_adam_step_on_both_stages_lowers_the_loss(wdf):
    tf = wdf.tf
    x, target = x_of(), cascade_target(wdf)
    a, tva, b, tvb = cascade(wdf)
    tv = tva + tvb
    opts = [tf.keras.optimizers.Adam(learning_rate=0.01 * abs(float(v))) for v in tv]
    with tf.GradientTape() as tape:
        l0 = tf.reduce_mean(tf.square(run_cascade(a, b, x) - target))
    grads = tape.gradient(l0, tv)
    assert all(g is not None and float(g) != 0.0 for g in grads)
    for opt, g, v in zip(opts, grads, tv):
        opt.apply_gradients([(g, v)])
    with torch.no_grad():
        l1 = tf.reduce_mean(tf.square(run_cascade(a, b, x) - target))
    print(f"cascade loss {float(l0)} -> {float(l1)}")
    assert float(l1) < float(l0)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
_PLAIN = {}


def plain_run(wdf, case):
    """y and the component gradients of a call with a plain x -> (y bits, gradient bits)"""
    tf = wdf.tf
    circ, tv, _ = build(wdf, case)
    x = x_of()
    y = circ(x)
    gy = tgc.cuda(np.random.default_rng(5).standard_normal((T, B)) / (B * T))
    grads = tf.GradientTape().gradient(tf.reduce_sum(y * gy), tv)
    return (y.as_subclass(torch.Tensor).detach().clone().view(torch.int32),
            torch.stack([g.as_subclass(torch.Tensor).detach().float().reshape(()).cpu() for g in grads]).view(torch.int32))


@pytest.fixture(scope="module", autouse=True)
def plain_first(wdf):
    """the plain-x results taken when this module starts (autouse: set up in front of the module's first test), before any
    input-gradient call of this module -- and of the process, where no module in front of this one makes one"""
    from wdf_hip import lowering
    return {case: plain_run(wdf, case) for case in ("lpf", "hpf")}, lowering._StateSpaceFn.launches["gx"]


@pytest.mark.parametrize("case", ["lpf", "hpf"])
def test_a_plain_input_launches_no_gx_kernel_and_keeps_its_bits(wdf, plain_first, case):
    from wdf_hip import lowering
    first, _ = plain_first
    # an input-gradient call in between
    circ, _, _ = build(wdf, case)
    xg = x_of().clone().requires_grad_(True)
    circ(xg).as_subclass(torch.Tensor).sum().backward()
    assert xg.grad is not None
    before = lowering._StateSpaceFn.launches["gx"]
    y, grads = plain_run(wdf, case)
    assert lowering._StateSpaceFn.launches["gx"] == before, "a plain x launched the input-gradient pass"
    assert bool(torch.equal(y, first[case][0])) and bool(torch.equal(grads, first[case][1]))
    # grad mode off: an x that requires grad is a plain x
    with torch.no_grad():
        y0 = circ(xg)
    assert lowering._StateSpaceFn.launches["gx"] == before and not y0.requires_grad


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def _xg(chans=None):
    shape = (4, 64) if chans is None else (4, 64, chans)
    return (0.3 * torch.ones(shape, dtype=torch.float32, device="cuda")).requires_grad_(True)


def test_refused_routes_name_themselves(wdf, golden):
    from wdf_hip import binding, workload
    tgt = torch.zeros((64, 4), device="cuda")
    # the streamed-coefficient kernels: a resistance channel off the clipper topology
    R1 = wdf.Resistor(33.0e3, True)
    Vs = wdf.ResistiveVoltageSource(1.0e3, trainable=True)
    C = wdf.Capacitor(22.0e-9, tgc.FS, True)
    top = wdf.Parallel(R1, wdf.Series(Vs, C))
    streamed = wdf.Circuit(top, wdf.DiodePair(top, 4.352e-9, Vt=0.0493, trainable=True), R1, per_sample_R=Vs)
    with pytest.raises(binding.WdfHipError, match="streamed-coefficient"):
        streamed(_xg(2))
    # the MLP root on the clipper topology
    from layers import DenseRootModel
    from test_gpu_ss_dyn import _net
    js, _, _ = _net(golden, "2x8")
    Vs, Cap, P1, _ = tgc.build_clipper(wdf, workload.clipper_theta())
    mlp = wdf.Circuit(P1, DenseRootModel(js), Cap, per_sample_R=Vs)
    with pytest.raises(binding.WdfHipError, match="MLP root|streamed-coefficient|per_sample_R"):
        mlp(_xg(2))
    Vs, Cap, P1, _ = tgc.build_clipper(wdf, workload.clipper_theta())
    mlp_static = wdf.Circuit(P1, DenseRootModel(js), Cap)
    with pytest.raises(binding.WdfHipError, match="MLP root"):
        mlp_static(_xg())
    # two different diodes on the clipper's own kernels, with and without a pot per sequence
    Vs, Cap, P1, _ = tgc.build_clipper(wdf, workload.clipper_theta())
    asym = wdf.Circuit(P1, wdf.AsymDiodePair(P1, 2.52e-9, 2.0e-6, trainable=True), Cap)
    for call in (lambda: asym(_xg()), lambda: asym.mse(_xg(), tgt), lambda: asym.mse_esr(_xg(), tgt), lambda: asym.loss(_xg(), tgt)):
        with pytest.raises(binding.WdfHipError, match="two-different-diode clipper's own kernels"):
            call()
    seq = wdf.Circuit(P1, wdf.AsymDiodePair(P1, 2.52e-9, 2.0e-6, trainable=True), Cap, per_sequence_R=Vs)
    with pytest.raises(binding.WdfHipError, match="per_sequence_R"):
        seq(_xg(2))
    # the resident diode-pair clipper
    Vs, Cap, P1, dp = tgc.build_clipper(wdf, workload.clipper_theta())
    res = wdf.Circuit(P1, dp, Cap).to_device()
    for call in (lambda: res(_xg()), lambda: res.mse(_xg(), tgt)):
        with pytest.raises(binding.WdfHipError, match="resident diode-pair clipper"):
            call()
    # and what is served says nothing: a resident tree through the device probe
    circ, tv, _ = build(wdf, "hpf")
    circ.to_device()
    xg = _xg()
    circ(xg).as_subclass(torch.Tensor).sum().backward()
    assert xg.grad is not None and bool(torch.any(xg.grad != 0))
