"""GPU: Circuit.loss -- the weighted loss family of clipper_pot.py:141-165 (mse_loss, esr_loss, esr_with_emph, avg_loss) as one
fused device stage behind the forward of any circuit -- on three circuits at (B, T) = (70, 300), skip 50, weights (1, 1, 1, 1):
the RC low-pass of lpf.py under the ideal source, the diode clipper Parallel(Vs, C) under DiodePair with host-resident
Variables, and the HPF tree of HPFDiodeClipper.h:28-32 under DiodePair.  Built with the helpers of tests/test_gpu_circuit.py;
the targets come from a teacher with moved component values (theta (1 + 0.12 (-1)^k), as tests/ss_asym_step_cases.py does it).

Loss and terms: the float64 reference of tests/test_gpu_loss_terms.py on `circ.last_output`, its bounds.
Component gradients: the same circuit's y = circ(x) followed by the torch composition of the four terms in float64 and
tape.gradient -- the forward and the reverse sweep are the same kernels, only dL/dy's fp32 rounding differs.  That bound
cannot be derived without sum |gy| |dy/dtheta|, so it is measured: the worst relative difference per circuit on one MI355X,
doubled (the reductions are fixed-order: the factor absorbs box-to-box differences in the compiler's fp contraction only), and
never above 1e-4.  Measured and chosen: GRAD_MEASURED, GRAD_BOUND.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_circuit as tgc                         # noqa: E402  (the circuits' builders)
import test_gpu_loss_terms as lt                       # noqa: E402  (the float64 reference and its bounds)

B, T, SKIP = 70, 300, 50
W4 = dict(mse=1.0, esr=1.0, esr_emph=1.0, avg=1.0)
WT = (1.0, 1.0, 1.0, 1.0)
C_EMPH = 0.85
# Worst relative difference of a component gradient, measured on one MI355X.  The gradients leave the sweep's reduction as
# fp32 numbers, so a difference below one fp32 ulp (2^-23 relative) cannot be told from none: the bound is 2 x max(measured,
# 2^-23), far below the 1e-4 it must not exceed.
ULP32 = 2.0 ** -23
GRAD_MEASURED = {"lpf": 6.07e-8, "clipper": 1.13e-7, "hpf": 0.0}
GRAD_BOUND = {k: 2.0 * max(v, ULP32) for k, v in GRAD_MEASURED.items()}
assert all(v <= 1e-4 for v in GRAD_BOUND.values())


@pytest.fixture(scope="module")
def wdf():
    import tf_wdf
    from wdf_hip import binding
    binding.require_gpu()
    return tf_wdf


def build(wdf, case):
    """-> circuit, its trainable Variables"""
    if case == "lpf":
        Vs, R1, C1, I1 = tgc.build_lpf(wdf)
        return wdf.Circuit(I1, Vs, C1), [R1.R, C1.C]
    if case == "clipper":
        from wdf_hip import workload
        Vs, Cap, P1, dp = tgc.build_clipper(wdf, workload.clipper_theta())
        return wdf.Circuit(P1, dp, Cap), [dp.Is, dp.nVt, Vs.R, Cap.C]
    return tgc._hpf_clipper(wdf, None)


_CASES = {}


def case_data(wdf, case):
    """x [B,T] and the teacher's output [T,B] (device float32), made once per case."""
    if case not in _CASES:
        x = tgc.cuda(np.random.default_rng(0).standard_normal((B, T)) * 1.2)
        teacher, tv = build(wdf, case)
        for k, v in enumerate(tv):
            v.assign(float(v) * (1.0 + 0.12 * (-1.0) ** k))
        with torch.no_grad():
            target = teacher(x).as_subclass(torch.Tensor).detach().clone()
        _CASES[case] = (x, target)
    return _CASES[case]


def composed(y, target):
    """The four terms from y [T,B] by torch operations in float64 (the reference's composition of them)."""
    o = y.as_subclass(torch.Tensor)[SKIP:].double()
    terms, _ = lt.four_terms(o, target[SKIP:].double(), float(o.numel()), C_EMPH)
    return sum(terms)


@pytest.mark.parametrize("case", ["lpf", "clipper", "hpf"])
def test_loss_terms_and_component_gradients(wdf, case):
    tf = wdf.tf
    x, target = case_data(wdf, case)
    circ, tv = build(wdf, case)
    with tf.GradientTape() as tape:
        loss = circ.loss(x, target, skip=SKIP, coeff=C_EMPH, **W4)
    grads = np.array([float(g) for g in tape.gradient(loss, tv)])
    ref = lt.reference(circ.last_output.cpu().numpy(), target.cpu().numpy(), SKIP, WT, C_EMPH)
    got = torch.stack([circ.last_loss_terms[k] for k in ("mse", "esr", "esr_emph", "avg")] + [loss.as_subclass(torch.Tensor).detach()])
    for name, g, r in zip(lt.NAMES, got.cpu().numpy().astype(np.float64), ref["terms5"]):
        tol = 5e-7 * abs(r) + float(np.spacing(np.float32(abs(r))))
        print(f"{case} {name}: got {g!r} want {r!r} |diff| {abs(g - r):.3e} tol {tol:.3e}")
        assert abs(g - r) <= tol, (name, g, r)
    assert all(not v.requires_grad and v.is_cuda and v.dim() == 0 for v in circ.last_loss_terms.values())
    with tf.GradientTape() as tape:
        y = circ(x)
        loss2 = composed(y, target)
    grads2 = np.array([float(g) for g in tape.gradient(loss2, tv)])
    rel = np.abs(grads - grads2) / np.abs(grads2)
    print(f"{case}: component gradients {grads} composed {grads2} relative difference {rel} worst {rel.max():.3e}")
    assert np.all(np.isfinite(grads)) and np.all(grads2 != 0.0)
    assert rel.max() <= GRAD_BOUND[case], (rel, GRAD_BOUND[case])


@pytest.mark.parametrize("case", ["lpf", "clipper", "hpf"])
def test_validation_pass_launches_no_gradient_kernel(wdf, case):
    """Under torch.no_grad(): the same bits of loss and terms as with gradients, and no dL/dy launch."""
    from wdf_hip import lowering
    tf = wdf.tf
    x, target = case_data(wdf, case)
    circ, tv = build(wdf, case)
    count = lowering._LossTermsFn.launches
    before = dict(count)
    with tf.GradientTape():
        l1 = circ.loss(x, target, skip=SKIP, coeff=C_EMPH, **W4)
    t1 = {k: float(v) for k, v in circ.last_loss_terms.items()}
    assert count["grad"] == before["grad"] + 1 and count["sums"] == before["sums"] + 1
    with torch.no_grad():
        l0 = circ.loss(x, target, skip=SKIP, coeff=C_EMPH, **W4)
    t0 = {k: float(v) for k, v in circ.last_loss_terms.items()}
    assert count["grad"] == before["grad"] + 1 and count["sums"] == before["sums"] + 2 and count["coef"] == before["coef"] + 2
    assert not l0.requires_grad
    assert float(l0) == float(l1) and t0 == t1
    # nothing requires a gradient: the same
    for v in tv:
        v.requires_grad_(False)
    l2 = circ.loss(x, target, skip=SKIP, coeff=C_EMPH, **W4)
    assert count["grad"] == before["grad"] + 1 and float(l2) == float(l1)


def test_one_adam_step_on_the_hpf_tree_lowers_the_loss(wdf):
    """tape.gradient -> apply_gradients through the whole chain: Adam's first step moves every Variable by its learning rate
    against its gradient's sign; 1 % of each value."""
    tf = wdf.tf
    x, target = case_data(wdf, "hpf")
    circ, tv = build(wdf, "hpf")
    opts = [tf.keras.optimizers.Adam(learning_rate=0.01 * abs(float(v))) for v in tv]
    with tf.GradientTape() as tape:
        l0 = circ.loss(x, target, skip=SKIP, coeff=C_EMPH, **W4)
    grads = tape.gradient(l0, tv)
    for opt, g, v in zip(opts, grads, tv):
        opt.apply_gradients([(g, v)])
    with torch.no_grad():
        l1 = circ.loss(x, target, skip=SKIP, coeff=C_EMPH, **W4)
    print(f"loss {float(l0)} -> {float(l1)}")
    assert float(l1) < float(l0)


def test_circuit_loss_rejects_a_skip_outside_the_sequence(wdf):
    x, target = case_data(wdf, "lpf")
    circ, _ = build(wdf, "lpf")
    with pytest.raises(ValueError, match="skip"):
        circ.loss(x, target, skip=T)
