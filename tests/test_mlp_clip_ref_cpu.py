"""CPU: tests/mlp_clip_ref.py, the float64 reference of the MLP-root clipper kernels, is right, and the inputs of
tests/test_gpu_mlp_clip_kernels.py are fit to judge a kernel by.

The reference is pinned from four independent sides: tests/mlp_step_ref.py (another restatement, its own autograd through the loss),
the C oracle (ROOT_MLP, complex-step derivatives) for static {R, C}, a central difference in C under per-sample R, and autograd
through the recursion for the closed forms (kappa, gb, a) and for the sweep at a held stash.  Then the conditions on EVERY case of
the one list (mlp_clip_ref.CASES) that make the GPU comparisons mean something: the circuit forgets, no tanh layer lives in
saturation, and no quantity is so cancelling that the float32 floor comes within a quarter of the bound the GPU file applies.
"""
import numpy as np
import pytest

import mlp_clip_ref as R
import mlp_step_ref as M

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _trained():
    from wdf_hip import workload
    R.set_trained_loader(workload.reference_mlp_weights)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def pick(H, NL, B, T, dyn, z0=False):
    seed, scale = R.SYNTH[(H, NL)]
    return R.Case("AB", H, NL, B, T, dyn, z0, seed, scale, None, "varying")


@pytest.mark.parametrize("H,NL", R.ARCHS)
@pytest.mark.parametrize("dyn", [False, True])
def test_agrees_with_the_step_reference(H, NL, dyn):
    """z0 = 0 and gy = d(MSE + ESR)/dy: y, kappa and the weight gradient are mlp_step_ref.run's to 1e-12."""
    c = pick(H, NL, 9, 70, dyn)
    i = R.inputs(c)
    tgt, skip = M.targets(i.x), 11
    step = M.run(i.x, i.R, i.w, H, NL, "tanh", tgt, skip, C=R.C_CLIPPER, fs=R.FS)
    gy = step.ga * (step.y - tgt.astype(np.float64)) + step.gb * step.y
    gy[:skip] = 0.0
    mine = R.run(i.x, i.R, i.w, H, NL, gy)
    e = {"y": rel(mine.y, step.y), "kappa": rel(mine.kappa, step.kappa), "gw": rel(mine.gw, step.gw)}
    print(f"{R.case_id(c)}: {e}")
    assert max(e.values()) <= 1e-12, e


@pytest.mark.parametrize("H,NL", [(8, 3), (4, 4), (8, 5)])
def test_static_resistance_against_the_oracle(oracle, H, NL):
    """Static R: y, dL/dR and dL/dC against oracle.tree_fwd / tree_grad under ROOT_MLP (the circuit of
    tests/test_gpu_mlp_root.py::test_static_resistance_and_capacitor_gradient), one network of each depth.  The oracle differentiates
    by complex step: no cancellation, so the two agree to rounding (1e-9 relative asserted)."""
    O = oracle
    c = pick(H, NL, 5, 60, False)
    i = R.inputs(c)
    sizes, acts = [2] + [H] * NL + [1], [O.ACT_TANH] * NL + [O.ACT_NONE]
    nodes = [(O.NODE_RES_VSOURCE, -1, -1, 0, 0, -1), (O.NODE_CAPACITOR, -1, -1, 1, -1, -1), (O.NODE_PARALLEL, 0, 1, -1, -1, -1)]
    oc = O.Circuit(nodes, top=2, probe=1, n_in=1, root_kind=O.ROOT_MLP, fs=R.FS, mlp_off=2, mlp_sizes=sizes, mlp_act=acts)
    theta = np.concatenate([[R.R_STATIC, R.C_CLIPPER], i.w.astype(np.float64)])
    x64, gy64 = i.x.astype(np.float64), i.gy.astype(np.float64)
    mine = R.run(i.x, i.R, i.w, H, NL, i.gy)
    y_ref = O.tree_fwd(oc, theta, x64)
    g_ref = O.tree_grad(oc, theta, x64, gy64, params=[0, 1])
    e = {"y": rel(mine.y, y_ref), "dR": abs(mine.gR - g_ref[0]) / abs(g_ref[0]), "dC": abs(mine.gC - g_ref[1]) / abs(g_ref[1])}
    print(f"{R.case_id(c)}: {e}  dR {mine.gR:.6e} dC {mine.gC:.6e}")
    assert max(e.values()) <= 1e-9, e


@pytest.mark.parametrize("H,NL", [(16, 3), (4, 4), (4, 5)])
def test_capacitor_gradient_under_a_moving_pot_against_a_central_difference(H, NL):
    """Per-sample R (where the oracle test above does not go): dL/dC against a central difference of the float64 reference in C, at
    the step where h and h/2 differ least.  Truncation h^2 and rounding 1e-16/h meet near a relative step of 1e-5 with an error
    around 1e-10; 1e-7 relative is asserted."""
    c = pick(H, NL, 5, 60, True, z0=True)
    i = R.inputs(c)
    gy64 = i.gy.astype(np.float64)

    def L(C):
        return float(np.sum(gy64 * R.forward(i.x, i.R, i.w, H, NL, z0=i.z0, C=C).y))

    def cd(h):
        return (L(R.C_CLIPPER + h) - L(R.C_CLIPPER - h)) / (2.0 * h)

    hs = [R.C_CLIPPER * 10.0 ** -k for k in (2, 3, 4, 5, 6, 7)]
    pairs = [(abs(cd(h) - cd(0.5 * h)), h) for h in hs]
    _, h = min(pairs)
    fd = cd(0.5 * h)
    mine = R.run(i.x, i.R, i.w, H, NL, i.gy, z0=i.z0)
    assert mine.gR is None
    e = abs(mine.gC - fd) / abs(fd)
    print(f"{R.case_id(c)}: step {h / R.C_CLIPPER:.0e} C (|cd(h) - cd(h/2)| {min(pairs)[0] / abs(fd):.1e} relative)  dC {mine.gC:.9e}  "
          f"central difference {fd:.9e}  relative error {e:.1e}")
    assert e <= 1e-7


@pytest.mark.parametrize("H,NL", R.ARCHS)
@pytest.mark.parametrize("dyn", [False, True])
def test_closed_forms_agree_with_autograd_through_the_recursion(H, NL, dyn):
    """kappa, gb (the adjoint recurrence written out), a, and the gradients of the sweep at a held stash, against autograd through
    the whole recursion from a non-zero z0: 1e-12."""
    c = pick(H, NL, 6, 40, dyn, z0=True)
    i = R.inputs(c)
    mine = R.run(i.x, i.R, i.w, H, NL, i.gy, z0=i.z0)
    ad = R.recursion_autograd(i.x, i.R, i.w, H, NL, i.gy, z0=i.z0)
    e = {"y": rel(mine.y, ad.y), "a": rel(mine.a, ad.a), "kappa": rel(mine.kappa, ad.kappa), "gb": rel(mine.gb, ad.gb),
         "gw": rel(mine.gw, ad.gw), "dC": abs(mine.gC - ad.gC) / abs(ad.gC)}
    if not dyn:
        e["dR"] = abs(mine.gR - ad.gR) / abs(ad.gR)
    # the identity behind `a`:  a = z + z' + MLP(a, lr)  (z' = b_temp - MLP, a = z + b_temp), with the network evaluated again
    zn = np.concatenate([mine.zstash[1:], mine.zT[None, :]])
    m = R.mlp_out(i.w, H, NL, mine.a.reshape(-1), mine.lr.reshape(-1)).reshape(mine.a.shape)
    e["a identity"] = rel(mine.zstash + zn + m, mine.a)
    print(f"{R.case_id(c)}: {e}")
    assert max(e.values()) <= 1e-12, e


def test_warmup_from_kappa():
    k = np.full((64, 2), 0.5)
    k[:, 1] = 0.25
    # 0.5^W < 2.5e-7  <=>  W >= 22
    assert R.warmup_from_kappa(k, 1e-6) == 32
    assert R.warmup_from_kappa(np.full((64, 1), 0.999), 1e-6) is None
    assert R.warmup_from_kappa(np.full((64, 1), 0.3), 1e-6) == 16


GROUPS = sorted({(c.sec, c.H, c.NL, c.net) for c in R.CASES}, key=str)


@pytest.mark.parametrize("sec,H,NL,net", GROUPS)
def test_every_case_is_fit_to_judge_a_kernel_by(sec, H, NL, net):
    """On every case the GPU file runs: max |kappa| < 1; no tanh layer saturated (|tanh| > 0.995) on more than 10 % of its (step,
    unit) pairs; the float32 mode of the reference within a QUARTER of every bound the GPU file applies to a kernel there -- y, stash
    and zT of the forward, and gw, dL/dC, dL/dR of the sweep at the float32-rounded stash (what sections B and C feed the kernels) and
    of the sweep at the float32 forward's own stash (C's stored-kappa path)."""
    worst = {}
    for c in R.CASES:
        if (c.sec, c.H, c.NL, c.net) != (sec, H, NL, net):
            continue
        r, r32 = R.ref(c), R.ref32(c)
        # (the committed trained networks carry units that sit in saturation on every sample, 2 of 16 and 1 of 8 in layer 0 -- constants
        # that no choice of input moves; for them the condition is asserted on the units that do move, and the whole figure printed)
        f = {"kappa": float(np.max(np.abs(r.kappa))), "sat": max(r.sat if net is None else r.sat_live)}
        scale = R.Y_BOUND * max(1.0, float(np.max(np.abs(r.zstash)))) + (2.0 * R.TP_TOL if sec == "Dt" else 0.0)
        f["y"] = max(np.max(np.abs(r32.y - r.y)), np.max(np.abs(r32.zstash - r.zstash)), np.max(np.abs(r32.zT - r.zT))) / scale
        if sec in ("AB", "C"):
            s64, s32 = R.sweep_at_stash32(c), R.sweep_at_stash32(c, torch.float32)
            for name, a32, a64 in (("held", s32, s64), ("own", r32, r)):
                f[f"gw {name}"] = R.grad_ratio(a32.gw, a64.gw)
                f[f"dC {name}"] = R.grad_ratio([a32.gC], [a64.gC])
                if not c.dyn:
                    f[f"dR {name}"] = R.grad_ratio([a32.gR], [a64.gR])
        if sec == "D":
            W = R.warmup_from_kappa(r.kappa, 1e-6)
            assert W is not None and W + 16 < c.T, (R.case_id(c), W)       # the warm-up is a real one: a chunk can start later than it
        print(f"{R.case_id(c)}: " + "  ".join(f"{k} {v:.3f}" for k, v in f.items()) + ("" if net is None else f"  sat, all units {max(r.sat):.3f}"))
        assert f["kappa"] < 1.0, (R.case_id(c), f)
        assert f["sat"] <= 0.10, (R.case_id(c), f)
        for k, v in f.items():
            if k not in ("kappa", "sat"):
                assert v < 0.25, (R.case_id(c), k, v)
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"worst of {sec} {NL - 1}x{H} {net or ''}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert worst
