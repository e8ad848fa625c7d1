"""CPU: tests/mlp_step_ref.py -- the fp64 restatement of the resident MLP training step that tests/test_gpu_mlp_step_edges.py
compares the kernels with -- against the oracle (tree interpreter, MLP root, complex-step gradient); its global-sums variant against
the whole batch; its closed-form kappa against autograd; the conditions on the synthetic networks of the GPU module; and the pure
Python planner of the step's work list (mlp_root.plan_step_items) against the rules wdf_clipper_mlp_step_plan validates."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mlp_step_ref as M

B0, T0, SKIP0 = 3, 48, 5


def _small(act):
    H, NL = 8, 3
    x = M.sweeps(B0, T0, seed=7)
    if act == "tanh":
        from wdf_hip import workload
        w, h, nl = workload.reference_mlp_weights("2x8")
        assert (h, nl) == (H, NL)
    else:
        w = M.synthetic_mlp(H, NL, "relu")
    return x, M.targets(x), w, H, NL


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("pot", ["static", "varying"])
def test_reference_against_the_oracle(oracle, act, pot):
    x, tg, w, H, NL = _small(act)
    r = M.varying_pot(B0, T0) if pot == "varying" else M.constant_pot(B0, T0, 8.0e3)
    res = M.run(x, r if pot == "varying" else 8.0e3, w, H, NL, act, tg, SKIP0)
    a = oracle.ACT_TANH if act == "tanh" else oracle.ACT_RELU
    oc = oracle.clipper_mlp_circuit(M.FS, [2] + [H] * NL + [1], [a] * NL + [oracle.ACT_NONE])
    theta = np.concatenate([[45.0e3, M.C_CLIPPER], w.astype(np.float64)])
    xin = np.stack([x.astype(np.float64), r.astype(np.float64)], axis=-1)
    y_o = oracle.tree_fwd(oc, theta, xin)
    e_y = float(np.max(np.abs(res.y - y_o)) / np.max(np.abs(y_o)))
    o, t = y_o[SKIP0:], tg.astype(np.float64)[SKIP0:]
    n = float(B0 * (T0 - SKIP0))
    S, E = np.sum((o - t) ** 2), np.sum(o ** 2) + M.EPS
    esr = np.sqrt(S / E / n)
    gy = np.zeros_like(y_o)
    gy[SKIP0:] = (2.0 / n + 1.0 / (esr * E * n)) * (o - t) - esr / E * o
    g_o = oracle.tree_grad(oc, theta, xin, gy, params=list(range(2, 2 + w.size)))
    e_g = float(np.max(np.abs(res.gw - g_o)) / np.max(np.abs(g_o)))
    print(f"{act} {pot}: y {e_y:.2e}  loss {abs(res.loss - (S / n + esr)):.2e}  gradient {e_g:.2e} of the largest")
    assert e_y <= 1e-12
    assert abs(res.S - S) <= 1e-12 * S and abs(res.E + M.EPS - E) <= 1e-12 * E
    assert abs(res.mse - S / n) <= 1e-12 * S / n and abs(res.esr - esr) <= 1e-12 * esr and abs(res.loss - (S / n + esr)) <= 1e-12 * res.loss
    assert e_g <= 1e-6
    # (every weight takes part; a relu unit that never fires leaves its own weights without a gradient)
    assert np.count_nonzero(res.gw) >= (w.size if act == "tanh" else w.size // 2)


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_kappa_is_the_steps_state_derivative(act):
    x, tg, w, H, NL = _small(act)
    r = M.varying_pot(B0, T0)
    res = M.run(x, r, w, H, NL, act, tg, SKIP0, grad=False)
    z = np.zeros((T0 + 1, B0))
    for t in range(T0):
        z[t + 1] = 2.0 * res.y[t] - z[t]                                      # y = (z' + z)/2
    layers = M.unpack(torch.as_tensor(w.astype(np.float64)), H, NL)
    G1, G2 = 1.0 / r.astype(np.float64), 2.0 * M.C_CLIPPER * M.FS
    for t in (0, 1, 17, T0 - 1):
        zt = torch.tensor(z[t], requires_grad=True)
        p = torch.as_tensor(G1[:, t] / (G1[:, t] + G2))
        lr = torch.as_tensor(np.log(1.0 / (G1[:, t] + G2)))
        bt = -p * (zt - torch.as_tensor(x[:, t].astype(np.float64)))
        zn = bt - M.mlp(layers, zt + bt, lr, act)[0]
        (k,) = torch.autograd.grad(zn.sum(), zt)
        assert np.allclose(zn.detach().numpy(), z[t + 1], rtol=0, atol=1e-13)
        assert np.allclose(k.numpy(), res.kappa[t], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_global_sums_variant_adds_up_to_the_whole_batch(act):
    """Two ranks: each runs its half with the ADDED sums as constants; the two gradients add to the whole batch's, the loss values
    are the whole batch's."""
    H, NL, B, T, skip = 8, 3, 6, 48, 5
    x = M.sweeps(B, T, seed=7)
    tg, r = M.targets(x), M.varying_pot(B, T)
    w = _small(act)[2]
    n = float(B * (T - skip))
    whole = M.run(x, r, w, H, NL, act, tg, skip)
    halves = [M.run(x[s], r[s], w, H, NL, act, tg[:, s], skip, n_global=n, grad=False) for s in (slice(0, 4), slice(4, 6))]
    sums = (halves[0].S + halves[1].S, halves[0].E + halves[1].E)
    assert abs(sums[0] - whole.S) <= 1e-13 * whole.S and abs(sums[1] - whole.E) <= 1e-13 * whole.E
    parts = [M.run(x[s], r[s], w, H, NL, act, tg[:, s], skip, n_global=n, global_sums=sums) for s in (slice(0, 4), slice(4, 6))]
    for pt in parts:
        assert abs(pt.loss - whole.loss) <= 1e-13 * whole.loss and abs(pt.mse - whole.mse) <= 1e-13 * whole.mse
    g = parts[0].gw + parts[1].gw
    assert np.max(np.abs(g - whole.gw)) <= 1e-11 * np.max(np.abs(whole.gw))
    assert np.max(np.abs(parts[0].gw - whole.gw)) > 1e-2 * np.max(np.abs(whole.gw))     # (a half is not the whole)


def test_adam64_is_the_keras_rule():
    rng = np.random.default_rng(0)
    w, lr = rng.standard_normal(5), np.array([1e-3, 2e-3, 1e-4, 5e-4, 1e-3])
    opt = M.Adam64(5, lr, beta_1=0.5)
    w1 = opt.apply(w, np.array([1.0, -2.0, 0.5, 0.0, 1e-9]))
    # step 1: m / (1 - b1) = g, sqrt(v / (1 - b2)) = |g|: the update is lr g / (|g| + eps sqrt(1 - b2)^-1 ...) -- sign(g) lr for |g| >> eps
    assert np.allclose((w - w1)[:3], lr[:3] * np.array([1.0, -1.0, 1.0]), rtol=1e-5)
    assert w1[3] == w[3] and 0.0 < (w - w1)[4] < 0.3 * lr[4]
    w2 = opt.apply(w1, np.zeros(5))
    m, v = 0.5 * 0.5 * 1.0, 0.999 * 0.001 * 1.0
    assert abs((w1 - w2)[0] - lr[0] * np.sqrt(1 - 0.999 ** 2) / (1 - 0.25) * m / (np.sqrt(v) + 1e-7)) <= 1e-17
    assert opt.step == 2


class _Dense:
    def __init__(self, k, b):
        self.kernel, self.bias = k.unsqueeze(0), b.unsqueeze(0)


def _log_r_grid():
    G2 = 2.0 * M.C_CLIPPER * M.FS
    return [float(np.log(1.0 / (1.0 / R + G2))) for R in (5.0e3, 8.0e3, 12.0e3)]


@pytest.mark.parametrize("H,NL,act", sorted(M.SYNTH))
def test_synthetic_networks_are_usable(H, NL, act):
    """The networks the GPU module runs where no committed weights exist: over ITS inputs chunks forget (max |kappa| <= 0.97) and the
    root is not nearly linear (slope range at least 0.2 wide)."""
    from wdf_hip import mlp_root
    S = M.A_SHAPE
    x = M.sweeps(S["B"], S["T"])
    tg, w = M.targets(x), M.synthetic_mlp(H, NL, act)
    pots = [M.varying_pot(S["B"], S["T"])] + ([M.A_STATIC_R] if (H, NL) in ((4, 4), (16, 5)) else [])
    for r in pots:
        res = M.run(x, r, w, H, NL, act, tg, S["skip"], grad=False)
        k = float(np.max(np.abs(res.kappa)))
        print(f"({H}, {NL}, {act}) pot {'static' if np.ndim(r) == 0 else 'varying'}: max |kappa| {k:.3f}, max |y| {np.max(np.abs(res.y)):.2f}")
        assert np.all(np.isfinite(res.y)) and k <= 0.97
    lo, hi = M.slope_range(w, H, NL, act, _log_r_grid(), 3.0)
    if act == "tanh":                                                        # (mlp_root.slope_range evaluates tanh networks)
        dense = [_Dense(k, b) for k, b in M.unpack(torch.as_tensor(w.astype(np.float64)), H, NL)]
        lo_p, hi_p = mlp_root.slope_range(dense, _log_r_grid(), 3.0)
        assert abs(lo - lo_p) <= 1e-12 and abs(hi - hi_p) <= 1e-12
        lo, hi = lo_p, hi_p
    print(f"    slope range [{lo:.3f}, {hi:.3f}]")
    assert hi - lo >= 0.2


def _check_plan(items, T, ncol, n_items):
    """the rules of wdf_clipper_mlp_step_plan (csrc/wdf_capi_mlp_step.hip), plus: never more than n_items"""
    items = np.asarray(items)
    assert items.dtype == np.int32 and items.ndim == 2 and items.shape[1] == 4
    assert ncol <= items.shape[0] <= n_items
    prev_col, expect_t, K = -1, 0, 0
    for i, (col, k, t0, t1) in enumerate(items.tolist()):
        assert 0 <= col < ncol and t0 % 16 == 0 and t1 % 16 == 0 and t0 < t1 <= T, (i, items)
        if col != prev_col:
            assert prev_col < 0 or expect_t == T
            assert col == prev_col + 1 and k == 0 and t0 == 0                   # columns in order, chunk 0 starts at 0
            prev_col, K = col, 0
        else:
            assert k == K and t0 == expect_t                                    # in order, gap-free
        K += 1
        expect_t = t1
    assert prev_col == ncol - 1 and expect_t == T


@pytest.mark.parametrize("T", [16, 32, 48, 64, 80, 128, 256])
def test_plan_step_items_tiles_every_column(T):
    from wdf_hip import mlp_root
    kmax = max(1, (T - 16) // 32)
    for warm in ([32], [16, 64], [32, 48, 16, 640], [64] * 5 + [16]):
        ncol = len(warm)
        for n_items in sorted({ncol, ncol + 1, 2 * ncol, ncol * kmax - 1, ncol * kmax, ncol * kmax + 3, 4 * ncol * kmax}):
            if n_items < ncol:
                continue
            items = mlp_root.plan_step_items(T, warm, n_items)
            _check_plan(items, T, ncol, n_items)
            if n_items >= ncol * kmax:
                assert items.shape[0] == ncol * kmax                            # (a request above the largest plan comes out smaller)
            else:
                assert items.shape[0] == n_items                                # (every wave asked for gets a chunk)
