"""GPU: the resident training step of the MLP-root pot clipper (csrc/wdf_mlp_step.h, wdf_clipper_mlp_step) where
tests/test_gpu_mlp_step.py never ran it -- every template instantiation (width x depth x activation x static / per-sample pot), a
pot that changes from one sample to the next, the shape edges (ragged and exact columns, single-chunk columns, the skip mask, plan
and reverse-sweep chunkings), the two repair launches with the counters that show they ran, two ranks with really different sums,
and Adam in the last launch -- all against tests/mlp_step_ref.py (one step restated in torch float64 on the CPU, itself held against
the oracle in tests/test_mlp_step_ref_cpu.py), on EVERY weight's gradient.

Bounds (measured against the oracle in tests/test_gpu_mlp_step.py): y and kappa 1e-5; the three loss values 2e-4 relative; the
gradient 2e-4 |g| + 2e-5 max |g| (tanh), 2e-3 |g| + 2e-4 max |g| (relu: a kink crossed by fp32 rounding moves a sample's gradient).
Each case also runs the reference in float32 on the CPU and prints that fp32 floor beside the observed error: a bound could rise to
4 x the floor where the floor demanded it, never to anything taken from the kernels' own error -- on an MI355X no case came within a
factor 2 of a bound (worst: y 3.6e-6, kappa 6.6e-6, losses 1.9e-6, gradient 0.39 of its bound), so the bounds stand as they are.
Every case prints a DIGEST line (profiles/mlp_step_edges_digest.txt)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mlp_step_ref as M

FS, C = M.FS, 4.7e-9


def cuda(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def network(H, NL, act):
    if act == "tanh" and (H, NL) in M.COMMITTED:
        from wdf_hip import workload
        w, h, nl = workload.reference_mlp_weights(M.COMMITTED[(H, NL)])
        assert (h, nl) == (H, NL)
        return w.astype(np.float32)
    return M.synthetic_mlp(H, NL, act)


def reference(x, r, w, H, NL, act, tg, skip, **kw):
    """(the fp64 reference, its fp32 floors: the same restatement in float32 against itself in float64)"""
    w = np.asarray(w, dtype=np.float32)
    ref = M.run(x, r, w, H, NL, act, tg, skip, **kw)
    f32 = M.run(x, r, w, H, NL, act, tg, skip, dtype=torch.float32, **kw)
    rel, ab = grad_bound(act)
    fl = {"y": float(np.max(np.abs(f32.y - ref.y))), "kappa": float(np.max(np.abs(f32.kappa - ref.kappa))),
          "loss": max(abs(f32.mse - ref.mse) / ref.mse, abs(f32.esr - ref.esr) / ref.esr, abs(f32.loss - ref.loss) / ref.loss),
          "g": float(np.max(np.abs(f32.gw - ref.gw) / (rel * np.abs(ref.gw) + ab * np.max(np.abs(ref.gw)))))}
    return ref, fl


def grad_bound(act):
    return (2e-4, 2e-5) if act == "tanh" else (2e-3, 2e-4)


def compare(st, ref, fl, act, tag):
    """y, kappa, the three loss values and the WHOLE gradient of the step's last call against the reference."""
    torch.cuda.synchronize()
    info, wc = st.read()
    e_y = float(np.max(np.abs(st.y.cpu().numpy().astype(np.float64) - ref.y)))
    e_k = float(np.max(np.abs(st.kappa.cpu().numpy().astype(np.float64) - ref.kappa)))
    l3 = st.loss3.cpu().numpy().astype(np.float64)
    e_l = max(abs(l3[0] - ref.mse) / ref.mse, abs(l3[1] - ref.esr) / ref.esr, abs(l3[2] - ref.loss) / ref.loss)
    got, want = st.gw.cpu().numpy().astype(np.float64), ref.gw
    rel, ab = grad_bound(act)
    assert got.shape == want.shape
    e_g = float(np.max(np.abs(got - want) / (rel * np.abs(want) + ab * np.max(np.abs(want)))))
    b_y, b_k, b_l, b_g = 1e-5, 1e-5, 2e-4, 1.0
    print(f"DIGEST {tag}: y {e_y:.2e} (floor {fl['y']:.1e}, bound {b_y:.0e})  kappa {e_k:.2e} (floor {fl['kappa']:.1e}, bound {b_k:.0e})  "
          f"loss {e_l:.2e} (floor {fl['loss']:.1e}, bound {b_l:.0e})  grad/bound {e_g:.3f} (floor {fl['g']:.3f})  "
          f"n_bad {info['n_bad']} flagged {info['flagged_columns']} sequential {info['sequential_columns']} "
          f"max_miss {info['max_miss']:.1e} W {wc.tolist()} items {st.n_items}")
    assert np.all(np.isfinite(got)) and e_y <= b_y and e_k <= b_k and e_l <= b_l and e_g <= b_g, tag
    return info, wc


def make_step(x, r, tg, w, H, NL, act, skip, R_static=None, **kw):
    from wdf_hip import mlp_root
    return mlp_root.MlpTrainStep(cuda(x), None if r is None else cuda(r), cuda(tg), w, H, NL, FS, C, R_static=R_static, skip=skip,
                                 activation=act, **kw)


def warm_starts(st, wc):
    """first step of every later chunk's warm-up in a call from the snapshots with the warm-ups wc (units of 16 steps)"""
    return [int(t0) - 16 * int(wc[col]) for col, k, t0, _ in st.items.tolist() if k > 0]


def run_three_calls(tag, x, r, tg, w, H, NL, act, skip, n_items, wgrad_chunks, R_static=None, want_items=None, want_warm=False):
    """cold, then twice from the snapshots: the same weights, so the same reference."""
    ref, fl = reference(x, r if r is not None else R_static, w, H, NL, act, tg, skip)
    st = make_step(x, r, tg, cuda(w), H, NL, act, skip, R_static=R_static, adam=None, n_items=n_items, wgrad_chunks=wgrad_chunks)
    if want_items is not None:
        assert st.n_items == want_items, st.items
    for call in range(3):
        _, wc = st.read()
        starts = warm_starts(st, wc)
        st.step()
        info, _ = compare(st, ref, fl, act, f"{tag} call {call}")
        assert info["calls"] == call + 1 and info["sequential_columns"] == 0, info
        if want_warm and call > 0:
            # (otherwise every chunk would have run from t = 0 and the verification compared a state with itself)
            assert any(t > 0 for t in starts), (st.items, wc)
    return st


# ---------------------------------------------------------------------------------------------- A: every instantiation
A_CASES = [(H, NL, act, True) for H, NL, act in M.A_ARCHS] + [(4, 4, "tanh", False), (4, 4, "relu", False),
                                                                (16, 5, "tanh", False), (16, 5, "relu", False)]


@pytest.mark.parametrize("H,NL,act,dyn", A_CASES)
def test_every_instantiation_with_a_pot_that_moves_inside_the_sequence(H, NL, act, dyn):
    S = M.A_SHAPE
    x = M.sweeps(S["B"], S["T"])
    tg = M.targets(x)
    r = M.varying_pot(S["B"], S["T"]) if dyn else None
    if dyn:
        assert 5.0e3 <= r.min() and r.max() <= 12.0e3 and np.all(r[:, 1:] != r[:, :-1])
    run_three_calls(f"A {H}x{NL} {act} {'pot[B,T]' if dyn else 'static R'}", x, r, tg, network(H, NL, act), H, NL, act, S["skip"],
                    S["n_items"], S["wgrad_chunks"], R_static=None if dyn else M.A_STATIC_R, want_items=6, want_warm=True)


# ---------------------------------------------------------------------------------------------- B: shape edges
B_NETS = [(16, 3), (8, 5)]                                                   # 2x16_pre, 4x8
B_BASE = dict(B=17, T=128, skip=5, n_items=5, wgrad_chunks=2)
B_ROWS = ([("B", dict(B=b)) for b in (1, 15, 16, 17, 33)] +
          [("T", dict(T=t)) for t in (16, 32, 48, 80)] +
          [("skip", dict(skip=s)) for s in (0, 16, 50, 127)] +
          # the smallest plan (one chunk per column); a request above ncol * kmax (T = 128: kmax = 3, two columns): the plan is smaller
          [("n_items", dict(n_items=2, want_items=2)), ("n_items", dict(n_items=100, want_items=6))] +
          [("wgrad_chunks", dict(wgrad_chunks=1)), ("wgrad_chunks", dict(T=80, wgrad_chunks=3)),      # (80: chunks of 32, 32, 16)
           ("wgrad_chunks", dict(wgrad_chunks=8)), ("wgrad_chunks", dict(wgrad_chunks=1000))] +
          # reverse-sweep waves per launch, n_cols * Kw: 3 x 3 = 9 = 1 (mod 4): three waves of the last workgroup idle; 2 x 2 = 4
          [("parts", dict(B=33, T=96, wgrad_chunks=3, parts=9)), ("parts", dict(B=17, wgrad_chunks=2, parts=4))])


@pytest.mark.parametrize("H,NL", B_NETS)
@pytest.mark.parametrize("name,change", B_ROWS, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in c.items())}" for n, c in B_ROWS])
def test_shape_edges(H, NL, name, change):
    from wdf_hip import binding as wb
    p = dict(B_BASE, **change)
    want_items, parts = p.pop("want_items", None), p.pop("parts", None)
    B, T = p["B"], p["T"]
    if parts is not None:
        assert ((B + 15) // 16) * wb.chunk_geom(T, p["wgrad_chunks"], 16)[1] == parts
    x = M.sweeps(B, T)
    r = M.varying_pot(B, T)
    assert r.max() <= 12.0e3
    run_three_calls(f"B {H}x{NL} {name} {change}", x, r, M.targets(x), network(H, NL, "tanh"), H, NL, "tanh", p["skip"], p["n_items"],
                    p["wgrad_chunks"], want_items=want_items)


# ---------------------------------------------------------------------------------------------- C: the repair launches
# |1 - 2p| per step with the diode off: 0.64 at 10 kOhm (a 16-step warm-up misses by ~0.64^16 = 8e-4 of what it started off by: flagged
# at tol = 4e-6, and a re-run meets the old trajectory within a few steps), 0.956 at 99.1 kOhm (a 16-step warm-up keeps half of what
# it was off by, and a re-run chunk of 16..64 steps does not meet the old trajectory before its end: the successor is flagged too and
# the column goes sequential).  The cold call starts its chunks off by the whole state (z = 0).  The call from the snapshots starts
# them off by what a push of the weights moves the trajectory: C_PUSH = 3e-4 x N(0, 1) on every weight, from the fp64 reference's two
# trajectories and its kappa (linearised, at the planned boundaries): 10 kOhm: arrival misses 1.3e-5 .. 3e-4, 1e-11 32 steps on;
# 99.1 kOhm: arrival misses 2e-2 .. 2e-1, still 1e-4 .. 4e-3 32 steps on.  (A larger push makes this network another system -- its
# state saturates, everything is forgotten in a few steps and nothing is flagged at 99.1 kOhm; a smaller one is not flagged at 10.)
C_PUSH = 3.0e-4
C_CASES = {
    "flagged chunks re-run": dict(pots=[10.0e3], n_items=4, sequential=[0]),
    "column goes sequential": dict(pots=[99.1e3], n_items=6, sequential=[1]),
    "one of two columns goes sequential": dict(pots=[10.0e3, 99.1e3], n_items=10, sequential=[0, 1]),
}


@pytest.mark.parametrize("case", sorted(C_CASES))
def test_repair_paths_run_and_leave_the_state_in_order(case):
    cs = C_CASES[case]
    H, NL, act, T, skip = 16, 3, "tanh", 256, 37
    ncol = len(cs["pots"])
    B = 16 * ncol
    x = np.concatenate([M.sweeps(16, T) for _ in cs["pots"]])                 # (every column the same 16 sweeps)
    tg = M.targets(x)
    r = M.constant_pot(B, T, np.repeat(cs["pots"], 16))
    w0 = network(H, NL, act)
    w1 = (w0 + C_PUSH * np.random.default_rng(5).standard_normal(w0.size)).astype(np.float32)
    n_seq = sum(cs["sequential"])
    w = cuda(w0)
    st = make_step(x, r, tg, w, H, NL, act, skip, adam=None, n_items=cs["n_items"], wgrad_chunks=4)
    assert st.n_items == cs["n_items"]
    lens = [int(t1 - t0) for _, _, t0, t1 in st.items.tolist()]
    print(f"DIGEST C {case}: chunk lengths {lens}")
    _, w_adequate = st.read()
    # ---- cold, one unit of warm-up from z = 0
    st.set_controller(cold16=1)
    ref, fl = reference(x, r, w0, H, NL, act, tg, skip)
    st.step()
    info, _ = compare(st, ref, fl, act, f"C {case}: cold, 16-step warm-up")
    assert info["n_bad"] > 0 and info["flagged_columns"] == ncol and info["sequential_columns"] == n_seq, info
    assert info["total_sequential"] == n_seq
    # ---- from the snapshots of the OLD weights, one unit of warm-up, the controller frozen
    st.set_wcol(np.ones(ncol, dtype=np.int32))
    st.freeze(True)
    w.copy_(cuda(w1))
    ref, fl = reference(x, r, w1, H, NL, act, tg, skip)
    st.step()
    info, wc = compare(st, ref, fl, act, f"C {case}: from snapshots, 16-step warm-up, weights pushed")
    assert np.all(wc == 1)
    assert info["n_bad"] > 0 and info["flagged_columns"] == ncol and info["sequential_columns"] == n_seq, info
    assert info["total_sequential"] == 2 * n_seq
    # ---- the call after: the planned warm-ups again, controller live -- flags, tickets and snapshots were left in order
    st.freeze(False)
    st.set_wcol(w_adequate)
    st.step()
    info, _ = compare(st, ref, fl, act, f"C {case}: the call after, planned warm-up")
    assert info["n_bad"] == 0 and info["flagged_columns"] == 0 and info["sequential_columns"] == 0, info
    assert info["calls"] == 3 and info["total_sequential"] == 2 * n_seq


# ---------------------------------------------------------------------------------------------- D: two ranks on one device
def test_two_ranks_with_different_sums():
    from wdf_hip import mlp_root
    H, NL, act = 16, 3, "tanh"
    S = M.A_SHAPE
    B, T, skip = S["B"], S["T"], S["skip"]
    x = M.sweeps(B, T)
    tg, r, w = M.targets(x), M.varying_pot(B, T), network(H, NL, act)
    n = float(B * (T - skip))
    whole, fl_w = reference(x, r, w, H, NL, act, tg, skip)
    halves = [slice(0, 16), slice(16, B)]
    own = [M.run(x[s], r[s], w, H, NL, act, tg[:, s], skip, n_global=n, grad=False) for s in halves]
    sums64 = (own[0].S + own[1].S, own[0].E + own[1].E)
    ranks = [make_step(x[s], r[s], tg[:, s], cuda(w), H, NL, act, skip, adam=None, n_global=n, n_items=3, wgrad_chunks=3) for s in halves]
    for call in range(2):                                                    # cold, then from the snapshots
        for st in ranks:
            st._call(mlp_root.PHASE_FWD | mlp_root.PHASE_SUMS, None)
        total = ranks[0].sums + ranks[1].sums                                # the all-reduce
        assert float((ranks[0].sums - ranks[1].sums).abs().min()) > 0.1 * float(total.min())     # (really different)
        for st in ranks:
            st.sums.copy_(total)
            st._call(mlp_root.PHASE_BWD | mlp_root.PHASE_GLOBAL_SUMS, None)
        torch.cuda.synchronize()
        assert abs(float(total[0]) - sums64[0]) <= 2e-4 * sums64[0] and abs(float(total[1]) - sums64[1]) <= 2e-4 * sums64[1]
        for st, s, tag in zip(ranks, halves, ("rank 0 (16 sequences)", "rank 1 (5 sequences)")):
            part, fl = reference(x[s], r[s], w, H, NL, act, tg[:, s], skip, n_global=n, global_sums=sums64)
            assert abs(part.loss - whole.loss) <= 1e-12 * whole.loss
            compare(st, part, fl, act, f"D {tag} call {call}")               # its y, its share of the gradient, the GLOBAL loss values
        rel, ab = grad_bound(act)
        g = (ranks[0].gw.double() + ranks[1].gw.double()).cpu().numpy()
        e_g = float(np.max(np.abs(g - whole.gw) / (rel * np.abs(whole.gw) + ab * np.max(np.abs(whole.gw)))))
        print(f"DIGEST D sum of the two ranks' gradients against the whole batch, call {call}: grad/bound {e_g:.3f} (floor {fl_w['g']:.3f})")
        assert e_g <= 1.0


# ---------------------------------------------------------------------------------------------- E: Adam in the last launch
@pytest.mark.parametrize("H,NL", [(4, 3), (16, 5)])                          # 57 weights: less than one block; 1153: 19 blocks, the last partial
def test_adam_inside_the_reduce_launch(H, NL):
    """Five steps; after each the reference's float64 Adam is fed the step's own gradient and the weights the step started from.
    The kernel's update differs from it by the fp32 rounding of w (2^-24 |w| = 6e-8 |w|) and of the update itself (a few 1e-7 of
    lr_t m / (sqrt(v) + eps) <= ~1e-3): 2e-7 |w| + 1e-9."""
    from wdf_hip import binding as wb
    act = "tanh"
    S = M.A_SHAPE
    B, T, skip = S["B"], S["T"], S["skip"]
    x = M.sweeps(B, T)
    tg, r, w0 = M.targets(x), M.varying_pot(B, T), network(H, NL, act)
    count = M.weight_count(H, NL)
    assert count == {(4, 3): 57, (16, 5): 1153}[(H, NL)] and w0.size == count
    lr = (1.0e-4 * (1.0 + (np.arange(count) % 4))).astype(np.float32)        # per-parameter learning rates
    w = cuda(w0)
    adam = wb.Adam(count, lr=lr, beta_1=0.5, device="cuda")
    st = make_step(x, r, tg, w, H, NL, act, skip, adam=adam, n_items=S["n_items"], wgrad_chunks=S["wgrad_chunks"])
    opt = M.Adam64(count, lr.astype(np.float64), beta_1=0.5, beta_2=adam.b2, epsilon=adam.eps)
    for call in range(5):
        w_before = w.cpu().numpy().copy()
        ref, fl = reference(x, r, w_before, H, NL, act, tg, skip)
        st.step()
        compare(st, ref, fl, act, f"E {H}x{NL} step {call + 1}")
        w_ref = opt.apply(w_before.astype(np.float64), st.gw.cpu().numpy().astype(np.float64))
        w_got = w.cpu().numpy().astype(np.float64)
        e_w = float(np.max(np.abs(w_got - w_ref) / (2e-7 * np.abs(w_ref) + 1e-9)))
        moved = float(np.max(np.abs(w_got - w_before)))
        print(f"DIGEST E {H}x{NL} step {call + 1}: |w - Adam64(w, gw)| / (2e-7 |w| + 1e-9) {e_w:.3f}; largest move {moved:.2e}")
        assert e_w <= 1.0 and moved >= 0.5e-4
        assert int(adam.step) == call + 1 == opt.step
