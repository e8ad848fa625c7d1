"""GPU: the MLP-root clipper's loss-only evaluation pass at kernel level (mlp_root.MlpEvalPass -> wdf_clipper_mlp_eval,
csrc/wdf_mlp_eval.h) against tests/mlp_step_ref.py (M.run(..., grad=False): the float64 CPU restatement, itself held against the
oracle in tests/test_mlp_step_ref_cpu.py).

  A  every instantiation (width x depth x activation, a pot that moves inside the sequence; four static-R cases), storing y and
     not: three calls at fixed weights -- cold, then two from the pass's OWN snapshots (a call commits itself)
  B  against the training step's forward, cold on the same plan: y within the verification tolerance, printed whether bit for bit;
     the sums of a pass that stores y and of one that does not, bit for bit
  C  the two repair launches, with the recipe of tests/test_gpu_mlp_step_edges.py part C -- the re-run of a flagged chunk is held
     against the snapshot rows here (the step holds it against its stash): a wrong row shows in y after these calls
  D  shape edges: ragged and exact columns, T of one to five blocks, the skip mask, the smallest and a clamped plan
  E  nothing else is written: the training step's state block, gw, zstash, kappa, the weights, loss3; y when it is not asked for

Bounds, the project's own (tests/test_gpu_mlp_step_edges.py): y 1e-5 absolute; the three loss values, S and E 2e-4 relative; 4e-6
(the chunk verification's tolerance) where two fp32 runs of the forward are compared with each other.  Every case prints the
observed error beside the bound and the reference's own fp32 floor, as a DIGEST line (profiles/mlp_eval_pass_digest_tests.txt)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import mlp_step_ref as M
import test_gpu_mlp_step_edges as ED      # noqa: E402  (its networks, cases and helpers; nothing of it runs here)

FS, C = ED.FS, ED.C
B_Y, B_L, B_TWO_RUNS = 1e-5, 2e-4, 4e-6
cuda, network, warm_starts = ED.cuda, ED.network, ED.warm_starts
_REF = {}


def reference(key, x, R, w, H, NL, act, tg, skip):
    """(the fp64 reference, its fp32 floors) -- computed once per key, shared, never modified"""
    if key not in _REF:
        w = np.asarray(w, dtype=np.float32)
        ref = M.run(x, R, w, H, NL, act, tg, skip, grad=False)
        f32 = M.run(x, R, w, H, NL, act, tg, skip, dtype=torch.float32, grad=False)
        fl = {"y": float(np.max(np.abs(f32.y - ref.y))),
              "loss": max(abs(f32.mse - ref.mse) / ref.mse, abs(f32.esr - ref.esr) / ref.esr, abs(f32.loss - ref.loss) / ref.loss),
              "sums": max(abs(f32.S - ref.S) / ref.S, abs(f32.E - ref.E) / ref.E)}
        ref.y.setflags(write=False)
        _REF[key] = (ref, fl)
    return _REF[key]


def measure(ev, ref, store):
    """y (when stored), S, E and the three loss values of the pass's last call against the reference, and the controller's words"""
    torch.cuda.synchronize()
    info, wc = ev.read()
    e_y = float(np.max(np.abs(ev.y.cpu().numpy().astype(np.float64) - ref.y))) if store else float("nan")
    l3 = ev.loss3.cpu().numpy().astype(np.float64)
    e_l = max(abs(l3[0] - ref.mse) / ref.mse, abs(l3[1] - ref.esr) / ref.esr, abs(l3[2] - ref.loss) / ref.loss)
    sm = ev.sums.cpu().numpy()
    e_s = max(abs(sm[0] - ref.S) / ref.S, abs(sm[1] - ref.E) / ref.E)
    return dict(y=e_y, loss=e_l, sums=e_s, finite=bool(np.all(np.isfinite(l3))), info=info, wc=wc)


def digest(tag, ms, fl, ev):
    """ONE line per case: the largest error over the case's calls beside the floor and the bound; per call the controller's words"""
    worst = {k: max(m[k] for m in ms) if not any(np.isnan(m[k]) for m in ms) else float("nan") for k in ("y", "loss", "sums")}
    print(f"DIGEST {tag}: y {worst['y']:.2e} (floor {fl['y']:.1e}, bound {B_Y:.0e})  loss {worst['loss']:.2e} (floor {fl['loss']:.1e}, bound "
          f"{B_L:.0e})  S,E {worst['sums']:.2e} (floor {fl['sums']:.1e}, bound {B_L:.0e})  per call: calls {[m['info']['calls'] for m in ms]} "
          f"n_bad {[m['info']['n_bad'] for m in ms]} flagged {[m['info']['flagged_columns'] for m in ms]} sequential "
          f"{[m['info']['sequential_columns'] for m in ms]} max_miss {['%.1e' % m['info']['max_miss'] for m in ms]} W after "
          f"{[m['wc'].tolist() for m in ms]} items {ev.n_items}")


def check(m, tag, store):
    assert m["finite"] and m["loss"] <= B_L and m["sums"] <= B_L, tag
    if store:
        assert m["y"] <= B_Y, tag


def compare(ev, ref, fl, tag, store):
    """one call: measured, printed, then held against the bounds -> the controller's words"""
    m = measure(ev, ref, store)
    digest(tag, [m], fl, ev)
    check(m, tag, store)
    return m["info"], m["wc"]


def make_pass(x, r, tg, w, H, NL, act, skip, R_static=None, **kw):
    from wdf_hip import mlp_root
    return mlp_root.MlpEvalPass(cuda(x), None if r is None else cuda(r), cuda(tg), w, H, NL, FS, C, R_static=R_static, skip=skip,
                                activation=act, **kw)


SENTINEL = -7.25


def run_three_calls(tag, key, x, r, tg, w, H, NL, act, skip, n_items, store, R_static=None, want_items=None, want_warm=False):
    """cold, then twice from the pass's own snapshots: the same weights, so the same reference."""
    ref, fl = reference(key, x, r if r is not None else R_static, w, H, NL, act, tg, skip)
    ev = make_pass(x, r, tg, cuda(w), H, NL, act, skip, R_static=R_static, n_items=n_items)
    if want_items is not None:
        assert ev.n_items == want_items, ev.items
    if not store:
        ev.y.fill_(SENTINEL)
    ms, starts = [], []
    for call in range(3):
        _, wc = ev.read()
        starts.append(warm_starts(ev, wc))
        ev.run(store_output=store)
        ms.append(measure(ev, ref, store))
    tag = f"{tag} {'y' if store else 'no y'}"
    digest(tag, ms, fl, ev)                                      # (printed before anything is asserted)
    for call, m in enumerate(ms):
        check(m, f"{tag} call {call}", store)
        info = m["info"]
        assert info["calls"] == call + 1 and info["have_snap"] == 1 and info["sequential_columns"] == 0, info
        if want_warm and call > 0:
            # (otherwise every chunk would have run from t = 0 and the verification compared a state with itself)
            assert any(t > 0 for t in starts[call]), (ev.items, m["wc"])
    assert ms[2]["info"]["n_bad"] == 0, ms[2]["info"]
    if not store:
        assert bool((ev.y == SENTINEL).all())
    return ev


# ---------------------------------------------------------------------------------------------- A: every instantiation
@pytest.mark.parametrize("store", [True, False], ids=["y", "no-y"])
@pytest.mark.parametrize("H,NL,act,dyn", ED.A_CASES)
def test_every_instantiation(H, NL, act, dyn, store):
    S = M.A_SHAPE
    x = M.sweeps(S["B"], S["T"])
    tg = M.targets(x)
    r = M.varying_pot(S["B"], S["T"]) if dyn else None
    run_three_calls(f"A {H}x{NL} {act} {'pot[B,T]' if dyn else 'static R'}", ("A", H, NL, act, dyn), x, r, tg, network(H, NL, act), H, NL,
                    act, S["skip"], S["n_items"], store, R_static=None if dyn else M.A_STATIC_R, want_items=6, want_warm=True)


# ---------------------------------------------------------------------------------------------- B: against the step, cold
@pytest.mark.parametrize("H,NL,act,dyn", [(16, 3, "tanh", True), (8, 5, "tanh", True), (4, 4, "relu", False), (16, 5, "relu", True)])
def test_cold_pass_against_the_steps_forward(H, NL, act, dyn):
    from wdf_hip import mlp_root
    S = M.A_SHAPE
    x = M.sweeps(S["B"], S["T"])
    tg = M.targets(x)
    r = M.varying_pot(S["B"], S["T"]) if dyn else None
    w = cuda(network(H, NL, act))
    st = ED.make_step(x, r, tg, w, H, NL, act, S["skip"], R_static=None if dyn else M.A_STATIC_R, adam=None, n_items=S["n_items"],
                      wgrad_chunks=S["wgrad_chunks"])
    ev = mlp_root.MlpEvalPass.of(st)
    ev2 = mlp_root.MlpEvalPass.of(st)
    assert np.array_equal(ev.items, st.items) and ev.cold == st.cold and ev.y is st.y and ev.p is st.p and ev.w is st.w
    st._call(mlp_root.PHASE_FWD | mlp_root.PHASE_SUMS, None)     # cold: every later chunk from z = 0, cold16 units of warm-up
    torch.cuda.synchronize()
    y_step, sums_step = st.y.clone(), st.sums.clone()
    st.y.fill_(SENTINEL)
    ev.run()                                                      # cold too: the same starts
    torch.cuda.synchronize()
    y_pass, sums_pass = st.y.clone(), ev.sums.clone()
    st.y.fill_(SENTINEL)
    ev2.run(store_output=False)
    torch.cuda.synchronize()
    e_y = float((y_pass - y_step).abs().max())
    e_s = float(((sums_pass - sums_step).abs() / sums_step.abs()).max())
    print(f"DIGEST B {H}x{NL} {act} {'pot[B,T]' if dyn else 'static R'}: |y_pass - y_step| {e_y:.2e} (bound {B_TWO_RUNS:.0e}), bit-identical y "
          f"{torch.equal(y_pass, y_step)}; sums rel {e_s:.2e} (bound {B_L:.0e}), bit-identical sums {torch.equal(sums_pass, sums_step)}; "
          f"with / without y bit-identical sums {torch.equal(ev2.sums, sums_pass)}")
    assert e_y <= B_TWO_RUNS and e_s <= B_L
    assert torch.equal(ev2.sums, sums_pass) and torch.equal(ev2.loss3, ev.loss3)      # STORE_Y removes a store and nothing else
    assert bool((st.y == SENTINEL).all())
    assert st.read()[0]["calls"] == 0 and st.read()[0]["have_snap"] == 0               # (FWD | SUMS commits nothing: the parent's route)
    assert ev.read()[0]["calls"] == 1 and ev.read()[0]["have_snap"] == 1


# ---------------------------------------------------------------------------------------------- C: the repair launches
@pytest.mark.parametrize("case", sorted(ED.C_CASES))
def test_repair_paths_run_and_leave_the_state_in_order(case):
    cs = ED.C_CASES[case]
    H, NL, act, T, skip = 16, 3, "tanh", 256, 37
    ncol = len(cs["pots"])
    B = 16 * ncol
    x = np.concatenate([M.sweeps(16, T) for _ in cs["pots"]])                 # (every column the same 16 sweeps)
    tg = M.targets(x)
    r = M.constant_pot(B, T, np.repeat(cs["pots"], 16))
    w0 = network(H, NL, act)
    w1 = (w0 + ED.C_PUSH * np.random.default_rng(5).standard_normal(w0.size)).astype(np.float32)
    n_seq = sum(cs["sequential"])
    w = cuda(w0)
    ev = make_pass(x, r, tg, w, H, NL, act, skip, n_items=cs["n_items"])
    assert ev.n_items == cs["n_items"]
    lens = [int(t1 - t0) for _, _, t0, t1 in ev.items.tolist()]
    print(f"DIGEST C {case}: chunk lengths {lens}")
    _, w_adequate = ev.read()
    # ---- cold, one unit of warm-up from z = 0
    ev.set_controller(cold16=1)
    ref, fl = reference(("C", case, 0), x, r, w0, H, NL, act, tg, skip)
    ev.run()
    info, _ = compare(ev, ref, fl, f"C {case}: cold, 16-step warm-up", True)
    assert info["n_bad"] > 0 and info["flagged_columns"] == ncol and info["sequential_columns"] == n_seq, info
    assert info["total_sequential"] == n_seq
    # ---- from the snapshots of the OLD weights, one unit of warm-up, the controller frozen
    ev.set_wcol(np.ones(ncol, dtype=np.int32))
    ev.freeze(True)
    w.copy_(cuda(w1))
    ref, fl = reference(("C", case, 1), x, r, w1, H, NL, act, tg, skip)
    ev.run()
    info, wc = compare(ev, ref, fl, f"C {case}: from snapshots, 16-step warm-up, weights pushed", True)
    assert np.all(wc == 1)
    assert info["n_bad"] > 0 and info["flagged_columns"] == ncol and info["sequential_columns"] == n_seq, info
    assert info["total_sequential"] == 2 * n_seq
    # ---- the call after: the planned warm-ups again, controller live -- flags, tickets and snapshots were left in order
    ev.freeze(False)
    ev.set_wcol(w_adequate)
    ev.run()
    info, _ = compare(ev, ref, fl, f"C {case}: the call after, planned warm-up", True)
    assert info["n_bad"] == 0 and info["flagged_columns"] == 0 and info["sequential_columns"] == 0, info
    assert info["calls"] == 3 and info["total_sequential"] == 2 * n_seq


# ---------------------------------------------------------------------------------------------- D: shape edges
D_BASE = dict(B=17, T=128, skip=5, n_items=5)
D_ROWS = ([("B", dict(B=b)) for b in (1, 15, 16, 17, 33)] +
          [("T", dict(T=t)) for t in (16, 32, 48, 80)] +
          [("skip", dict(skip=s)) for s in (0, 16, 50, 127)] +
          # the smallest plan (one chunk per column); a request above ncol * kmax (T = 128: kmax = 3, two columns): the plan is smaller
          [("n_items", dict(n_items=2, want_items=2)), ("n_items", dict(n_items=100, want_items=6))])


@pytest.mark.parametrize("H,NL", ED.B_NETS)
@pytest.mark.parametrize("name,change", D_ROWS, ids=[f"{n}-{'-'.join(f'{k}{v}' for k, v in c.items())}" for n, c in D_ROWS])
def test_shape_edges(H, NL, name, change):
    p = dict(D_BASE, **change)
    want_items = p.pop("want_items", None)
    B, T = p["B"], p["T"]
    x = M.sweeps(B, T)
    r = M.varying_pot(B, T)
    run_three_calls(f"D {H}x{NL} {name} {change}", ("D", H, NL, B, T, p["skip"]), x, r, M.targets(x), network(H, NL, "tanh"), H, NL, "tanh",
                    p["skip"], p["n_items"], True, want_items=want_items)


# ---------------------------------------------------------------------------------------------- E: nothing else is written
def test_nothing_of_the_training_step_is_written():
    from wdf_hip import mlp_root
    H, NL, act = 16, 3, "tanh"
    S = M.A_SHAPE
    x = M.sweeps(S["B"], S["T"])
    tg, r = M.targets(x), M.varying_pot(S["B"], S["T"])
    st = ED.make_step(x, r, tg, cuda(network(H, NL, act)), H, NL, act, S["skip"], adam=None, n_items=S["n_items"],
                      wgrad_chunks=S["wgrad_chunks"])
    st.step()
    st.step()
    torch.cuda.synchronize()
    ev = mlp_root.MlpEvalPass.of(st)
    for name in ("x", "p", "lr", "theta2", "target", "w", "y"):
        assert getattr(ev, name) is getattr(st, name), name      # shared, not copied
    assert ev.state is not st.state and ev.sums is not st.sums and ev.loss3 is not st.loss3
    kept = {name: getattr(st, name).clone() for name in ("state", "gw", "zstash", "kappa", "w", "loss3", "sums", "gcoef")}
    for store in (True, False, True, False):
        if not store:
            st.y.fill_(SENTINEL)
        ev.run(store_output=store)
        torch.cuda.synchronize()
        for name, was in kept.items():
            assert torch.equal(getattr(st, name), was), (name, store)
        assert bool((st.y == SENTINEL).all()) != store
    info, _ = ev.read()
    assert info["calls"] == 4 and info["have_snap"] == 1 and st.read()[0]["calls"] == 2
