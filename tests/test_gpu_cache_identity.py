"""GPU: the per-tensor caches of the Python layer (which kernel variant runs, which resident copy the kernels read) answer for
THIS call's data when a training loop builds every batch anew.

PyTorch's caching allocator hands a freed block of the same size straight back, and a fresh tensor starts at version 0: a
batch built with `torch.from_numpy(batch).to(dev)` then has the address, shape, strides and version of the batch before it.
Every test below is a short loop of calls; every call is held against the fp64 oracle on its own data.  Where a test relies on
the allocator reusing an address, it first checks that the reuse happened (or that a cache still holds the earlier tensor,
which is what keeps the address from being reused), so it cannot pass for the wrong reason.

Tolerances as in the files these paths come from: the one-pass step y 2e-6 V / gradients 1e-4 relative
(test_gpu_fused_step.py); circuits y 3e-6 V / gradients 3e-4 relative (test_gpu_circuit.py, test_gpu_ss_dyn.py).
"""
import gc
import weakref

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FS = 48000.0
Y_TOL, G_RTOL = 2.0e-6, 1.0e-4


@pytest.fixture(scope="module")
def wb():
    from wdf_hip import binding
    binding.require_gpu()
    return binding


@pytest.fixture
def wdf():
    import tf_wdf
    from wdf_hip import binding
    binding.require_gpu()
    return tf_wdf


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def key(t):
    from wdf_hip import lowering
    with torch._C.DisableTorchFunctionSubclass():
        return lowering.tensor_key(t)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def moving_pot(B, T, seed):
    """a pot that moves inside every sequence, within the clip range: a jump to another grid value at a point of its own,
    then a ramp"""
    from wdf_hip import workload
    rng = np.random.default_rng(seed)
    r = workload.dataset_resistance_batch(B, T).astype(np.float64)
    at = rng.integers(T // 8, T // 2, B)
    other = rng.choice([10.0e3, 25.2e3, 75.0e3, 99.1e3], B)
    t = np.arange(T)[None, :]
    r = np.where(t < at[:, None], r, other[:, None])
    return (r * (1.0 + 0.2 * t / T)).astype(np.float32)


def esr_grad_and_loss(y64, t64, skip):
    """dL/dy [T,B] and L of the scripts' loss MSE + ESR past skip (clipper_pot.py:146-156,177)"""
    o, t = y64[skip:], t64[skip:]
    n, eps = o.size, float(np.finfo(float).eps)
    S, E = float(np.sum((o - t) ** 2)), float(np.sum(o * o)) + eps
    mse, esr = S / n, float(np.sqrt(S / E / n))
    gy = np.zeros_like(y64)
    gy[skip:] = (2.0 / n + (1.0 / (esr * E * n) if esr > 0 else 0.0)) * (o - t) - esr / E * o
    return gy, mse + esr


# ---------------------------------------------------------------- a. the one-pass step, r built fresh every batch
@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("n_up,n_down", [(1, 1), (1, 2)])
def test_one_pass_step_with_a_fresh_resistance_channel_every_batch(wb, oracle, time_major, n_up, n_down):
    """Batch 0: one pot value per sequence (the per-sequence fast path).  Batch 1: the pot moves inside every sequence, its
    channel built fresh at batch 0's address.  Batch 2: one value per sequence again.  MSE and MSE + ESR steps, y and the
    gradient against the oracle on each batch's own channel, and the verify status clean."""
    from wdf_hip import workload
    B, T, K, W, skip = 200, 2048, 8, 448, 50
    x = workload.sweep_batch(B, T, seed=17)
    th = workload.clipper_theta()
    th64 = th.astype(np.float32).astype(np.float64)
    x64 = x.astype(np.float64)
    tgt64 = oracle.clipper_fwd(workload.target_theta(), FS, x64, r=workload.dataset_resistance_batch(B, T).astype(np.float64))
    # every device buffer of the loop made up front: the only block freed and asked for again is the channel's
    xin = cuda(x.T) if time_major else cuda(x)
    thd, tgt = cuda(th), cuda(tgt64)
    Kr = wb.lib().wdf_clipper_tp_chunks(T, K)
    ws = wb.step_mse_workspace(B, Kr, xin.device)
    y = torch.empty((T, B), dtype=torch.float32, device="cuda")
    status = torch.empty((4,), dtype=torch.int32, device="cuda")
    g = torch.empty((4,), dtype=torch.float32, device="cuda")
    sse = torch.empty((1,), dtype=torch.float32, device="cuda")
    sums10 = torch.empty((10,), dtype=torch.float32, device="cuda")
    loss3 = torch.empty((3,), dtype=torch.float32, device="cuda")
    channels = [workload.dataset_resistance_batch(B, T), moving_pot(B, T, 3 + n_down), workload.dataset_resistance_batch(B, T)[::-1]]
    first_key, per_seq, r = None, [], None
    for i, r_host in enumerate(channels):
        r = None                                                          # the previous batch's channel goes back to the allocator
        r = torch.from_numpy(np.ascontiguousarray(r_host.T if time_major else r_host)).to("cuda")
        if first_key is None:
            first_key = key(r)
        else:
            assert key(r) == first_key, "the allocator did not hand the freed channel's block back: no collision to test"
        per_seq.append(wb.r_is_per_sequence(r, time_major))
        r64 = np.ascontiguousarray(r_host, dtype=np.float64)
        y64 = oracle.clipper_fwd(th64, FS, x64, r=r64, n_up=n_up, n_down=n_down)
        # MSE
        wb.clipper_step_mse_tp(xin, thd, FS, tgt, 2.0 / (B * T), K, W, r=r, n_up=n_up, n_down=n_down, y=y, ws=ws, status=status,
                               gtheta=g, sse=sse, time_major=time_major)
        assert wb.tp_status(status)["n_bad"] == 0
        e_y = float(np.max(np.abs(y.cpu().numpy() - y64)))
        _, g64 = oracle.clipper_fwd_bwd(th64, FS, x64, 2.0 * (y64 - tgt64) / (B * T), r=r64, n_up=n_up, n_down=n_down)
        got = g.cpu().numpy().astype(np.float64)
        print(f"batch {i} ({'per sequence' if per_seq[-1] else 'moving'}): MSE step max|y - oracle| {e_y:.2e}, "
              f"grad {rel(got[[0, 1, 3]], g64[[0, 1, 3]]):.2e}")
        assert e_y <= Y_TOL, (i, e_y)
        assert all(abs(got[j] - g64[j]) <= G_RTOL * abs(g64[j]) for j in (0, 1, 3)), (i, got, g64)
        # MSE + ESR past skip
        wb.clipper_step_esr_tp(xin, thd, FS, tgt, float(B * (T - skip)), float(np.finfo(float).eps), skip, K, W, r=r, n_up=n_up,
                               n_down=n_down, y=y, ws=ws, status=status, sums10=sums10, gtheta=g, loss3=loss3, time_major=time_major)
        assert wb.tp_status(status)["n_bad"] == 0
        e_y = float(np.max(np.abs(y.cpu().numpy() - y64)))
        gy, L = esr_grad_and_loss(y64, tgt64, skip)
        _, g64 = oracle.clipper_fwd_bwd(th64, FS, x64, gy, r=r64, n_up=n_up, n_down=n_down)
        got = g.cpu().numpy().astype(np.float64)
        assert e_y <= Y_TOL, (i, e_y)
        assert abs(float(loss3[2]) - L) <= 1e-5 * L
        assert all(abs(got[j] - g64[j]) <= G_RTOL * abs(g64[j]) for j in (0, 1, 3)), (i, got, g64)
    assert per_seq == [True, False, True]


def test_one_pass_step_flag_under_stream_capture(wb):
    """A channel first seen while a graph is captured: r_is_per_sequence answers False (the per-sample path is exact for any
    channel) without synchronising, and caches nothing -- outside the capture the same tensor is looked at properly."""
    r = torch.full((64, 256), 2.5e4, device="cuda")
    g = torch.cuda.CUDAGraph()
    a = torch.zeros((16,), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        flag = wb.r_is_per_sequence(r, False)
        a.add_(1.0)
    torch.cuda.synchronize()
    assert flag is False
    assert wb.r_is_per_sequence(r, False) is True


# ---------------------------------------------------------------- b. the resident clipper, its entries evicted
def _clipper(wdf, theta):
    Vs = wdf.ResistiveVoltageSource(float(theta[2]), trainable=False)
    Cap = wdf.Capacitor(float(theta[3]), FS, trainable=True)
    P1 = wdf.Parallel(Vs, Cap)
    dp = wdf.DiodePair(P1, float(theta[0]), Vt=float(theta[1]), nDiodes=1.0, trainable=True)
    return wdf.Circuit(P1, dp, Cap, per_sample_R=Vs), [dp.Is, dp.nVt, Cap.C]


@pytest.mark.parametrize("loss_kind", ["mse", "mse+esr"])
def test_resident_clipper_with_evicted_entries_and_a_batch_at_a_recycled_address(wdf, oracle, loss_kind):
    """Circuit(per_sample_R=Vs).to_device(), one resident entry at a time: batch A (one pot value per sequence), batch B, then
    A' -- A's input shape, a pot that moves, built fresh where A was.  Loss and tape.gradient against the oracle every call."""
    from wdf_hip import workload
    tf = wdf.tf
    B, T, skip = 128, 2048, 50
    theta = workload.clipper_theta()
    th64 = theta.astype(np.float32).astype(np.float64)
    circ, params = _clipper(wdf, theta)
    circ.to_device()
    circ._res_cache.max_entries = 1
    batches = [(workload.sweep_batch(B, T, seed=51), workload.dataset_resistance_batch(B, T)),
               (workload.sweep_batch(B, T, seed=52), workload.pot_resistance_batch(B, T)),
               (workload.sweep_batch(B, T, seed=53), moving_pot(B, T, 9))]
    a_key, a_ref, xin, tgt = None, None, None, None
    for i, (x, r) in enumerate(batches):
        x64, r64 = x.astype(np.float64), r.astype(np.float64)
        t64 = 0.9 * oracle.clipper_fwd(workload.target_theta(), FS, x64, r=r64)
        xin = tgt = None
        xin, tgt = cuda(np.stack([x, r], axis=-1)), cuda(t64)
        if i == 0:
            a_key, a_ref = key(xin), weakref.ref(xin)
        if i == 2:
            gc.collect()
            assert a_ref() is None and key(xin) == a_key, "batch A' did not land where A was: no collision to test"
        with tf.GradientTape() as tape:
            loss = circ.mse(xin, tgt) if loss_kind == "mse" else circ.mse_esr(xin, tgt, skip)
        grads = [float(v) for v in tape.gradient(loss, params)]
        y64 = oracle.clipper_fwd(th64, FS, x64, r=r64)
        if loss_kind == "mse":
            L = float(np.mean((y64 - t64) ** 2))
            gy = 2.0 * (y64 - t64) / y64.size
        else:
            gy, L = esr_grad_and_loss(y64, t64, skip)
        _, g64 = oracle.clipper_fwd_bwd(th64, FS, x64, gy, r=r64)
        print(f"batch {i}: loss {abs(float(loss) - L) / L:.2e}, grads {rel(grads, g64[[0, 1, 3]]):.2e}")
        assert abs(float(loss) - L) <= 2e-5 * L, (i, float(loss), L)
        assert rel(grads, g64[[0, 1, 3]]) < 3e-4, (i, grads, g64)
        assert len(circ._res_cache) == 1
        loss = tape = None


# ---------------------------------------------------------------- c. the streamed-coefficient tree, pot constant then moving
@pytest.mark.parametrize("root,pot_on", [("diode", "Vs"), ("diode", "R"), ("mlp", "Vs")])
def test_streamed_tree_pot_constant_then_moving_at_the_same_address(wdf, oracle, golden, root, pot_on):
    """The HPF clipper (test_gpu_ss_dyn.build_hpf) with a pot channel: x1 with one pot value per sequence (one coefficient row
    per sequence), then x2 -- a pot that moves inside every sequence -- where x1 was, then x3 constant again.  y and the
    component gradients against the oracle's tree interpreter on each call's own data."""
    from test_gpu_ss_dyn import _net, build_hpf, hpf_oracle
    tf = wdf.tf
    O = oracle
    B, T = 128, 2048
    if root == "diode":
        vals = [33.0e3, 1.0e3, 22.0e-9, 4.352e-9, 25.85e-3 * 1.906]
        net, oc = None, hpf_oracle(O, "diode", pot_on)
        theta = np.array(vals, dtype=np.float32).astype(np.float64)
    else:
        vals = [33.0e3, 1.0e3, 22.0e-9]
        net, wts, sizes = _net(golden, "2x8")
        oc = hpf_oracle(O, "mlp", pot_on, sizes=sizes, acts=[O.ACT_TANH] * (len(sizes) - 2) + [O.ACT_NONE])
        theta = np.concatenate([np.array(vals, dtype=np.float32).astype(np.float64), wts.astype(np.float32).astype(np.float64)])
    grid = np.array([300.0, 1.0e3, 2.5e3, 5.0e3]) if pot_on == "Vs" else np.array([10.0e3, 25.2e3, 45.2e3, 75.0e3])
    const = np.repeat(grid[np.arange(B) % len(grid)][:, None], T, axis=1)
    step = np.where(np.arange(T)[None, :] < (T // 4 + 7 * np.arange(B))[:, None] % T, const, const[::-1])
    moving = step * (1.0 + 0.25 * np.sin(2 * np.pi * np.arange(T)[None, :] / 700.0))
    chans = [const, moving, const[::-1]]
    rng = np.random.default_rng(11)
    gyd = cuda(rng.standard_normal((T, B)) / (B * T))
    gy = gyd.cpu().numpy().astype(np.float64)
    circ, params, _ = build_hpf(wdf, root, pot_on, vals, net)
    n_comp = 5 if root == "diode" else 3
    live = [i for i in range(n_comp) if not (i == 0 and pot_on == "R") and not (i == 1 and pot_on == "Vs")]
    k1 = w1 = xin = None
    for i, r in enumerate(chans):
        x = (1.5 * rng.standard_normal((B, T))).astype(np.float32)
        xin = None
        xin = cuda(np.stack([x, r], axis=-1))
        if i == 0:
            k1, w1 = key(xin), weakref.ref(xin)
        elif i == 1:
            gc.collect()
            # the address comes back unless a cache holds x1 -- which is what keeps it from holding other data
            assert w1() is not None or key(xin) == k1, "x2 did not land where x1 was: no collision to test"
        with tf.GradientTape() as tape:
            y = circ(xin)
            loss = tf.reduce_sum(y * gyd)
        grads = tape.gradient(loss, params)
        xin64 = np.stack([x, r], axis=-1).astype(np.float32).astype(np.float64)
        y_ref = O.tree_fwd(oc, theta, xin64)
        e_y = float(np.max(np.abs(y.cpu().numpy() - y_ref)))
        g_ref = O.tree_grad(oc, theta, xin64, gy, params=live)
        got = np.array([float(grads[j]) for j in live])
        print(f"{root} pot on {pot_on}, call {i}: max|y - oracle| {e_y:.2e}, grads {rel(got, g_ref):.2e}")
        assert e_y < 3e-6, (i, e_y)
        assert rel(got, g_ref) < 3e-4, (i, got, g_ref)
        # drop everything that refers to this call's input: only the circuit's own caches may keep it
        y = loss = grads = tape = None
        circ._anchor = None
        circ.__dict__.pop("_dyn_warm", None)


# ---------------------------------------------------------------- d. caches that hold their tensor: regression guards
def test_resident_linear_tree_with_evicted_entries(wdf, oracle):
    """lpf.py's tree, to_device(), one resident entry at a time: a batch, another, then a fresh batch of the first shape at a
    recycled address -- y and the loss against the oracle every call."""
    tf = wdf.tf
    B, T = 256, 1024
    R1, C1 = wdf.Resistor(1000.0, True), wdf.Capacitor(1.0e-6, FS, True)
    circ = wdf.Circuit(wdf.Inverter(wdf.Series(R1, C1)), wdf.IdealVoltageSource(), C1).to_device()
    circ._lin.cache.max_entries = 1
    oc = oracle.rc_lowpass_circuit(FS)
    theta = np.array([1000.0, 1.0e-6], dtype=np.float32).astype(np.float64)
    rng = np.random.default_rng(21)
    xd = td = None
    for i in range(4):
        x = rng.standard_normal((B, T)).astype(np.float32)
        tgt = (0.5 * rng.standard_normal((T, B))).astype(np.float32)
        xd = td = None
        xd, td = cuda(x), cuda(tgt)
        with tf.GradientTape() as tape:
            loss = circ.mse(xd, td)
        tape.gradient(loss, [R1.R, C1.C])
        yref = oracle.tree_fwd(oc, theta, x.astype(np.float64))
        L = float(np.mean((yref - tgt) ** 2))
        assert float(np.max(np.abs(circ.last_output.cpu().numpy() - yref))) < 2e-6, i
        assert abs(float(loss) - L) <= 1e-5 * L, (i, float(loss), L)
        loss = tape = None


def test_host_clipper_split_channels_with_fresh_inputs(wdf, oracle):
    """Circuit.__call__ on the clipper with a pot channel (engine.split_channels caches its de-interleaved copies per input
    object): a batch with a constant pot, then fresh batches whose pot moves, and an in-place change of the last one."""
    from wdf_hip import workload
    B, T = 128, 2048
    theta = workload.clipper_theta()
    th64 = theta.astype(np.float32).astype(np.float64)
    circ, _ = _clipper(wdf, theta)
    xin = None
    for i, r in enumerate([workload.dataset_resistance_batch(B, T), moving_pot(B, T, 31), moving_pot(B, T, 32)]):
        x = workload.sweep_batch(B, T, seed=60 + i)
        xin = None
        xin = cuda(np.stack([x, r], axis=-1))
        y = circ(xin)
        y64 = oracle.clipper_fwd(th64, FS, x.astype(np.float64), r=r.astype(np.float64))
        assert float(np.max(np.abs(y.cpu().numpy() - y64))) < 3e-6, i
    # e. in place: the version counter moves and the next call reads the new data
    xin[:, :, 0].mul_(0.5)
    xin[:, T // 2:, 1].mul_(1.5)
    y = circ(xin)
    xh = xin.cpu().numpy().astype(np.float64)
    y64 = oracle.clipper_fwd(th64, FS, xh[:, :, 0], r=xh[:, :, 1])
    assert float(np.max(np.abs(y.cpu().numpy() - y64))) < 3e-6


def test_resident_clipper_in_place_change_of_the_batch(wdf, oracle):
    """e. The resident clipper's entry is keyed on the input's version: x.mul_ between calls gives a new entry, and the loss
    is the oracle's on the new data (test_resident_circuit_mini_batch_loop_with_fresh_slices counts entries only)."""
    from wdf_hip import workload
    B, T = 128, 2048
    theta = workload.clipper_theta()
    th64 = theta.astype(np.float32).astype(np.float64)
    circ, _ = _clipper(wdf, theta)
    circ.to_device()
    x, r = workload.sweep_batch(B, T, seed=71), workload.dataset_resistance_batch(B, T)
    xin = cuda(np.stack([x, r], axis=-1))
    t64 = 0.9 * oracle.clipper_fwd(th64, FS, x.astype(np.float64), r=r.astype(np.float64))
    tgt = cuda(t64)
    for i in range(3):
        loss = float(circ.mse(xin, tgt))
        xh = xin.cpu().numpy().astype(np.float64)
        y64 = oracle.clipper_fwd(th64, FS, xh[:, :, 0], r=xh[:, :, 1])
        L = float(np.mean((y64 - t64) ** 2))
        assert abs(loss - L) <= 2e-5 * L, (i, loss, L)
        xin.mul_(torch.tensor([0.7, 1.0], device="cuda") if i == 0 else torch.tensor([1.0, 1.3], device="cuda"))
    assert len(circ._res_cache) == 3


# ---------------------------------------------------------------- 4. state and weights the resident paths publish
def test_resident_linear_tree_last_state_is_kept_by_value(wdf, oracle):
    """mse(carry_state=True) on a resident linear tree: the last_state kept after call 1 is the oracle's final state and stays
    so through two more calls; last_output right after each call is that call's y.  (A time constant of 480 samples over
    256-sample calls: every call ends in a state of its own, so a kept state that is overwritten shows.)"""
    B, T = 70, 256
    R1, C1 = wdf.Resistor(1000.0, True), wdf.Capacitor(1.0e-5, FS, True)
    circ = wdf.Circuit(wdf.Inverter(wdf.Series(R1, C1)), wdf.IdealVoltageSource(), C1).to_device()
    oc = oracle.rc_lowpass_circuit(FS)
    theta = np.array([1000.0, 1.0e-5], dtype=np.float32).astype(np.float64)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, T)).astype(np.float32)
    tgt = (0.5 * rng.standard_normal((T, B))).astype(np.float32)
    xd, td = cuda(x), cuda(tgt)
    z, kept = None, None
    for call in range(3):
        circ.mse(xd, td, carry_state=True)
        yref, zT = oracle.tree_fwd(oc, theta, x.astype(np.float64), z0=z, return_state=True)
        assert float(np.max(np.abs(circ.last_output.cpu().numpy() - yref))) < 3e-6, call
        if call == 0:
            kept, kept_val, z1 = circ.last_state, circ.last_state.clone(), zT[:, 1]
        z = zT
    assert float(np.max(np.abs(circ.last_state.cpu().numpy()[0] - z1))) > 1e-3       # (the calls did end in other states)
    assert torch.equal(kept, kept_val)
    assert float(np.max(np.abs(kept.cpu().numpy()[0] - z1))) < 3e-6


def test_streamed_tree_network_weights_belong_to_one_circuit(wdf, oracle, golden):
    """_DynResident moves a DenseRootModel's weights into its flat vector and marks them: a second circuit's to_device() on the
    same network is refused, the first still matches the oracle, and the one-launch Adam of MlpResident's vector declines
    these weights (their gradients are not slices of a one-pass step's output)."""
    from wdf_hip import binding
    from test_gpu_ss_dyn import _net, hpf_oracle
    from layers import DenseRootModel
    tf = wdf.tf
    js, wts, sizes = _net(golden, "2x8")
    vals = [33.0e3, 1.0e3, 22.0e-9]

    def tree(model):
        R = wdf.Resistor(vals[0], True)
        Vs = wdf.ResistiveVoltageSource(vals[1], trainable=True)
        C = wdf.Capacitor(vals[2], FS, True)
        top = wdf.Parallel(R, wdf.Series(Vs, C))
        return wdf.Circuit(top, model, R, per_sample_R=Vs)

    model = DenseRootModel(js)
    first = tree(model).to_device()
    with pytest.raises(binding.WdfHipError):
        tree(model).to_device()
    B, T = 40, 512
    rng = np.random.default_rng(8)
    x = (0.8 * rng.standard_normal((B, T))).astype(np.float32)
    r = np.repeat(np.array([300.0, 1.0e3, 2.5e3, 5.0e3])[np.arange(B) % 4][:, None], T, axis=1).astype(np.float32)
    weights = list(model.trainable_variables)
    with tf.GradientTape() as tape:
        y = first(cuda(np.stack([x, r], axis=-1)))
        loss = tf.reduce_sum(y * y)
    grads = tape.gradient(loss, weights)
    oc = hpf_oracle(oracle, "mlp", "Vs", sizes=sizes, acts=[oracle.ACT_TANH] * (len(sizes) - 2) + [oracle.ACT_NONE])
    theta = np.concatenate([np.array(vals, dtype=np.float32).astype(np.float64), wts.astype(np.float32).astype(np.float64)])
    y_ref = oracle.tree_fwd(oc, theta, np.stack([x, r], axis=-1).astype(np.float64))
    assert float(np.max(np.abs(y.cpu().numpy() - y_ref))) < 3e-6
    opt = tf.keras.optimizers.Adam(learning_rate=1.0e-3)
    assert opt._apply_flat(list(zip(grads, weights))) is False
