"""GPU: Circuit.mse / mse_esr(..., grad=False) on a resident diode-root tree through the loss-only evaluation pass
(lowering.NL_EVAL_PASS_SERVES = True for the duration of each test; _LinResident.eval_entry / evaluate, csrc/wdf_ss_nl_eval.h).
Reference: the fp64 oracle's tree interpreter at the parameters of the call.  Bounds: tests/test_gpu_ss_nl_eval.py's rows."""
import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_ss_nl_step import cuda, hpf  # noqa: E402
from test_gpu_ss_nl_esr_step import _ORACLE, entry_of, esr_step, esr_terms, hpf_oracle  # noqa: E402
from test_gpu_ss_nl_step_edges import data, theta_of  # noqa: E402


@pytest.fixture
def wdf():
    import tf_wdf
    return tf_wdf


@pytest.fixture(autouse=True)
def _oracle(oracle):
    _ORACLE["o"] = oracle


@pytest.fixture
def serves():
    from wdf_hip import lowering
    was = lowering.NL_EVAL_PASS_SERVES
    lowering.NL_EVAL_PASS_SERVES = True
    yield lowering
    lowering.NL_EVAL_PASS_SERVES = was


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def oracle_y(theta, x, n=(2, 3)):
    O = _ORACLE["o"]
    return O.tree_fwd(hpf_oracle(O, *n), theta, x.astype(np.float64))


def eval_entries(circ):
    return [e for e in circ._tree.cache.values() if "sums" in e]


def test_losses_against_the_oracle(wdf, serves):
    B, T, skip = 70, 1000, 50
    x, tgt = data((1, 1), B, T, 7070)
    circ, params = hpf(wdf)
    circ.to_device()
    xd, td = cuda(x), cuda(tgt)
    yref = oracle_y(theta_of(params), x)
    _, _, l0, _ = esr_terms(yref, tgt, 0)
    _, E50, l50, _ = esr_terms(yref, tgt, skip)
    assert E50 / (B * (T - skip)) > 1e-4
    mse = circ.mse(xd, td, grad=False, store_output=False)
    assert circ.last_output is None
    ents = eval_entries(circ)
    assert len(ents) == 1 and ents[0]["y"] is None and len(circ._tree.cache) == 1
    both = circ.mse_esr(xd, td, skip=skip, grad=False, store_output=False)
    assert circ.last_output is None and eval_entries(circ)[0] is ents[0] and ents[0]["y"] is None     # (one entry: both losses, every skip)
    for v in (mse, both):
        assert not v.requires_grad and v.grad_fn is None and getattr(v, "_wdf_fused", None) is None
    e_m, e_b = abs(float(mse) - l0[0]) / l0[0], abs(float(both) - l50[2]) / l50[2]
    print(f"FIG circuit | mse={e_m:.2e} mse+esr={e_b:.2e}")
    assert e_m < 2e-6 and e_b < 1e-5
    again = circ.mse_esr(xd, td, skip=skip, grad=False)          # a later call that wants y makes it
    y = circ.last_output
    assert y is ents[0]["y"] and y is not None and tuple(y.shape) == (T, B)
    e_y = float(np.max(np.abs(y.cpu().numpy() - yref)))
    print(f"FIG circuit | y={e_y:.2e} (from snapshots)")
    assert e_y < 4e-6 and abs(float(again) - l50[2]) / l50[2] < 1e-5
    assert abs(float(mse) - l0[0]) / l0[0] < 2e-6      # (its row was not written again)
    ctl = circ._tree.read_eval_ctl(ents[0])
    assert ctl["call"] == 3 and ctl["gated_groups"] == 0


def _epochs(wdf, train, val, validate, steps=12, skip=50):
    tf = wdf.tf
    circ, params = hpf(wdf)
    circ.to_device()
    pb = circ._tree.pb
    opts = [tf.keras.optimizers.Adam(learning_rate=1.0e-3 * float(p)) for p in params]
    (xd, td), (xv, tv) = train, val
    rec = {"loss": [], "grads": [], "block": [], "val": {}, "theta": {}, "gated": []}
    for step in range(steps):
        with tf.GradientTape() as tape:
            loss = esr_step(circ, xd, td, skip)                   # the one-pass MSE + ESR step: a training entry of its own
        grads = tape.gradient(loss, params)
        assert len(pb.pending) == 0
        rec["loss"].append(loss.detach().as_subclass(torch.Tensor).clone())
        rec["grads"].append(torch.stack([g.detach().as_subclass(torch.Tensor).reshape(()) for g in grads]).clone())
        rec["block"].append(pb.block.detach().clone())            # (every update so far is in it: the step's probe applied them)
        for o, g, p in zip(opts, grads, params):
            o.apply_gradients([(g, p)])
        if validate:
            v = circ.mse_esr(xv, tv, skip=skip, grad=False, store_output=False)
            assert len(pb.pending) == 0                            # (the validation call's probe took the queued updates along)
            ent = eval_entries(circ)[0]
            if step in (0, 1, 2, 5, 11):
                rec["val"][step] = float(v)
                rec["theta"][step] = theta_of(params)
                rec["gated"].append(circ._tree.read_eval_ctl(ent)["gated_groups"])
    pb.flush()
    rec["block"].append(pb.block.detach().clone())
    assert len([e for e in circ._tree.cache.values() if "sums" not in e]) == 1
    rec["ctl"] = circ._tree.read_ctl(entry_of(circ, skip))
    if validate:
        end = circ._tree.read_eval_ctl(eval_entries(circ)[0])
        rec["eval_calls"], rec["total_gated"], rec["replans"] = end["call"], end["total_gated"], eval_entries(circ)[0]["replans"]
    rec["n_eval"] = len(eval_entries(circ))
    return rec


def test_an_epoch_loop_trains_bit_for_bit_as_without_the_validation_call(wdf, serves):
    B, T, skip = 128, 2048, 50
    x, _ = data((1, 1), B, T, 1212)
    xv, _ = data((1, 1), B, T, 1313)
    ref, _ = hpf(wdf)
    tgt = (ref(cuda(x)) * 0.8).as_subclass(torch.Tensor).detach().cpu().numpy()
    tgv = (ref(cuda(xv)) * 0.8).as_subclass(torch.Tensor).detach().cpu().numpy()
    train, val = (cuda(x), cuda(tgt)), (cuda(xv), cuda(tgv))
    a = _epochs(wdf, train, val, True)
    b = _epochs(wdf, train, val, False)
    assert a["n_eval"] == 1 and b["n_eval"] == 0
    for key in ("loss", "grads", "block"):
        assert len(a[key]) == len(b[key])
        for step, (u, v) in enumerate(zip(a[key], b[key])):
            assert torch.equal(u, v), (key, step)
    assert a["ctl"] == b["ctl"]
    worst = 0.0
    for step, v in a["val"].items():
        yref = oracle_y(a["theta"][step], xv)
        _, E, l3, _ = esr_terms(yref, tgv, skip)
        assert E / (B * (T - skip)) > 1e-4
        worst = max(worst, abs(v - l3[2]) / l3[2])
    print(f"FIG epochs | validation loss {worst:.2e}; gated after each checked call {a['gated']}")
    assert worst < 1e-5
    assert all(g == 0 for g in a["gated"][1:])
    # every call, not only the sampled ones: the groups repaired since the plan are the first call's (no re-plan zeroed the count)
    assert a["eval_calls"] == 12 and a["replans"] == 0 and a["total_gated"] == a["gated"][0]


def test_what_does_not_take_the_pass(wdf, serves):
    B, T, skip = 70, 1000, 50
    x, tgt = data((1, 1), B, T, 7070)
    xd, td = cuda(x), cuda(tgt)
    circ, _ = hpf(wdf)
    circ.to_device()
    want = float(circ.mse_esr(xd, td, skip=skip, grad=False))
    want_mse = float(circ.mse(xd, td, grad=False))
    assert len(eval_entries(circ)) == 1

    def old_route(build, kw=dict):
        """every call on a circuit of its own, with arguments of its own: a stateful call leaves `last_state` behind, and the next
        `carry_state=True` call on the same circuit would start from it"""
        got = {}
        for name in ("mse+esr", "mse"):
            c, _ = hpf(wdf)
            build(c)
            args = kw()
            v = c.mse_esr(xd, td, skip=skip, grad=False, **args) if name == "mse+esr" else c.mse(xd, td, grad=False, **args)
            got[name] = float(v)
            assert not v.requires_grad and v.grad_fn is None
            assert getattr(c, "_tree", None) is None or len(eval_entries(c)) == 0
        print(f"FIG old route | mse+esr={abs(got['mse+esr'] - want) / want:.2e} mse={abs(got['mse'] - want_mse) / want_mse:.2e}")
        assert abs(got["mse+esr"] - want) < 1e-5 * want, (got, want)
        assert abs(got["mse"] - want_mse) < 1e-5 * want_mse, (got, want_mse)

    old_route(lambda c: c.to_device(), lambda: dict(z0=torch.zeros((1, B), device="cuda")))
    old_route(lambda c: c.to_device(), lambda: dict(carry_state=True))

    def generic(c):
        c.force_generic = True
        c.to_device()
    old_route(generic)
    old_route(lambda c: None)                                      # a host-resident circuit
    serves.NL_EVAL_PASS_SERVES = False
    old_route(lambda c: c.to_device())
