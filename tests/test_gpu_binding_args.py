"""GPU: argument handling of the one-pass step wrappers in wdf_hip/binding.py -- clipper_step_mse_tp / _esr_tp,
clipper_bwd_mse_tp_adam, clipper_asym_step_mse / _esr, ss_asym_step_mse / _esr, ss_lin_step_mse / _esr and the three *_esr_finish --
which share one set of helpers (allocate-or-check an output, a workspace, y / zT, the ESR outputs, the Adam tail).

  refusals  a wrong-shape target or y, a workspace one byte short, a wrong-size out / out7 / sums / g / loss3, a z0 of the wrong
            size, an optimizer of the wrong length or with finish=False, an rseq of the wrong length or dtype or with the closed
            form: each raises WdfHipError on the host.  No launch follows: every output buffer handed in is filled with a sentinel
            and holds it after a synchronise.  Nothing here reaches a kernel with a bad buffer.
  accepted  one call with every optional buffer None and one with every buffer preallocated give the same bits, and the second
            returns the very objects passed in; x_rseq(x, rseq, ...) and x(..., rseq=rseq) give the same bits.  The numbers
            themselves are the oracle tests' business (test_gpu_fused_step, test_gpu_asym_step, test_gpu_ss_asym_step, ...).

Shapes: B = 65 (two waves, the second with one live lane); T = 64 in two chunks for the clipper (32-step units), T = 16 in two
chunks for the two-different-diode and state-space steps (8-step units); the smallest trees the state-space steps are built for
(no state and one input for the linear step -- one state where z0 is the argument under test --, HPFDiodeClipper's one state for
the two-different-diode root)."""
import numpy as np
import pytest

import ss_asym_cases as cases
import ss_lin_esr_ref as E

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FS, B, EPS = 48000.0, 65, float(np.finfo(float).eps)
SENT, SENT_INT = -7.25, 90                              # no output of these steps: what an untouched buffer still holds
THETA6 = [4.352e-9, 25.85e-3 * 1.906, 2.0e-6, 25.85e-3 * 1.4, 45.0e3, 4.7e-9]
INPUTS = ("target", "rseq", "x_tm", "coef", "jac", "mode", "opt", "finish")


@pytest.fixture(scope="module")
def wb():
    from wdf_hip import binding
    binding.require_gpu()
    return binding


def cuda(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def full(*shape, dtype=torch.float32):
    return torch.full(shape, SENT if dtype == torch.float32 else SENT_INT, dtype=dtype, device="cuda")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def untouched(bufs):
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t == (SENT if t.dtype == torch.float32 else SENT_INT)).all()), f"{name} was written to"


def signal(T, seed):
    rng = np.random.default_rng(seed)
    return cuda(0.5 * rng.standard_normal((B, T))), cuda(0.3 * rng.standard_normal((T, B)))


class Step:
    """One wrapper at one set of good arguments.  call(**over) runs it; buffers(clean) makes every optional buffer, filled with
    the sentinel (clean: the workspace as the wrapper itself would make it); outs(result) names what the call wrote; bad maps a
    refusal's name to the keywords that provoke it; twin(rseq) is the *_rseq spelling of call(rseq=rseq)."""

    def __init__(self, call, buffers, outs, bad, twin=None):
        self.call, self.buffers, self.outs, self.bad, self.twin = call, buffers, outs, bad, twin


def clipper(wb, loss):
    from wdf_hip import workload
    T, K, W = 64, 2, 32
    x, tgt = signal(T, 1)
    theta = cuda(workload.clipper_theta())
    need = wb.lib().wdf_clipper_step_mse_tp_ws_bytes(B, K)

    def common(clean):
        return dict(y=full(T, B), ws=wb.step_mse_workspace(B, K, "cuda") if clean else full(need, dtype=torch.uint8),
                    status=full(4, dtype=torch.int32))

    bad = {"target": dict(target=tgt[:-1].contiguous()), "y": dict(y=full(T, B - 1)), "ws": dict(ws=full(need - 1, dtype=torch.uint8)),
           "z0": dict(z0=full(B - 1)), "opt_n": dict(opt=wb.Adam(6, 1e-3))}
    if loss == "mse":
        return Step(lambda target=tgt, **kw: wb.clipper_step_mse_tp(x, theta, FS, target, 2.0 / (B * T), K, W, **kw),
                    lambda clean=False: dict(common(clean), gtheta=full(4), sse=full(1)),
                    lambda r: dict(y=r[0], gtheta=r[2], sse=r[3], status=r[4]),
                    dict(bad, gtheta=dict(gtheta=full(5)), sse=dict(sse=full(2))))
    return Step(lambda target=tgt, **kw: wb.clipper_step_esr_tp(x, theta, FS, target, float(B * (T - 5)), EPS, 5, K, W, **kw),
                lambda clean=False: dict(common(clean), sums10=full(10), gtheta=full(4), loss3=full(3)),
                lambda r: dict(y=r[0], sums10=r[2], gtheta=r[3], loss3=r[4], status=r[5]),
                dict(bad, sums10=dict(sums10=full(9)), gtheta=dict(gtheta=full(3)), loss3=dict(loss3=full(2)),
                     opt_without_finish=dict(opt=wb.Adam(4, 1e-3), finish=False)))


def asym(wb, loss):
    T, K, W = 16, 2, 8
    x, tgt = signal(T, 2)
    th6, newton = cuda(THETA6), wb.ASYM_NEWTON_F32
    need = getattr(wb.lib(), f"wdf_clipper_asym_step_{loss}_ws_bytes")(B, K)

    def common(clean):
        return dict(y=full(T, B), ws=full(need, dtype=torch.uint8), status=full(4, dtype=torch.int32))

    pots = torch.full((B,), 45.0e3, device="cuda")
    bad = {"target": dict(target=tgt[:-1].contiguous()), "y": dict(y=full(T - 1, B)), "ws": dict(ws=full(need - 1, dtype=torch.uint8)),
           "z0": dict(z0=full(B + 1)), "opt_n": dict(opt=wb.Adam(4, 1e-3)), "rseq_short": dict(rseq=pots[:-1].contiguous()),
           "rseq_dtype": dict(rseq=pots.double()), "rseq_closed_form": dict(rseq=pots, mode=wb.ASYM_OMEGA_F32)}
    if loss == "mse":
        return Step(lambda target=tgt, mode=newton, **kw: wb.clipper_asym_step_mse(x, th6, FS, mode, target, 2.0 / (B * T), K, W, **kw),
                    lambda clean=False: dict(common(clean), out7=full(7)),
                    lambda r: dict(y=r[0], out7=r[2], status=r[3]),
                    dict(bad, out7=dict(out7=full(6))),
                    twin=lambda rseq: wb.clipper_asym_step_mse_rseq(x, rseq, th6, FS, newton, tgt, 2.0 / (B * T), K, W))
    n = float(B * (T - 3))
    return Step(lambda target=tgt, mode=newton, **kw: wb.clipper_asym_step_esr(x, th6, FS, mode, target, n, EPS, 3, K, W, **kw),
                lambda clean=False: dict(common(clean), sums14=full(14), gtheta6=full(6), loss3=full(3)),
                lambda r: dict(y=r[0], sums14=r[2], gtheta6=r[3], loss3=r[4], status=r[5]),
                dict(bad, sums14=dict(sums14=full(10)), gtheta6=dict(gtheta6=full(4)), loss3=dict(loss3=full(4)),
                     opt_without_finish=dict(opt=wb.Adam(6, 1e-3), finish=False)),
                twin=lambda rseq: wb.clipper_asym_step_esr_rseq(x, rseq, th6, FS, newton, tgt, n, EPS, 3, K, W))


def ss_asym(wb, loss):
    import tf_wdf
    T, K, W = 16, 2, 8
    x, tgt = signal(T, 3)
    circ, _ = cases.hpf(tf_wdf)                                                  # one state, one input: the smallest tree built
    coef64, r_port = circ.matrices()
    dp = circ.root
    coef = coef64.float().cuda().contiguous()
    rootp = torch.tensor([float(torch.as_tensor(v).detach()) for v in (dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down, r_port)], device="cuda")
    ns, ni, ng = circ.ns, circ.ni, coef.numel() + 5
    assert (ns, ni) == (1, 1) and wb.ss_asym_step_built(ns, ni, "mse") and wb.ss_asym_step_built(ns, ni, "mse_esr")
    xs = x.unsqueeze(-1).contiguous()
    need = wb.lib().wdf_ss_asym_step_ws_bytes(ns, ni, B, T, K)

    def common(clean):
        return dict(y=full(T, B), ws=full(need, dtype=torch.uint8), status=full(4, dtype=torch.int32))

    bad = {"target": dict(target=tgt[:, :-1].contiguous()), "y": dict(y=full(T, B + 1)), "ws": dict(ws=full(need - 1, dtype=torch.uint8)),
           "z0": dict(z0=full(ns + 1, B))}
    if loss == "mse":
        return Step(lambda target=tgt, **kw: wb.ss_asym_step_mse(xs, coef, rootp, ns, ni, target, 2.0 / (B * T), K, W, **kw),
                    lambda clean=False: dict(common(clean), out=full(1 + ng)),
                    lambda r: dict(y=r[0], out=r[2], status=r[3]),
                    dict(bad, out=dict(out=full(ng))))
    return Step(lambda target=tgt, **kw: wb.ss_asym_step_esr(xs, coef, rootp, ns, ni, target, float(B * (T - 3)), EPS, 3, K, W, **kw),
                lambda clean=False: dict(common(clean), sums=full(2 + 2 * ng), g=full(ng), loss3=full(3)),
                lambda r: dict(y=r[0], sums=r[2], g=r[3], loss3=r[4], status=r[5]),
                dict(bad, sums=dict(sums=full(2 + ng)), g=dict(g=full(ng + 1)), loss3=dict(loss3=full(2))))


def ss_lin(wb, loss):
    T, K = 16, 2
    c = E.case(0, 1, B, T, 3)                                                    # no state, one input: the smallest tree built
    good = dict(x_tm=cuda(c.x), coef=cuda(c.coef), jac=cuda(c.jac, np.float64), target=cuda(c.target), n_chunks=K)
    ws_bytes = wb.lib().wdf_ss_lin_step_ws_bytes if loss == "mse" else wb.lib().wdf_ss_lin_step_esr_ws_bytes
    need = ws_bytes(0, 1, B, T, K)
    assert need > 0
    c1 = E.case(1, 1, B, T, 3)                                                   # (z0 is only looked at where there is a state)
    bad = {"target": dict(target=good["target"][:-1].contiguous()), "y": dict(y=full(T, B - 1)), "ws": dict(ws=full(need - 1, dtype=torch.uint8)),
           "z0": dict(x_tm=cuda(c1.x), coef=cuda(c1.coef), jac=cuda(c1.jac, np.float64), target=cuda(c1.target), z0=full(2, B),
                      ws=full(ws_bytes(1, 1, B, T, K), dtype=torch.uint8))}

    def buffers(clean=False):
        return dict(y=full(T, B), ws=torch.zeros(need, dtype=torch.uint8, device="cuda") if clean else full(need, dtype=torch.uint8))

    if loss == "mse":
        return Step(lambda **kw: wb.ss_lin_step_mse(**{**good, "gscale": 2.0 / (B * T), **kw}), buffers,
                    lambda r: dict(y=r["y"], out=r["out"], loss=r["loss"], ws=r["ws"]), bad)
    return Step(lambda **kw: wb.ss_lin_step_esr(**{**good, "skip": 3, **kw}), buffers,
                lambda r: dict(y=r["y"], sums=r["sums"], g=r["g"], loss3=r["loss3"], ws=r["ws"]), bad)


FAMILIES = {"clipper": clipper, "asym": asym, "ss_asym": ss_asym, "ss_lin": ss_lin}
STEPS = [(f, loss) for f in FAMILIES for loss in ("mse", "esr")]
BAD = {"clipper": ["target", "y", "ws", "z0", "opt_n"],
       "asym": ["target", "y", "ws", "z0", "opt_n", "rseq_short", "rseq_dtype", "rseq_closed_form"],
       "ss_asym": ["target", "y", "ws", "z0"], "ss_lin": ["target", "y", "ws", "z0"]}
BAD_OUT = {("clipper", "mse"): ["gtheta", "sse"], ("clipper", "esr"): ["sums10", "gtheta", "loss3", "opt_without_finish"],
           ("asym", "mse"): ["out7"], ("asym", "esr"): ["sums14", "gtheta6", "loss3", "opt_without_finish"],
           ("ss_asym", "mse"): ["out"], ("ss_asym", "esr"): ["sums", "g", "loss3"], ("ss_lin", "mse"): [], ("ss_lin", "esr"): []}


@pytest.fixture(scope="module")
def steps(wb):
    memo = {}

    def get(family, loss):
        if (family, loss) not in memo:
            memo[family, loss] = FAMILIES[family](wb, loss)
        return memo[family, loss]
    return get


@pytest.mark.parametrize("family,loss,what", [(f, ls, w) for f, ls in STEPS for w in BAD[f] + BAD_OUT[f, ls]])
def test_refused_on_the_host_and_nothing_is_launched(wb, steps, family, loss, what):
    st = steps(family, loss)
    assert set(st.bad) == set(BAD[family] + BAD_OUT[family, loss])
    bufs = {**st.buffers(), **st.bad[what]}
    with pytest.raises(wb.WdfHipError):
        st.call(**bufs)
    untouched({k: v for k, v in bufs.items() if k not in INPUTS})


@pytest.mark.parametrize("family,loss", STEPS)
def test_allocated_and_preallocated_buffers_give_the_same_bits(steps, family, loss):
    st = steps(family, loss)
    a = st.outs(st.call())
    bufs = st.buffers(clean=True)
    b = st.outs(st.call(**bufs))
    torch.cuda.synchronize()
    for name, t in b.items():
        if name in bufs:
            assert t is bufs[name], f"{name}: the buffer handed in is not the one handed back"
        if name not in ("ws", "status"):
            assert same_bits(a[name], t), name
            assert not bool((t == SENT).all()), f"{name} was not written"


@pytest.mark.parametrize("loss", ["mse", "esr"])
def test_rseq_keyword_and_rseq_twin_give_the_same_bits(steps, loss):
    st = steps("asym", loss)
    rseq = cuda(np.linspace(10.0e3, 99.1e3, B))
    a, b, plain = st.outs(st.call(rseq=rseq)), st.outs(st.twin(rseq)), st.outs(st.call())
    torch.cuda.synchronize()
    for name in a:
        if name != "status":
            assert same_bits(a[name], b[name]), name
    assert not same_bits(a["y"], plain["y"])                  # (the pot per sequence is not theta6[4]: the keyword did something)


def test_bwd_mse_tp_adam_allocated_and_preallocated(wb):
    """clipper_bwd_mse_tp_adam (the Adam tail and the flag word): the same bits with gtheta, sse and ws handed in, theta updated
    alike; an optimizer of another length is refused and nothing is written."""
    from wdf_hip import workload
    T, K = 64, 2
    x, tgt = signal(T, 4)
    th0 = cuda(workload.clipper_theta())
    _, zs, zT = wb.clipper_fwd(x, th0, FS, want_stash=True, want_zT=True)
    runs = []
    for pre in (False, True):
        theta, opt = th0.clone(), wb.Adam(4, 1e-3 * workload.clipper_theta())
        kw = dict(gtheta=full(4), sse=full(1), ws=wb.bwd_tp_workspace(B, K, "cuda")) if pre else {}
        g, sse = wb.clipper_bwd_mse_tp_adam(x, theta, FS, zs, zT, tgt, 2.0 / (B * T), K, opt, **kw)
        if pre:
            assert g is kw["gtheta"] and sse is kw["sse"]
        runs.append((g, sse, theta))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert same_bits(a, b)
    assert not same_bits(runs[0][2], th0)
    bufs, theta = dict(gtheta=full(4), sse=full(1)), th0.clone()
    with pytest.raises(wb.WdfHipError):
        wb.clipper_bwd_mse_tp_adam(x, theta, FS, zs, zT, tgt, 2.0 / (B * T), K, wb.Adam(6, 1e-3), **bufs)
    untouched(bufs)
    assert same_bits(theta, th0)


@pytest.mark.parametrize("name,gname,n", [("esr_finish", "gtheta", 4), ("asym_esr_finish", "gtheta6", 6), ("ss_lin_esr_finish", "g", 3)])
def test_esr_finish_allocated_preallocated_and_refusals(wb, name, gname, n):
    """The three finish functions (one body): the same bits into buffers handed in, which come back; a gradient or loss3 of
    another size and sums of another length are refused and nothing is written."""
    fin = getattr(wb, name)
    sums = cuda(np.concatenate([[3.0, 40.0], np.random.default_rng(5).standard_normal(2 * n)]))
    g0, l0 = fin(sums, 1000.0, EPS)
    bufs = {gname: full(n), "loss3": full(3)}
    g1, l1 = fin(sums, 1000.0, EPS, **bufs)
    torch.cuda.synchronize()
    assert g1 is bufs[gname] and l1 is bufs["loss3"]
    assert same_bits(g0, g1) and same_bits(l0, l1) and tuple(g0.shape) == (n,) and tuple(l0.shape) == (3,)
    for over, s in (({gname: full(n + 1)}, sums), ({"loss3": full(2)}, sums), ({}, cuda(np.ones(2 + 2 * n + 1)))):
        b = {gname: full(n), "loss3": full(3), **over}
        with pytest.raises(wb.WdfHipError):
            fin(s, 1000.0, EPS, **b)
        untouched(b)
