"""GPU: the loss-only evaluation pass of small diode-root trees (csrc/wdf_ss_nl_eval.h) through binding.ss_nl_eval, with the
probe's coefficients of a resident circuit.

Reference, everywhere: the fp64 oracle's tree interpreter (oracle.tree_fwd); S, E and the three loss terms formed from its y in
numpy fp64.  Trees, node lists, data and tier values are tests/test_gpu_ss_nl_step_edges.py's.

Bounds (the project's own for this circuit family, tests/test_gpu_ss_nl_step.py and test_gpu_ss_nl_step_edges.py):
                      first call, or repaired      two states / two sources, or calls that start from snapshots
  y                   3e-6 V                       4e-6 V
  S, E                1e-5 relative                1e-5 relative
  mse                 2e-6 relative                1e-5 relative
  esr, mse + esr      1e-5 relative                1e-5 relative
Before a case is relied on, the oracle's E / (B (T - skip)) > 1e-4 is asserted, so that relative bounds on E and esr mean something.

Every check prints `FIG <section> | <case> | y=... S=... E=... mse=... esr=...` before it asserts (run with -s).
Measured on an MI355X (worst figure of each section; y in V, the others relative): first call y 7.1e-7, S 6.7e-7, E 1.5e-6, mse 6.7e-7,
esr 4.3e-7 (the sums' figures are the one-sample cases B = 1, skip = T - 1); tiers 6.9e-7 / 1.7e-7 / 3.1e-7 / 2.2e-7 / 1.8e-7; from
snapshots 6.4e-7 / 1.3e-7 / 1.7e-7 / 1.2e-7 / 9.4e-8; repaired and after 5.9e-7 / 1.3e-7 / 1.7e-7 / 1.6e-7 / 1.5e-7; one group of two
repaired 5.8e-7 / 9.8e-8 / 1.7e-7 / 9.9e-8 / 1.2e-7; against the training step y bit for bit at K = 1 and K = 8, S 3.4e-8.

(64, 520, 8): eight chunks do not tile 520 steps in 32-step units (six of 96 do), and the entry point refuses a count that does
not tile; the case runs with the count the asked-for one comes down to, as Circuit does (_LinResident._nl_eval_k): six chunks,
the last one 40 steps long.
"""
import functools
import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_ss_nl_step import FS, cuda, hpf  # noqa: E402,F401
from test_gpu_ss_nl_esr_step import _ORACLE, esr_terms  # noqa: E402
from test_gpu_ss_nl_step_edges import TIERS, build_tree, data, oracle_circuit, theta_of, tier_theta  # noqa: E402

FIRST = dict(y=3e-6, sums=1e-5, mse=2e-6, terms=1e-5)           # one capacitor, one source: first call, or repaired
WIDER = dict(y=4e-6, sums=1e-5, mse=1e-5, terms=1e-5)           # larger trees; calls that start from snapshots
TREES = [(1, 1), (2, 1), (1, 2), (2, 2)]
N_OF = {(1, 1): (2, 3), (2, 1): (1, 2), (1, 2): (3, 2), (2, 2): (2, 3)}      # n_up != n_down on every tree


@pytest.fixture
def wdf():
    import tf_wdf
    return tf_wdf


@pytest.fixture(autouse=True)
def _oracle(oracle):
    _ORACLE["o"] = oracle


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def bound_of(tree, first=True):
    return FIRST if tree == (1, 1) and first else WIDER


def oracle_y(tree, theta, x, n):
    O = _ORACLE["o"]
    return O.tree_fwd(oracle_circuit(O, tree, *n), theta, x.astype(np.float64))


@functools.lru_cache(maxsize=None)
def case_at_the_trees_own_values(tree, B, T, n, seed):
    """x, target and the oracle's y at the values the tree is built with: once per case, shared, never modified"""
    import tf_wdf
    x, tgt = data(tree, B, T, seed)
    circ, params = build_tree(tf_wdf, tree)
    y = oracle_y(tree, theta_of(params), x, n)
    for a in (x, tgt, y):
        a.setflags(write=False)
    return x, tgt, y


class Pass:
    """A resident circuit's probe outputs and one planned workspace of the pass"""

    def __init__(self, circ, x, tgt, K, n, cold=None, ws=None):
        from wdf_hip import binding
        self.b = binding
        self.lin, self.n = circ._tree, n
        self.ns, self.ni = circ.ns, circ.ni
        xd = cuda(x)
        if xd.dim() == 2:
            xd = xd.unsqueeze(-1)
        self.x = xd.permute(1, 2, 0).contiguous()                 # [T][ni][B]
        self.t = cuda(tgt)
        self.T, _, self.B = self.x.shape
        Lc = binding.lib().wdf_ss_nl_step_chunk_len(self.T, K)
        self.K = -(-self.T // Lc)
        self.groups = -(-self.B // (128 if self.B % 2 == 0 else 64))
        self.cold = self.lin.cold_warmup() if cold is None else cold
        self.ws = binding.ss_nl_eval_plan(self.ns, self.ni, self.B, self.T, self.K, self.cold, max(16, min(Lc // 16 * 16, 64)), 16,
                                          max(16, Lc // 16 * 16), 1e-6, self.x)

    def run(self, skip=0, store_y=True, y=None):
        self.lin.probe()
        r = self.b.ss_nl_eval(self.x, self.lin.coef, self.lin.pb.block, self.lin.n_tree, self.ns, self.ni, self.t, self.K, self.ws, skip=skip,
                              n_up=self.n[0], n_down=self.n[1], y=y, store_y=store_y)
        torch.cuda.synchronize()
        return r

    def ctl(self):
        return self.b.ss_nl_eval_read(self.ws)

    def set(self, field, value):
        self.b.ss_nl_eval_set(self.ws, field, value)


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)))


def check(section, case, r, yref, tgt, skip, bound, y=True):
    B, T = yref.shape[1], yref.shape[0]
    Sr, Er, l3r, _ = esr_terms(yref, tgt, skip)
    assert Er / (B * (T - skip)) > 1e-4, (case, Er)               # (the oracle's: relative bounds on E and esr mean something)
    S, E = (float(v) for v in r["sums"].cpu().numpy())
    l3 = r["loss3"].cpu().numpy().astype(np.float64)
    e_y = float(np.max(np.abs(r["y"].cpu().numpy() - yref))) if y else 0.0
    e_S, e_E, e_m, e_t = abs(S - Sr) / Sr, abs(E - Er) / Er, abs(l3[0] - l3r[0]) / l3r[0], rel(l3[1:], l3r[1:])
    print(f"FIG {section} | {case} skip {skip} | y={e_y:.2e} S={e_S:.2e} E={e_E:.2e} mse={e_m:.2e} esr={e_t:.2e} | {l3} / {l3r}")
    assert e_y < bound["y"], (case, e_y)
    assert e_S < bound["sums"] and e_E < bound["sums"], (case, e_S, e_E)
    assert e_m < bound["mse"], (case, e_m)
    assert e_t < bound["terms"], (case, e_t)


def same_bits(a, b):
    return torch.equal(a["sums"], b["sums"]) and torch.equal(a["loss3"], b["loss3"])


# ---- first call against the oracle ------------------------------------------------------------------------------------------
SHAPES = [(1, 40, 1), (70, 1000, 7), (131, 1501, 12), (130, 1501, 12), (64, 520, 8)]


@pytest.mark.parametrize("B,T,K", SHAPES, ids=[f"B{b}-T{t}-K{k}" for b, t, k in SHAPES])
@pytest.mark.parametrize("tree", TREES, ids=lambda t: f"{t[0]}{t[1]}")
def test_first_call_against_the_oracle(wdf, tree, B, T, K):
    """Odd and even B (both lane widths), T % 8 != 0 (the tail block), a last chunk shorter than the others, one case with
    T < 64; n_up != n_down; skip 0, 50 (inside a block) and T - 1; with and without the y store: without, sums and loss3 are the
    storing call's bit for bit (a workspace planned alike: both are first calls) -- with the register report, the evidence that
    STORE_Y = false is the same pass less the store.  A y handed in with store_y=False is refused before any launch, and the pass
    is then called with y = NULL: that a sentinel-filled buffer of y's size stays as it was shows only that nothing wild is written."""
    n = N_OF[tree]
    x, tgt, yref = case_at_the_trees_own_values(tree, B, T, n, 100 * B + T + 10 * tree[0] + tree[1])
    circ, _ = build_tree(wdf, tree)
    for skip in sorted({0, min(50, T - 1), T - 1}):
        p = Pass(circ, x, tgt, K, n)
        assert p.K == {520: 6}.get(T, K)
        r = p.run(skip)
        ctl = p.ctl()
        assert ctl["call"] == 1 and ctl["w_used"] == p.cold and ctl["gated_groups"] == 0 and ctl["n_bad"] == 0, ctl
        check("first", f"{tree} B {B} T {T} K {p.K}", r, yref, tgt, skip, bound_of(tree))
        q = Pass(circ, x, tgt, K, n)
        sentinel = torch.full((T, B), -77.25, dtype=torch.float32, device="cuda")
        with pytest.raises(q.b.WdfHipError):
            q.run(skip, store_y=False, y=sentinel)
        r0 = q.run(skip, store_y=False)
        assert r0["y"] is None and bool(torch.all(sentinel == -77.25))
        assert same_bits(r, r0), (tree, B, T, skip)


def test_a_y_of_another_shape_a_short_workspace_and_wrong_sums_are_refused(wdf):
    tree, B, T, K = (1, 1), 70, 1000, 7
    x, tgt, _ = case_at_the_trees_own_values(tree, B, T, N_OF[tree], 100 * B + T + 11)
    circ, _ = build_tree(wdf, tree)
    p = Pass(circ, x, tgt, K, N_OF[tree])
    E = p.b.WdfHipError
    args = (p.x, p.lin.coef, p.lin.pb.block, p.lin.n_tree, 1, 1, p.t, p.K)
    with pytest.raises(E):
        p.b.ss_nl_eval(*args, p.ws, y=torch.zeros((B, T), device="cuda"))
    with pytest.raises(E):
        p.b.ss_nl_eval(*args, p.ws, y=torch.zeros((T, B), dtype=torch.float64, device="cuda"))
    with pytest.raises(E):
        p.b.ss_nl_eval(*args, p.ws, y=torch.zeros((T, B)))
    with pytest.raises(E):
        p.b.ss_nl_eval(*args, p.ws[:1024])
    with pytest.raises(E):
        p.b.ss_nl_eval(*args, p.ws[::2])
    with pytest.raises(E):
        p.b.ss_nl_eval(*args, p.ws, sums=torch.zeros(2, device="cuda"))
    with pytest.raises(E):
        p.b.ss_nl_eval(*args, p.ws, loss3=torch.zeros(2, device="cuda"))
    assert p.ctl()["call"] == 0


# ---- the root tiers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l0,tier", TIERS)
def test_root_tiers_against_the_oracle(wdf, l0, tier):
    tree, B, T, K = (1, 1), 130, 512, 4
    theta = tier_theta(l0, 1)
    circ, params = hpf(wdf, 1, 1, theta=theta)
    circ.to_device()
    assert np.array_equal(theta_of(params), theta)
    x, tgt = data(tree, B, T, 5500 + B)
    yref = oracle_y(tree, theta, x, (1, 1))
    p = Pass(circ, x, tgt, K, (1, 1))
    for call in range(2):
        r = p.run(50)
        check("tiers", f"l0 {l0} ({tier}) call {call}", r, yref, tgt, 50, FIRST if call == 0 else WIDER)
        assert p.ctl()["gated_groups"] == 0


# ---- calls from snapshots ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secant", [True, False], ids=["secant", "last-snapshot"])
def test_calls_from_snapshots_against_the_oracle(wdf, secant):
    """Three calls with every component value moved by 1e-3 of itself between them: cold, from the last snapshot, from the
    secant (or, with the switch off, from the last snapshot again); each against the oracle at that call's values."""
    tree, B, T, K = (1, 1), 128, 2048, 8
    n = (1, 1)
    circ, params = build_tree(wdf, tree)
    x, tgt = data(tree, B, T, 8800)
    p = Pass(circ, x, tgt, K, n)
    if not secant:
        p.set(p.b.NL_EVAL_SECANT, 0)
    used = []
    for call in range(3):
        if call:
            for v in params:
                v.assign(float(v) * 1.001)
        yref = oracle_y(tree, theta_of(params), x, n)
        r = p.run(50)
        ctl = p.ctl()
        print(f"call {call}: {ctl}")
        used.append(ctl["w_used"])
        check("snapshots", f"secant {secant} call {call}", r, yref, tgt, 50, FIRST if call == 0 else WIDER)
        assert ctl["call"] == call + 1 and ctl["gated_groups"] == 0
    assert used[2] <= used[0], used


# ---- repair -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", [False, True], ids=["general", "sym"])
@pytest.mark.parametrize("B", [130, 131])
@pytest.mark.parametrize("tree", TREES, ids=lambda t: f"{t[0]}{t[1]}")
def test_the_repair_on_every_instantiation(wdf, tree, B, sym):
    """A tolerance nothing meets: every group is re-run by its finishing wave from the first boundary on; then the tolerance
    back, and a call that starts from the snapshots the repair rewrote.  sym: n_up == n_down, the SYM instantiations of the chunk
    kernel (and with them the LEAN / FAST root tiers) on every tree and both lane widths; else n_up != n_down."""
    T, K, n = 1000, 7, ((1, 1) if sym else N_OF[tree])
    x, tgt, yref = case_at_the_trees_own_values(tree, B, T, n, 3300 + 10 * tree[0] + tree[1] + B)
    circ, _ = build_tree(wdf, tree)
    p = Pass(circ, x, tgt, K, n)
    p.set(8, -1.0)
    r = p.run(50)
    ctl = p.ctl()
    print(f"repaired: {ctl}")
    check("repair", f"{tree} B {B} repaired", r, yref, tgt, 50, bound_of(tree))
    assert ctl["gated_groups"] == p.groups and ctl["n_bad"] > 0
    p.set(8, 1e-6)
    r = p.run(50)
    ctl = p.ctl()
    print(f"after: {ctl}")
    check("repair", f"{tree} B {B} after", r, yref, tgt, 50, WIDER)
    assert ctl["gated_groups"] == 0 and ctl["n_bad"] == 0 and ctl["have_snap"] == 1


def test_some_groups_repaired_and_others_not(wdf):
    """Cold warm-up 0: every chunk starts from z = 0 at its own first sample.  The first group's input is identically zero, so
    its states are zero and its boundaries miss by exactly 0; the other group misses and is re-run."""
    tree, B, T, K, n = (1, 1), 256, 1000, 7, (1, 1)
    x, tgt = data(tree, B, T, 4400 + B)
    x[:128] = 0.0
    circ, params = build_tree(wdf, tree)
    yref = oracle_y(tree, theta_of(params), x, n)
    assert np.all(yref[:, :128] == 0.0)
    p = Pass(circ, x, tgt, K, n, cold=0)
    r = p.run(0)
    ctl = p.ctl()
    print(ctl)
    assert bool(torch.all(r["y"][:, :128] == 0.0))
    check("partial", "B 256", r, yref, tgt, 0, FIRST)
    assert ctl["w_used"] == 0 and 1 <= ctl["gated_groups"] <= p.groups - 1 and ctl["n_bad"] > 0


# ---- the same bits twice ------------------------------------------------------------------------------------------------------
def test_the_same_calls_give_the_same_bits(wdf):
    """Two workspaces planned alike, the same sequence of calls on each (cold, a repaired call, two from snapshots)."""
    tree, B, T, K, n = (2, 1), 130, 1000, 7, (1, 1)
    x, tgt, _ = case_at_the_trees_own_values(tree, B, T, n, 9900)
    circ, _ = build_tree(wdf, tree)
    runs = []
    for _ in range(2):
        p = Pass(circ, x, tgt, K, n)
        out = []
        for call in range(4):
            p.set(8, -1.0 if call == 1 else 1e-6)
            r = p.run(50)
            out.append((r["sums"].clone(), r["loss3"].clone(), r["y"].clone()))
        runs.append(out)
    for a, b in zip(*runs):
        assert all(torch.equal(u, v) for u, v in zip(a, b))


# ---- path against path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
def test_against_the_training_step(wdf, K):
    """y of the pass against y of wdf_ss_nl_step_mse at the same parameters, both cold with K chunks: 2e-6 V; S: 1e-5."""
    tree, B, T, n = (1, 1), 128, 2048, (1, 1)
    x, tgt, _ = case_at_the_trees_own_values(tree, B, T, n, 8800)
    circ, _ = build_tree(wdf, tree)
    p = Pass(circ, x, tgt, K, n)
    r = p.run(0)
    lin, b = p.lin, p.b
    ws = lin._plan_nl(B, T, K, p.x.device)
    y = torch.empty((T, B), dtype=torch.float32, device="cuda")
    out = torch.zeros(1 + lin.pb.n, dtype=torch.float32, device="cuda")
    loss = torch.zeros((), dtype=torch.float32, device="cuda")
    b._check(b.lib().wdf_ss_nl_step_mse(b._ptr(p.x), b._ptr(lin.coef), b._ptr(lin.pb.block), b._ptr(lin.jac), lin.n_tree, 1, 1, 1, 1,
                                        b._ptr(p.t), 2.0 / (B * T), b._ptr(y), b._ptr(ws), b._ptr(out), b._ptr(loss), B, T, K, b._stream()),
             "wdf_ss_nl_step_mse")
    torch.cuda.synchronize()
    e_y = float(torch.max(torch.abs(y - r["y"])))
    S, Ss = float(r["sums"][0]), float(out[0])
    print(f"FIG path | K {K} | y={e_y:.2e} S={abs(S - Ss) / Ss:.2e} bit for bit: {bool(torch.equal(y, r['y']))}")
    assert e_y < 2e-6 and abs(S - Ss) / Ss < 1e-5
