"""GPU: the input gradient of the static state-space kernels at kernel level, through binding.ss_bwd_gx (csrc/wdf_statespace.h:
ss_bwd_gx_kernel, ss_bwd_gx_lamin_kernel), against the float64 reference of tests/ss_gx_ref.py.

Sequential form: every (ns, ni) in 0..4 x 1..2 and every root it is built for, the "plain" family at ss_static_ref.SHAPES_A --
(65, 43) a dead-lane wave and a tail, (65, 44) whole blocks with 16-byte loads, (1, 1) and (1, 7) calls shorter than a block,
(130, 8) three waves of one block, (64, 44) with x one float into its storage (no 16-byte loads).
Chunked form: behind binding.ss_bwd_tp at ss_static_ref.GEOM_C, families "plain" and "fast" -- a last partial chunk with a tail
(131 in 3), whole chunks (128 in 4), a second chunk of 4 steps (44 in 2), a second chunk of one step (9 in 2), more chunks asked
for than fit (131 in 16 -> 9), one chunk through the chunked entry (131 in 1).

Bounds, per unit of the channel's magnitude (ss_gx_ref.channel_mag: the adjoint walk on absolute values, its maximum over t and b):
ss_static_ref's own -- G_NL under a root, g_lin(ns + ni + 2) on linear trees -- against the reference, and the same between the
chunked and the sequential form (the two differ in the float64 walk's rounding of the entering adjoints to float32 and nothing
else: the gradients' counterpart of Y_PATH).  lamin[0] pushed one chunk further, in float64 from the sweep's own record, is the
gz0 the sweep returned up to the float32 rounding of lamin[0] and of gz0: 2^-23 (|beta| + |Phi| |lamin[0]|).  The sweep's own
results are compared bit for bit with and without the gx call behind it.
"""
import functools
import gc

import numpy as np
import pytest

import ss_gx_ref as G
import ss_static_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENTINEL = -7.0e30
GUARD = 3            # guard rows of ni x B floats in front of gx and behind it


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    yield
    dev.cache_clear()
    stash.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def cuda(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def one_float_in(a):
    a = np.asarray(a, dtype=np.float32)
    base = torch.empty((a.size + 1,), dtype=torch.float32, device="cuda")
    v = base[1:].view(*a.shape)
    v.copy_(torch.as_tensor(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def np64(t):
    return t.cpu().numpy().astype(np.float64)


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def dev(key):
    c = G.case(*key)
    return (cuda(c.x), cuda(c.coef), None if c.root.p is None else cuda(c.root.p), None if c.z0 is None else cuda(c.z0), cuda(c.gy))


def root_kw(c):
    return dict(root_kind=c.root.kind, n_up=c.root.n_up, n_down=c.root.n_down)


@functools.lru_cache(maxsize=None)
def stash(key):
    from wdf_hip import binding as wb
    c = G.case(*key)
    x, coef, rootp, z0, _ = dev(key)
    return wb.ss_fwd(x, coef, c.ns, c.ni, rootp=rootp, want_stash=True, z0=z0, **root_kw(c))[1]


def guarded(c):
    """gx [T,ni,B] as a view into a sentinel-filled buffer with GUARD rows in front and behind -> (whole buffer, view)"""
    row = c.ni * c.B
    buf = torch.full(((c.T + 2 * GUARD) * row,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD * row:(GUARD + c.T) * row].view(c.T, c.ni, c.B)


def check_guarded(buf, view, c):
    row = c.ni * c.B
    assert bool(torch.all(buf[:GUARD * row] == SENTINEL)) and bool(torch.all(buf[(GUARD + c.T) * row:] == SENTINEL)), "gx wrote outside [T][ni][B]"
    assert not bool(torch.any(view == SENTINEL)), "an entry of gx was not written"
    assert bool(torch.all(torch.isfinite(view)))


def figure(c, gx, ref, bound):
    err = np.max(np.abs(np64(gx) - ref), axis=(0, 2))
    return R.ratio(err, bound * G.channel_mag(G.ref(c).mag))


# ---- the sequential form --------------------------------------------------------------------------------------------------------
SEQ = G.seq_keys()


@pytest.mark.parametrize("key", SEQ, ids=[f"ns{k[0]}-ni{k[1]}-{k[2]}-B{k[4]}-T{k[5]}" for k in SEQ])
def test_sequential_form(key):
    from wdf_hip import binding as wb
    c = G.case(*key)
    x, coef, rootp, _, gy = dev(key)
    label = "x 16-byte aligned"
    if (c.B, c.T) == (64, 44):
        x, label = one_float_in(c.x), "x one float in"
    buf, view = guarded(c)
    gx = wb.ss_bwd_gx(x, coef, c.ns, c.ni, stash(key), gy, rootp=rootp, gx=view, **root_kw(c))
    assert gx.data_ptr() == view.data_ptr() and tuple(gx.shape) == (c.T, c.ni, c.B)
    check_guarded(buf, view, c)
    f = figure(c, gx, G.ref(c).gx, G.cap(c))
    print(f"FIG gx seq | {label} {c} | gx={f:.3f}")
    assert f <= 1.0, (repr(c), f)


# ---- the chunked form -----------------------------------------------------------------------------------------------------------
CHUNK = G.chunk_keys()


def records(ws, c, K):
    """Phi [K,ns,ns,B] and beta [K,ns,B] from the workspace wdf_ss_bwd_tp left (rec [K][NREC][B] behind the per-wave sums; NREC
    counts the root's own sums: 5 for two different diodes, else 2)"""
    from wdf_hip import binding as wb
    ns, ni, B = c.ns, c.ni, c.B
    nacc = wb.lib().wdf_ss_ncoef(ns, ni) + (5 if c.root.name == "asym" else 2)
    nrec = ns * ns + ns + nacc * (ns + 1)
    off = wb.lib().wdf_ss_bwd_ws_bytes(ns, ni, B)
    rec = ws[off:off + K * nrec * B * 4].view(torch.float32).view(K, nrec, B)
    return np64(rec[:, :ns * ns]).reshape(K, ns, ns, B), np64(rec[:, ns * ns:ns * ns + ns])


@pytest.mark.parametrize("key", CHUNK, ids=[f"ns{k[0]}-ni{k[1]}-{k[2]}-{k[3]}-B{k[4]}-T{k[5]}-k{k[6]}" for k in CHUNK])
def test_chunked_form(key):
    from wdf_hip import binding as wb
    key, K = key[:6], key[6]
    c = G.case(*key)
    ns, ni, B, T = c.ns, c.ni, c.B, c.T
    x, coef, rootp, _, gy = dev(key)
    zs = stash(key)
    Kc = wb.lib().wdf_ss_tp_chunks(T, K)
    alone = wb.ss_bwd_tp(x, coef, ns, ni, zs, gy, K, rootp=rootp, want_gz0=True, **root_kw(c))
    alone = [None if t is None else t.clone() for t in alone]
    gcoef, groot, gz0, ws = wb.ss_bwd_tp(x, coef, ns, ni, zs, gy, K, rootp=rootp, want_gz0=True, return_ws=True, **root_kw(c))
    lamin = torch.full((max(Kc, 1), ns, B), SENTINEL, dtype=torch.float32, device="cuda")
    buf, view = guarded(c)
    gx = wb.ss_bwd_gx(x, coef, ns, ni, zs, gy, rootp=rootp, n_chunks=K, ws_bwd_tp=ws, gx=view, ws_gx=lamin, **root_kw(c))
    check_guarded(buf, view, c)
    f = {"ref": figure(c, gx, G.ref(c).gx, G.cap(c))}
    gx_seq = wb.ss_bwd_gx(x, coef, ns, ni, zs, gy, rootp=rootp, **root_kw(c))
    f["path"] = figure(c, gx, np64(gx_seq), G.cap(c))
    # the sweep's own results: the bits they are without the gx call
    for a, b_ in zip(alone, (gcoef, groot, gz0)):
        assert (a is None and b_ is None) or bool(torch.equal(bits(a), bits(b_))), "the gx call changed the sweep's results"
    if Kc > 1:
        Phi, beta = records(ws, c, Kc)
        lam = np64(lamin)
        assert not np.any(lam == np.float64(np.float32(SENTINEL))) and np.all(lam[Kc - 1] == 0.0)
        pushed = beta[0] + np.einsum("srb,rb->sb", Phi[0], lam[0])
        room = 2.0 ** -23 * (np.abs(beta[0]) + np.einsum("srb,rb->sb", np.abs(Phi[0]), np.abs(lam[0])))
        f["gz0"] = R.ratio(np.abs(pushed - np64(gz0)), room)
        for k in range(Kc - 1, 0, -1):                                       # every chunk's entering adjoint is the walk's
            want = beta[k] + np.einsum("srb,rb->sb", Phi[k], lam[k])
            assert np.all(np.abs(want - lam[k - 1]) <= 2.0 ** -23 * (np.abs(beta[k]) + np.einsum("srb,rb->sb", np.abs(Phi[k]), np.abs(lam[k]))))
    else:
        assert bool(torch.all(lamin == SENTINEL))                             # one chunk: no entering adjoint is formed
    print(f"FIG gx tp | K={Kc} (asked {K}) {c} | " + " ".join(f"{k}={v:.3f}" for k, v in f.items()))
    assert all(v <= 1.0 for v in f.values()), (repr(c), f)


# ---- refusals leave the buffer alone ---------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_the_sentinel_everywhere():
    from wdf_hip import binding as wb
    key = (2, 1, "pair11", "plain", 65, 44)
    c = G.case(*key)
    x, coef, rootp, _, gy = dev(key)
    zs = stash(key)
    buf, view = guarded(c)
    kw = dict(rootp=rootp, gx=view, **root_kw(c))
    K = wb.lib().wdf_ss_tp_chunks(c.T, 2)
    _, _, _, ws = wb.ss_bwd_tp(x, coef, c.ns, c.ni, zs, gy, K, rootp=rootp, return_ws=True, **root_kw(c))
    calls = [
        lambda: wb.ss_bwd_gx(x, coef, c.ns, c.ni, zs, gy, n_chunks=K, **kw),                              # no sweep workspace
        lambda: wb.ss_bwd_gx(x, coef, c.ns, c.ni, zs, gy, n_chunks=K, ws_bwd_tp=ws[:64], **kw),           # a ws that is too short
        lambda: wb.ss_bwd_gx(x, coef, c.ns, c.ni, zs, gy, n_chunks=K, ws_bwd_tp=ws, ws_gx=ws[:8], **kw),  # lamin too short
        lambda: wb.ss_bwd_gx(x, coef, c.ns, c.ni, zs, gy, n_chunks=0, **kw),
        lambda: wb.ss_bwd_gx(x, coef, c.ns, c.ni, zs[:-1], gy, **kw),                                     # a stash of the wrong shape
        lambda: wb.ss_bwd_gx(x, coef, c.ns, c.ni, zs, gy[:-1], **kw),
        lambda: wb.ss_bwd_gx(x, coef, c.ns, c.ni, zs, gy.double(), **kw),                                 # dtype
        lambda: wb.ss_bwd_gx(x, coef, c.ns, c.ni, zs, gy.cpu(), **kw),                                    # device
        lambda: wb.ss_bwd_gx(x.transpose(0, 1), coef, c.ns, c.ni, zs, gy, **kw),                          # contiguity
        lambda: wb.ss_bwd_gx(x, coef[:-1], c.ns, c.ni, zs, gy, **kw),
        lambda: wb.ss_bwd_gx(x, coef, c.ns, c.ni, zs, gy, rootp=None, gx=view, **root_kw(c)),             # a root without rootp
        lambda: wb.ss_bwd_gx(x, coef, c.ns, c.ni, zs, gy, rootp=rootp, gx=view[:-1], **root_kw(c)),       # gx of the wrong shape
        lambda: wb.ss_bwd_gx(x, coef, c.ns, c.ni, zs, gy, rootp=rootp, gx=view, root_kind=3),             # no such root kind
    ]
    for i, call in enumerate(calls):
        with pytest.raises(wb.WdfHipError):
            call()
        torch.cuda.synchronize()
        assert bool(torch.all(buf == SENTINEL)), f"refused call {i} wrote into gx"
    # ns = 0 has the sequential form only
    k0 = (0, 1, "pair11", "plain", 65, 44)
    c0 = G.case(*k0)
    x0, coef0, rootp0, _, gy0 = dev(k0)
    with pytest.raises(wb.WdfHipError, match="n_chunks"):
        wb.ss_bwd_gx(x0, coef0, 0, 1, None, gy0, rootp=rootp0, n_chunks=2, **root_kw(c0))
    assert not wb.ss_bwd_gx_built(4, 1, wb.ROOT_ASYM_PAIR) and wb.ss_bwd_gx_built(3, 2, wb.ROOT_ASYM_PAIR)
