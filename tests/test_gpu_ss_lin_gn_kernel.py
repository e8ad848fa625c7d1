"""GPU: the Gauss-Newton form of the linear one-pass step (csrc/wdf_ss_lin_gn.h: wdf_ss_lin_step_gn) at kernel level, through
binding.ss_lin_step_gn, against tests/ss_lin_gn_ref.py only (the recursion restated directly in float64; pinned on the CPU by
tests/test_ss_lin_gn_cpu.py).

Cases (ss_lin_gn_ref.gpu_case_keys): all six trees at (B, T, chunks) = (1, 40, 1), (65, 100, 4), (130, 257, 3), (2, 33, 2) -- dead
lanes, a second wave with one live lane, both lane widths, a ragged last chunk; a pointer at 4 mod 8 dropping to one sequence per
lane; (2,2) at even B (one per lane by construction); z0 and zT; (2,1) B = 65, T = 2048 in 64 chunks; `slow` poles; n_params 1, 2
and 15 (120 entries of H: more than one trip of the finishing wave); two calls on one workspace giving the same bits, the ticket 0.

Bounds (none taken from what the kernel gives):
  hcoef_ij     B_H magH_ij                    magH_ij = sum |d_i| |d_j|.  The fp32 restatement stays within 5.64e-7 magH of the fp64 one
                                              over these very cases (asserted on the CPU under FLOOR = 5.7e-7); B_H = 8 x FLOOR
                                              + 32 x 2^-24 (the kernel's fp32 block sum) = 6.5e-6
  H_qr         sum_ij B_H magH_ij |J_iq| |J_jr| (x gscale; the contraction is in fp64)
  y, SSE, loss, gradient, zT                  the MSE step's documented bounds (tests/test_gpu_ss_lin_step_kernel.py: 3e-6, 1e-5, 4e-6 mag)
Bit for bit against binding.ss_lin_step_mse at the same n_chunks: y and zT always; out[0 : 1 + P], rounded to float as the MSE
step rounds, where both ran at the same lane width (everywhere but (2,2) at even B).

Every check prints `FIG | <case> | ...` before it asserts, each error divided by its bound (run with -s).

Measured on an MI355X (worst figure of each column, error / bound; 33 tests, 36 FIG lines, all passing, 3 s in all):
  hcoef 0.205 ((2,2) B = 1, T = 40: 40 rows, nothing averages out; `slow` (1,1) in 8 chunks 0.159)   H 0.124 (`slow` (1,1) in 8 chunks)
  y 0.051   sse 0.016   loss 0.020   g 0.045 (`slow` (1,1))   zT 0.080 ((2,2) B = 130 from z0)
  n_params 1, 2, 15: H 0.001, 0.001, 0.002; calls 2 and 3 on the first call's workspace give call 1's bits, the ticket 0
  y, zT bit for bit the MSE step's in every case; out[0 : 1 + P] and loss in every case of equal lane width
"""
import gc

import numpy as np
import pytest

import ss_lin_gn_ref as G
import ss_lin_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B_Y, B_SSE, B_G = 3e-6, 1e-5, 4e-6                                # tests/test_gpu_ss_lin_step_kernel.py's


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def cuda(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def one_float_in(a):
    """The array on the device as a dense view that starts one float into its storage: 4 mod 8 bytes."""
    a = np.asarray(a, dtype=np.float32)
    base = torch.empty((a.size + 1,), dtype=torch.float32, device="cuda")
    v = base[1:].view(*a.shape)
    v.copy_(torch.as_tensor(a))
    assert v.is_contiguous() and v.data_ptr() % 8 == 4
    return v


def jac_of(c, n_params):
    return np.random.default_rng([c.ns, c.ni, c.B, c.T, n_params]).standard_normal((R.ncoef(c.ns, c.ni) + 1, n_params))


def ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0


def run_both(key, n_chunks, n_params=3, want_zT=False, x=None, target=None, y=None, ws=None):
    """one launch of the Gauss-Newton step and one of the MSE step on the same inputs -> (gn dict, mse dict, jac)"""
    from wdf_hip import binding as wb
    c = R.case(*key)
    jac = jac_of(c, n_params)
    args = dict(x_tm=cuda(c.x) if x is None else x, coef=cuda(c.coef), jac=cuda(jac, np.float64),
                target=cuda(c.target) if target is None else target, gscale=c.gscale, n_chunks=n_chunks,
                z0=None if c.z0 is None else cuda(c.z0), want_zT=want_zT)
    gn = wb.ss_lin_step_gn(**args, want_hcoef=True, ws=ws, y=y)
    mse = wb.ss_lin_step_mse(**args, y=None if y is None else torch.empty_like(y))
    return gn, mse, jac


def check(label, key, gn, mse, jac, same_width=True):
    """every output of one call against the reference, and against the MSE step bit for bit; prints the figures, then asserts"""
    c = R.case(*key)
    ns, ni = c.ns, c.ni
    ref = G.ref(key)
    gs = float(np.float32(c.gscale))
    P = jac.shape[1]
    y = gn["y"].cpu().numpy().astype(np.float64)
    out = gn["out"].cpu().numpy()
    assert out.dtype == np.float64 and out.shape == (1 + P + P * (P + 1) // 2,)
    rows = R.rows(ns, ni)
    mag = R.case(*key).ref().mag
    f = {"y": ratio(np.max(np.abs(y - ref.y)), B_Y * max(1.0, np.max(np.abs(ref.y)))),
         "sse": ratio(abs(out[0] - ref.sse), B_SSE * ref.sse),
         "loss": ratio(abs(float(gn["loss"].cpu()) - 0.5 * gs * ref.sse), B_SSE * 0.5 * gs * ref.sse)}
    want = ref.g @ jac[rows]
    f["g"] = ratio(np.abs(out[1:1 + P] - want), (B_G * mag) @ np.abs(jac[rows]))
    f["hcoef"] = ratio(np.abs(gn["hcoef"].cpu().numpy() - G.upper(ref.Hc)), G.B_H * G.upper(ref.magH))
    Hw, Hb = G.chain(ns, ni, ref.Hc, jac, c.gscale), G.chain_bound(ns, ni, ref.magH, jac, G.B_H, c.gscale)
    f["H"] = ratio(np.abs(out[1 + P:] - G.upper(Hw)), G.upper(Hb))
    H = gn["H"].cpu().numpy()
    if gn["zT"] is not None:
        f["zT"] = ratio(np.max(np.abs(gn["zT"].cpu().numpy().astype(np.float64) - ref.zT)), B_Y * max(1.0, np.max(np.abs(ref.zT))))
    print(f"FIG | {label} {c} P={P} | " + " ".join(f"{k}={v:.3f}" for k, v in f.items()))
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(out))
    assert all(v <= 1.0 for v in f.values()), (label, repr(c), f)
    assert H.shape == (P, P) and np.array_equal(H, H.T) and np.array_equal(G.upper(H), out[1 + P:])
    # bit for bit against the MSE step
    assert torch.equal(gn["y"].view(torch.int32), mse["y"].view(torch.int32)), label
    assert (gn["zT"] is None) == (mse["zT"] is None)
    if gn["zT"] is not None:
        assert torch.equal(gn["zT"].view(torch.int32), mse["zT"].view(torch.int32)), label
    if same_width:
        assert torch.equal(gn["out"][:1 + P].float().view(torch.int32), mse["out"].view(torch.int32)), label
        assert torch.equal(gn["loss"].view(torch.int32), mse["loss"].view(torch.int32)), label
    assert int(gn["ws"][:4].view(torch.int32)[0]) == 0            # the ticket
    return f


def lanes(ns, ni, B):
    return "one" if (B % 2 or (ns, ni) == (2, 2)) else "two"


@pytest.mark.parametrize("B,T,k", G.SHAPES, ids=[f"B{B}-T{T}-k{k}" for B, T, k in G.SHAPES])
@pytest.mark.parametrize("ns,ni", R.TREES, ids=[f"ns{a}-ni{b}" for a, b in R.TREES])
def test_every_instantiation(ns, ni, B, T, k):
    """(2,2) at even B runs one sequence per lane where the MSE step runs two: y and zT still agree bit for bit"""
    from wdf_hip import binding as wb
    key = (ns, ni, "plain", B, T, False)
    gn, mse, jac = run_both(key, k, want_zT=True)
    assert (gn["zT"] is None) == (ns == 0)
    K = wb.chunk_geom(T, k, 32)[1]
    assert gn["ws"].numel() == wb.lib().wdf_ss_lin_step_gn_ws_bytes(ns, ni, B, T, K)
    check(f"{lanes(ns, ni, B)} per lane k={k}", key, gn, mse, jac, same_width=not ((ns, ni) == (2, 2) and B % 2 == 0))


def test_even_batch_drops_to_one_per_lane_when_a_pointer_is_4_mod_8():
    key = G.MISALIGNED
    c = R.case(*key)
    y = one_float_in(np.zeros((c.T, c.B)))
    gn, mse, jac = run_both(key, 4, want_zT=True, x=one_float_in(c.x), target=one_float_in(c.target), y=y)
    assert gn["y"].data_ptr() == y.data_ptr()
    check("4 mod 8", key, gn, mse, jac)


@pytest.mark.parametrize("B", G.STATE_BATCHES)
@pytest.mark.parametrize("ns,ni", G.STATE_TREES, ids=[f"ns{a}-ni{b}" for a, b in G.STATE_TREES])
def test_initial_and_final_state(ns, ni, B):
    key = (ns, ni, "plain", B, 257, True)
    gn, mse, jac = run_both(key, 3, want_zT=True)
    assert gn["zT"] is not None and tuple(gn["zT"].shape) == (ns, B)
    check("z0 and zT", key, gn, mse, jac, same_width=not ((ns, ni) == (2, 2) and B % 2 == 0))


def test_the_longest_walk():
    gn, mse, jac = run_both(G.LONG_WALK, 64)
    check("64 chunks", G.LONG_WALK, gn, mse, jac)


@pytest.mark.parametrize("key,k", G.SLOW, ids=[f"ns{k[0]}-ni{k[1]}-B{k[3]}-k{n}" for k, n in G.SLOW])
def test_slow_poles(key, k):
    gn, mse, jac = run_both(key, k)
    check(f"slow k={k}", key, gn, mse, jac)


@pytest.mark.parametrize("n_params", G.PARAMS)
def test_parameter_counts_and_a_reused_workspace(n_params):
    """two more calls on the first call's workspace give the same bits; the ticket (the workspace's first word) is 0 after each"""
    key = G.PARAMS_CASE
    gn, mse, jac = run_both(key, 3, n_params=n_params)
    check(f"n_params={n_params} call 1", key, gn, mse, jac, same_width=False)
    ws = gn["ws"]
    keep = {k: gn[k].clone() for k in ("y", "out", "loss", "hcoef", "H")}
    for n in (2, 3):
        gn, mse, _ = run_both(key, 3, n_params=n_params, ws=ws)
        assert gn["ws"].data_ptr() == ws.data_ptr() and int(ws[:4].view(torch.int32)[0]) == 0
        for k, v in keep.items():
            assert torch.equal(gn[k].view(torch.int64 if v.dtype == torch.float64 else torch.int32),
                               v.view(torch.int64 if v.dtype == torch.float64 else torch.int32)), (k, n)
    check(f"n_params={n_params} call 3", key, gn, mse, jac, same_width=False)


def test_wrapper_refuses_shapes_that_do_not_fit():
    from wdf_hip import binding as wb
    c = R.case(1, 1, "plain", 65, 100)
    x, coef, tgt = cuda(c.x), cuda(c.coef), cuda(c.target)
    jac = cuda(jac_of(c, 3), np.float64)
    good = dict(x_tm=x, coef=coef, jac=jac, target=tgt, gscale=c.gscale, n_chunks=4)
    for over in (dict(coef=coef[:7]), dict(jac=jac[:5].contiguous()), dict(jac=cuda(np.zeros((9, 16)), np.float64)), dict(jac=jac.float()),
                 dict(target=tgt[:99]), dict(z0=cuda(np.zeros((2, 65)))), dict(y=cuda(np.zeros((100, 64)))),
                 dict(ws=torch.zeros(wb.lib().wdf_ss_lin_step_ws_bytes(1, 1, 65, 100, 4), dtype=torch.uint8, device="cuda")),
                 dict(n_chunks=0)):
        with pytest.raises(wb.WdfHipError):
            wb.ss_lin_step_gn(**{**good, **over})
    res = wb.ss_lin_step_gn(**good)
    assert tuple(res["y"].shape) == (100, 65) and res["hcoef"] is None and res["zT"] is None and tuple(res["H"].shape) == (3, 3)
