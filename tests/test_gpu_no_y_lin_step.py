"""GPU: the linear one-pass steps WITHOUT the y store (wdf_ss_lin_step_mse_noy / _esr_noy; binding.ss_lin_step_mse / _esr with
store_y=False) at kernel level, against the references and at the bounds of tests/test_gpu_ss_lin_step_kernel.py (MSE:
tests/ss_lin_ref.py) and tests/test_gpu_ss_lin_esr_step.py (MSE + ESR: tests/ss_lin_esr_ref.py).

Those modules' own `check` functions judge every output: SSE / S / E at 1e-5, gcoef at 4e-6 mag_i, out / sums / g / loss3 as they
form them, zT at 3e-6 max(1, max |z|).  Their y row has nothing to judge here -- the call returns None in y's place, which is
asserted -- and is handed the reference's own y.

  MSE        every instantiation (SHAPES_A x TREES: both lane widths, dead lanes, short last chunks); the drop to one sequence per
             lane when x / target, or only z0, sit at 4 mod 8; the carried state (a second call from the first call's zT); 64
             chunks at (65, 2048); 1 and 15 parameters
  MSE + ESR  that module's sections A (with the 4 mod 8 case), B (skip positions), C (chunk geometry), D (the state handed over)
             and E's parameter counts
  both       the ticket left 0; a reused workspace gives the same bits; one planned workspace serves a storing call followed by a
             no-y call; against the storing step on the same inputs the results are compared bit for bit and the outcome printed
             (equality is not required: dropping a use of y may change how the compiler contracts a multiply-add).  On one MI355X
             all 60 such comparisons printed True
"""
import gc

import numpy as np
import pytest

import ss_lin_esr_ref as E
import ss_lin_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_ss_lin_esr_step as KE     # noqa: E402  (check, one_float_in and the bounds of the storing steps' modules)
import test_gpu_ss_lin_step_kernel as KM  # noqa: E402

cuda, one_float_in = KM.cuda, KM.one_float_in


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def mse(c, n_chunks, n_params=3, want_zT=False, z0="case", x=None, target=None, ws=None, store_y=False):
    from wdf_hip import binding as wb
    jac = KM.jac_of(c, n_params)
    z0 = (None if c.z0 is None else cuda(c.z0)) if isinstance(z0, str) else z0
    res = wb.ss_lin_step_mse(cuda(c.x) if x is None else x, cuda(c.coef), cuda(jac, np.float64), cuda(c.target) if target is None else target,
                             c.gscale, n_chunks, z0=z0, want_zT=want_zT, want_gcoef=True, ws=ws, store_y=store_y)
    return res, jac


def esr(c, n_chunks, want_zT=False, z0="case", misaligned=False, ws=None, store_y=False, finish=True):
    from wdf_hip import binding as wb
    z0 = (None if c.z0 is None else cuda(c.z0)) if isinstance(z0, str) else z0
    xs = one_float_in(c.x) if misaligned else cuda(c.x)
    tg = one_float_in(c.target) if misaligned else cuda(c.target)
    return wb.ss_lin_step_esr(xs, cuda(c.coef), cuda(c.jac, np.float64), tg, c.skip, n_chunks, n_global=c.n_global, z0=z0, want_zT=want_zT,
                              want_gcoef=True, ws=ws, finish=finish, store_y=store_y)


def with_ref_y(res, ref):
    """The call left no y (asserted); the storing modules' check gets the reference's own in its place."""
    assert res["y"] is None
    return dict(res, y=torch.as_tensor(ref.y))


def check_mse(section, label, c, res, jac):
    return KM.check(section, label + " no-y", c, with_ref_y(res, c.ref()), jac)


def check_esr(section, label, c, res):
    return KE.check(section, label + " no-y", c, with_ref_y(res, c.ref()))


def same_bits(a, b, keys):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in keys)


def lanes(B):
    return "two" if B % 2 == 0 else "one"


# ---- MSE ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,k", R.SHAPES_A, ids=[f"{lanes(B)}-B{B}-T{T}-k{k}" for B, T, k in R.SHAPES_A])
@pytest.mark.parametrize("ns,ni", R.TREES, ids=[f"ns{a}-ni{b}" for a, b in R.TREES])
def test_mse_every_instantiation(ns, ni, B, T, k):
    c = R.case(ns, ni, "plain", B, T)
    res, jac = mse(c, k, want_zT=True)
    assert (res["zT"] is None) == (ns == 0)
    check_mse("A", f"{lanes(B)} per lane k={k}", c, res, jac)
    assert int(res["ws"][:4].view(torch.int32)[0]) == 0
    sto, _ = mse(c, k, want_zT=True, store_y=True)
    print(f"BITS mse {c} k={k}: no-y == storing: {same_bits(res, sto, ('out', 'loss', 'gcoef', 'zT'))}")


@pytest.mark.parametrize("what", ["x_target", "z0"])
@pytest.mark.parametrize("ns,ni", R.MISALIGNED_A, ids=[f"ns{a}-ni{b}" for a, b in R.MISALIGNED_A])
def test_mse_even_batch_drops_to_one_per_lane_when_a_pointer_is_4_mod_8(ns, ni, what):
    if what == "z0":
        c = R.case(ns, ni, "plain", 64, 100, True)
        res, jac = mse(c, 4, want_zT=True, z0=one_float_in(c.z0))
    else:
        c = R.case(ns, ni, "plain", 64, 100)
        res, jac = mse(c, 4, want_zT=True, x=one_float_in(c.x), target=one_float_in(c.target))
    check_mse("A", f"4 mod 8: {what}", c, res, jac)


@pytest.mark.parametrize("B", R.BATCHES, ids=["one-B65", "two-B130"])
@pytest.mark.parametrize("ns,ni", R.TREES_C, ids=[f"ns{a}-ni{b}" for a, b in R.TREES_C])
def test_mse_two_calls_with_the_state_handed_over(ns, ni, B):
    whole, first, second = R.carried(ns, ni, B)
    z0 = cuda(first.z0)
    before = z0.clone()
    res1, jac1 = mse(first, 3, want_zT=True, z0=z0)
    check_mse("C", "first half", first, res1, jac1)
    assert torch.equal(z0.view(torch.int32), before.view(torch.int32)) and res1["zT"].data_ptr() != z0.data_ptr()
    res2, jac2 = mse(second, 3, want_zT=True, z0=res1["zT"])
    check_mse("C", "second half from the first's zT", second, res2, jac2)
    wref = whole.ref()
    assert np.max(np.abs(res2["zT"].cpu().numpy() - wref.zT)) <= KM.B_Y * max(1.0, np.max(np.abs(wref.zT)))


@pytest.mark.parametrize("ns,ni", R.TREES_B, ids=[f"ns{a}-ni{b}" for a, b in R.TREES_B])
def test_mse_64_chunks(ns, ni):
    c = R.case(ns, ni, "plain", 65, 2048)
    res, jac = mse(c, 64)
    check_mse("B", "L=32 K=64", c, res, jac)


@pytest.mark.parametrize("n_params", [1, 15])
def test_mse_parameter_counts_ticket_and_workspaces(n_params):
    """1 and 15 parameters; the ticket (the workspace's first word) 0 after each call; the same bits from a second call on the
    workspace; ONE workspace, zeroed once, serves a storing call and then a no-y call, which gives the bits it gave before"""
    c = R.case(2, 2, "plain", 130, 257)
    res, jac = mse(c, 3, n_params=n_params, want_zT=True)
    check_mse("E", f"n_params={n_params} call 1", c, res, jac)
    ws = res["ws"]
    assert int(ws[:4].view(torch.int32)[0]) == 0
    keep = {k: res[k].clone() for k in ("out", "loss", "gcoef", "zT")}
    res2, _ = mse(c, 3, n_params=n_params, want_zT=True, ws=ws)
    assert res2["ws"].data_ptr() == ws.data_ptr() and int(ws[:4].view(torch.int32)[0]) == 0 and same_bits(res2, keep, keep)
    from wdf_hip import binding as wb
    planned = torch.zeros((wb.lib().wdf_ss_lin_step_ws_bytes(2, 2, 130, 257, 3),), dtype=torch.uint8, device="cuda")
    sto, jac_s = mse(c, 3, n_params=n_params, want_zT=True, ws=planned, store_y=True)
    KM.check("E", "storing call on the shared workspace", c, sto, jac_s)
    res3, _ = mse(c, 3, n_params=n_params, want_zT=True, ws=planned)
    assert res3["y"] is None and int(planned[:4].view(torch.int32)[0]) == 0 and same_bits(res3, keep, keep)
    check_mse("E", f"n_params={n_params} behind a storing call", c, res3, jac)


# ---- MSE + ESR ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,k,mis", KE.CASES_A,
                         ids=[f"B{B}-T{T}-k{k}-" + ("one-4mod8" if m else lanes(B)) for B, T, k, m in KE.CASES_A])
@pytest.mark.parametrize("ns,ni", R.TREES, ids=[f"ns{a}-ni{b}" for a, b in R.TREES])
def test_esr_every_instantiation(ns, ni, B, T, k, mis):
    c = E.case(ns, ni, B, T, E.SKIP_A)
    res = esr(c, k, want_zT=True, misaligned=mis)
    assert (res["zT"] is None) == (ns == 0)
    check_esr("A", ("4 mod 8 " if mis else "") + f"k={k}", c, res)
    assert int(res["ws"][:4].view(torch.int32)[0]) == 0
    sto = esr(c, k, want_zT=True, misaligned=mis, store_y=True)
    print(f"BITS esr {c} k={k}: no-y == storing: {same_bits(res, sto, ('sums', 'g', 'loss3', 'gcoef', 'zT'))}")


@pytest.mark.parametrize("ns,ni,B,T,k,skip", KE.CASES_B, ids=[f"ns{a}-ni{b}-B{B}-T{T}-skip{s}" for a, b, B, T, k, s in KE.CASES_B])
def test_esr_skip_positions(ns, ni, B, T, k, skip):
    c = E.case(ns, ni, B, T, skip)
    check_esr("B", f"k={k}", c, esr(c, k, want_zT=True))


@pytest.mark.parametrize("T,k", E.GEOM_C, ids=[f"T{T}-k{k}" for T, k in E.GEOM_C])
@pytest.mark.parametrize("B", E.BATCHES_C, ids=["one-B65", "two-B130"])
def test_esr_chunk_geometry(B, T, k):
    c = E.case(2, 1, B, T, E.skip_c(T))
    check_esr("C", f"asked {k}", c, esr(c, k))


def test_esr_two_calls_with_the_state_handed_over():
    long, first, second = E.carried()
    z0 = cuda(first.z0)
    before = z0.clone()
    r1 = esr(first, 3, want_zT=True, z0=z0)
    check_esr("D", "first half", first, r1)
    assert torch.equal(z0.view(torch.int32), before.view(torch.int32)) and r1["zT"].data_ptr() != z0.data_ptr()
    r2 = esr(second, 3, want_zT=True, z0=r1["zT"])
    check_esr("D", "second half from the first's zT", second, r2)


@pytest.mark.parametrize("n_params", E.PARAMS_E)
def test_esr_parameter_counts_ticket_and_workspaces(n_params):
    c = E.case(2, 2, 130, 257, E.SKIP_E, n_params=n_params)
    res = esr(c, 3, want_zT=True)
    check_esr("E", f"n_params={n_params} call 1", c, res)
    ws = res["ws"]
    assert int(ws[:4].view(torch.int32)[0]) == 0
    keep = {k: res[k].clone() for k in ("sums", "g", "loss3", "gcoef", "zT")}
    res2 = esr(c, 3, want_zT=True, ws=ws)
    assert res2["ws"].data_ptr() == ws.data_ptr() and int(ws[:4].view(torch.int32)[0]) == 0 and same_bits(res2, keep, keep)
    from wdf_hip import binding as wb
    planned = torch.zeros((wb.lib().wdf_ss_lin_step_esr_ws_bytes(2, 2, 130, 257, 3),), dtype=torch.uint8, device="cuda")
    sto = esr(c, 3, want_zT=True, ws=planned, store_y=True)
    KE.check("E", "storing call on the shared workspace", c, sto)
    res3 = esr(c, 3, want_zT=True, ws=planned)
    assert res3["y"] is None and int(planned[:4].view(torch.int32)[0]) == 0 and same_bits(res3, keep, keep)
    # the two-stage form: sums only, then the finish export that serves both steps
    half = esr(c, 3, finish=False)
    assert half["y"] is None and half["g"] is None and half["loss3"] is None and same_bits(half, keep, ("sums",))
    g2, l2 = wb.ss_lin_esr_finish(half["sums"], c.n_global if c.n_global is not None else c.ref().n)
    assert torch.allclose(g2, keep["g"], rtol=1e-6, atol=0) and torch.allclose(l2, keep["loss3"], rtol=1e-6, atol=0)
