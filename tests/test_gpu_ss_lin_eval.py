"""GPU: the loss-only evaluation pass of linear trees (csrc/wdf_ss_lin_eval.h: wdf_ss_lin_eval) at kernel level, through
binding.ss_lin_eval, against ss_lin_esr_ref.run(..., grads=False) in float64 (tests/ss_lin_esr_ref.py, pinned on the CPU by
tests/test_ss_lin_esr_ref_cpu.py) and, bit for bit, against the one-pass training steps it is the sibling of.

  A  every instantiation: ns in {0,1,2} x ni in {1,2} x {one, two sequences per lane}, with and without the y store, at (B, T, k) =
     (1, 40, 1), (65, 100, 4), (130, 257, 3), and B = 130 dropping to one per lane when x, target and y sit at 4 mod 8;
  B  skip in {0, 1, 7, 32, inside chunk 2 and no multiple of 8, T - 1} on trees (1,1) and (2,2): y is right on the rows before skip too;
  C  chunk geometry (T, k) in {(33, 2), (65, 3), (1000, 5), (2048, 64)} on (2,1), both lane widths: (2048, 64) is the single-lane walk
     over 64 chunks, and at B = 65 the finishing wave adds 128 partials;
  D  z0 / zT handed across two calls on (2,2), against the references of the halves and one call of double length;
  E  an n_global above the call's own n; esr = 0; NaN and Inf in the target's rows before skip; two half batches whose sums add up
     to the whole's; a reused workspace and the ticket left 0; the same sums and losses with and without y;
  F  against the steps, all twelve (ns, ni, width) at (65, 100, 4) and (130, 257, 3), the same n_chunks: y, zT, (float)sums, loss3 equal
     ss_lin_step_esr's BIT FOR BIT, and at skip = 0 loss equals ss_lin_step_mse's loss.

Bounds (tests/ss_lin_esr_ref.py's and tests/test_gpu_ss_lin_esr_step.py's; none taken from what the kernel gives):
  y, zT     3e-6 max(1, max |ref|)
  S, E      1e-5 relative
  loss3     1e-5 relative + one fp32 ulp, each of mse, esr, mse + esr
  loss      1e-5 relative against 0.5 gscale S_ref

Every check prints `FIG <section> | <case> | ...` with each error divided by its bound before it asserts (run with -s).
"""
import gc

import numpy as np
import pytest

import ss_lin_esr_ref as E
import ss_lin_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B_Y, B_SUM = 3e-6, 1e-5
GSCALE = 0.125                                                    # (any float: loss = 0.5 gscale S)


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


_REFS = {}


def ref_of(c):
    """the float64 reference of a case without its gradients, computed once"""
    if id(c) not in _REFS:
        _REFS[id(c)] = (c, E.run(c.ns, c.ni, c.coef, c.x, c.target, c.skip, z0=c.z0, n_global=c.n_global, grads=False))
    return _REFS[id(c)][1]


def call(c, n_chunks, want_zT=False, z0="case", misaligned=False, ws=None, target=None, n_global="case", store_y=True):
    from wdf_hip import binding as wb
    z0 = (None if c.z0 is None else cuda(c.z0)) if isinstance(z0, str) else z0
    xs = one_float_in(c.x) if misaligned else cuda(c.x)
    tg = (one_float_in(c.target) if misaligned else cuda(c.target)) if target is None else target
    y = one_float_in(np.zeros((c.T, c.B))) if (misaligned and store_y) else None
    return wb.ss_lin_eval(xs, cuda(c.coef), tg, n_chunks, skip=c.skip, n_global=c.n_global if isinstance(n_global, str) else n_global,
                          gscale=GSCALE, z0=z0, want_zT=want_zT, ws=ws, y=y, store_y=store_y)


def ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def check(section, label, c, res, ref=None):
    """every output of one call against the reference; prints the figures (error / bound), then asserts"""
    ref = ref_of(c) if ref is None else ref
    sums = res["sums"].cpu().numpy()
    l3 = res["loss3"].cpu().numpy().astype(np.float64)
    loss = float(res["loss"].cpu())
    want = 0.5 * float(np.float32(GSCALE)) * ref.S
    f = {"S": ratio(abs(sums[0] - ref.S), B_SUM * ref.S), "E": ratio(abs(sums[1] - ref.E), B_SUM * ref.E),
         "mse": ratio(abs(l3[0] - ref.mse), B_SUM * ref.mse + ulp32(ref.mse)),
         "esr": ratio(abs(l3[1] - ref.esr), B_SUM * ref.esr + ulp32(ref.esr)),
         "loss3": ratio(abs(l3[2] - ref.loss), B_SUM * ref.loss + ulp32(ref.loss)),
         "loss": ratio(abs(loss - want), B_SUM * want)}
    fin = [sums, l3, np.asarray(loss)]
    if res["y"] is not None:
        y = res["y"].cpu().numpy().astype(np.float64)
        fin.append(y)
        f["y"] = ratio(np.max(np.abs(y - ref.y)), B_Y * max(1.0, np.max(np.abs(ref.y))))
    if res["zT"] is not None:
        zT = res["zT"].cpu().numpy().astype(np.float64)
        fin.append(zT)
        f["zT"] = ratio(np.max(np.abs(zT - ref.zT)), B_Y * max(1.0, np.max(np.abs(ref.zT))))
    print(f"FIG {section} | {label} {c} | " + " ".join(f"{k}={v:.3f}" for k, v in f.items()))
    assert all(np.all(np.isfinite(a)) for a in fin)
    assert all(v <= 1.0 for v in f.values()), (section, label, repr(c), f)
    return f


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- A: every instantiation --------------------------------------------------------------------------------------------------
CASES_A = [(B, T, k, False) for B, T, k in E.SHAPES_A] + [(130, 257, 3, True)]


@pytest.mark.parametrize("store_y", [True, False], ids=["y", "noy"])
@pytest.mark.parametrize("B,T,k,mis", CASES_A, ids=[f"B{B}-T{T}-k{k}-" + ("one-4mod8" if m else ("two" if B % 2 == 0 else "one")) for B, T, k, m in CASES_A])
@pytest.mark.parametrize("ns,ni", R.TREES, ids=[f"ns{a}-ni{b}" for a, b in R.TREES])
def test_a_every_instantiation(ns, ni, B, T, k, mis, store_y):
    c = E.case(ns, ni, B, T, E.SKIP_A)
    res = call(c, k, want_zT=True, misaligned=mis, store_y=store_y)
    assert (res["zT"] is None) == (ns == 0) and (res["y"] is None) == (not store_y)
    if store_y:
        assert (res["y"].data_ptr() % 8 == 4) == mis
    check("A", ("4 mod 8 " if mis else "") + f"k={k} " + ("y" if store_y else "no y"), c, res)


# ---- B: skip positions -------------------------------------------------------------------------------------------------------
CASES_B = [(ns, ni, B, T, k, s) for ns, ni in E.TREES_B for B, T, k in E.SHAPES_B for s in E.skips_b(T)]


@pytest.mark.parametrize("ns,ni,B,T,k,skip", CASES_B, ids=[f"ns{a}-ni{b}-B{B}-T{T}-skip{s}" for a, b, B, T, k, s in CASES_B])
def test_b_skip_positions(ns, ni, B, T, k, skip):
    c = E.case(ns, ni, B, T, skip)
    check("B", f"k={k}", c, call(c, k, want_zT=True))


# ---- C: chunk geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,k", E.GEOM_C, ids=[f"T{T}-k{k}" for T, k in E.GEOM_C])
@pytest.mark.parametrize("B", E.BATCHES_C, ids=["one-B65", "two-B130"])
def test_c_chunk_geometry(B, T, k):
    from wdf_hip import binding as wb
    c = E.case(2, 1, B, T, E.skip_c(T))
    res = call(c, k)
    L, K = wb.chunk_geom(T, k, 32)
    assert res["ws"].numel() == wb.lib().wdf_ss_lin_eval_ws_bytes(2, 1, B, T, K)
    check("C", f"L={L} K={K} (asked {k})", c, res)


# ---- D: the state handed over ------------------------------------------------------------------------------------------------
def test_d_two_calls_with_the_state_handed_over():
    """the first half from a random z0, the second from the first's zT: each against its own reference; and against ONE call over
    all 514 steps with skip = 257 + the second call's skip: the same y rows, final states, S and E"""
    long, first, second = E.carried()
    z0 = cuda(first.z0)
    before = z0.clone()
    r1 = call(first, 3, want_zT=True, z0=z0)
    check("D", "first half", first, r1)
    assert same_bits(z0, before) and r1["zT"].data_ptr() != z0.data_ptr()
    r2 = call(second, 3, want_zT=True, z0=r1["zT"])
    check("D", "second half from the first's zT", second, r2)
    rl = call(long, 6, want_zT=True)
    check("D", "one call of double length", long, rl)
    both = torch.cat([r1["y"], r2["y"]]).cpu().numpy().astype(np.float64)
    yl, wref = rl["y"].cpu().numpy().astype(np.float64), ref_of(long)
    assert np.max(np.abs(both - yl)) <= 2 * B_Y * max(1.0, np.max(np.abs(wref.y)))
    assert np.max(np.abs((r2["zT"] - rl["zT"]).cpu().numpy())) <= 2 * B_Y * max(1.0, np.max(np.abs(wref.zT)))
    s2, sl = r2["sums"].cpu().numpy(), rl["sums"].cpu().numpy()
    assert abs(s2[0] - sl[0]) <= 2 * B_SUM * wref.S and abs(s2[1] - sl[1]) <= 2 * B_SUM * wref.E


# ---- E: the finish -----------------------------------------------------------------------------------------------------------
def test_e_n_global_larger_than_the_calls_own_n():
    c = E.case(2, 2, 130, 257, E.SKIP_E, n_global=E.N_GLOBAL_E)
    assert ref_of(c).n == 4 * 130 * (257 - E.SKIP_E)
    check("E", "n_global = 4 n", c, call(c, 3))


def test_e_esr_zero():
    """target = the y of a first call: e = 0 on every row, S = 0, esr = 0 -- every loss is 0 and finite, E is not"""
    c = E.case(2, 2, 130, 257, E.SKIP_E)
    first = call(c, 3)
    res = call(c, 3, target=first["y"])
    sums, l3 = res["sums"].cpu().numpy(), res["loss3"].cpu().numpy()
    assert same_bits(res["y"], first["y"])
    assert sums[0] == 0.0 and sums[1] > 0 and np.all(l3 == 0) and float(res["loss"].cpu()) == 0.0


@pytest.mark.parametrize("B", [65, 130], ids=["one-B65", "two-B130"])
def test_e_skipped_rows_of_the_target_count_for_nothing_whatever_they_hold(B):
    """NaN and Inf in the rows of target before skip (padding) leave every output bit for bit what a clean target gives -- skip = 203
    sits inside an 8-step block, inside a 32-step window, inside the last chunk"""
    c = E.case(2, 2, 130, 257, 203) if B == 130 else E.case(2, 2, 65, 100, 75)
    k = 3 if B == 130 else 4
    clean = call(c, k, want_zT=True)
    bad = c.target.copy()
    bad[:c.skip:2], bad[1:c.skip:2] = np.nan, np.inf
    res = call(c, k, want_zT=True, target=cuda(bad))
    for key in ("y", "loss3", "loss", "zT"):
        assert same_bits(res[key], clean[key]), key
    assert torch.equal(res["sums"].view(torch.int64), clean["sums"].view(torch.int64))
    assert np.all(np.isfinite(res["sums"].cpu().numpy()))


def test_e_two_half_batches_add_up_to_the_whole():
    """B = 130 as 65 + 65 (one sequence per lane each; the whole batch runs two per lane), each with n_global of the whole: the
    double sums added give the whole's S and E within their bound, and ss_lin_esr_ref.finish on them the whole's loss within its"""
    c = E.case(2, 2, 130, 257, E.SKIP_E)
    ref = ref_of(c)
    whole = call(c, 3)
    total = np.zeros(2)
    for lo in (0, 65):
        h = object.__new__(E.Case)
        h.__dict__.update(c.__dict__)
        h.B, h.x, h.target, h.z0 = 65, c.x[:, :, lo:lo + 65], c.target[:, lo:lo + 65], None
        total += call(h, 3, n_global=ref.n)["sums"].cpu().numpy()
    w = whole["sums"].cpu().numpy()
    r = E.Result()
    r.S, r.E, r.n = float(total[0]), float(total[1]), ref.n
    E.finish(r)
    l3 = whole["loss3"].cpu().numpy().astype(np.float64)
    f = {"S": ratio(abs(total[0] - ref.S), B_SUM * ref.S), "E": ratio(abs(total[1] - ref.E), B_SUM * ref.E),
         "S whole": ratio(abs(total[0] - w[0]), B_SUM * ref.S), "E whole": ratio(abs(total[1] - w[1]), B_SUM * ref.E),
         "loss": ratio(abs(r.loss - ref.loss), B_SUM * ref.loss + ulp32(ref.loss)),
         "loss whole": ratio(abs(r.loss - l3[2]), B_SUM * ref.loss + ulp32(ref.loss))}
    print("FIG E | halves | " + " ".join(f"{k}={v:.3f}" for k, v in f.items()))
    assert all(v <= 1.0 for v in f.values()), f


def test_e_a_reused_workspace_with_and_without_y():
    """calls on the workspace of the first, storing y and not, in turn: the same bits every time, the ticket (the first word) 0"""
    c = E.case(2, 2, 130, 257, E.SKIP_E)
    res = call(c, 3, want_zT=True)
    check("E", "call 1", c, res)
    ws = res["ws"]
    assert int(ws[:4].view(torch.int32)[0]) == 0
    keep = {k: res[k].clone() for k in ("y", "sums", "loss3", "loss", "zT")}
    for n, store_y in ((2, False), (3, True), (4, False)):
        res = call(c, 3, want_zT=True, ws=ws, store_y=store_y)
        assert res["ws"].data_ptr() == ws.data_ptr() and int(ws[:4].view(torch.int32)[0]) == 0
        assert (res["y"] is None) == (not store_y)
        for k, v in keep.items():
            if res[k] is not None:
                assert torch.equal(res[k].view(torch.int64 if k == "sums" else torch.int32), v.view(torch.int64 if k == "sums" else torch.int32)), (k, n)
    check("E", "call 4, no y", c, res)


def test_e_wrapper_refuses_what_does_not_fit():
    from wdf_hip import binding as wb
    c = E.case(1, 1, 65, 100, 7)
    x, coef, tgt = cuda(c.x), cuda(c.coef), cuda(c.target)
    good = dict(x_tm=x, coef=coef, target=tgt, skip=7, n_chunks=4)
    for over in (dict(skip=-1), dict(skip=100), dict(n_global=0.0), dict(eps=-1.0), dict(coef=coef[:7]), dict(target=tgt[:99]),
                 dict(z0=cuda(np.zeros((2, 65)))), dict(y=cuda(np.zeros((100, 64)))), dict(y=torch.zeros((100, 65))), dict(n_chunks=0),
                 dict(y=cuda(np.zeros((100, 65))), store_y=False), dict(sums=torch.zeros(2, device="cuda")),
                 dict(ws=torch.zeros(16, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(wb.WdfHipError):
            wb.ss_lin_eval(**{**good, **over})
    res = wb.ss_lin_eval(**good)
    assert tuple(res["y"].shape) == (100, 65) and res["zT"] is None and res["sums"].dtype == torch.float64


# ---- F: the steps' bits ------------------------------------------------------------------------------------------------------
CASES_F = [(65, 100, 4, False), (130, 257, 3, False), (130, 257, 3, True)]       # one per lane; two; 130 at 4 mod 8: one per lane


@pytest.mark.parametrize("B,T,k,mis", CASES_F, ids=["one-B65", "two-B130", "one-B130-4mod8"])
@pytest.mark.parametrize("ns,ni", R.TREES, ids=[f"ns{a}-ni{b}" for a, b in R.TREES])
def test_f_the_steps_bits(ns, ni, B, T, k, mis):
    """y, zT, (float)S, (float)E and loss3 are ss_lin_step_esr's, and at skip = 0 the loss is ss_lin_step_mse's: BIT FOR BIT"""
    from wdf_hip import binding as wb
    put = one_float_in if mis else cuda
    for skip in (E.SKIP_A, 0):
        c = E.case(ns, ni, B, T, skip)
        z0 = None if c.z0 is None else cuda(c.z0)
        x, tgt, coef, jac = put(c.x), put(c.target), cuda(c.coef), cuda(c.jac, np.float64)
        gscale = 2.0 / (B * T)
        ev = wb.ss_lin_eval(x, coef, tgt, k, skip=skip, gscale=gscale, z0=z0, want_zT=True, y=put(np.zeros((T, B))))
        st = wb.ss_lin_step_esr(x, coef, jac, tgt, skip, k, z0=z0, want_zT=True, y=put(np.zeros((T, B))))
        assert same_bits(ev["y"], st["y"]), skip
        if ns > 0:
            assert same_bits(ev["zT"], st["zT"]), skip
        assert same_bits(ev["sums"].float(), st["sums"][:2]), (skip, ev["sums"], st["sums"][:2])
        assert same_bits(ev["loss3"], st["loss3"]), (skip, ev["loss3"], st["loss3"])
        noy = wb.ss_lin_eval(x, coef, tgt, k, skip=skip, gscale=gscale, z0=z0, want_zT=True, store_y=False)
        assert torch.equal(noy["sums"].view(torch.int64), ev["sums"].view(torch.int64)) and same_bits(noy["loss3"], ev["loss3"])
        assert same_bits(noy["loss"], ev["loss"]) and (ns == 0 or same_bits(noy["zT"], ev["zT"]))
        if skip == 0:
            ms = wb.ss_lin_step_mse(x, coef, jac, tgt, gscale, k, z0=z0, want_zT=True, y=put(np.zeros((T, B))))
            assert same_bits(ev["loss"], ms["loss"]), (ev["loss"], ms["loss"])
            assert same_bits(ev["y"], ms["y"]) and same_bits(ev["sums"][:1].float(), ms["out"][:1])
