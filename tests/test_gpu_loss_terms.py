"""GPU: the weighted loss family (mse_loss, esr_loss, esr_with_emph, avg_loss of clipper_pot.py:141-165) as the fused device
stage of csrc/wdf_elementwise.h, kernel level through binding.loss_terms_sums / _coef / _grad (and the autograd function's
sums_allreduce / n hooks).

Reference: reference() below, the four formulas restated in float64 torch on the CPU over the same float32 y / target values,
dL/dy from torch.autograd.  Data per shape from a fixed seed: y = 0.5 sin(ramp) + 0.05 noise, target = 0.9 y + 0.02 noise + 0.01
(the offset keeps |mean(o) - mean(t)| ~ 0.01, far from the sign's kink; S and Sp stay far from 0).

Bounds (derived, not tuned):
  S, E, Sp, Ep   5e-7 relative: non-negative addends with at most 4 fp32 roundings each (<= 4 * 2^-24 = 2.4e-7), the double
                 accumulation is negligible.
  So, St         1e-12 relative: sums of exactly converted floats.
  terms          5e-7 relative plus one fp32 ulp of the value.
  gy             1e-6 (|ga||e| + |gb||o| + |al|(|ep| + c|ep+|) + |be|(|op| + c|op+|) + |gm|) per element: at most 16 fp32
                 roundings of the magnitude sum.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = float(np.finfo(float).eps)
C_EMPH = 0.85
SHAPES = [(1, 1, 0), (3, 2, 1), (64, 5, 0), (65, 33, 7), (256, 300, 50), (4100, 1200, 50)]          # (B, T, skip)
UNALIGNED = (64, 40, 3)
WEIGHTS = [(1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0), (1.0, 1.0, 1.0, 1.0)]
NAMES = ("mse", "esr", "esr_emph", "avg", "loss")


@pytest.fixture(scope="module")
def wb():
    from wdf_hip import binding
    binding.require_gpu()
    return binding


@functools.lru_cache(maxsize=None)
def data(B, T):
    rng = np.random.default_rng(1000 * B + T)
    ramp = 0.05 * np.arange(T)[:, None] + 0.3 * np.arange(B)[None, :]
    y = (0.5 * np.sin(ramp) + 0.05 * rng.standard_normal((T, B))).astype(np.float32)
    t = (0.9 * y + 0.02 * rng.standard_normal((T, B)) + 0.01).astype(np.float32)
    y.setflags(write=False)
    t.setflags(write=False)
    return y, t


def pre_emphasis(v, c):
    """f(v)[0] = v[0], f(v)[k] = v[k] - c v[k-1] along axis 0 (time) -- clipper_pot.py:141-144's filter on this engine's [T,B]."""
    return torch.cat([v[:1], v[1:] - c * v[:-1]])


def four_terms(o, t, n, c):
    """clipper_pot.py:141-165 in float64: mse_loss, esr_loss and esr_with_emph with (outs, target) passed as (target_y,
    predicted_y) -- the energy is the output's -- and avg_loss."""
    S, E = ((o - t) ** 2).sum(), (o ** 2).sum()
    fo, ft = pre_emphasis(o, c), pre_emphasis(t, c)
    Sp, Ep = ((fo - ft) ** 2).sum(), (fo ** 2).sum()
    So, St = o.sum(), t.sum()
    terms = [S / n, torch.sqrt(S / (E + EPS) / n), torch.sqrt(Sp / (Ep + EPS) / n), torch.abs(So - St) / n]
    return terms, [S, E, Sp, Ep, So, St]


def reference(y32, t32, skip, w, c, n=None):
    """-> dict(sums6, terms5, gy [T,B], bound [T,B]) in float64 from float32 arrays; bound is the per-element gy bound above."""
    y = torch.tensor(np.array(y32), dtype=torch.float64, requires_grad=True)
    t = torch.tensor(np.array(t32), dtype=torch.float64)
    o, tt = y[skip:], t[skip:]
    n = float(o.numel()) if n is None else float(n)
    terms, sums = four_terms(o, tt, n, c)
    loss = sum(wk * tk for wk, tk in zip(w, terms))
    gy, = torch.autograd.grad(loss, y)
    with torch.no_grad():
        S, E, Sp, Ep, So, St = [float(v.detach()) for v in sums]
        esr, emph = float(terms[1].detach()), float(terms[2].detach())
        ga = w[0] * 2.0 / n + (w[1] / (esr * (E + EPS) * n) if esr > 0 else 0.0)
        gb = -w[1] * esr / (E + EPS)
        al = w[2] / (emph * (Ep + EPS) * n) if emph > 0 else 0.0
        be = -w[2] * emph / (Ep + EPS)
        gm = w[3] * float(np.sign(So - St)) / n
        e = (o - tt).abs()
        ep, op = pre_emphasis(o - tt, c).abs(), pre_emphasis(o, c).abs()
        zero = torch.zeros_like(e[:1])
        epn, opn = torch.cat([ep[1:], zero]), torch.cat([op[1:], zero])
        mag = abs(ga) * e + abs(gb) * o.abs() + abs(al) * (ep + c * epn) + abs(be) * (op + c * opn) + abs(gm)
        bound = torch.cat([torch.zeros_like(t[:skip]), 1.0e-6 * mag])
    return {"sums6": np.array([S, E, Sp, Ep, So, St]), "terms5": np.array([float(v.detach()) for v in terms] + [float(loss.detach())]),
            "gy": gy.numpy(), "bound": bound.numpy(), "coef": (ga, gb, al, be, gm), "n": n}


@functools.lru_cache(maxsize=None)
def cached_reference(B, T, skip, w, c):
    y, t = data(B, T)
    r = reference(y, t, skip, w, c)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float32), device="cuda")


def one_float_in(a):
    """The array on the device as a dense [T,B] view that starts one float into its storage: 4 mod 16 bytes."""
    T, B = a.shape
    base = torch.empty((T * B + 1,), dtype=torch.float32, device="cuda")
    v = base[1:].view(T, B)
    v.copy_(torch.as_tensor(np.array(a, dtype=np.float32)))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def stage(wb, y, t, skip, w, c, n=None):
    sums6 = wb.loss_terms_sums(y, t, skip, c)
    n = float((y.shape[0] - skip) * y.shape[1]) if n is None else n
    gcoef, terms = wb.loss_terms_coef(sums6, n, EPS, w, c)
    gy = wb.loss_terms_grad(y, t, gcoef, skip, c)
    torch.cuda.synchronize()
    return sums6, gcoef, terms, gy


def check_sums_and_terms(sums6, terms, ref):
    got, want = sums6.cpu().numpy(), ref["sums6"]
    rel = np.abs(got - want) / np.abs(want)
    print("sums6 relative error", rel)
    assert np.all(rel[:4] <= 5e-7), (got, want)
    assert np.all(rel[4:] <= 1e-12), (got, want)
    tg = terms.cpu().numpy().astype(np.float64)
    for name, g, r in zip(NAMES, tg, ref["terms5"]):
        tol = 5e-7 * abs(r) + float(np.spacing(np.float32(abs(r))))
        print(f"{name}: got {g!r} want {r!r} |diff| {abs(g - r):.3e} tol {tol:.3e}")
        assert abs(g - r) <= tol, (name, g, r)


def check_gy(gy, ref, skip):
    g = gy.cpu().numpy().astype(np.float64)
    assert g.shape == ref["gy"].shape
    assert not g[:skip].any()                                        # rows before skip: exactly 0
    assert np.all(np.isfinite(g))
    err = np.abs(g - ref["gy"])
    worst = float(np.max(err[skip:] / np.maximum(ref["bound"][skip:], 1e-300)))
    print(f"gy: worst |gy - ref| / bound = {worst:.3f}")
    assert np.all(err <= ref["bound"]), worst


@pytest.mark.parametrize("w", WEIGHTS, ids=lambda w: "w" + "".join(str(int(v)) for v in w))
@pytest.mark.parametrize("shape", SHAPES + [UNALIGNED + ("unaligned",)], ids=lambda s: "x".join(str(v) for v in s))
def test_sums_terms_and_gradient_against_float64(wb, shape, w):
    """Checks 1 and 2: sums6, the five terms and dL/dy, each weight alone and all four, at c = 0.85; the last shape through
    views that start one float into their storage (B % 4 == 0: only the alignment test sends them to the scalar loads)."""
    B, T, skip = shape[:3]
    y, t = data(B, T)
    ref = cached_reference(B, T, skip, w, C_EMPH)
    yd, td = (one_float_in(y), one_float_in(t)) if len(shape) == 4 else (dev(y), dev(t))
    sums6, gcoef, terms, gy = stage(wb, yd, td, skip, w, C_EMPH)
    check_sums_and_terms(sums6, terms, ref)
    check_gy(gy, ref, skip)
    assert float(gcoef[5]) == float(np.float32(C_EMPH))
    if len(shape) == 4:                                              # ... and an output that is not 16-byte aligned either
        gy2 = wb.loss_terms_grad(yd, td, gcoef, skip, C_EMPH, gy=one_float_in(np.zeros((T, B), np.float32)))
        assert torch.equal(gy2, gy)


@pytest.mark.parametrize("B,T,skip", [(65, 33, 7), (256, 300, 50)])
def test_zero_coefficient_makes_the_filter_the_identity(wb, B, T, skip):
    """Check 3: c = 0 -> Sp and Ep are S and E bit for bit (fmaf(-0, ., e) is e) and terms[esr_emph] == terms[esr]."""
    y, t = data(B, T)
    sums6, _, terms, gy = stage(wb, dev(y), dev(t), skip, (1.0, 1.0, 1.0, 1.0), 0.0)
    s = sums6.cpu().numpy()
    assert s[2].tobytes() == s[0].tobytes() and s[3].tobytes() == s[1].tobytes()
    tn = terms.cpu().numpy()
    assert tn[2].tobytes() == tn[1].tobytes()
    check_gy(gy, cached_reference(B, T, skip, (1.0, 1.0, 1.0, 1.0), 0.0), skip)


@pytest.mark.parametrize("B,T,skip", [(65, 33, 7), (256, 300, 50), (4100, 1200, 50)])
def test_tie_to_the_mse_esr_stage(wb, B, T, skip):
    """Check 4: with weights (1, 1, 0, 0) the stage is wdf_loss_sums / wdf_esr_coef / wdf_loss_esr_grad: S, E to 1e-12 relative
    (the partition may differ), loss to 2 fp32 ulp, gy to 2e-7 (|ga e| + |gb o|)."""
    y, t = data(B, T)
    yd, td = dev(y), dev(t)
    n = float((T - skip) * B)
    sums6, gcoef, terms, gy = stage(wb, yd, td, skip, (1.0, 1.0, 0.0, 0.0), C_EMPH)
    sums2 = wb.loss_sums(yd, td, skip)
    gcoef2, loss3 = wb.esr_coef(sums2, n, EPS)
    gy2 = wb.loss_esr_grad(yd, td, gcoef2, skip)
    torch.cuda.synchronize()
    a, b = sums6.cpu().numpy()[:2], sums2.cpu().numpy()
    assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), (a, b)
    l, l2 = float(terms[4]), float(loss3[2])
    assert abs(l - l2) <= 2.0 * float(np.spacing(np.float32(l2))), (l, l2)
    ga, gb = float(gcoef2[0]), float(gcoef2[1])
    y64, t64 = y.astype(np.float64), t.astype(np.float64)
    tol = 2e-7 * (np.abs(ga * (y64 - t64)) + np.abs(gb * y64))
    err = np.abs(gy.cpu().numpy().astype(np.float64) - gy2.cpu().numpy().astype(np.float64))
    print("worst |gy - loss_esr_grad| / tol", float(np.max(err[skip:] / tol[skip:])))
    assert np.all(err[skip:] <= tol[skip:]) and not err[:skip].any()
    assert float(gcoef[2]) == 0.0 and float(gcoef[3]) == 0.0 and float(gcoef[4]) == 0.0


@pytest.mark.parametrize("shape", SHAPES + [UNALIGNED + ("unaligned",)], ids=lambda s: "x".join(str(v) for v in s))
def test_two_calls_give_the_same_bits(wb, shape):
    """Check 5: fixed-order reductions, no floating-point atomics."""
    B, T, skip = shape[:3]
    y, t = data(B, T)
    yd, td = (one_float_in(y), one_float_in(t)) if len(shape) == 4 else (dev(y), dev(t))
    w = (1.0, 1.0, 1.0, 1.0)
    s1, _, t1, g1 = stage(wb, yd, td, skip, w, C_EMPH)
    s2, _, t2, g2 = stage(wb, yd, td, skip, w, C_EMPH)
    for a, b in ((s1, s2), (t1, t2), (g1, g2)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("B,T,skip", [(1, 1, 0), (65, 33, 7), (256, 300, 50)])
def test_output_equal_to_target(wb, B, T, skip):
    """Check 6: y == target -> every term and the loss exactly 0; gy finite everywhere and 0 (both ESRs are 0, so ga's ESR part
    and al drop out, gb and be are -0, sign(0) = 0)."""
    y, _ = data(B, T)
    yd = dev(y)
    _, gcoef, terms, gy = stage(wb, yd, yd.clone(), skip, (1.0, 1.0, 1.0, 1.0), C_EMPH)
    assert not terms.cpu().numpy().any()
    g = gy.cpu().numpy()
    assert np.all(np.isfinite(g)) and not g.any()
    assert np.all(np.isfinite(gcoef.cpu().numpy()))


def test_sums_allreduce_and_global_count(wb):
    """Check 7: a callable that doubles sums6 with n = 2 T' B is the batch concatenated with itself along B."""
    from wdf_hip import lowering
    B, T, skip = 65, 33, 7
    w = (1.0, 1.0, 1.0, 1.0)
    y, t = data(B, T)
    ref = reference(np.concatenate([y, y], axis=1), np.concatenate([t, t], axis=1), skip, w, C_EMPH)
    assert ref["n"] == 2.0 * (T - skip) * B
    seen = []

    def double(sums6):
        seen.append(sums6.clone())
        sums6.mul_(2.0)

    yd = dev(y).requires_grad_(True)
    loss, terms = lowering._LossTermsFn.apply(yd, dev(t), skip, w, C_EMPH, ref["n"], double, True)
    gy, = torch.autograd.grad(loss, yd)
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0].dtype == torch.float64 and seen[0].numel() == 6
    check_sums_and_terms(seen[0] * 2.0, terms, ref)
    assert float(loss) == float(terms[4])
    half = {"gy": ref["gy"][:, :B], "bound": ref["bound"][:, :B]}
    check_gy(gy, half, skip)
