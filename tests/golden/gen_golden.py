#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by EXECUTING THE REFERENCE.

Run in the build container only (needs /root/reference):  python tests/golden/gen_golden.py
Nothing here runs on the GPU box; the tests read only the committed .npz files.

What is executed from the reference checkout (never copied into this repo):
  wdf_py/lib/tf_wdf.py, wdf_py/lib/layers.py           imported as modules
  wdf_py/simple_circuits/lpf.py  class Model            AST-extracted, exec'd
  wdf_py/simple_circuits/voltage_divider.py class Model AST-extracted, exec'd
  wdf_py/diode_clipper/clipper_pot.py  class ClipperModel, esr_loss, mse_loss, loss_func
  wdf_py/diode_clipper/diode_pretraining.py  diode_pair_func   (numpy + scipy, no TF needed)
  wdf_py/diode_clipper/diode_config.py                 imported
  wdf_py/diode_clipper/models/*.json                   read as data
  modules/toms917/toms917.cpp                          via oracle/_ref/libtoms917_ref.so
`import tensorflow` inside those files resolves to tests/golden/_tf_shim (torch-backed; TF
is not installable here) -- see that module's docstring for what this does to the claim.

Goldens:
  g1_rc_lowpass.npz     lpf.py Model: y, MSE loss, dL/dR, dL/dC  (f32 = reference dtype, and f64)
  g2_voltage_divider.npz
  g3_mlp_clipper.npz    clipper_pot.py ClipperModel with 2x4 / 2x8 / 2x16 / 4x4 / 4x8 trained weights:
                        y, MSE+ESR loss (with the script's argument swap), all weight grads
  g4_diode_pair.npz     diode_pair_func table over a, R, 6 diode configs
  g5_omega.npz          Wright omega: reference toms917 build, scipy, mpmath(40 digits)
  g7_recorded_programs.npz   the reference's own Model / ClipperModel classes run through THIS
                        repo's drop-in tf_wdf with the kernel launch captured: the programs the loop
                        recorder lowered them to (state-space coefficients + their Jacobian to the
                        trainable components; MLP-clipper weights / inputs).  The GPU tests launch
                        the kernels on these programs and compare with g1-g3, so no line of the
                        reference scripts has to travel to the GPU box.
  g8_dataimport.npz     the reference's dataimport.createDataset / load_diode_data and clipper_pot's
                        batch_data run on CSV files written by this repo's synthetic-dataset writer
  g9_mlp_relu.npz       clipper_pot.py ClipperModel on a ReLU network (layers.py:63-67): the pretrained 2x16 JSON
                        with its activations switched to "relu" and its weights halved; same arrays as g3
  g10_reference_models.npz  the model JSON files under wdf_py/diode_clipper/models (all but old/), byte for
                        byte: `names` (path below models/), `blob` (the files' bytes, concatenated), `ends` (offsets)
  g6_diode_clipper.npz  tf_wdf.py Parallel(ResVs, C) tree + diode-pair root:
                        (a) forward from reference pieces only (tf_wdf elements + diode_pair_func)
                        (b) f64 forward + autograd grads wrt Is, nVt, R, C with a torch
                            autograd diode-pair root written here (omega' = omega/(1+omega))
"""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("WDF_REFERENCE", "/root/reference")

sys.path.insert(0, os.path.join(HERE, "_tf_shim"))
sys.path.insert(0, os.path.join(REF, "wdf_py", "lib"))
sys.path.insert(0, os.path.join(REF, "wdf_py", "diode_clipper"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

import torch  # noqa: E402
import tensorflow as tf  # noqa: E402  (the shim)
from scipy.special import wrightomega  # noqa: E402

torch.manual_seed(0)
FS = 48000


def extract(path, names, ns):
    """exec the top-level definitions `names` of a reference script inside namespace ns."""
    tree = ast.parse(open(path).read())
    body = []
    for node in tree.body:
        if isinstance(node, (ast.ClassDef, ast.FunctionDef)) and node.name in names:
            body.append(node)
        elif isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id in names for t in node.targets):
            body.append(node)
    exec(compile(ast.Module(body, []), path, "exec"), ns)
    return ns


def fresh_lib():
    """(re)import the reference library modules against the shim's current dtype."""
    for m in ("tf_wdf", "layers"):
        sys.modules.pop(m, None)
    import tf_wdf as wdf
    import layers
    return wdf, layers


def log_sweep(f0, f1, n, fs):
    """exponential sine sweep (stands in for audio_dspy.sweep_log of lpf.py:58, absent here)."""
    t = np.arange(n) / fs
    dur = n / fs
    k = np.log(f1 / f0)
    return np.sin(2 * np.pi * f0 * dur / k * (np.exp(t / dur * k) - 1.0))


def lpf1(fc, fs, x):
    """bilinear one-pole lowpass (stands in for adsp.design_LPF1 + lfilter, lpf.py:61-62)."""
    c = 1.0 / np.tan(np.pi * fc / fs)
    b0 = 1.0 / (1.0 + c)
    a1 = (1.0 - c) / (1.0 + c)
    y = np.zeros_like(x)
    xm1 = ym1 = 0.0
    for i, xi in enumerate(x):
        y[i] = b0 * (xi + xm1) - a1 * ym1
        xm1, ym1 = xi, y[i]
    return y


def npy(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------
def g1_rc_lowpass():
    out = {}
    x = log_sweep(100.0, 10000.0, 1280, FS)
    target = lpf1(720.0, FS, x)
    out["x"] = x
    out["target"] = target
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        tf._DTYPE = dt
        wdf, _ = fresh_lib()
        ns = extract(os.path.join(REF, "wdf_py/simple_circuits/lpf.py"), {"Model"}, {"tf": tf, "wdf": wdf, "FS": FS})
        model = ns["Model"]()
        data_in = np.array([x])
        outs = model.forward(data_in)[..., 0]                # lpf.py:88  [T,1]
        loss = tf.keras.losses.MeanSquaredError()(outs, np.transpose(np.array([target])))
        tv = model.trainable_variables                       # [C1.C, R1.R]  (lpf.py:98-99)
        grads = torch.autograd.grad(loss, tv)
        assert tv[0] is model.C1.C and tv[1] is model.R1.R
        out[f"y_{tag}"] = npy(outs)[:, 0]
        out[f"loss_{tag}"] = npy(loss)
        out[f"dC_{tag}"] = npy(grads[0])
        out[f"dR_{tag}"] = npy(grads[1])
        # reference quirk: lpf.py never resets C1, so a second forward() starts from the
        # final state of the first one
        out[f"z_after_{tag}"] = npy(model.C1.z).ravel()
        # (round 6) ... and its gradient: a new `with tf.GradientTape()` block (lpf.py:87) records nothing of the previous
        # epoch, so the stored state is a CONSTANT of the second epoch's tape -- torch's graph would still reach into the
        # first forward, hence the detach (values unchanged)
        model.C1.z = model.C1.z.detach()
        outs2 = model.forward(data_in)[..., 0]
        out[f"y_second_call_{tag}"] = npy(outs2)[:, 0]
        loss2 = tf.keras.losses.MeanSquaredError()(outs2, np.transpose(np.array([target])))
        grads2 = torch.autograd.grad(loss2, tv)
        out[f"loss_second_call_{tag}"] = npy(loss2)
        out[f"dC_second_call_{tag}"] = npy(grads2[0])
        out[f"dR_second_call_{tag}"] = npy(grads2[1])
        out[f"z_after_second_call_{tag}"] = npy(model.C1.z).ravel()
    out["R"] = 1000.0
    out["C"] = 1.0e-6
    np.savez(os.path.join(HERE, "g1_rc_lowpass.npz"), **out)
    print("g1", out["loss_f32"], out["dR_f32"], out["dC_f32"], out["dR_f64"], out["dC_f64"])


def g2_voltage_divider():
    out = {}
    n = 512
    x = np.sin(2 * np.pi * np.arange(n) * 100.0 / FS)         # voltage_divider.py:56
    out["x"] = x
    out["target"] = 0.5 * x
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        tf._DTYPE = dt
        wdf, _ = fresh_lib()
        ns = extract(os.path.join(REF, "wdf_py/simple_circuits/voltage_divider.py"), {"Model"}, {"tf": tf, "wdf": wdf})
        model = ns["Model"]()
        outs = model.forward(np.array([x]))[..., 0]
        loss = tf.keras.losses.MeanSquaredError()(outs, np.transpose(np.array([0.5 * x])))
        tv = model.trainable_variables
        assert tv[0] is model.R1.R and tv[1] is model.R2.R
        grads = torch.autograd.grad(loss, tv)
        out[f"y_{tag}"] = npy(outs)[:, 0]
        out[f"loss_{tag}"] = npy(loss)
        out[f"dR1_{tag}"] = npy(grads[0])
        out[f"dR2_{tag}"] = npy(grads[1])
    out["R1"] = 2000.0
    out["R2"] = 100.0
    np.savez(os.path.join(HERE, "g2_voltage_divider.npz"), **out)
    print("g2", out["loss_f32"], out["dR1_f32"], out["dR2_f32"], "gain", out["y_f64"][5] / x[5])


def clipper_inputs(B, T, seed):
    rng = np.random.default_rng(seed)
    amps = np.array([0.1, 1.0, 2.5, 5.0, 0.5, 3.5, 1.7, 4.2])[:B]
    x = np.stack([a * log_sweep(100.0, 10000.0, T, FS) * np.cos(0.3 * k) + 0.02 * a * rng.standard_normal(T)
                  for k, a in enumerate(amps)])
    return x


def g3_mlp_clipper():
    out = {}
    B, T, skip = 4, 256, 50
    C_val = 4.7e-9
    x = clipper_inputs(B, T, 7)
    R = np.array([10.0e3, 25.2e3, 45.2e3, 99.1e3])
    data = np.stack([x, np.repeat(R[:, None], T, axis=1)], axis=-1)      # [B,T,2] (clipper_pot.py:68-70)
    target = np.tanh(1.5 * x)[:, :, None] * 0.4                          # synthetic train_Y [B,T,1]
    out["x"] = data
    out["target"] = target
    models = {
        "2x4": "1N4148 (1U-1D)_2x4_training_3.json",
        "2x8": "1N4148 (1U-1D)_2x8_training_3.json",
        "2x16": "1N4148 (1U-1D)_2x16_training_2000.json",
        "2x16_pre": "pretrained/1N4148 (1U-1D)_2x16_pretrained_model.json",
        "4x4": "1N4148 (1U-1D)_4x4_training_4.json",
        "4x8": "1N4148 (1U-1D)_4x8_training_500.json",
    }
    for name, fn in models.items():
        mj = json.load(open(os.path.join(REF, "wdf_py/diode_clipper/models", fn)))
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            tf._DTYPE = dt
            wdf, layers = fresh_lib()
            ns = {"tf": tf, "wdf": wdf, "np": np, "DenseRootModel": layers.DenseRootModel,
                  "DenseLayer": layers.DenseLayer, "C_val": C_val, "FS": FS}
            extract(os.path.join(REF, "wdf_py/diode_clipper/clipper_pot.py"),
                    {"ClipperModel", "esr_loss", "eps", "mse_loss", "loss_func"}, ns)
            import contextlib, io
            with contextlib.redirect_stdout(io.StringIO()):
                model = ns["ClipperModel"](mj)
            outs = tf.transpose(model.forward(data)[..., 0], perm=[1, 0, 2])     # clipper_pot.py:247 [B,T,1]
            tgt = tf.constant(target)                                            # train_Y
            loss = ns["loss_func"](outs[:, skip:, :], tgt[:, skip:, :])          # :248 (outs is "target")
            mse = ns["mse_loss"](outs[:, skip:, :], tgt[:, skip:, :])
            esr = ns["esr_loss"](outs[:, skip:, :], tgt[:, skip:, :])
            tv = model.trainable_variables
            grads = torch.autograd.grad(loss, tv)
            out[f"{name}_y_{tag}"] = npy(outs)[:, :, 0].T                       # [T,B]
            out[f"{name}_loss_{tag}"] = npy(loss)
            out[f"{name}_mse_{tag}"] = npy(mse)
            out[f"{name}_esr_{tag}"] = npy(esr)
            # flatten weights / grads in layer order: kernel[in][out], bias[out]
            dl = [l for l in model.model.layers if isinstance(l, layers.DenseLayer)]
            order = []
            for l in dl:
                order += [l.kernel, l.bias]
            idx = [next(i for i, v in enumerate(tv) if v is p) for p in order]
            out[f"{name}_grad_{tag}"] = np.concatenate([npy(grads[i]).ravel() for i in idx])
            if tag == "f64":
                out[f"{name}_theta"] = np.concatenate([npy(p).ravel() for p in order])
                out[f"{name}_sizes"] = np.array([2] + [l.bias.shape[-1] for l in dl])
                acts = []
                for i, l in enumerate(model.model.layers):
                    if isinstance(l, layers.DenseLayer):
                        nxt = model.model.layers[i + 1] if i + 1 < len(model.model.layers) else None
                        acts.append(1 if nxt is tf.nn.tanh else (2 if nxt is tf.nn.relu else 0))
                out[f"{name}_acts"] = np.array(acts)
        print("g3", name, out[f"{name}_loss_f32"], out[f"{name}_loss_f64"], out[f"{name}_sizes"], out[f"{name}_acts"])
    out["C"] = C_val
    out["skip"] = skip
    np.savez(os.path.join(HERE, "g3_mlp_clipper.npz"), **out)


def g4_diode_pair():
    import diode_config as dc
    ns = extract(os.path.join(REF, "wdf_py/diode_clipper/diode_pretraining.py"), {"diode_pair_func"},
                 {"np": np, "wrightomega": wrightomega})
    f = ns["diode_pair_func"]
    a = np.linspace(-5, 5, 401)
    Rs = np.array([10.0, 2112.0, 1.0e5, 1.0e9])
    cfgs = [dc.diode_1n4148_1u1d, dc.diode_1n4148_1u2d, dc.diode_1n4148_1u3d,
            dc.diode_1n4148_2u2d, dc.diode_1n4148_2u3d, dc.diode_1n4148_3u3d]
    b = np.zeros((len(cfgs), len(Rs), len(a)), dtype=np.float32)
    for i, d in enumerate(cfgs):
        for j, R in enumerate(Rs):
            for k, ak in enumerate(a):
                b[i, j, k] = f(ak, R, d)
    np.savez(os.path.join(HERE, "g4_diode_pair.npz"), a=a, R=Rs, b=b,
             Is=np.array([d.Is for d in cfgs]), nabla=np.array([d.nabla for d in cfgs]),
             Vt=np.array([d.Vt for d in cfgs]), n_up=np.array([d.N_up for d in cfgs]),
             n_down=np.array([d.N_down for d in cfgs]), names=np.array([d.name for d in cfgs]))
    print("g4", b.shape, b[0, 1, ::100])


def g5_omega():
    import mpmath as mp
    import oracle as O
    O.build(ref=True)
    x = np.concatenate([np.linspace(-120, 120, 4001), np.array([-2.0, 1.0 + np.pi, 0.0, 1.0, -1.0])])
    w_ref = O.ref_wright_omega(x)
    w_scipy = wrightomega(x).real
    mp.mp.dps = 40
    w_mp = np.array([float(mp.lambertw(mp.exp(mp.mpf(float(xi))))) for xi in x])
    np.savez(os.path.join(HERE, "g5_omega.npz"), x=x, w_toms917=w_ref, w_scipy=w_scipy, w_mpmath=w_mp)
    rel = np.max(np.abs(w_ref - w_mp) / np.abs(w_mp))
    print("g5 toms917 vs mpmath max rel", rel)


class _OmegaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        w = torch.from_numpy(wrightomega(x.detach().numpy()).real.copy())
        ctx.save_for_backward(w)
        return w

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return g * w / (1.0 + w)


class DiodePairRootF64:
    """torch-autograd diode-pair root for the f64 gradient golden.  Formula:
    diode_pretraining.py:39-60; element protocol: Toms917DiodePair.h:37-59."""

    def __init__(self, nxt, Is, nVt, n_up, n_down):
        self.next = nxt
        self.Is = torch.tensor(Is, dtype=torch.float64, requires_grad=True)
        self.nVt = torch.tensor(nVt, dtype=torch.float64, requires_grad=True)
        self.n_up, self.n_down = n_up, n_down

    def incident(self, x):
        self.a = x

    def reflected(self):
        a = self.a
        R_Is_overVt = self.Is * self.next.R / self.nVt
        pos = (a >= 0)
        nd_ = torch.tensor(float(self.n_down), dtype=torch.float64)
        nu_ = torch.tensor(float(self.n_up), dtype=torch.float64)
        mu0 = torch.where(pos, nd_, nu_)
        mu1 = torch.where(pos, nu_, nd_)
        lam = torch.sign(a)
        w0 = _OmegaFn.apply(torch.log(R_Is_overVt / mu0) + lam * a / (mu0 * self.nVt))
        w1 = _OmegaFn.apply(torch.log(R_Is_overVt / mu1) - lam * a / (mu1 * self.nVt))
        self.b = a - 2 * self.nVt * lam * (mu0 * w0 - mu1 * w1)
        assert self.b.dtype == torch.float64
        return self.b


def g6_diode_clipper():
    import diode_config as dc
    out = {}
    B, T = 4, 512
    x = clipper_inputs(B, T, 11)
    rng = np.random.default_rng(5)
    rpot = 45.0e3 * np.exp(0.8 * np.sin(2 * np.pi * np.arange(T)[None, :] / T * (1 + np.arange(B)[:, None])))
    out["x"] = x
    out["r"] = rpot
    d = dc.diode_1n4148_1u1d
    Is, nVt, R, C = d.Is, d.Vt * d.nabla, 45.0e3, 4.7e-9
    out["theta"] = np.array([Is, nVt, R, C])
    target = None

    # (a) reference pieces only, reference dtype (f32 tree, diode_pair_func returns np.float32)
    ns = extract(os.path.join(REF, "wdf_py/diode_clipper/diode_pretraining.py"), {"diode_pair_func"},
                 {"np": np, "wrightomega": wrightomega})
    dpf = ns["diode_pair_func"]
    for cfg_name, cfg in (("1u1d", dc.diode_1n4148_1u1d), ("2u3d", dc.diode_1n4148_2u3d)):
        tf._DTYPE = torch.float32
        wdf, _ = fresh_lib()
        Vs = wdf.ResistiveVoltageSource(R)
        Cap = wdf.Capacitor(C, FS)
        P1 = wdf.Parallel(Vs, Cap)
        Vs.reset(); Cap.reset()
        ys = []
        xin = torch.tensor(x, dtype=torch.float32)
        for i in range(T):
            Vs.set_voltage(xin[:, i:i + 1])
            P1.calc_impedance()
            a = P1.reflected()
            b = np.array([[dpf(float(ai), float(P1.R), cfg)] for ai in npy(a)[:, 0]], dtype=np.float32)
            P1.incident(torch.tensor(b))
            ys.append(npy(wdf.voltage(Cap))[:, 0])
        out[f"y_refpieces_{cfg_name}_f32"] = np.stack(ys)          # [T,B]

    # (b) f64 tree (reference tf_wdf.py) + autograd root; scalar trainable R
    tf._DTYPE = torch.float64
    for cfg_name, (nu, nd_), use_r in (("1u1d", (1, 1), False), ("2u3d", (2, 3), False), ("1u1d_rpot", (1, 1), True)):
        wdf, _ = fresh_lib()
        Vs = wdf.ResistiveVoltageSource(R, trainable=True)
        Cap = wdf.Capacitor(C, FS, trainable=True)
        P1 = wdf.Parallel(Vs, Cap)
        dp = DiodePairRootF64(P1, Is, nVt, nu, nd_)
        Rvar = Vs.R
        Vs.reset(); Cap.reset()
        xin = torch.tensor(x, dtype=torch.float64)
        rin = torch.tensor(rpot, dtype=torch.float64)
        ys = []
        for i in range(T):
            Vs.set_voltage(xin[:, i:i + 1])
            if use_r:
                Vs.set_resistance(rin[:, i:i + 1])
            P1.calc_impedance()
            dp.incident(P1.reflected())
            P1.incident(dp.reflected())
            ys.append(wdf.voltage(Cap))
        y = torch.stack(ys)[..., 0]                                # [T,B]
        if target is None:
            # target: same circuit at perturbed parameters would need the oracle; use a fixed
            # smooth function instead so the golden does not depend on our own code
            target = 0.35 * np.tanh(2.0 * x.T) + 0.01 * rng.standard_normal((T, B))
            out["target"] = target
        loss = torch.mean((y - torch.tensor(target)) ** 2)
        vars_ = [dp.Is, dp.nVt, Cap.C] if use_r else [dp.Is, dp.nVt, Rvar, Cap.C]
        grads = torch.autograd.grad(loss, vars_)
        out[f"y_{cfg_name}_f64"] = npy(y)
        out[f"loss_{cfg_name}_f64"] = npy(loss)
        out[f"grad_{cfg_name}_f64"] = np.array([float(g) for g in grads])
        print("g6", cfg_name, float(loss), out[f"grad_{cfg_name}_f64"])
    d1 = np.max(np.abs(out["y_refpieces_1u1d_f32"] - out["y_1u1d_f64"]))
    print("g6 refpieces(f32) vs autograd-root(f64) max abs:", d1)
    np.savez(os.path.join(HERE, "g6_diode_clipper.npz"), **out)


def _dropin(fn):
    """Run fn with THIS repo's drop-in library (not the reference's) as tf_wdf / layers."""
    lib = os.path.join(REPO, "differentiable-wdfs_amd", "lib")
    saved_path, saved_mods = list(sys.path), {m: sys.modules.pop(m, None) for m in ("tf_wdf", "layers", "dataimport", "model_utils")}
    sys.path[:] = [lib] + [q for q in sys.path if os.path.join(REF, "wdf_py") not in q and "_tf_shim" not in q]
    saved_tf = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "tensorflow" or k.startswith("tensorflow.")}
    try:
        return fn()
    finally:
        sys.path[:] = saved_path
        for m in ("tf_wdf", "layers", "dataimport", "model_utils"):
            sys.modules.pop(m, None)
            if saved_mods[m] is not None:
                sys.modules[m] = saved_mods[m]
        sys.modules.update(saved_tf)


def g7_recorded_programs():
    g1 = np.load(os.path.join(HERE, "g1_rc_lowpass.npz"))
    g2 = np.load(os.path.join(HERE, "g2_voltage_divider.npz"))
    g3 = np.load(os.path.join(HERE, "g3_mlp_clipper.npz"))

    def run():
        import tf_wdf as wdf                      # the drop-in
        from layers import DenseRootModel
        from wdf_hip import lowering, mlp_root, trace
        assert "differentiable-wdfs_amd" in wdf.__file__
        out, got = {}, {}

        def fake_ss(coef, rootp, x, z0, ns, ni, kind, n_up, n_down, want_zT):
            got.update(coef=coef, x=x, z0=z0, ns=ns, ni=ni, kind=kind)
            T, B = x.shape[1], x.shape[0]
            return (coef.sum() * 0.0 + torch.zeros(T, B)).float(), torch.zeros(ns, B)

        def fake_mlp(theta2, w, x, r, z0, fs, hidden, n_tanh, C, R_static=None, time_parallel="auto"):
            got.update(theta2=theta2, w=w, x=x, r=r, hidden=hidden, n_tanh=n_tanh, fs=fs, C=C)
            B, T = x.shape
            return torch.zeros(T, B) + 0.0 * w.sum(), torch.zeros(B)

        trace._device = lambda: torch.device("cpu")
        lowering._StateSpaceFn.apply = staticmethod(fake_ss)
        mlp_root.clipper_mlp = fake_mlp
        for tag, script, xin, comps in (("lpf", "wdf_py/simple_circuits/lpf.py", g1["x"], ("C1.C", "R1.R")),
                                        ("vdiv", "wdf_py/simple_circuits/voltage_divider.py", g2["x"], ("R1.R", "R2.R"))):
            ns = extract(os.path.join(REF, script), {"Model"}, {"tf": wdf.tf, "wdf": wdf, "FS": FS})
            model = ns["Model"]()
            got.clear()
            y = model.forward(np.array([xin]))
            assert tuple(y.shape) == (len(xin), 1, 1)
            coef = got["coef"]
            tv = list(model.trainable_variables)
            want = [getattr(getattr(model, c.split(".")[0]), c.split(".")[1]) for c in comps]
            assert all(a is b for a, b in zip(tv, want)), "trainable_variables order"
            J = np.zeros((coef.numel(), len(tv)))
            for i in range(coef.numel()):
                gi = torch.autograd.grad(coef[i], tv, retain_graph=True, allow_unused=True)
                J[i] = [0.0 if g is None else float(g) for g in gi]
            out[f"{tag}_coef"] = coef.detach().double().numpy()
            out[f"{tag}_dcoef_dtheta"] = J
            out[f"{tag}_x"] = got["x"].detach().numpy()
            out[f"{tag}_dims"] = np.array([got["ns"], got["ni"], got["kind"]])
            out[f"{tag}_theta_names"] = np.array(comps)
            print("g7", tag, "ns/ni/kind", out[f"{tag}_dims"], "coef", out[f"{tag}_coef"])
        for name, fn in (("2x8", "1N4148 (1U-1D)_2x8_training_3.json"), ("4x8", "1N4148 (1U-1D)_4x8_training_500.json")):
            mj = json.load(open(os.path.join(REF, "wdf_py/diode_clipper/models", fn)))
            ns = {"tf": wdf.tf, "wdf": wdf, "FS": FS, "C_val": float(g3["C"]), "DenseRootModel": DenseRootModel}
            extract(os.path.join(REF, "wdf_py/diode_clipper/clipper_pot.py"), {"ClipperModel"}, ns)
            model = ns["ClipperModel"](mj)
            got.clear()
            y = model.forward(g3["x"])
            assert tuple(y.shape) == (g3["x"].shape[1], g3["x"].shape[0], 1, 1)
            out[f"clip{name}_w"] = got["w"].detach().double().numpy()
            out[f"clip{name}_theta2"] = got["theta2"].detach().double().numpy()
            out[f"clip{name}_x"] = got["x"].detach().numpy()
            out[f"clip{name}_r"] = got["r"].detach().numpy()
            out[f"clip{name}_arch"] = np.array([got["hidden"], got["n_tanh"]])
            out[f"clip{name}_fs_C"] = np.array([got["fs"], got["C"]])
            assert np.allclose(out[f"clip{name}_w"], g3[f"{name}_theta"], rtol=1e-6), "flat weight order == golden order"
            print("g7 clipper", name, out[f"clip{name}_arch"], out[f"clip{name}_w"].shape)
        return out

    out = _dropin(run)
    np.savez(os.path.join(HERE, "g7_recorded_programs.npz"), **out)


def g8_dataimport():
    """f1 pinned to the reference loader: CSVs in the reference's format written by the drop-in's
    write_synthetic_dataset, loaded by the REFERENCE's dataimport (createDataset, load_diode_data:
    dataimport.py:10-59,82-137) and batched by clipper_pot.py's batch_data (:61-80)."""
    import tempfile
    from collections import namedtuple
    DiodeConfig = namedtuple("DiodeConfig", ["name", "Is", "nabla", "Vt", "N_up", "N_down"])
    cfg = DiodeConfig("1N4148 (1U-1D)", 4.352e-9, 1.906, 25.85e-3, 1, 1)
    tmp = tempfile.mkdtemp(prefix="g8_")
    fs_data, seconds = 48000.0, 2.5 + 0.30

    def write():
        import dataimport as di                   # the drop-in
        assert "differentiable-wdfs_amd" in di.__file__
        sim = lambda x, R: np.tanh(2.0 * x) * (0.3 + 1.0e-6 * R)      # any deterministic "measurement"
        return [os.path.basename(f) for f in di.write_synthetic_dataset(tmp, sim, fs=fs_data, seconds=seconds)]

    files = _dropin(write)
    import matplotlib
    matplotlib.use("Agg")
    sys.modules.pop("dataimport", None)
    import dataimport as ref_di                   # the reference's (REF/wdf_py/lib is on sys.path)
    assert REF in ref_di.__file__
    cwd = os.getcwd()
    import contextlib, io
    # Path.iterdir() order is whatever the file system returns; the fixture is taken with the files
    # enumerated in sorted order (the order the drop-in loader fixes), nothing else is touched
    from pathlib import Path
    real_iterdir = Path.iterdir
    Path.iterdir = lambda self: iter(sorted(real_iterdir(self)))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            train_data, train_N, val_data, val_N, FSr = ref_di.load_diode_data(cfg, tmp + os.sep)
    finally:
        Path.iterdir = real_iterdir
    batch = 2048
    ns = extract(os.path.join(REF, "wdf_py/diode_clipper/clipper_pot.py"), {"batch_data"}, {"np": np, "batch_size": batch})
    with contextlib.redirect_stdout(io.StringIO()):
        train_X, train_Y = ns["batch_data"](train_data, train_N)
        val_X, val_Y = ns["batch_data"](val_data, val_N)
    os.chdir(cwd)
    out = {"files": np.array(sorted(files)), "fs": np.array(FSr), "train_N": np.array(train_N), "val_N": np.array(val_N),
           "seconds": np.array(seconds), "batch": np.array(batch),
           "train_data_shape": np.array(np.asarray(train_data).shape), "val_data_shape": np.array(np.asarray(val_data).shape),
           "train_X_shape": np.array(train_X.shape), "train_Y_shape": np.array(train_Y.shape),
           "val_X_shape": np.array(val_X.shape), "val_Y_shape": np.array(val_Y.shape),
           "train_X_head": train_X[:, :4, :], "train_X_tail": train_X[:, -4:, :], "train_Y_head": train_Y[:, :4], "train_Y_tail": train_Y[:, -4:],
           "val_X_head": val_X[:, :4, :], "val_Y_tail": val_Y[:, -4:],
           "train_X_sum": np.array([train_X[..., 0].astype(np.float64).sum(), train_X[..., 1].astype(np.float64).sum()]),
           "train_Y_sum": np.array(train_Y.astype(np.float64).sum()),
           "val_X_sum": np.array([val_X[..., 0].astype(np.float64).sum(), val_X[..., 1].astype(np.float64).sum()]),
           "val_Y_sum": np.array(val_Y.astype(np.float64).sum()),
           "train_R_per_sequence": train_X[:, 0, 1], "val_R_per_sequence": val_X[:, 0, 1]}
    np.savez(os.path.join(HERE, "g8_dataimport.npz"), **out)
    print("g8", files, "train", train_X.shape, train_Y.shape, "val", val_X.shape, val_Y.shape, "fs", FSr)
    import shutil
    shutil.rmtree(tmp)


def g9_mlp_relu():
    """clipper_pot.py ClipperModel with a ReLU network (layers.py:63-67 accepts activation "relu"): the reference's pretrained
    2x16 JSON with its hidden activations switched to "relu" (weights scaled by 0.5 so the unbounded units keep the loop tame),
    same inputs / loss / gradient layout as g3.  Numeric arrays only."""
    out = {}
    B, T, skip = 4, 256, 50
    C_val = 4.7e-9
    x = clipper_inputs(B, T, 7)
    R = np.array([10.0e3, 25.2e3, 45.2e3, 99.1e3])
    data = np.stack([x, np.repeat(R[:, None], T, axis=1)], axis=-1)
    target = np.tanh(1.5 * x)[:, :, None] * 0.4
    out["x"], out["target"] = data, target
    mj = json.load(open(os.path.join(REF, "wdf_py/diode_clipper/models", "pretrained/1N4148 (1U-1D)_2x16_pretrained_model.json")))
    for l in mj["layers"]:
        if l.get("activation") == "tanh":
            l["activation"] = "relu"
        if l.get("type") == "dense":
            l["weights"] = [(0.5 * np.asarray(w)).tolist() for w in l["weights"]]
    name = "2x16_relu"
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        tf._DTYPE = dt
        wdf, layers = fresh_lib()
        ns = {"tf": tf, "wdf": wdf, "np": np, "DenseRootModel": layers.DenseRootModel, "DenseLayer": layers.DenseLayer, "C_val": C_val, "FS": FS}
        extract(os.path.join(REF, "wdf_py/diode_clipper/clipper_pot.py"), {"ClipperModel", "esr_loss", "eps", "mse_loss", "loss_func"}, ns)
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):
            model = ns["ClipperModel"](mj)
        outs = tf.transpose(model.forward(data)[..., 0], perm=[1, 0, 2])
        tgt = tf.constant(target)
        loss = ns["loss_func"](outs[:, skip:, :], tgt[:, skip:, :])
        tv = model.trainable_variables
        grads = torch.autograd.grad(loss, tv)
        out[f"{name}_y_{tag}"] = npy(outs)[:, :, 0].T
        out[f"{name}_loss_{tag}"] = npy(loss)
        dl = [l for l in model.model.layers if isinstance(l, layers.DenseLayer)]
        order = []
        for l in dl:
            order += [l.kernel, l.bias]
        idx = [next(i for i, v in enumerate(tv) if v is p) for p in order]
        out[f"{name}_grad_{tag}"] = np.concatenate([npy(grads[i]).ravel() for i in idx])
        if tag == "f64":
            out[f"{name}_theta"] = np.concatenate([npy(p).ravel() for p in order])
            out[f"{name}_sizes"] = np.array([2] + [l.bias.shape[-1] for l in dl])
            acts = []
            for i, l in enumerate(model.model.layers):
                if isinstance(l, layers.DenseLayer):
                    nxt = model.model.layers[i + 1] if i + 1 < len(model.model.layers) else None
                    acts.append(1 if nxt is tf.nn.tanh else (2 if nxt is tf.nn.relu else 0))
            out[f"{name}_acts"] = np.array(acts)
    print("g9", name, out[f"{name}_loss_f32"], out[f"{name}_loss_f64"], out[f"{name}_sizes"], out[f"{name}_acts"],
          "max |y|", float(np.max(np.abs(out[f"{name}_y_f64"]))))
    out["C"], out["skip"] = C_val, skip
    np.savez(os.path.join(HERE, "g9_mlp_relu.npz"), **out)


def g10_reference_models():
    root = os.path.join(REF, "wdf_py", "diode_clipper", "models")
    names, chunks = [], []
    for dp, dn, fns in sorted(os.walk(root)):
        dn.sort()
        if os.path.basename(dp) == "old":
            continue
        for fn in sorted(fns):
            if fn.endswith(".json"):
                names.append(os.path.relpath(os.path.join(dp, fn), root))
                chunks.append(np.frombuffer(open(os.path.join(dp, fn), "rb").read(), dtype=np.uint8))
    print("g10", len(names), "model files,", sum(c.size for c in chunks), "bytes")
    np.savez_compressed(os.path.join(HERE, "g10_reference_models.npz"), names=np.array(names),
                        blob=np.concatenate(chunks), ends=np.cumsum([c.size for c in chunks]))


if __name__ == "__main__":
    which = sys.argv[1:] or ["g1", "g2", "g3", "g4", "g5", "g6", "g7", "g8"]
    fns = {"g1": g1_rc_lowpass, "g2": g2_voltage_divider, "g3": g3_mlp_clipper,
           "g4": g4_diode_pair, "g5": g5_omega, "g6": g6_diode_clipper, "g7": g7_recorded_programs,
           "g8": g8_dataimport, "g9": g9_mlp_relu, "g10": g10_reference_models}
    for w in which:
        fns[w]()
