#!/usr/bin/env python3
"""Host time per call of the one-pass step wrappers of wdf_hip/binding.py, this checkout against another one (the parent commit
in a second worktree) on one GPU in one session.

    python tools/binding_host_time.py --other <path of the other checkout> [--what wrappers bench] [--rounds 3] [--out FILE]
    python tools/binding_host_time.py --worker <path of a checkout> --label <text>        # what the driver starts; one JSON line

The driver starts one fresh worker process per checkout and round, the other checkout first, the two alternating, each under its
own time limit, and stops at the first that fails.  A worker imports THAT checkout's package and times every wrapper with every
buffer preallocated at the shortest T its export accepts (one chunk unit: 32 steps for the clipper, 8 for the others), B = 64, one
chunk: 200 untimed calls, then 5 blocks of 2000 calls, a synchronise after each block and none inside; per wrapper it reports the
five per-call block times and their median (microseconds).  A checkout whose asym wrappers do not take rseq= is given _rseq=.
The driver then prints, per wrapper, both checkouts' medians of each round and whether this checkout's median of medians is no
higher than the other's slowest round median; --what bench runs bench.py's default run in both checkouts the same way (value per
round; higher is better there).  Every line is appended to --out as it comes."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, BLOCKS, CALLS = 200, 5, 2000
FS, B = 48000.0, 64


def wrappers(wb, torch, np):
    """name -> a zero-argument callable: one call of the wrapper with every buffer preallocated."""
    import inspect
    import tf_wdf as W
    dev = "cuda"
    rng = np.random.default_rng(0)
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)  # noqa: E731
    empty = lambda *s, dtype=torch.float32: torch.empty(s, dtype=dtype, device=dev)  # noqa: E731
    out = {}

    # the clipper: T = 32
    T, eps = 32, float(np.finfo(float).eps)
    x, tgt = f32(0.5 * rng.standard_normal((B, T))), f32(0.3 * rng.standard_normal((T, B)))
    from wdf_hip import workload
    theta = f32(workload.clipper_theta())
    c = dict(y=empty(T, B), ws=wb.step_mse_workspace(B, 1, dev), status=empty(4, dtype=torch.int32))
    g4, sse, s10, l3 = empty(4), empty(1), empty(10), empty(3)
    out["clipper_step_mse_tp"] = lambda: wb.clipper_step_mse_tp(x, theta, FS, tgt, 2.0 / (B * T), 1, 0, gtheta=g4, sse=sse, **c)
    out["clipper_step_esr_tp"] = lambda: wb.clipper_step_esr_tp(x, theta, FS, tgt, float(B * T), eps, 0, 1, 0, sums10=s10, gtheta=g4,
                                                                loss3=l3, **c)
    _, zs, zT = wb.clipper_fwd(x, theta, FS, want_stash=True, want_zT=True)
    opt, th_a, ws_b = wb.Adam(4, 0.0), theta.clone(), wb.bwd_tp_workspace(B, 1, dev)         # lr 0: theta stays where it is
    out["clipper_bwd_mse_tp_adam"] = lambda: wb.clipper_bwd_mse_tp_adam(x, th_a, FS, zs, zT, tgt, 2.0 / (B * T), 1, opt, gtheta=g4,
                                                                        sse=sse, ws=ws_b)
    out["esr_finish"] = lambda: wb.esr_finish(s10, float(B * T), eps, gtheta=g4, loss3=l3)

    # the two-different-diode clipper: T = 8, with and without a pot per sequence
    T = 8
    x8, tgt8 = f32(0.5 * rng.standard_normal((B, T))), f32(0.3 * rng.standard_normal((T, B)))
    th6 = f32([4.352e-9, 25.85e-3 * 1.906, 2.0e-6, 25.85e-3 * 1.4, 45.0e3, 4.7e-9])
    pots = f32(np.linspace(10.0e3, 99.1e3, B))
    key = "rseq" if "rseq" in inspect.signature(wb.clipper_asym_step_mse).parameters else "_rseq"
    L, mode = wb.lib(), wb.ASYM_NEWTON_F32
    am = dict(y=empty(T, B), ws=empty(L.wdf_clipper_asym_step_mse_ws_bytes(B, 1), dtype=torch.uint8), status=empty(4, dtype=torch.int32),
              out7=empty(7))
    ae = dict(y=am["y"], ws=empty(L.wdf_clipper_asym_step_esr_ws_bytes(B, 1), dtype=torch.uint8), status=am["status"], sums14=empty(14),
              gtheta6=empty(6), loss3=l3)
    for tag, kw in (("", {}), ("[rseq]", {key: pots})):
        out["clipper_asym_step_mse" + tag] = lambda kw=kw: wb.clipper_asym_step_mse(x8, th6, FS, mode, tgt8, 2.0 / (B * T), 1, 0, **am, **kw)
        out["clipper_asym_step_esr" + tag] = lambda kw=kw: wb.clipper_asym_step_esr(x8, th6, FS, mode, tgt8, float(B * T), eps, 0, 1, 0,
                                                                                    **ae, **kw)
    out["asym_esr_finish"] = lambda: wb.asym_esr_finish(ae["sums14"], float(B * T), eps, gtheta6=ae["gtheta6"], loss3=l3)

    # a tree under the two-different-diode root: HPFDiodeClipper's (one state, one input), the smallest the step is built for
    R, Vs, C = W.Resistor(33.0e3, True), W.ResistiveVoltageSource(1.0e3, trainable=True), W.Capacitor(22.0e-9, FS, True)
    top = W.Parallel(R, W.Series(Vs, C))
    dp = W.AsymDiodePair(top, 4.352e-9, 2.0e-6, nDiodes_up=1.906, nDiodes_down=1.4, trainable=True, any_tree=True)
    circ = W.Circuit(top, dp, R)
    coef64, r_port = circ.matrices()
    coef = coef64.float().to(dev).contiguous()
    rootp = f32([float(torch.as_tensor(v).detach()) for v in (dp.Is_up, dp.nVt_up, dp.Is_down, dp.nVt_down, r_port)])
    ns, ni, ng = circ.ns, circ.ni, coef.numel() + 5
    xs = x8.unsqueeze(-1).contiguous()
    s = dict(y=empty(T, B), ws=empty(L.wdf_ss_asym_step_ws_bytes(ns, ni, B, T, 1), dtype=torch.uint8), status=empty(4, dtype=torch.int32))
    so, ss_, sg = empty(1 + ng), empty(2 + 2 * ng), empty(ng)
    out["ss_asym_step_mse"] = lambda: wb.ss_asym_step_mse(xs, coef, rootp, ns, ni, tgt8, 2.0 / (B * T), 1, 0, out=so, **s)
    out["ss_asym_step_esr"] = lambda: wb.ss_asym_step_esr(xs, coef, rootp, ns, ni, tgt8, float(B * T), eps, 0, 1, 0, sums=ss_, g=sg, loss3=l3,
                                                          **s)

    # a linear tree: no state, one input, three parameters
    x_tm = f32(0.5 * rng.standard_normal((T, 1, B)))
    lcoef = f32([0.5] * L.wdf_ss_ncoef(0, 1))
    jac = torch.as_tensor(rng.standard_normal((lcoef.numel(), 3)), device=dev)
    y_l = empty(T, B)
    ws_m = torch.zeros(L.wdf_ss_lin_step_ws_bytes(0, 1, B, T, 1), dtype=torch.uint8, device=dev)
    ws_e = torch.zeros(L.wdf_ss_lin_step_esr_ws_bytes(0, 1, B, T, 1), dtype=torch.uint8, device=dev)
    out["ss_lin_step_mse"] = lambda: wb.ss_lin_step_mse(x_tm, lcoef, jac, tgt8, 2.0 / (B * T), 1, ws=ws_m, y=y_l)
    out["ss_lin_step_esr"] = lambda: wb.ss_lin_step_esr(x_tm, lcoef, jac, tgt8, 0, 1, ws=ws_e, y=y_l)
    lin_sums, lin_g = wb.ss_lin_step_esr(x_tm, lcoef, jac, tgt8, 0, 1, finish=False)["sums"], empty(3)
    out["ss_lin_esr_finish"] = lambda: wb.ss_lin_esr_finish(lin_sums, float(B * T), g=lin_g, loss3=l3)
    return out


def worker(repo, label):
    sys.path.insert(0, os.path.join(repo, "differentiable-wdfs_amd", "lib"))
    import numpy as np
    import torch
    from wdf_hip import binding as wb
    assert os.path.realpath(wb.__file__).startswith(os.path.realpath(repo)), wb.__file__
    wb.require_gpu()
    rows = {}
    for name, call in wrappers(wb, torch, np).items():
        for _ in range(WARM):
            call()
        torch.cuda.synchronize()
        blocks = []
        for _ in range(BLOCKS):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                call()
            torch.cuda.synchronize()
            blocks.append((time.perf_counter() - t0) / CALLS * 1e6)
        rows[name] = {"median_us": round(statistics.median(blocks), 3), "blocks_us": [round(b, 3) for b in blocks]}
    print(json.dumps({"kind": "binding_host_time", "label": label, "binding_lines": sum(1 for _ in open(wb.__file__)),
                      "B": B, "warm": WARM, "blocks": BLOCKS, "calls": CALLS, "wrappers": rows}), flush=True)


def run(cmd, limit, cwd=None):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(cmd)} ended with {p.returncode}: nothing more is started")
    return [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")][-1]


def verdict(new, other):
    """this checkout's median of the rounds' medians against the other's slowest and fastest round"""
    m = statistics.median(new)
    return {"new_us": new, "other_us": other, "new_median": round(m, 3), "other_slowest": max(other), "other_spread": round(max(other) - min(other), 3),
            "holds": m <= max(other), "over_by": round(max(0.0, m - max(other)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--label", default="")
    ap.add_argument("--other")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--what", nargs="+", default=["wrappers"], choices=["wrappers", "bench"],
                    help="wrappers: the host time per call; bench: bench.py's default run in both checkouts, alternating the same way")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "binding_host_time.jsonl"), help="appended to")
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.worker), a.label)
    if not a.other:
        ap.error("--other <path of the checkout to compare with>")
    sides = (("other", os.path.abspath(a.other)), ("new", HERE))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "a")

    def keep(line):
        out.write(json.dumps(line) + "\n")
        out.flush()

    if "wrappers" in a.what:
        host = {"other": [], "new": []}
        for rnd in range(a.rounds):
            for label, repo in sides:
                r = run([sys.executable, os.path.abspath(__file__), "--worker", repo, "--label", label], 240)
                keep(dict(r, round=rnd))
                host[label].append(r["wrappers"])
                print(f"round {rnd} {label}: {len(r['wrappers'])} wrappers timed", flush=True)
        table = {n: verdict([w[n]["median_us"] for w in host["new"]], [w[n]["median_us"] for w in host["other"]]) for n in host["new"][0]}
        keep({"kind": "summary", "wrappers": table})
        for n, v in table.items():
            print(f"{n:32s} new {v['new_us']} median {v['new_median']}  other {v['other_us']}  holds {v['holds']} over_by {v['over_by']} us")
    if "bench" in a.what:
        bench = {"other": [], "new": []}
        for rnd in range(a.rounds):
            for label, repo in sides:
                r = run([sys.executable, "bench.py", "--gpus", "1"], 400, cwd=repo)
                keep({"kind": "bench", "label": label, "round": rnd, "value": r.get("value"), "unit": r.get("unit"),
                      "ms_per_step": r.get("ms_per_step"), "lib_sha16": (r.get("library") or {}).get("sha16")})
                bench[label].append(r.get("value"))
                print(f"round {rnd} {label}: bench.py {r.get('value'):.6g} {r.get('unit')}", flush=True)
        nb, ob = bench["new"], bench["other"]                   # samples/s: higher is better, the other's slowest run is its lowest
        v = {"kind": "summary", "bench": {"new": nb, "other": ob, "new_median": statistics.median(nb), "other_slowest": min(ob),
                                          "other_spread": max(ob) - min(ob), "holds": statistics.median(nb) >= min(ob)}}
        keep(v)
        print(v)


if __name__ == "__main__":
    main()
