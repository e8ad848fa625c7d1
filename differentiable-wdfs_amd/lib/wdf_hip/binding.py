"""ctypes binding of libwdf_hip.so (C ABI: include/wdf_hip.h).

PyTorch is used here only as plumbing: it owns device memory (tensor.data_ptr()) and the
HIP stream the kernels are enqueued on.  There is NO fallback: if the HIP library is
missing or a call fails, this raises -- the product never computes on the CPU.
"""
import ctypes as C
import os

import numpy as np

import torch

from .tensor_cache import ObjectMemo

_HERE = os.path.dirname(os.path.abspath(__file__))
# WDF_HIP_LIB: another build of the same library (A/B timing of kernel variants on one box)
LIB_PATH = os.environ.get("WDF_HIP_LIB") or os.path.join(_HERE, "libwdf_hip.so")

WDF_X_TIME_MAJOR = 1 << 0
WDF_PREC_F64 = 1 << 1
WDF_GENERAL_ROOT = 1 << 3
WDF_MLP_LANE_PER_SEQUENCE = 1 << 4
WDF_ONE_SEQUENCE_PER_LANE = 1 << 5
WDF_R_PER_SEQUENCE = 1 << 6
WDF_NO_Y_STORE = 1 << 7

# Set True to run the one-lane-per-sequence MLP kernels (csrc/wdf_mlp.h) instead of the default
# 16-lane row per sequence (csrc/wdf_mlp_row.h): parity tests and A/B timing.
MLP_LANE_PER_SEQUENCE = False

# Set True to run the one-pass step with one sequence per lane even for even batches (WDF_ONE_SEQUENCE_PER_LANE)
ONE_SEQUENCE_PER_LANE = os.environ.get("WDF_ONE_SEQUENCE_PER_LANE", "") not in ("", "0")     # (env: A/B runs of bench.py)

# Set True to make every clipper call take the general per-step root evaluation (WDF_GENERAL_ROOT):
# parity tests compare it with the default path, tools time one against the other on the same box.
GENERAL_ROOT = False


ABI_VERSION = 6                # include/wdf_hip.h WDF_HIP_ABI_VERSION


def _root_flag():
    return WDF_GENERAL_ROOT if GENERAL_ROOT else 0


class WdfHipError(RuntimeError):
    pass


_lib = None


# ---- the C ABI, once: name -> (restype, argtypes) of every declaration in include/wdf_hip.h (tests/test_cabi_cpu.py compares
# the two, parameter by parameter) ------------------------------------------------------------------------------------------
_p, _i64, _ci, _cf, _cd, _sz = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_double, C.c_size_t
_ip, _dp, _i64p, _f32p = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_float)
_ADAM = [_p, _p, _p, _p, _cf, _cf, _cf, _p, _p]                        # m, v, step, lr, beta1, beta2, eps, lo, hi
_CLIP = [_p, _p, _p, _cf, _ci, _ci]                                    # x, r, theta, fs, n_up, n_down
_ASYM = [_p, _p, _cf, _ci, _cd, _ci]                                   # x, theta6, fs, mode, tol, max_iter
_MLP = [_p, _p, _p, _p, _ci, _ci, _cf]                                 # x, r, theta2, w, hidden, n_tanh_layers, fs
_SS = [_p, _p, _p, _ci, _ci, _ci, _ci, _ci]                            # x, coef, rootp, ns, ni, root, n_up, n_down
_DYN = [_p, _p, _ci, _ci, _ci, _ci, _p, _p, _ci, _ci, _ci, _ci]        # x, rows, per_sample, ns, ni, root, rootp, w, hidden, n_tanh_layers, n_up, n_down
_STEP_WS = [_ci, _ci, _i64, _i64, _ci]                                 # ns, ni, B, T, n_chunks
_PROBE = [_p, _ci, _p, _p, _ci, _p, _ci, _p, _p, _p, _p]               # tape, n_ops, consts, params, n_params, outs, n_out, coef, coef64, jac, stream
_ROWS = [_ip, _ci, _dp, _ci, _ip, _ci, _p, _ci, _ci, _p]               # ops, n_ops, consts, n_consts, outs, n_out, params, n_params, chan, r

SIGNATURES = {
    "wdf_abi_version": (_ci, []),
    "wdf_last_error": (C.c_char_p, []),
    "wdf_device_info": (_ci, [_ci, C.c_char_p, _ci]),
    "wdf_clipper_fwd": (_ci, _CLIP + [_p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_clipper_bwd": (_ci, _CLIP + [_p, _p, _p, _p, _p, _p, _ci, _i64, _i64, _ci, _p]),
    "wdf_clipper_bwd_ws_bytes": (_sz, [_i64]),
    "wdf_clipper_tp_chunks": (_ci, [_i64, _ci]),
    "wdf_clipper_tp_warm_unit": (_ci, []),
    "wdf_clipper_fwd_tp_ws_bytes": (_sz, [_i64, _ci]),
    "wdf_clipper_fwd_tp": (_ci, _CLIP + [_p, _p, _p, _p, _i64, _i64, _ci, _ci, _cf, _p, _p, _ci, _p]),
    "wdf_clipper_fwd_tp_state_bytes": (_sz, [_i64, _ci, _ci]),
    "wdf_clipper_fwd_tp_state_reset": (_ci, [_p, _i64, _ci, _p]),
    "wdf_clipper_fwd_tp_warm": (_ci, _CLIP + [_p, _p, _p, _p, _i64, _i64, _ci, _ci, _cf, _p, _p, _p, _ci, _ci, _p]),
    "wdf_clipper_bwd_tp_ws_bytes": (_sz, [_i64, _ci]),
    "wdf_clipper_bwd_tp_ws_init": (_ci, [_p, _i64, _ci, _p]),
    "wdf_clipper_bwd_tp": (_ci, _CLIP + [_p, _p, _p, _p, _p, _ci, _i64, _i64, _ci, _ci, _p]),
    "wdf_clipper_bwd_mse_tp": (_ci, _CLIP + [_p, _p, _p, _cf, _p, _p, _p, _p, _ci, _i64, _i64, _ci, _ci, _p]),
    "wdf_clipper_bwd_mse_tp_adam": (_ci, _CLIP + [_p, _p, _p, _cf, _p, _p, _p, _i64, _i64, _ci, _ci] + _ADAM + [_p]),
    "wdf_clipper_step_mse_tp_ws_bytes": (_sz, [_i64, _ci]),
    "wdf_clipper_step_mse_tp_ws_init": (_ci, [_p, _i64, _ci, _p]),
    "wdf_clipper_step_mse_tp": (_ci, _CLIP + [_p, _cf, _i64, _p, _p, _p, _i64, _i64, _ci, _ci, _cf, _p, _p, _p, _ci, _p, _p, _ci]
                                + _ADAM + [_ci, _p]),
    "wdf_clipper_step_esr_tp": (_ci, _CLIP + [_p, _cd, _cd, _i64, _p, _p, _p, _i64, _i64, _ci, _ci, _cf, _p, _p, _p, _ci, _p, _p, _p]
                                + _ADAM + [_ci, _p]),
    "wdf_esr_finish": (_ci, [_p, _cd, _cd, _p, _p, _p]),
    "wdf_loss_sums_ws_bytes": (_i64, []),
    "wdf_loss_sums": (_ci, [_p, _p, _i64, _i64, _i64, _p, _p, _p]),
    "wdf_esr_coef": (_ci, [_p, _cd, _cd, _p, _p, _p]),
    "wdf_loss_esr_grad": (_ci, [_p, _p, _p, _i64, _i64, _i64, _p, _p]),
    "wdf_loss_terms_ws_bytes": (_i64, []),
    "wdf_loss_terms_sums": (_ci, [_p, _p, _i64, _i64, _i64, _cd, _p, _p, _p]),
    "wdf_loss_terms_coef": (_ci, [_p, _cd, _cd, _dp, _cd, _p, _p, _p]),
    "wdf_loss_terms_grad": (_ci, [_p, _p, _p, _cd, _i64, _i64, _i64, _p, _p]),
    "wdf_clipper_bwd_esr_tp": (_ci, _CLIP + [_p, _p, _p, _p, _i64, _p, _p, _p, _p, _ci, _i64, _i64, _ci, _ci, _p]),
    "wdf_clipper_asym_fwd": (_ci, _ASYM + [_p, _p, _p, _p, _p, _i64, _i64, _p]),
    "wdf_clipper_asym_fwd_tp_ws_bytes": (_sz, [_i64, _ci]),
    "wdf_clipper_asym_fwd_tp": (_ci, _ASYM + [_p, _p, _p, _p, _i64, _i64, _ci, _ci, _cf, _p, _p, _p]),
    "wdf_clipper_asym_bwd_ws_bytes": (_sz, [_i64]),
    "wdf_clipper_asym_bwd": (_ci, [_p, _p, _cf, _cd, _ci, _p, _p, _p, _p, _i64, _i64, _p]),
    "wdf_clipper_asym_bwd_tp_ws_bytes": (_sz, [_i64, _ci]),
    "wdf_clipper_asym_bwd_tp": (_ci, [_p, _p, _cf, _ci, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_asym_root": (_ci, _ASYM + [_p, _i64, _p]),
    "wdf_clipper_asym_step_mse_ws_bytes": (_sz, [_i64, _ci]),
    "wdf_clipper_asym_step_mse": (_ci, _ASYM + [_p, _cf, _p, _p, _p, _i64, _i64, _ci, _ci, _cf, _p, _p, _p] + _ADAM + [_p]),
    "wdf_clipper_asym_step_esr_ws_bytes": (_sz, [_i64, _ci]),
    "wdf_clipper_asym_step_esr": (_ci, _ASYM + [_p, _cd, _cd, _i64, _p, _p, _p, _i64, _i64, _ci, _ci, _cf, _p, _p, _p, _p, _p]
                                  + _ADAM + [_p]),
    "wdf_asym_esr_finish": (_ci, [_p, _cd, _cd, _p, _p, _p]),
    "wdf_ss_dyn_row_len": (_ci, [_ci, _ci]),
    "wdf_ss_dyn_fwd": (_ci, _DYN + [_p, _p, _p, _p, _i64, _i64, _p]),
    "wdf_ss_dyn_bwd_ws_bytes": (_sz, [_i64]),
    "wdf_ss_dyn_bwd_root_ws_bytes": (_sz, [_ci, _i64]),
    "wdf_ss_dyn_bwd_tp_root_ws_bytes": (_sz, [_ci, _ci, _i64, _i64, _ci]),
    "wdf_ss_dyn_bwd": (_ci, _DYN + [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _p]),
    "wdf_ss_dyn_fwd_tp_ws_bytes": (_sz, [_ci, _i64, _ci]),
    "wdf_ss_dyn_fwd_tp": (_ci, _DYN + [_p, _p, _p, _p, _i64, _i64, _ci, _ci, _cf, _p, _p, _p, _p]),
    "wdf_ss_dyn_bwd_tp_ws_bytes": (_sz, [_ci, _i64, _i64, _ci]),
    "wdf_ss_dyn_bwd_tp": (_ci, _DYN + [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_ss_dyn_rows": (_ci, _ROWS + [_p, _i64, _i64, _p]),
    "wdf_ss_dyn_rows_bwd_ws_bytes": (_sz, [_ci, _i64, _i64]),
    "wdf_ss_dyn_rows_bwd": (_ci, _ROWS + [_p, _p, _p, _i64, _i64, _p]),
    "wdf_clipper_mlp_wgrad_matrix_core_chunks": (_ci, [_i64, _i64]),
    "wdf_mlp_weight_count": (_ci, [_ci, _ci]),
    "wdf_clipper_mlp_fwd": (_ci, _MLP + [_p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_clipper_mlp_bwd_w_ws_bytes": (_i64, [_ci, _ci, _i64]),
    "wdf_clipper_mlp_bwd_w": (_ci, _MLP + [_p, _p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_clipper_mlp_tp_chunks": (_ci, [_i64, _ci]),
    "wdf_clipper_mlp_fwd_tp_ws_bytes": (_sz, [_i64, _ci]),
    "wdf_clipper_mlp_fwd_tp": (_ci, _MLP + [_p, _p, _p, _p, _i64, _i64, _ci, _ci, _p, _cf, _p, _p, _p]),
    "wdf_clipper_mlp_bwd_w_tp_ws_bytes": (_i64, [_ci, _ci, _i64, _i64, _ci]),
    "wdf_clipper_mlp_bwd_w_tp": (_ci, _MLP + [_p, _p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_clipper_mlp_fwd_tp_kappa": (_ci, _MLP + [_p, _p, _p, _p, _p, _p, _i64, _i64, _ci, _ci, _p, _cf, _p, _p, _p]),
    "wdf_clipper_mlp_tp_starts": (_ci, [_i64, _ci, _ci, _i64p]),
    "wdf_clipper_mlp_bwd_w_tp_kappa": (_ci, _MLP + [_p, _p, _p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_clipper_mlp_bwd_ws_bytes": (_sz, [_i64]),
    "wdf_clipper_mlp_bwd": (_ci, _MLP + [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_mlp_eval": (_ci, [_p, _p, _p, _ci, _ci, _p, _i64, _p]),
    "wdf_mlp_fit_epoch": (_ci, [_p, _p, _p, _i64, _ci, _p, _p, _p, _p, _cf, _cf, _cf, _cf, _cf, _cf, _p, _ci, _ci, _p]),
    "wdf_clipper_mlp_wgrad_ws_bytes": (_i64, [_ci, _ci, _i64]),
    "wdf_clipper_mlp_wgrad": (_ci, [_p, _p, _p, _p, _p, _ci, _ci, _cf, _p, _p, _i64, _p]),
    "wdf_clipper_mlp_step_state_bytes": (_sz, [_ci, _ci, _i64, _i64, _ci, _ci]),
    "wdf_clipper_mlp_step_plan": (_ci, [_p, _ci, _ci, _i64, _i64, _ci, _ci, _ip, _ci, _ci, _ci, _ci, _ci, _cf, _p]),
    "wdf_clipper_mlp_step_read": (_ci, [_p, _ci, _ci, _i64, _i64, _ci, _ci, _ip, _ip, _ip, _ip, _f32p, _p]),
    "wdf_clipper_mlp_step_set": (_ci, [_p, _ci, C.c_int32, _p]),
    "wdf_clipper_mlp_step_set_wcol": (_ci, [_p, _ci, _ci, _i64, _i64, _ci, _ci, _ip, _p]),
    "wdf_clipper_mlp_step_prepare": (_ci, [_p, _p, _cf, _i64, _i64, _p, _p, _p]),
    "wdf_clipper_mlp_step": (_ci, [_p, _p, _p, _p, _p, _ci, _ci, _ci, _cf, _p, _i64, _cd, _cd, _p, _p, _p, _p, _i64, _i64, _ci, _ci, _ci,
                                   _p, _p, _p, _p, _p, _p, _p, _p, _cf, _cf, _cf, _p]),
    "wdf_ss_probe": (_ci, _PROBE),
    "wdf_ss_probe_adam": (_ci, [_p, _ci] + _PROBE),
    "wdf_ss_lin_step_ws_bytes": (_sz, _STEP_WS),
    "wdf_ss_lin_step_mse": (_ci, [_p, _p, _p, _ci, _ci, _ci, _p, _cf, _p, _p, _p, _p, _p, _i64, _i64, _ci, _p, _p, _p]),
    "wdf_ss_lin_step_esr_ws_bytes": (_sz, _STEP_WS),
    "wdf_ss_lin_step_esr": (_ci, [_p, _p, _p, _ci, _ci, _ci, _p, _cd, _cd, _i64, _p, _p, _p, _p, _p, _p, _i64, _i64, _ci, _p, _p, _p]),
    "wdf_ss_lin_esr_finish": (_ci, [_p, _ci, _cd, _cd, _p, _p, _p]),
    "wdf_ss_nl_step_ws_bytes": (_sz, _STEP_WS),
    "wdf_ss_nl_step_chunk_len": (_ci, [_i64, _ci]),
    "wdf_ss_nl_step_plan": (_ci, [_p, _ci, _ci, _i64, _i64, _ci, _ci, _ci, _ci, _ci, _cf, _p]),
    "wdf_ss_nl_step_set": (_ci, [_p, _ci, _cd, _p]),
    "wdf_ss_nl_step_read": (_ci, [_p, _p, _p]),
    "wdf_ss_nl_step_mse": (_ci, [_p, _p, _p, _p, _ci, _ci, _ci, _ci, _ci, _p, _cf, _p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_ss_nl_step_esr_ws_bytes": (_sz, _STEP_WS),
    "wdf_ss_nl_step_esr": (_ci, [_p, _p, _p, _p, _ci, _ci, _ci, _ci, _ci, _p, _i64, _cd, _p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_ss_ncoef": (_ci, [_ci, _ci]),
    "wdf_ss_fwd": (_ci, _SS + [_p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_ss_fwd_lin_tp_ws_bytes": (_sz, [_ci, _i64, _ci]),
    "wdf_ss_fwd_lin_tp": (_ci, [_p, _p, _ci, _ci, _p, _p, _p, _p, _i64, _i64, _ci, _p, _p]),
    "wdf_ss_bwd": (_ci, _SS + [_p, _p, _p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_ss_bwd_ws_bytes": (_sz, [_ci, _ci, _i64]),
    "wdf_ss_tp_chunks": (_ci, [_i64, _ci]),
    "wdf_ss_tp_starts": (_ci, [_i64, _ci, _ci, _i64p]),
    "wdf_ss_fwd_tp_ws_bytes": (_sz, [_ci, _i64, _ci]),
    "wdf_ss_fwd_tp": (_ci, [_p, _p, _p, _ci, _ci, _ci, _ci, _p, _p, _p, _p, _i64, _i64, _ci, _ci, _cf, _p, _p, _p, _p]),
    "wdf_ss_fwd_tp_root": (_ci, _SS + [_p, _p, _p, _p, _i64, _i64, _ci, _ci, _cf, _p, _p, _p, _p]),
    "wdf_ss_bwd_tp_ws_bytes": (_sz, [_ci, _ci, _i64, _ci]),
    "wdf_ss_bwd_tp": (_ci, _SS + [_p, _p, _p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_ss_bwd_gx_ws_bytes": (_sz, [_ci, _i64, _ci]),
    "wdf_ss_bwd_gx": (_ci, _SS + [_p, _p, _p, _p, _p, _i64, _i64, _ci, _p]),
    "wdf_ss_asym_step_ws_bytes": (_sz, _STEP_WS),
    "wdf_ss_asym_step_esr_ws_bytes": (_sz, _STEP_WS),
    "wdf_ss_asym_step_mse": (_ci, [_p, _p, _p, _ci, _ci, _p, _cf, _p, _p, _p, _i64, _i64, _ci, _ci, _cf, _p, _p, _p, _p]),
    "wdf_ss_asym_step_esr": (_ci, [_p, _p, _p, _ci, _ci, _p, _cd, _cd, _i64, _p, _p, _p, _i64, _i64, _ci, _ci, _cf, _p, _p, _p, _p, _p, _p]),
    "wdf_omega_f32": (_ci, [_p, _p, _p, _i64, _p]),
    "wdf_omega_f64": (_ci, [_p, _p, _p, _i64, _p]),
    "wdf_diode_pair_f32": (_ci, [_p, _p, _cf, _cf, _ci, _ci, _p, _i64, _p]),
    "wdf_adam_step": (_ci, [_p, _p] + _ADAM + [_ci, _p]),
    "wdf_adam_step_multi": (_ci, [_p, _ci, _p]),
    "wdf_event_create": (_p, []),
    "wdf_event_record": (_ci, [_p, _p]),
    "wdf_event_elapsed_ms": (_ci, [_p, _p, _f32p]),
    "wdf_event_destroy": (None, [_p]),
    "wdf_event_bracket_next": (None, [_p, _p]),
    "wdf_clock_stamp": (_ci, [_p, _p]),
}
# one pot resistance per sequence: the static twins' argument lists with rseq behind x
for _twin in ("wdf_clipper_asym_fwd", "wdf_clipper_asym_fwd_tp", "wdf_clipper_asym_bwd_tp", "wdf_clipper_asym_step_mse",
              "wdf_clipper_asym_step_esr"):
    SIGNATURES[_twin + "_rseq"] = (_ci, SIGNATURES[_twin][1][:1] + [_p] + SIGNATURES[_twin][1][1:])
# the linear one-pass steps without y: their bases' argument lists less the y pointer (argument 8 of the MSE step, 10 of MSE + ESR)
for _twin, _at in (("wdf_ss_lin_step_mse", 8), ("wdf_ss_lin_step_esr", 10)):
    SIGNATURES[_twin + "_noy"] = (_ci, SIGNATURES[_twin][1][:_at] + SIGNATURES[_twin][1][_at + 1:])
# the clipper's loss-only evaluation pass: the MSE + ESR step's arguments up to max_warm_tiles (theta const), then sums, loss3, flags, stream
SIGNATURES["wdf_clipper_eval_tp_ws_bytes"] = SIGNATURES["wdf_clipper_step_mse_tp_ws_bytes"]
SIGNATURES["wdf_clipper_eval_tp_ws_init"] = SIGNATURES["wdf_clipper_step_mse_tp_ws_init"]
SIGNATURES["wdf_clipper_eval_tp"] = (_ci, SIGNATURES["wdf_clipper_step_esr_tp"][1][:22] + [_p, _p, _ci, _p])
# the MLP-root clipper's loss-only evaluation pass: the resident step's head up to y (x, p, lr, theta2, w, hidden, n_layers,
# activation, fs, target, skip, n_global, eps_energy, y), then state, B, T, n_items, sums, loss3, stream
SIGNATURES["wdf_clipper_mlp_eval"] = (_ci, SIGNATURES["wdf_clipper_mlp_step"][1][:14] + [_p, _i64, _i64, _ci, _p, _p, _p])
# the diode-root trees' loss-only evaluation pass: the step's workspace walk, plan, set and read; the entry point takes the MSE + ESR
# step's head less jac (x, coef, params, n_tree, ns, ni, n_up, n_down, target, skip), then n_global, eps, y, ws, sums, loss3, B, T,
# n_chunks, stream
for _fn in ("ws_bytes", "plan", "set", "read"):
    SIGNATURES["wdf_ss_nl_eval_" + _fn] = SIGNATURES["wdf_ss_nl_step_" + _fn]
_nl = SIGNATURES["wdf_ss_nl_step_esr"][1]
SIGNATURES["wdf_ss_nl_eval"] = (_ci, _nl[:3] + _nl[4:11] + [_cd, _cd, _p, _p, _p, _p, _i64, _i64, _ci, _p])
# the linear trees' loss-only evaluation pass: the step's workspace arguments; x, coef, ns, ni, target, skip, n_global, eps_energy,
# gscale, y, ws, sums, loss3, loss_out, B, T, n_chunks, z0, zT, stream
SIGNATURES["wdf_ss_lin_eval_ws_bytes"] = (_sz, _STEP_WS)
SIGNATURES["wdf_ss_lin_eval"] = (_ci, [_p, _p, _ci, _ci, _p, _i64, _cd, _cd, _cf, _p, _p, _p, _p, _p, _i64, _i64, _ci, _p, _p, _p])
# the Gauss-Newton form of the two-different-diode clipper's MSE step: that step's arguments without the Adam tail (out28 for out7)
SIGNATURES["wdf_clipper_asym_step_gn_ws_bytes"] = SIGNATURES["wdf_clipper_asym_step_mse_ws_bytes"]
SIGNATURES["wdf_clipper_asym_step_gn"] = (_ci, SIGNATURES["wdf_clipper_asym_step_mse"][1][:-len(_ADAM) - 1] + [_p])
# the Gauss-Newton form of the linear trees' MSE step: that step's arguments (out and the matrix before the Jacobian are double)
SIGNATURES["wdf_ss_lin_step_gn_ws_bytes"] = (_sz, _STEP_WS)
SIGNATURES["wdf_ss_lin_step_gn"] = (_ci, list(SIGNATURES["wdf_ss_lin_step_mse"][1]))
EXPORTED_SYMBOLS = tuple(SIGNATURES)


def lib():
    """Load libwdf_hip.so (once).  Raises WdfHipError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WdfHipError(
            f"{LIB_PATH} not found: build it with `make -C differentiable-wdfs_amd/csrc` "
            "(or __graft_entry__.build()). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.wdf_abi_version.restype = _ci
    if L.wdf_abi_version() != ABI_VERSION:
        raise WdfHipError(f"{LIB_PATH} has ABI version {L.wdf_abi_version()}, this host layer needs {ABI_VERSION}: "
                          "rebuild it (make -C differentiable-wdfs_amd/csrc)")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _check(rc, what):
    if rc != 0:
        raise WdfHipError(f"{what} failed (rc={rc}): {lib().wdf_last_error().decode()}")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    # torch's current stream on the current device, as the raw hipStream_t (no Stream object: this runs per launch)
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _f32_dev(t, name):
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise WdfHipError(f"{name}: expected a contiguous float32 tensor on the GPU, got "
                          f"{type(t).__name__} {getattr(t, 'dtype', None)} {getattr(t, 'device', None)}")
    return t


_GPU_SEEN = False


def require_gpu():
    """(A device once seen stays visible for the life of the process: torch is asked until it says yes, not at every launch.)"""
    global _GPU_SEEN
    if not _GPU_SEEN:
        if not torch.cuda.is_available():
            raise WdfHipError("no HIP device visible: the WDF engine runs on MI355X only (no CPU fallback)")
        _GPU_SEEN = True


# ---- what the one-pass step wrappers share: a buffer handed in is checked and handed back as it is, a missing one allocated on
# the device of `like` (an input of the call: its device is looked up only where something is allocated) -----------------------------
def _out(t, n, name, holds, like):
    """The float32 output `name` of n elements (`holds` says which, for the refusal)."""
    if t is None:
        return torch.empty((n,), dtype=torch.float32, device=like.device)
    if isinstance(t, torch.Tensor) and t.numel() == n and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous():
        return t                                    # (what _f32_dev asks for, without the call: this runs per buffer and launch)
    _f32_dev(t, name)
    raise WdfHipError(f"{name} must hold {holds} ({n} floats)")


def _no_y(who, y, store_y):
    """store_y=False (the training-only steps: y is never stored) with a y handed in: refused before anything else is looked
    at -- the buffer would silently stay unwritten."""
    if not store_y and y is not None:
        raise WdfHipError(f"{who}: y= was given together with store_y=False: the step would leave it unwritten")


def _y_zT(y, want_zT, T, B, like, ns=None, store_y=True):
    """y [T,B] (None with store_y=False: none is allocated), and zT ([B]; [ns,B] for a tree) where the final state is wanted."""
    if not store_y:
        y = None
    elif y is None:
        y = torch.empty((T, B), dtype=torch.float32, device=like.device)
    elif tuple(_f32_dev(y, "y").shape) != (T, B):
        raise WdfHipError(f"y must be [T,B] = [{T},{B}]")
    zT = torch.empty((B,) if ns is None else (ns, B), dtype=torch.float32, device=like.device) if want_zT else None
    return y, zT


def _ws(ws, need, like, zeroed=False):
    """The workspace of `need` bytes (what the step's *_ws_bytes export reports)."""
    if ws is None:
        return (torch.zeros if zeroed else torch.empty)((need,), dtype=torch.uint8, device=like.device)
    if not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.is_contiguous()):
        raise WdfHipError("ws must be a contiguous tensor on the GPU")
    if ws.numel() * ws.element_size() < need:
        raise WdfHipError(f"ws holds {ws.numel() * ws.element_size()} bytes, the step needs {need}")
    return ws


def _esr_outs(finish, g, n, gname, loss3, like):
    """(g [n], loss3 [3]) of an MSE + ESR step that finishes itself; (None, None) where the caller all-reduces the sums first."""
    if not finish:
        return None, None
    return _out(g, n, gname, "one gradient per parameter", like), _out(loss3, 3, "loss3", "{mse, esr, mse + esr}", like)


_NO_ADAM = (None, None, None, None, 0.0, 0.0, 0.0, None, None)


def _adam_args(opt):
    """The nine Adam arguments {m, v, step, lr, beta1, beta2, eps, lo, hi} of an export that applies `opt`."""
    return _ptr(opt.m), _ptr(opt.v), _ptr(opt.step), _ptr(opt.lr), opt.b1, opt.b2, opt.eps, _ptr(opt.lo), _ptr(opt.hi)


def _adam_tail(opt, n, who, holds, finish=True):
    """The Adam arguments of a step that updates its n parameters in its own last launch; nulls without an optimizer.  A step
    that does not finish (one shard of several) forms no gradient to apply."""
    if opt is None:
        return _NO_ADAM
    if opt.n != n:
        raise WdfHipError(f"{who}: the optimizer holds {holds}")
    if not finish:
        raise WdfHipError(f"{who}: the optimizer needs finish=True")
    return _adam_args(opt)


def _clipper_flags(time_major, fp64=False):
    return (WDF_X_TIME_MAJOR if time_major else 0) | _root_flag() | (WDF_PREC_F64 if fp64 else 0)


def _clipper_step_flags(r, time_major, store_y=True):
    return (_clipper_flags(time_major) | (WDF_ONE_SEQUENCE_PER_LANE if ONE_SEQUENCE_PER_LANE else 0) |
            (WDF_R_PER_SEQUENCE if r_is_per_sequence(r, time_major) else 0) | (0 if store_y else WDF_NO_Y_STORE))


def _esr_finish(export, sums, sname, n, lead, n_global, eps, g, gname, loss3):
    """The body of esr_finish, asym_esr_finish and ss_lin_esr_finish (export: lib().wdf_*_esr_finish; lead: what it takes between
    sums and n_global): sums = {S, E, gP[n], gQ[n]} -> (g [n], loss3)."""
    require_gpu()
    if _f32_dev(sums, sname).numel() != 2 + 2 * n:
        raise WdfHipError(f"{sname} must hold {{S, E, gP[{n}], gQ[{n}]}}")
    g, loss3 = _esr_outs(True, g, n, gname, loss3, sums)
    _check(export(_ptr(sums), *lead, float(n_global), float(eps), _ptr(g), _ptr(loss3), _stream()), export.__name__)
    return g, loss3


def omega64(x, want_iters=False):
    """Wright omega in fp64 on the device (toms917's iteration structure); x: float64 device tensor."""
    require_gpu()
    if not (x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()):
        raise WdfHipError("omega64: expected a contiguous float64 device tensor")
    w = torch.empty_like(x)
    it = torch.empty(x.shape, dtype=torch.int32, device=x.device) if want_iters else None
    _check(lib().wdf_omega_f64(_ptr(x), _ptr(w), _ptr(it), x.numel(), _stream()), "wdf_omega_f64")
    return (w, it) if want_iters else w


def clipper_fwd(x, theta, fs, r=None, n_up=1, n_down=1, want_stash=True, z0=None, want_zT=False,
                time_major=False, fp64=False):
    """x [B,T] (or [T,B] if time_major) -> y [T,B], zstash [T,B] | None, zT [B] | None.
    fp64: tree and root arithmetic in double (WDF_PREC_F64; sequential, the accuracy reference on the device)."""
    require_gpu()
    x = _f32_dev(x, "x")
    r = _f32_dev(r, "r")
    theta = _f32_dev(theta, "theta")
    z0 = _f32_dev(z0, "z0")
    if theta.numel() != 4:
        raise WdfHipError("theta must hold {Is, nVt, R, C}")
    B, T = (x.shape[1], x.shape[0]) if time_major else x.shape
    if r is not None and r.shape != x.shape:
        raise WdfHipError("r must have the shape of x")
    y = torch.empty((T, B), dtype=torch.float32, device=x.device)
    zs = torch.empty((T, B), dtype=torch.float32, device=x.device) if want_stash else None
    zT = torch.empty((B,), dtype=torch.float32, device=x.device) if want_zT else None
    flags = _clipper_flags(time_major, fp64)
    rc = lib().wdf_clipper_fwd(_ptr(x), _ptr(r), _ptr(theta), float(fs), int(n_up), int(n_down),
                               _ptr(y), _ptr(zs), _ptr(z0), _ptr(zT), B, T, flags, _stream())
    _check(rc, "wdf_clipper_fwd")
    return y, zs, zT


def clipper_bwd(x, theta, fs, zstash, gy, r=None, n_up=1, n_down=1, want_gz0=False, time_major=False,
                gtheta=None, accumulate=False, ws=None, gzT=None, fp64=False):
    """dL/d{Is, nVt, R, C} as a float32[4] device tensor (and dL/dz0 [B] if requested).
    gzT: optional dL/dzT [B] (a loss that also reads the forward's final state).
    fp64: the adjoint in double (WDF_PREC_F64; sequential, the accuracy reference on the device)."""
    require_gpu()
    x = _f32_dev(x, "x")
    r = _f32_dev(r, "r")
    theta = _f32_dev(theta, "theta")
    zstash = _f32_dev(zstash, "zstash")
    gy = _f32_dev(gy, "gy")
    B, T = (x.shape[1], x.shape[0]) if time_major else x.shape
    if tuple(gy.shape) != (T, B) or tuple(zstash.shape) != (T, B):
        raise WdfHipError(f"gy / zstash must be [T,B] = [{T},{B}]")
    if ws is None:
        ws = torch.empty((lib().wdf_clipper_bwd_ws_bytes(B),), dtype=torch.uint8, device=x.device)
    if gtheta is None:
        gtheta = torch.empty((4,), dtype=torch.float32, device=x.device)
        accumulate = False
    gz0 = torch.empty((B,), dtype=torch.float32, device=x.device) if want_gz0 else None
    flags = _clipper_flags(time_major, fp64)
    rc = lib().wdf_clipper_bwd(_ptr(x), _ptr(r), _ptr(theta), float(fs), int(n_up), int(n_down),
                               _ptr(zstash), _ptr(gy), _ptr(ws), _ptr(gtheta), _ptr(gz0), _ptr(_f32_dev(gzT, "gzT")),
                               1 if accumulate else 0, B, T, flags, _stream())
    _check(rc, "wdf_clipper_bwd")
    return gtheta, gz0


class TpWarmState:
    """Persistent warm-start state of the time-parallel forward for ONE resident input batch
    (include/wdf_hip.h, wdf_clipper_fwd_tp_warm): control block + snapshot ring on the device."""

    def __init__(self, B, T, n_chunks, max_warm_tiles, device, min_warm_tiles=0):
        """max_warm_tiles / min_warm_tiles: in warm-start units of warm_unit() steps (16)."""
        L = lib()
        self.K = L.wdf_clipper_tp_chunks(int(T), int(n_chunks))
        chunk_len = chunk_geom(T, n_chunks, 32)[0]
        # snapshots reach back at most three quarters of a chunk: the one-pass step may shorten the younger chunks by a quarter
        # (skewed spans, csrc/wdf_clipper_fused.h chunk_span) and they must still hold every snapshot
        self.unit = warm_unit()
        self.max_warm_tiles = max(1, min(int(max_warm_tiles), 32, (3 * chunk_len // 4) // self.unit))
        if os.environ.get("WDF_MAX_WARM_TILES"):                # (probing: a shallower snapshot ring, e.g. under WDF_FUSED_SKEW_STEPS)
            self.max_warm_tiles = max(1, min(self.max_warm_tiles, int(os.environ["WDF_MAX_WARM_TILES"])))
        self.B, self.T, self.n_chunks = int(B), int(T), int(n_chunks)
        self.min_warm_tiles = max(0, min(int(min_warm_tiles), self.max_warm_tiles))
        self.buf = torch.empty((L.wdf_clipper_fwd_tp_state_bytes(self.B, self.K, self.max_warm_tiles),),
                               dtype=torch.uint8, device=device)
        self.reset()

    def reset(self):
        _check(lib().wdf_clipper_fwd_tp_state_reset(_ptr(self.buf), self.B, self.min_warm_tiles, _stream()),
               "wdf_clipper_fwd_tp_state_reset")

    def info(self):
        """Host view of the control block (synchronises): snapshot sets available, warm-up tiles the next
        call will run, tiles the last call ran (-1: cold), its largest boundary miss, calls so far."""
        c = self.buf[:96].cpu()
        i, f = c.view(torch.int32), c.view(torch.float32)
        return {"valid": int(i[0]), "next_warm_tiles": int(i[2]), "last_warm_tiles": int(i[3]),
                "last_miss": float(f[12]), "n_calls": int(i[13]), "warm_unit_steps": self.unit, "cold_hold": int(i[20])}


def chunk_geom(T, n_chunks, unit):
    """(L, K): T steps in at most n_chunks chunks of L steps, L a multiple of `unit` -- csrc/wdf_capi_common.h chunk_geom, for
    the families whose count the library does not export (it does: wdf_clipper_tp_chunks, wdf_ss_tp_chunks,
    wdf_clipper_mlp_tp_chunks, wdf_ss_nl_step_chunk_len)."""
    T, unit = int(T), int(unit)
    L = -(-(-(-T // max(1, int(n_chunks)))) // unit) * unit
    return L, -(-T // L)


def warm_unit():
    """Steps per warm-start unit ("warm tile") of the time-parallel clipper kernels."""
    return int(lib().wdf_clipper_tp_warm_unit())


def clipper_fwd_tp(x, theta, fs, n_chunks, warmup, tol=1e-6, r=None, n_up=1, n_down=1, want_stash=True, z0=None,
                   want_zT=False, ws=None, status=None, time_major=False, state=None):
    """Time-parallel forward.  Returns y [T,B], zstash | None, zT | None, status (device int32[4]:
    n_bad, max-miss float bits, chunk re-runs, ticket -- read it with tp_status()).
    state: a TpWarmState kept with this input batch -> warm-started chunks (wdf_clipper_fwd_tp_warm)."""
    require_gpu()
    x = _f32_dev(x, "x")
    r = _f32_dev(r, "r")
    theta = _f32_dev(theta, "theta")
    z0 = _f32_dev(z0, "z0")
    B, T = (x.shape[1], x.shape[0]) if time_major else x.shape
    if r is not None and r.shape != x.shape:
        raise WdfHipError("r must have the shape of x")
    y = torch.empty((T, B), dtype=torch.float32, device=x.device)
    zs = torch.empty((T, B), dtype=torch.float32, device=x.device) if want_stash else None
    zT = torch.empty((B,), dtype=torch.float32, device=x.device) if want_zT else None
    if ws is None:
        ws = torch.empty((lib().wdf_clipper_fwd_tp_ws_bytes(B, int(n_chunks)),), dtype=torch.uint8, device=x.device)
    if status is None:
        status = torch.empty((4,), dtype=torch.int32, device=x.device)
    flags = _clipper_flags(time_major)
    if state is not None:
        if (state.B, state.T, state.n_chunks) != (B, T, int(n_chunks)) or state.buf.device != x.device:
            raise WdfHipError("warm-start state was made for another batch shape / chunking / device")
        rc = lib().wdf_clipper_fwd_tp_warm(_ptr(x), _ptr(r), _ptr(theta), float(fs), int(n_up), int(n_down), _ptr(y),
                                           _ptr(zs), _ptr(z0), _ptr(zT), B, T, int(n_chunks), int(warmup), float(tol),
                                           _ptr(ws), _ptr(status), _ptr(state.buf), state.max_warm_tiles, flags, _stream())
        _check(rc, "wdf_clipper_fwd_tp_warm")
        return y, zs, zT, status
    rc = lib().wdf_clipper_fwd_tp(_ptr(x), _ptr(r), _ptr(theta), float(fs), int(n_up), int(n_down), _ptr(y),
                                  _ptr(zs), _ptr(z0), _ptr(zT), B, T, int(n_chunks), int(warmup), float(tol),
                                  _ptr(ws), _ptr(status), flags, _stream())
    _check(rc, "wdf_clipper_fwd_tp")
    return y, zs, zT, status


def clipper_bwd_mse_tp_adam(x, theta, fs, zstash, zT, target, gscale, n_chunks, opt, r=None, n_up=1, n_down=1,
                            gtheta=None, sse=None, ws=None, time_major=False):
    """The MSE-fused reverse sweep with the Adam update of theta (in place, `opt` = binding.Adam(4, ...))
    folded into its last kernel; -> gtheta[4], sse[1]."""
    require_gpu()
    x, r, theta = _f32_dev(x, "x"), _f32_dev(r, "r"), _f32_dev(theta, "theta")
    zstash, zT, target = _f32_dev(zstash, "zstash"), _f32_dev(zT, "zT"), _f32_dev(target, "target")
    B, T = (x.shape[1], x.shape[0]) if time_major else x.shape
    if opt is None or opt.n != 4 or theta.numel() != 4:
        raise WdfHipError("clipper_bwd_mse_tp_adam: theta and the optimizer hold {Is, nVt, R, C}")
    if ws is None:
        ws = bwd_tp_workspace(B, int(n_chunks), x.device)
    if gtheta is None:
        gtheta = torch.empty((4,), dtype=torch.float32, device=x.device)
    if sse is None:
        sse = torch.empty((1,), dtype=torch.float32, device=x.device)
    rc = lib().wdf_clipper_bwd_mse_tp_adam(_ptr(x), _ptr(r), _ptr(theta), float(fs), int(n_up), int(n_down), _ptr(zstash),
                                           _ptr(zT), _ptr(target), float(gscale), _ptr(ws), _ptr(gtheta), _ptr(sse), B, T,
                                           int(n_chunks), _clipper_flags(time_major), *_adam_args(opt), _stream())
    _check(rc, "wdf_clipper_bwd_mse_tp_adam")
    return gtheta, sse


_R_SEQ_CACHE = ObjectMemo(64)       # (r, layout) -> bool
_R_VEC_CACHE = ObjectMemo(64)       # r [B,T] -> its [B] vector of per-sequence values (r_per_sequence)
R_PER_SEQUENCE = os.environ.get("WDF_R_PER_SEQUENCE", "1") not in ("", "0")     # (0: always the per-sample evaluation, for A/B runs and tests)


def r_is_per_sequence(r, time_major):
    """Is the resistance channel constant along every sequence (the reference's recordings: one pot value per file,
    dataimport.py:96 -- batch_data cuts the sequences out of it)?  One comparison pass per tensor OBJECT and version
    (tensor_cache.ObjectMemo: a fresh channel at a freed one's address may hold a pot that moves): the one-pass step then
    evaluates calc_impedance once per chunk instead of every step (WDF_R_PER_SEQUENCE).  A miss during stream capture answers
    False (the per-sample path is exact for every channel) and caches nothing: the comparison would have to synchronise."""
    if r is None or not R_PER_SEQUENCE:
        return False
    hit = _R_SEQ_CACHE.get(r, bool(time_major))
    if hit is not None:
        return hit
    if r.is_cuda and torch.cuda.is_current_stream_capturing():
        return False
    with torch.no_grad():
        first = r[0:1, :] if time_major else r[:, 0:1]
        return _R_SEQ_CACHE.put(r, bool((r == first).all()), bool(time_major))


def step_mse_workspace(B, n_chunks, device):
    """Workspace of the one-pass training step with its ticket words cleared: allocate once, reuse."""
    ws = torch.empty((lib().wdf_clipper_step_mse_tp_ws_bytes(int(B), int(n_chunks)),), dtype=torch.uint8, device=device)
    _check(lib().wdf_clipper_step_mse_tp_ws_init(_ptr(ws), int(B), int(n_chunks), _stream()), "wdf_clipper_step_mse_tp_ws_init")
    return ws


def eval_workspace(B, n_chunks, device):
    """Workspace of the loss-only evaluation pass (clipper_eval_tp) with its ticket words cleared: allocate once, reuse."""
    ws = torch.empty((lib().wdf_clipper_eval_tp_ws_bytes(int(B), int(n_chunks)),), dtype=torch.uint8, device=device)
    _check(lib().wdf_clipper_eval_tp_ws_init(_ptr(ws), int(B), int(n_chunks), _stream()), "wdf_clipper_eval_tp_ws_init")
    return ws


def _clipper_step_args(who, x, r, theta, target, n_chunks, y, z0, want_zT, ws, status, state, opt, time_major, finish=True,
                       store_y=True, workspace=(step_mse_workspace, "wdf_clipper_step_mse_tp_ws_bytes")):
    """The checks and buffers the two one-pass clipper steps and the evaluation pass share (workspace: who makes one, and the
    export that sizes it)
    -> x, r, theta, target, z0, B, T, K, y, zT, ws, status, (state buffer, max_warm_tiles), Adam tail, flags."""
    _no_y(who, y, store_y)
    require_gpu()
    x, r, theta = _f32_dev(x, "x"), _f32_dev(r, "r"), _f32_dev(theta, "theta")
    target, z0 = _f32_dev(target, "target"), _f32_dev(z0, "z0")
    B, T = (x.shape[1], x.shape[0]) if time_major else x.shape
    if theta.numel() != 4:
        raise WdfHipError("theta must hold {Is, nVt, R, C}")
    if tuple(target.shape) != (T, B):
        raise WdfHipError(f"target must be [T,B] = [{T},{B}]")
    if r is not None and r.shape != x.shape:
        raise WdfHipError("r must have the shape of x")
    if z0 is not None and z0.numel() != B:
        raise WdfHipError(f"z0 must hold one state per sequence ({B})")
    K = lib().wdf_clipper_tp_chunks(T, int(n_chunks))
    y, zT = _y_zT(y, want_zT, T, B, x, store_y=store_y)
    ws = workspace[0](B, K, x.device) if ws is None else _ws(ws, getattr(lib(), workspace[1])(B, K), x)
    if state is not None and ((state.B, state.T, state.K) != (B, T, K) or state.buf.device != x.device):
        raise WdfHipError("warm-start state was made for another batch shape / chunking / device")
    warm = (None, 0) if state is None else (_ptr(state.buf), state.max_warm_tiles)
    if status is None:
        status = torch.empty((4,), dtype=torch.int32, device=x.device)
    return (x, r, theta, target, z0, B, T, K, y, zT, ws, status, warm,
            _adam_tail(opt, 4, who, "{Is, nVt, R, C}", finish), _clipper_step_flags(r, time_major, store_y))


def clipper_step_mse_tp(x, theta, fs, target, gscale, n_chunks, warmup, tol=1e-6, r=None, n_up=1, n_down=1, skip=0, y=None,
                        z0=None, want_zT=False, ws=None, status=None, state=None, gtheta=None, sse=None, accumulate=False,
                        opt=None, time_major=False, store_y=True):
    """The whole MSE training step in one pass over the data (include/wdf_hip.h, wdf_clipper_step_mse_tp):
    forward, loss and d(gscale/2 sum (y - target)^2)/d{Is, nVt, R, C}, x and target read once, y written once, no
    state stash.  n_chunks: time chunks asked for (rounded like wdf_clipper_tp_chunks does); state: a TpWarmState
    made for (B, T, n_chunks); opt: a binding.Adam(4, ...) to update theta in the same launch.
    store_y=False: the training-only step (WDF_NO_Y_STORE) -- y is never stored or allocated, None comes back in its place, a
    y= handed in is refused; everything else is the same call.
    -> y [T,B] | None, zT [B] | None, gtheta[4], sse[1], status (device int32[4], read with tp_status())."""
    x, r, theta, target, z0, B, T, K, y, zT, ws, status, warm, adam, flags = _clipper_step_args(
        "clipper_step_mse_tp", x, r, theta, target, n_chunks, y, z0, want_zT, ws, status, state, opt, time_major, store_y=store_y)
    if gtheta is None:
        accumulate = False
    gtheta = _out(gtheta, 4, "gtheta", "four gradients", x)
    sse = _out(sse, 1, "sse", "one sum", x)
    rc = lib().wdf_clipper_step_mse_tp(
        _ptr(x), _ptr(r), _ptr(theta), float(fs), int(n_up), int(n_down), _ptr(target), float(gscale), int(skip), _ptr(y),
        _ptr(z0), _ptr(zT), B, T, K, int(warmup), float(tol), _ptr(ws), _ptr(status), *warm, _ptr(gtheta), _ptr(sse),
        1 if accumulate else 0, *adam, flags, _stream())
    _check(rc, "wdf_clipper_step_mse_tp")
    return y, zT, gtheta, sse, status


def clipper_step_esr_tp(x, theta, fs, target, n_global, eps_energy, skip, n_chunks, warmup, tol=1e-6, r=None, n_up=1, n_down=1,
                        y=None, z0=None, want_zT=False, ws=None, status=None, state=None, sums10=None, gtheta=None, loss3=None,
                        finish=True, opt=None, time_major=False, store_y=True):
    """The one-pass training step for the scripts' loss MSE + ESR past `skip` (include/wdf_hip.h, wdf_clipper_step_esr_tp).
    finish=True: the kernel finishes the step as a single rank -> gtheta[4], loss3 = {mse, esr, mse + esr} (and the Adam
    update of theta with `opt`).  finish=False: only sums10 = {S, E, gP[4], gQ[4]} of this batch comes back -- all-reduce it
    and call esr_finish.  store_y=False: as clipper_step_mse_tp's (no y stored or allocated, None in its place).
    -> y [T,B] | None, zT | None, sums10, gtheta | None, loss3 | None, status."""
    x, r, theta, target, z0, B, T, K, y, zT, ws, status, warm, adam, flags = _clipper_step_args(
        "clipper_step_esr_tp", x, r, theta, target, n_chunks, y, z0, want_zT, ws, status, state, opt, time_major, finish, store_y)
    sums10 = _out(sums10, 10, "sums10", "{S, E, gP[4], gQ[4]}", x)
    gtheta, loss3 = _esr_outs(finish, gtheta, 4, "gtheta", loss3, x)
    rc = lib().wdf_clipper_step_esr_tp(
        _ptr(x), _ptr(r), _ptr(theta), float(fs), int(n_up), int(n_down), _ptr(target), float(n_global), float(eps_energy),
        int(skip), _ptr(y), _ptr(z0), _ptr(zT), B, T, K, int(warmup), float(tol), _ptr(ws), _ptr(status), *warm, _ptr(sums10),
        _ptr(gtheta), _ptr(loss3), *adam, flags, _stream())
    _check(rc, "wdf_clipper_step_esr_tp")
    return y, zT, sums10, gtheta, loss3, status


def clipper_eval_tp(x, theta, fs, target, n_global, eps_energy, skip, n_chunks, warmup, tol=1e-6, r=None, n_up=1, n_down=1, y=None,
                    store_y=True, z0=None, want_zT=False, ws=None, status=None, state=None, sums=None, loss3=None, time_major=False):
    """The loss-only evaluation pass (include/wdf_hip.h, wdf_clipper_eval_tp): forward and the loss sums S = sum (y - target)^2,
    E = sum y^2 past `skip` in one pass -- no tangent, no gradient, theta untouched.  Arguments as clipper_step_esr_tp's;
    store_y=False: y is never stored or allocated (8 B/sample), None comes back in its place, a y= handed in is refused.
    sums: float64[2] on the device (what several ranks all-reduce before esr_coef); loss3 = {S/n, sqrt(S/(E + eps)/n), their sum}
    with n = n_global.  ws: eval_workspace(B, K, device).
    -> y [T,B] | None, zT [B] | None, sums, loss3, status (device int32[4], read with tp_status())."""
    x, r, theta, target, z0, B, T, K, y, zT, ws, status, warm, _, flags = _clipper_step_args(
        "clipper_eval_tp", x, r, theta, target, n_chunks, y, z0, want_zT, ws, status, state, None, time_major, store_y=store_y,
        workspace=(eval_workspace, "wdf_clipper_eval_tp_ws_bytes"))
    if sums is None:
        sums = torch.empty((2,), dtype=torch.float64, device=x.device)
    elif not (isinstance(sums, torch.Tensor) and sums.dtype == torch.float64 and sums.is_cuda and sums.numel() == 2 and sums.is_contiguous()):
        raise WdfHipError("sums must be a float64[2] device tensor")
    loss3 = _out(loss3, 3, "loss3", "{mse, esr, mse + esr}", x)
    rc = lib().wdf_clipper_eval_tp(
        _ptr(x), _ptr(r), _ptr(theta), float(fs), int(n_up), int(n_down), _ptr(target), float(n_global), float(eps_energy),
        int(skip), _ptr(y), _ptr(z0), _ptr(zT), B, T, K, int(warmup), float(tol), _ptr(ws), _ptr(status), *warm, _ptr(sums),
        _ptr(loss3), flags & ~WDF_NO_Y_STORE, _stream())        # (no y: a null pointer says it, the entry point knows no such flag)
    _check(rc, "wdf_clipper_eval_tp")
    return y, zT, sums, loss3, status


def esr_finish(sums10, n_global, eps_energy, gtheta=None, loss3=None):
    """(gtheta[4], loss3 = {mse, esr, mse + esr}) from the all-reduced sums10 of clipper_step_esr_tp(finish=False)."""
    return _esr_finish(lib().wdf_esr_finish, sums10, "sums10", 4, (), n_global, eps_energy, gtheta, "gtheta", loss3)


def loss_sums(y, target, skip, sums=None, ws=None):
    """S = sum (y - target)^2 and E = sum y^2 over rows skip.. of [T,B] arrays -> float64[2] on the device."""
    require_gpu()
    y, target = _f32_dev(y, "y"), _f32_dev(target, "target")
    T, B = y.shape
    if tuple(target.shape) != (T, B):
        raise WdfHipError("target must have y's shape [T,B]")
    if ws is None:
        ws = torch.empty((lib().wdf_loss_sums_ws_bytes(),), dtype=torch.uint8, device=y.device)
    if sums is None:
        sums = torch.empty((2,), dtype=torch.float64, device=y.device)
    _check(lib().wdf_loss_sums(_ptr(y), _ptr(target), B, T, int(skip), _ptr(ws), _ptr(sums), _stream()), "wdf_loss_sums")
    return sums


def esr_coef(sums, n, eps, gcoef=None, loss=None):
    """(gcoef[2] = {ga, gb}, loss[3] = {mse, esr, mse + esr}) from the global sums; see include/wdf_hip.h."""
    require_gpu()
    if sums.dtype != torch.float64 or not sums.is_cuda or sums.numel() != 2:
        raise WdfHipError("sums must be a float64[2] device tensor")
    if gcoef is None:
        gcoef = torch.empty((2,), dtype=torch.float32, device=sums.device)
    if loss is None:
        loss = torch.empty((3,), dtype=torch.float32, device=sums.device)
    _check(lib().wdf_esr_coef(_ptr(sums), float(n), float(eps), _ptr(gcoef), _ptr(loss), _stream()), "wdf_esr_coef")
    return gcoef, loss


def loss_esr_grad(y, target, gcoef, skip, gy=None):
    """dL/dy [T,B] of MSE + ESR past `skip` from the device coefficients of esr_coef()."""
    require_gpu()
    y, target, gcoef = _f32_dev(y, "y"), _f32_dev(target, "target"), _f32_dev(gcoef, "gcoef")
    T, B = y.shape
    if tuple(target.shape) != (T, B) or gcoef.numel() != 2:
        raise WdfHipError("target must have y's shape [T,B]; gcoef = {ga, gb}")
    if gy is None:
        gy = torch.empty_like(y)
    _check(lib().wdf_loss_esr_grad(_ptr(y), _ptr(target), _ptr(gcoef), B, T, int(skip), _ptr(gy), _stream()), "wdf_loss_esr_grad")
    return gy


def check_loss_weights(weights, coeff):
    """The four weights {mse, esr, esr_emph, avg} (each >= 0, not all 0) and the pre-emphasis coefficient (0 <= c < 1) as
    floats; ValueError otherwise -- what wdf_loss_terms_coef rejects, said before anything touches the device."""
    w = tuple(float(v) for v in weights)
    c = float(coeff)
    if len(w) != 4:
        raise ValueError(f"the loss takes four weights {{mse, esr, esr_emph, avg}}, got {len(w)}")
    if not all(v >= 0.0 for v in w):
        raise ValueError(f"the loss weights {{mse, esr, esr_emph, avg}} must not be negative, got {w}")
    if not sum(w) > 0.0:
        raise ValueError("the loss weights {mse, esr, esr_emph, avg} are all zero")
    if not 0.0 <= c < 1.0:
        raise ValueError(f"the pre-emphasis coefficient must be in [0, 1), got {c}")
    return w, c


def _loss_terms_pair(y, target):
    """y, target as float32 device tensors of one shape [T,B].  Dense, but not necessarily at a 16-byte address: a view that
    starts one float into its storage takes the kernels' scalar loads."""
    y, target = _f32_dev(y, "y"), _f32_dev(target, "target")
    if y.dim() != 2 or tuple(target.shape) != tuple(y.shape):
        raise WdfHipError("y and target must have one shape [T,B]")
    return y, target


def loss_terms_sums(y, target, skip, coeff=0.85, sums6=None, ws=None):
    """sums6 = {S, E, Sp, Ep, So, St} over rows skip.. of [T,B] arrays -> float64[6] on the device (wdf_loss_terms_sums):
    S = sum (y-t)^2, E = sum y^2, Sp / Ep the same behind the pre-emphasis filter v[k] - coeff v[k-1] along time, So = sum y,
    St = sum t.  Fixed-order reduction: the same inputs give the same bits."""
    require_gpu()
    y, target = _loss_terms_pair(y, target)
    T, B = y.shape
    if ws is None:
        ws = torch.empty((lib().wdf_loss_terms_ws_bytes(),), dtype=torch.uint8, device=y.device)
    if sums6 is None:
        sums6 = torch.empty((6,), dtype=torch.float64, device=y.device)
    elif sums6.dtype != torch.float64 or not sums6.is_cuda or sums6.numel() != 6 or not sums6.is_contiguous():
        raise WdfHipError("sums6 must be a float64[6] device tensor")
    _check(lib().wdf_loss_terms_sums(_ptr(y), _ptr(target), B, T, int(skip), float(coeff), _ptr(ws), _ptr(sums6), _stream()),
           "wdf_loss_terms_sums")
    return sums6


def loss_terms_coef(sums6, n, eps, weights, coeff=0.85, gcoef=None, terms=None):
    """(gcoef[6] = {ga, gb, al, be, gm, c}, terms[5] = {mse, esr, esr_emph, avg, loss}) from the global sums6 and sample count n;
    weights = (w_mse, w_esr, w_emph, w_avg); see include/wdf_hip.h (wdf_loss_terms_coef)."""
    require_gpu()
    if sums6.dtype != torch.float64 or not sums6.is_cuda or sums6.numel() != 6 or not sums6.is_contiguous():
        raise WdfHipError("sums6 must be a float64[6] device tensor")
    if len(weights) != 4:
        raise WdfHipError("weights = (w_mse, w_esr, w_emph, w_avg)")
    gcoef, terms = _f32_dev(gcoef, "gcoef"), _f32_dev(terms, "terms")
    if gcoef is None:
        gcoef = torch.empty((6,), dtype=torch.float32, device=sums6.device)
    if terms is None:
        terms = torch.empty((5,), dtype=torch.float32, device=sums6.device)
    if gcoef.numel() != 6 or terms.numel() != 5:
        raise WdfHipError("gcoef holds 6 floats, terms 5")
    w4 = (C.c_double * 4)(*[float(v) for v in weights])
    _check(lib().wdf_loss_terms_coef(_ptr(sums6), float(n), float(eps), w4, float(coeff), _ptr(gcoef), _ptr(terms), _stream()),
           "wdf_loss_terms_coef")
    return gcoef, terms


def loss_terms_grad(y, target, gcoef, skip, coeff=0.85, gy=None):
    """dL/dy [T,B] of the weighted loss past `skip` from the device coefficients of loss_terms_coef() (wdf_loss_terms_grad);
    coeff: the same pre-emphasis coefficient (gcoef[5] is its float32 copy).  Rows before skip are exactly 0."""
    require_gpu()
    y, target = _loss_terms_pair(y, target)
    gcoef = _f32_dev(gcoef, "gcoef")
    T, B = y.shape
    if gcoef.numel() != 6:
        raise WdfHipError("gcoef = {ga, gb, al, be, gm, c}")
    if gy is None:
        gy = torch.empty((T, B), dtype=torch.float32, device=y.device)
    elif _f32_dev(gy, "gy").shape != y.shape:
        raise WdfHipError("gy must have y's shape [T,B]")
    _check(lib().wdf_loss_terms_grad(_ptr(y), _ptr(target), _ptr(gcoef), float(coeff), B, T, int(skip), _ptr(gy), _stream()),
           "wdf_loss_terms_grad")
    return gy


def clipper_bwd_esr_tp(x, theta, fs, zstash, zT, target, gcoef, skip, n_chunks, r=None, n_up=1, n_down=1, gtheta=None,
                       sse=None, ws=None, time_major=False):
    """Reverse sweep with dL/dy = ga (y - target) + gb y past `skip` (MSE + ESR); -> gtheta[4], sse[1]."""
    require_gpu()
    x, r, theta = _f32_dev(x, "x"), _f32_dev(r, "r"), _f32_dev(theta, "theta")
    zstash, zT, target, gcoef = _f32_dev(zstash, "zstash"), _f32_dev(zT, "zT"), _f32_dev(target, "target"), _f32_dev(gcoef, "gcoef")
    B, T = (x.shape[1], x.shape[0]) if time_major else x.shape
    if tuple(target.shape) != (T, B) or tuple(zstash.shape) != (T, B):
        raise WdfHipError(f"target / zstash must be [T,B] = [{T},{B}]")
    if ws is None:
        ws = bwd_tp_workspace(B, int(n_chunks), x.device)
    if gtheta is None:
        gtheta = torch.empty((4,), dtype=torch.float32, device=x.device)
    if sse is None:
        sse = torch.empty((1,), dtype=torch.float32, device=x.device)
    rc = lib().wdf_clipper_bwd_esr_tp(_ptr(x), _ptr(r), _ptr(theta), float(fs), int(n_up), int(n_down), _ptr(zstash),
                                      _ptr(zT), _ptr(target), _ptr(gcoef), int(skip), _ptr(ws), _ptr(gtheta), _ptr(sse),
                                      None, 0, B, T, int(n_chunks), _clipper_flags(time_major),
                                      _stream())
    _check(rc, "wdf_clipper_bwd_esr_tp")
    return gtheta, sse


def bwd_tp_workspace(B, n_chunks, device):
    """A reverse-sweep workspace with its ticket words cleared (wdf_clipper_bwd_tp_ws_init): allocate once, reuse."""
    ws = torch.empty((lib().wdf_clipper_bwd_tp_ws_bytes(int(B), int(n_chunks)),), dtype=torch.uint8, device=device)
    _check(lib().wdf_clipper_bwd_tp_ws_init(_ptr(ws), int(B), int(n_chunks), _stream()), "wdf_clipper_bwd_tp_ws_init")
    return ws


def tp_status(status):
    """Host view of a time-parallel status word (synchronises)."""
    s = status.cpu()
    return {"n_bad": int(s[0]), "max_miss": float(s[1:2].view(torch.float32)[0]), "fallback_ran": bool(int(s[2])),
            "repaired_tiles": int(s[2])}


def clipper_bwd_tp(x, theta, fs, zstash, gy, n_chunks, r=None, n_up=1, n_down=1, want_gz0=False, gtheta=None,
                   accumulate=False, ws=None, time_major=False):
    require_gpu()
    x = _f32_dev(x, "x")
    r = _f32_dev(r, "r")
    theta = _f32_dev(theta, "theta")
    zstash = _f32_dev(zstash, "zstash")
    gy = _f32_dev(gy, "gy")
    B, T = (x.shape[1], x.shape[0]) if time_major else x.shape
    if tuple(gy.shape) != (T, B) or tuple(zstash.shape) != (T, B):
        raise WdfHipError(f"gy / zstash must be [T,B] = [{T},{B}]")
    if ws is None:
        ws = bwd_tp_workspace(B, int(n_chunks), x.device)
    if gtheta is None:
        gtheta = torch.empty((4,), dtype=torch.float32, device=x.device)
        accumulate = False
    gz0 = torch.empty((B,), dtype=torch.float32, device=x.device) if want_gz0 else None
    rc = lib().wdf_clipper_bwd_tp(_ptr(x), _ptr(r), _ptr(theta), float(fs), int(n_up), int(n_down), _ptr(zstash),
                                  _ptr(gy), _ptr(ws), _ptr(gtheta), _ptr(gz0), 1 if accumulate else 0, B, T,
                                  int(n_chunks),
                                  _clipper_flags(time_major), _stream())
    _check(rc, "wdf_clipper_bwd_tp")
    return gtheta, gz0


def clipper_bwd_mse_tp(x, theta, fs, zstash, zT, target, gscale, n_chunks, r=None, n_up=1, n_down=1, gtheta=None,
                       sse=None, accumulate=False, ws=None, time_major=False):
    """MSE-fused reverse sweep: y is rebuilt from the state stash (zstash [T,B], zT [B]) and
    dL/dy = gscale (y - target) is formed in the kernel.
    Returns (gtheta float32[4], sse float32[1] = sum (y - target)^2 over this batch)."""
    require_gpu()
    x = _f32_dev(x, "x")
    r = _f32_dev(r, "r")
    theta = _f32_dev(theta, "theta")
    zstash = _f32_dev(zstash, "zstash")
    zT = _f32_dev(zT, "zT")
    target = _f32_dev(target, "target")
    B, T = (x.shape[1], x.shape[0]) if time_major else x.shape
    for name, t in (("target", target), ("zstash", zstash)):
        if tuple(t.shape) != (T, B):
            raise WdfHipError(f"{name} must be [T,B] = [{T},{B}]")
    if zT.numel() != B:
        raise WdfHipError("zT must hold the B final states of the forward")
    if ws is None:
        ws = bwd_tp_workspace(B, int(n_chunks), x.device)
    if gtheta is None:
        gtheta = torch.empty((4,), dtype=torch.float32, device=x.device)
        accumulate = False
    if sse is None:
        sse = torch.empty((1,), dtype=torch.float32, device=x.device)
    rc = lib().wdf_clipper_bwd_mse_tp(_ptr(x), _ptr(r), _ptr(theta), float(fs), int(n_up), int(n_down),
                                      _ptr(zstash), _ptr(zT), _ptr(target), float(gscale), _ptr(ws), _ptr(gtheta),
                                      _ptr(sse), None, 1 if accumulate else 0, B, T, int(n_chunks),
                                      _clipper_flags(time_major),
                                      _stream())
    _check(rc, "wdf_clipper_bwd_mse_tp")
    return gtheta, sse


def _mlp_check_shapes(who, x, theta2, w, hidden, n_tanh, r=None, z0=None, zstash=None, gy=None, sweep=False):
    """What the wdf_clipper_mlp_* kernels index by (B, T) and by the architecture without the C ABI knowing the arrays' sizes
    -> (B, T): x [B,T]; theta2 at least the 2 values {R, C}; w wdf_mlp_weight_count(hidden, n_tanh) values; r [B,T]; z0 B values;
    for a reverse sweep (sweep=True) zstash and gy [T,B]."""
    if x.dim() != 2:
        raise WdfHipError(f"{who}: x must be [B,T], got {tuple(x.shape)}")
    B, T = int(x.shape[0]), int(x.shape[1])
    if theta2 is None or theta2.numel() < 2:
        raise WdfHipError(f"{who}: theta2 must hold the 2 values {{R, C}}, got {None if theta2 is None else theta2.numel()}")
    n = lib().wdf_mlp_weight_count(int(hidden), int(n_tanh))
    if w is None or w.numel() != n:
        raise WdfHipError(f"{who}: a {n_tanh - 1}x{hidden} network has {n} weights, got {None if w is None else w.numel()}")
    if r is not None and tuple(r.shape) != (B, T):
        raise WdfHipError(f"{who}: r must be [B,T] = [{B},{T}], got {tuple(r.shape)}")
    if z0 is not None and tuple(z0.shape) != (B,):
        raise WdfHipError(f"{who}: z0 must be [B] = [{B}], got {tuple(z0.shape)}")
    if sweep:
        if zstash is None or tuple(zstash.shape) != (T, B):
            raise WdfHipError(f"{who}: zstash must be [T,B] = [{T},{B}], got {None if zstash is None else tuple(zstash.shape)}")
        if gy is None or tuple(gy.shape) != (T, B):
            raise WdfHipError(f"{who}: gy must be [T,B] = [{T},{B}], got {None if gy is None else tuple(gy.shape)}")
    return B, T


def clipper_mlp_fwd(x, theta2, w, hidden, n_tanh, fs, r=None, want_stash=True, z0=None, want_zT=False):
    """MLP-root clipper forward.  x [B,T], theta2 = {R, C}, w flat weights.  -> y [T,B], zstash, zT."""
    require_gpu()
    x = _f32_dev(x, "x")
    r = _f32_dev(r, "r")
    theta2 = _f32_dev(theta2, "theta2")
    w = _f32_dev(w, "w")
    z0 = _f32_dev(z0, "z0")
    B, T = _mlp_check_shapes("clipper_mlp_fwd", x, theta2, w, hidden, n_tanh, r=r, z0=z0)
    y = torch.empty((T, B), dtype=torch.float32, device=x.device)
    zs = torch.empty((T, B), dtype=torch.float32, device=x.device) if want_stash else None
    zT = torch.empty((B,), dtype=torch.float32, device=x.device) if want_zT else None
    rc = lib().wdf_clipper_mlp_fwd(_ptr(x), _ptr(r), _ptr(theta2), _ptr(w), int(hidden), int(n_tanh), float(fs),
                                   _ptr(y), _ptr(zs), _ptr(z0), _ptr(zT), B, T, WDF_MLP_LANE_PER_SEQUENCE if MLP_LANE_PER_SEQUENCE else 0, _stream())
    _check(rc, "wdf_clipper_mlp_fwd")
    return y, zs, zT


def clipper_mlp_bwd(x, theta2, w, hidden, n_tanh, fs, zstash, gy, r=None):
    """-> gtheta2 [2], gb [T,B], ain [T,B], lrin [T,B] | None (see include/wdf_hip.h)."""
    require_gpu()
    x = _f32_dev(x, "x")
    r = _f32_dev(r, "r")
    theta2 = _f32_dev(theta2, "theta2")
    w = _f32_dev(w, "w")
    zstash = _f32_dev(zstash, "zstash")
    gy = _f32_dev(gy, "gy")
    B, T = _mlp_check_shapes("clipper_mlp_bwd", x, theta2, w, hidden, n_tanh, r=r, zstash=zstash, gy=gy, sweep=True)
    gb = torch.empty((T, B), dtype=torch.float32, device=x.device)
    ain = torch.empty((T, B), dtype=torch.float32, device=x.device)
    lrin = torch.empty((T, B), dtype=torch.float32, device=x.device) if r is not None else None
    ws = torch.empty((lib().wdf_clipper_mlp_bwd_ws_bytes(B),), dtype=torch.uint8, device=x.device)
    gth = torch.empty((2,), dtype=torch.float32, device=x.device)
    rc = lib().wdf_clipper_mlp_bwd(_ptr(x), _ptr(r), _ptr(theta2), _ptr(w), int(hidden), int(n_tanh), float(fs),
                                   _ptr(zstash), _ptr(gy), _ptr(gb), _ptr(ain), _ptr(lrin), _ptr(ws), _ptr(gth),
                                   B, T, WDF_MLP_LANE_PER_SEQUENCE if MLP_LANE_PER_SEQUENCE else 0, _stream())
    _check(rc, "wdf_clipper_mlp_bwd")
    return gth, gb, ain, lrin


def clipper_mlp_bwd_w(x, theta2, w, hidden, n_tanh, fs, zstash, gy, r=None):
    """-> gtheta2 [2], gw [wdf_mlp_weight_count]: the reverse sweep with the weight gradient folded in."""
    require_gpu()
    x, r, theta2, w = _f32_dev(x, "x"), _f32_dev(r, "r"), _f32_dev(theta2, "theta2"), _f32_dev(w, "w")
    zstash, gy = _f32_dev(zstash, "zstash"), _f32_dev(gy, "gy")
    B, T = x.shape
    nbytes = lib().wdf_clipper_mlp_bwd_w_ws_bytes(int(hidden), int(n_tanh), B)
    if nbytes <= 0:
        raise WdfHipError(f"unsupported MLP root: width {hidden}, {n_tanh} tanh layers")
    _mlp_check_shapes("clipper_mlp_bwd_w", x, theta2, w, hidden, n_tanh, r=r, zstash=zstash, gy=gy, sweep=True)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    gth = torch.empty((2,), dtype=torch.float32, device=x.device)
    gw = torch.empty((w.numel(),), dtype=torch.float32, device=x.device)
    rc = lib().wdf_clipper_mlp_bwd_w(_ptr(x), _ptr(r), _ptr(theta2), _ptr(w), int(hidden), int(n_tanh), float(fs),
                                     _ptr(zstash), _ptr(gy), _ptr(ws), _ptr(gth), _ptr(gw), B, T, 0, _stream())
    _check(rc, "wdf_clipper_mlp_bwd_w")
    return gth, gw


def clipper_mlp_fwd_tp(x, theta2, w, hidden, n_tanh, fs, n_chunks, warmup, r=None, warmup_per_wave=None, tol=1e-6,
                       want_stash=True, z0=None, want_zT=False, ws=None, status=None, want_kappa=False, zinit=None):
    """Time-parallel MLP-root forward (csrc/wdf_mlp_tp.h).  warmup_per_wave: int32[ceil(B/4)] device tensor
    (multiples of 16) or None.  -> y [T,B], zstash | None, zT | None, status (int32[4]: n_bad, max-miss bits,
    gated waves, 0; read with mlp_tp_status()).  want_kappa: the forward also stores the adjoint recurrence's
    coefficient kappa [T,B] (for clipper_mlp_bwd_w_tp(kappa=...)); returned as a fifth value.  zinit [chunks,B]
    (with want_kappa): the states the chunks start their warm-up from (mlp_tp_starts() names the samples)."""
    require_gpu()
    x, r, theta2, w, z0 = _f32_dev(x, "x"), _f32_dev(r, "r"), _f32_dev(theta2, "theta2"), _f32_dev(w, "w"), _f32_dev(z0, "z0")
    B, T = _mlp_check_shapes("clipper_mlp_fwd_tp", x, theta2, w, hidden, n_tanh, r=r, z0=z0)
    if warmup_per_wave is not None and not (warmup_per_wave.is_cuda and warmup_per_wave.dtype == torch.int32
                                            and warmup_per_wave.numel() == (B + 3) // 4 and warmup_per_wave.is_contiguous()):
        raise WdfHipError("warmup_per_wave: expected a contiguous int32 device tensor with ceil(B/4) entries")
    y = torch.empty((T, B), dtype=torch.float32, device=x.device)
    zs = torch.empty((T, B), dtype=torch.float32, device=x.device) if want_stash else None
    zT = torch.empty((B,), dtype=torch.float32, device=x.device) if want_zT else None
    if ws is None:
        ws = torch.empty((lib().wdf_clipper_mlp_fwd_tp_ws_bytes(B, int(n_chunks)),), dtype=torch.uint8, device=x.device)
    if status is None:
        status = torch.empty((4,), dtype=torch.int32, device=x.device)
    if want_kappa:
        if zs is None:
            raise WdfHipError("want_kappa needs the stash (want_stash=True)")
        kap = torch.empty((T, B), dtype=torch.float32, device=x.device)
        if zinit is not None:
            zinit = _f32_dev(zinit, "zinit")
            if tuple(zinit.shape) != (lib().wdf_clipper_mlp_tp_chunks(T, int(n_chunks)), B) or warmup_per_wave is not None:
                raise WdfHipError("zinit: expected [chunks, B] and no warmup_per_wave")
        rc = lib().wdf_clipper_mlp_fwd_tp_kappa(_ptr(x), _ptr(r), _ptr(theta2), _ptr(w), int(hidden), int(n_tanh), float(fs),
                                                _ptr(y), _ptr(zs), _ptr(kap), _ptr(z0), _ptr(zT), _ptr(zinit), B, T, int(n_chunks),
                                                int(warmup), _ptr(warmup_per_wave), float(tol), _ptr(ws), _ptr(status),
                                                _stream())
        _check(rc, "wdf_clipper_mlp_fwd_tp_kappa")
        return y, zs, zT, status, kap
    rc = lib().wdf_clipper_mlp_fwd_tp(_ptr(x), _ptr(r), _ptr(theta2), _ptr(w), int(hidden), int(n_tanh), float(fs), _ptr(y),
                                      _ptr(zs), _ptr(z0), _ptr(zT), B, T, int(n_chunks), int(warmup), _ptr(warmup_per_wave),
                                      float(tol), _ptr(ws), _ptr(status), _stream())
    _check(rc, "wdf_clipper_mlp_fwd_tp")
    return y, zs, zT, status


def mlp_tp_starts(T, n_chunks, warmup):
    """The sample every chunk's wave begins at (warm-up included) for one warm-up value -> list of ints."""
    K = lib().wdf_clipper_mlp_tp_chunks(int(T), int(n_chunks))
    out = (C.c_int64 * K)()
    _check(lib().wdf_clipper_mlp_tp_starts(int(T), int(n_chunks), int(warmup), out), "wdf_clipper_mlp_tp_starts")
    return list(out)


def mlp_tp_status(status):
    s = status.cpu()
    # gated_waves: 4-sequence waves with a miss at the first pass (re-run chunk-locally from their predecessors' end
    # states); sequential_waves: those that still missed and went through the sequential kernel
    return {"n_bad": int(s[0]), "max_miss": float(s[1:2].view(torch.float32)[0]), "gated_waves": int(s[2]),
            "sequential_waves": int(s[3])}


def clipper_mlp_bwd_w_tp(x, theta2, w, hidden, n_tanh, fs, zstash, gy, n_chunks, r=None, ws=None, kappa=None):
    """Exact reverse sweep parallel over all steps (kappa / adjoint scan / weight-gradient kernels) -> gtheta2 [2], gw.
    kappa [T,B]: the coefficient a want_kappa forward left -- the kappa pass is skipped."""
    require_gpu()
    x, r, theta2, w = _f32_dev(x, "x"), _f32_dev(r, "r"), _f32_dev(theta2, "theta2"), _f32_dev(w, "w")
    zstash, gy = _f32_dev(zstash, "zstash"), _f32_dev(gy, "gy")
    B, T = x.shape
    nbytes = lib().wdf_clipper_mlp_bwd_w_tp_ws_bytes(int(hidden), int(n_tanh), B, T, int(n_chunks))
    if nbytes <= 0:
        raise WdfHipError(f"unsupported MLP root: width {hidden}, {n_tanh} tanh layers")
    _mlp_check_shapes("clipper_mlp_bwd_w_tp", x, theta2, w, hidden, n_tanh, r=r, zstash=zstash, gy=gy, sweep=True)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    gth = torch.empty((2,), dtype=torch.float32, device=x.device)
    gw = torch.empty((w.numel(),), dtype=torch.float32, device=x.device)
    if kappa is not None:
        kappa = _f32_dev(kappa, "kappa")
        if tuple(kappa.shape) != (T, B):
            raise WdfHipError(f"kappa: expected [{T}, {B}], got {tuple(kappa.shape)}")
        rc = lib().wdf_clipper_mlp_bwd_w_tp_kappa(_ptr(x), _ptr(r), _ptr(theta2), _ptr(w), int(hidden), int(n_tanh), float(fs),
                                                  _ptr(zstash), _ptr(kappa), _ptr(gy), _ptr(ws), _ptr(gth), _ptr(gw), B, T,
                                                  int(n_chunks), _stream())
        _check(rc, "wdf_clipper_mlp_bwd_w_tp_kappa")
        return gth, gw
    rc = lib().wdf_clipper_mlp_bwd_w_tp(_ptr(x), _ptr(r), _ptr(theta2), _ptr(w), int(hidden), int(n_tanh), float(fs),
                                        _ptr(zstash), _ptr(gy), _ptr(ws), _ptr(gth), _ptr(gw), B, T, int(n_chunks), _stream())
    _check(rc, "wdf_clipper_mlp_bwd_w_tp")
    return gth, gw


def mlp_eval(ain, lrin, w, hidden, n_tanh):
    """out[n] = MLP(ain[n], lrin[n]) (flat float32 device tensors)."""
    require_gpu()
    ain = _f32_dev(ain, "ain")
    lrin = _f32_dev(lrin, "lrin")
    w = _f32_dev(w, "w")
    if lrin.numel() != ain.numel():
        raise WdfHipError("mlp_eval: ain and lrin must have the same number of samples")
    n = lib().wdf_mlp_weight_count(int(hidden), int(n_tanh))
    # (a network no kernel is built for is the library's to refuse; one that has kernels must come with all its weights)
    if lib().wdf_clipper_mlp_bwd_w_ws_bytes(int(hidden), int(n_tanh), 1) > 0 and w.numel() != n:
        raise WdfHipError(f"mlp_eval: a {n_tanh - 1}x{hidden} network has {n} weights, got {w.numel()}")
    out =torch.empty((ain.numel(),), dtype=torch.float32, device=ain.device)
    rc = lib().wdf_mlp_eval(_ptr(ain), _ptr(lrin), _ptr(w), int(hidden), int(n_tanh), _ptr(out), ain.numel(), _stream())
    _check(rc, "wdf_mlp_eval")
    return out


def mlp_fit_epoch(xa, xl, ys, batch, w, opt, hidden, n_tanh, esr_n, eps_energy, loss_sum):
    """One epoch of mini-batch Adam on the table (xa, xl, ys) in the given order; w and the Adam
    state `opt` (binding.Adam with a scalar learning rate) are updated in place; loss_sum: device
    float64[1] receiving the sum of batch losses."""
    require_gpu()
    xa, xl, ys, w = _f32_dev(xa, "xa"), _f32_dev(xl, "xl"), _f32_dev(ys, "ys"), _f32_dev(w, "w")
    if not (xa.numel() == xl.numel() == ys.numel()):
        raise WdfHipError("mlp_fit_epoch: xa, xl, ys must have the same length")
    if loss_sum.dtype != torch.float64 or not loss_sum.is_cuda:
        raise WdfHipError("loss_sum must be a float64 device tensor")
    rc = lib().wdf_mlp_fit_epoch(_ptr(xa), _ptr(xl), _ptr(ys), xa.numel(), int(batch), _ptr(w), _ptr(opt.m), _ptr(opt.v),
                                 _ptr(opt.step), float(opt.lr_scalar), opt.b1, opt.b2, opt.eps, float(esr_n),
                                 float(eps_energy), _ptr(loss_sum), int(hidden), int(n_tanh), _stream())
    _check(rc, "wdf_mlp_fit_epoch")


def clipper_mlp_wgrad(ain, lrin, gb, theta2, w, hidden, n_tanh, fs):
    """-> gw [wdf_mlp_weight_count]: dL/dw from what clipper_mlp_bwd wrote (see include/wdf_hip.h)."""
    require_gpu()
    ain = _f32_dev(ain, "ain")
    lrin = _f32_dev(lrin, "lrin")
    gb = _f32_dev(gb, "gb")
    theta2 = _f32_dev(theta2, "theta2")
    w = _f32_dev(w, "w")
    S = ain.numel()
    if gb.numel() != S or (lrin is not None and lrin.numel() != S):
        raise WdfHipError("clipper_mlp_wgrad: ain, lrin and gb must have the same number of samples")
    nbytes = lib().wdf_clipper_mlp_wgrad_ws_bytes(int(hidden), int(n_tanh), S)
    if nbytes <= 0:
        raise WdfHipError(f"unsupported MLP root: width {hidden}, {n_tanh} tanh layers")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=ain.device)
    gw = torch.empty((w.numel(),), dtype=torch.float32, device=ain.device)
    rc = lib().wdf_clipper_mlp_wgrad(_ptr(ain), _ptr(lrin), _ptr(gb), _ptr(theta2), _ptr(w), int(hidden), int(n_tanh),
                                     float(fs), _ptr(ws), _ptr(gw), S, _stream())
    _check(rc, "wdf_clipper_mlp_wgrad")
    return gw


# WDF_ASYM_*: the closed form is a model approximation (it drops the reverse diode's saturation current), kept for comparison;
# the two Newton modes solve the exact pair -- in fp64, or entirely in fp32 (tolerance floor 4 FLT_EPSILON, fp32 state)
ASYM_OMEGA_F32, ASYM_NEWTON_F64, ASYM_NEWTON_F32 = 0, 1, 2


def _asym_call(name, rseq, x, *rest):
    """wdf_<name>(x, ...) or, with a pot per sequence, wdf_<name>_rseq(x, rseq, ...): the twins share every other argument."""
    if rseq is None:
        return getattr(lib(), name)(_ptr(x), *rest), name
    return getattr(lib(), name + "_rseq")(_ptr(x), _ptr(_f32_dev(rseq, "rseq")), *rest), name + "_rseq"


def _rseq_arg(rseq, x, mode, who):
    """The rseq= keyword of the two-different-diode wrappers, checked before anything is launched: None (the pot is theta6[4]), or
    one float32 resistance per sequence and then a Newton mode."""
    if rseq is None:
        return None
    B = int(x.shape[0])
    if not isinstance(rseq, torch.Tensor) or rseq.dtype != torch.float32 or rseq.dim() != 1 or rseq.numel() != B:
        raise WdfHipError(f"{who}: rseq must be a float32 tensor [B] = [{B}] (one resistance per sequence), got "
                          f"{type(rseq).__name__} {tuple(getattr(rseq, 'shape', ()))} {getattr(rseq, 'dtype', None)}")
    if int(mode) == ASYM_OMEGA_F32:
        raise WdfHipError(f"{who}: mode 0 (the closed form, a model approximation kept for comparison) has no per-sequence pot: "
                          "use ASYM_NEWTON_F32 or ASYM_NEWTON_F64")
    return rseq


def _required(rseq, who):
    """The *_rseq wrappers take their pot positionally and need one; what it must be, the wrapper they forward to checks."""
    if rseq is None:
        raise WdfHipError(f"{who}: rseq is required (one resistance per sequence, a float32 tensor [B])")
    return rseq


def r_per_sequence(r):
    """A pot channel r [B,T] (clipper_pot.py:68-70: channel 1 of the input) -> the [B] vector of its per-sequence values
    (contiguous, cached with the channel); WdfHipError if the channel moves inside a sequence: the two-different-diode kernels
    take one resistance per sequence.  One cached comparison per tensor (r_is_per_sequence)."""
    if not isinstance(r, torch.Tensor) or r.dim() != 2:
        raise WdfHipError(f"r_per_sequence: expected a [B,T] tensor, got {type(r).__name__} {tuple(getattr(r, 'shape', ()))}")
    hit = _R_VEC_CACHE.get(r)
    if hit is not None:
        return hit
    const = r_is_per_sequence(r, False)
    if not const and not (r.is_cuda and torch.cuda.is_current_stream_capturing()):
        const = bool((r == r[:, 0:1]).all())       # (WDF_R_PER_SEQUENCE=0 switches the cached answer off, not this contract)
    if not const:
        raise WdfHipError("the two-different-diode clipper takes one resistance per sequence (clipper_pot.py's recordings: "
                          "dataimport.py:96); this channel moves inside a sequence (or could not be looked at during stream capture)")
    return _R_VEC_CACHE.put(r, r[:, 0].float().contiguous())


def clipper_asym_fwd_rseq(x, rseq, theta6, fs, mode, **kw):
    """clipper_asym_fwd with one pot resistance per sequence, rseq [B] (wdf_clipper_asym_fwd_rseq): theta6[4] is ignored."""
    return clipper_asym_fwd(x, theta6, fs, mode, rseq=_required(rseq, "clipper_asym_fwd_rseq"), **kw)


def clipper_asym_fwd_tp_rseq(x, rseq, theta6, fs, mode, n_chunks, warmup, **kw):
    """clipper_asym_fwd_tp with one pot resistance per sequence, rseq [B] (wdf_clipper_asym_fwd_tp_rseq): theta6[4] is ignored;
    the warm-up has to outlast the LARGEST pot's memory."""
    return clipper_asym_fwd_tp(x, theta6, fs, mode, n_chunks, warmup, rseq=_required(rseq, "clipper_asym_fwd_tp_rseq"), **kw)


def clipper_asym_bwd_tp_rseq(x, rseq, theta6, fs, mode, zstash, zT, gy, n_chunks, **kw):
    """clipper_asym_bwd_tp with one pot resistance per sequence, rseq [B] (wdf_clipper_asym_bwd_tp_rseq): component 4 of the
    gradient is exactly 0 (the pot is data), component 5 is dL/dC with the chain rule applied per sequence."""
    return clipper_asym_bwd_tp(x, theta6, fs, mode, zstash, zT, gy, n_chunks,
                               rseq=_required(rseq, "clipper_asym_bwd_tp_rseq"), **kw)


def clipper_asym_step_mse_rseq(x, rseq, theta6, fs, mode, target, gscale, n_chunks, warmup, **kw):
    """clipper_asym_step_mse with one pot resistance per sequence, rseq [B] (wdf_clipper_asym_step_mse_rseq): out7[5] (dR) is
    exactly 0 and opt never writes theta6[4]."""
    return clipper_asym_step_mse(x, theta6, fs, mode, target, gscale, n_chunks, warmup,
                                 rseq=_required(rseq, "clipper_asym_step_mse_rseq"), **kw)


def clipper_asym_step_esr_rseq(x, rseq, theta6, fs, mode, target, n_global, eps_energy, skip, n_chunks, warmup, **kw):
    """clipper_asym_step_esr with one pot resistance per sequence, rseq [B] (wdf_clipper_asym_step_esr_rseq): component 4 of
    gP, gQ and gtheta6 is exactly 0 and opt never writes theta6[4]."""
    return clipper_asym_step_esr(x, theta6, fs, mode, target, n_global, eps_energy, skip, n_chunks, warmup,
                                 rseq=_required(rseq, "clipper_asym_step_esr_rseq"), **kw)


def clipper_asym_fwd(x, theta6, fs, mode, tol=1e-12, max_iter=50, z0=None, want_zT=False, want_iters=False, want_stash=False,
                     rseq=None):
    """Two-different-diode clipper forward.  Returns y [T,B], zT | None, iters (int64 per wave) | None
    (and the state stash [T,B] as a fourth value when want_stash).  rseq [B]: one pot resistance per sequence in place of
    theta6[4] (wdf_clipper_asym_fwd_rseq; Newton modes)."""
    rseq = _rseq_arg(rseq, x, mode, "clipper_asym_fwd")
    require_gpu()
    x = _f32_dev(x, "x")
    theta6 = _f32_dev(theta6, "theta6")
    z0 = _f32_dev(z0, "z0")
    if theta6.numel() != 6:
        raise WdfHipError("theta6 must hold {Is_up, nVt_up, Is_down, nVt_down, R, C}")
    B, T = x.shape
    y = torch.empty((T, B), dtype=torch.float32, device=x.device)
    zT = torch.empty((B,), dtype=torch.float32, device=x.device) if want_zT else None
    it = torch.zeros(((B + 63) // 64,), dtype=torch.int64, device=x.device) if want_iters else None
    zs = torch.empty((T, B), dtype=torch.float32, device=x.device) if want_stash else None
    rc, name = _asym_call("wdf_clipper_asym_fwd", rseq, x, _ptr(theta6), float(fs), int(mode), float(tol), int(max_iter), _ptr(y),
                          _ptr(zs), _ptr(z0), _ptr(zT), _ptr(it), B, T, _stream())
    _check(rc, name)
    return (y, zT, it, zs) if want_stash else (y, zT, it)


def clipper_asym_fwd_tp(x, theta6, fs, mode, n_chunks, warmup, tol=1e-12, max_iter=50, verify_tol=1e-6, z0=None, want_zT=False,
                        want_stash=False, rseq=None):
    """Time-parallel two-different-diode clipper forward (wdf_clipper_asym_fwd_tp).  n_chunks is rounded to a count that
    tiles T in 8-step units.  rseq [B]: one pot resistance per sequence in place of theta6[4] (wdf_clipper_asym_fwd_tp_rseq).
    -> y [T,B], zT | None, zstash | None, status (int32[4]; read with mlp_tp_status())."""
    rseq = _rseq_arg(rseq, x, mode, "clipper_asym_fwd_tp")
    require_gpu()
    x, theta6, z0 = _f32_dev(x, "x"), _f32_dev(theta6, "theta6"), _f32_dev(z0, "z0")
    if theta6.numel() != 6:
        raise WdfHipError("theta6 must hold {Is_up, nVt_up, Is_down, nVt_down, R, C}")
    B, T = x.shape
    K = asym_chunks(T, n_chunks)
    y = torch.empty((T, B), dtype=torch.float32, device=x.device)
    zs = torch.empty((T, B), dtype=torch.float32, device=x.device) if want_stash else None
    zT = torch.empty((B,), dtype=torch.float32, device=x.device) if want_zT else None
    ws = torch.empty((lib().wdf_clipper_asym_fwd_tp_ws_bytes(B, K),), dtype=torch.uint8, device=x.device)
    status = torch.empty((4,), dtype=torch.int32, device=x.device)
    rc, name = _asym_call("wdf_clipper_asym_fwd_tp", rseq, x, _ptr(theta6), float(fs), int(mode), float(tol), int(max_iter), _ptr(y),
                          _ptr(zs), _ptr(z0), _ptr(zT), B, T, K, int(warmup), float(verify_tol), _ptr(ws), _ptr(status), _stream())
    _check(rc, name)
    return y, zT, zs, status


def clipper_asym_bwd(x, theta6, fs, zstash, gy, tol=1e-12, max_iter=50):
    """dL/d{Is_up, nVt_up, Is_down, nVt_down, R, C} of the Newton-mode loop for dL/dy = gy [T,B]."""
    require_gpu()
    x, theta6, zstash, gy = _f32_dev(x, "x"), _f32_dev(theta6, "theta6"), _f32_dev(zstash, "zstash"), _f32_dev(gy, "gy")
    B, T = x.shape
    if tuple(gy.shape) != (T, B) or tuple(zstash.shape) != (T, B):
        raise WdfHipError(f"gy / zstash must be [T,B] = [{T},{B}]")
    ws = torch.empty((lib().wdf_clipper_asym_bwd_ws_bytes(B),), dtype=torch.uint8, device=x.device)
    g = torch.empty((6,), dtype=torch.float32, device=x.device)
    rc = lib().wdf_clipper_asym_bwd(_ptr(x), _ptr(theta6), float(fs), float(tol), int(max_iter), _ptr(zstash), _ptr(gy),
                                    _ptr(ws), _ptr(g), B, T, _stream())
    _check(rc, "wdf_clipper_asym_bwd")
    return g


def clipper_asym_bwd_tp(x, theta6, fs, mode, zstash, zT, gy, n_chunks, gzT=None, want_gz0=False, ws=None, rseq=None):
    """Time-parallel reverse sweep of the two-different-diode clipper, any mode (wdf_clipper_asym_bwd_tp): no root
    re-solve (consecutive stash entries give b), chunks composed exactly.  zT [B]: the forward's final state.  rseq [B]: the
    forward's pot resistance per sequence (wdf_clipper_asym_bwd_tp_rseq).
    -> gtheta6 (and dL/dz0 [B] when want_gz0)."""
    rseq = _rseq_arg(rseq, x, mode, "clipper_asym_bwd_tp")
    require_gpu()
    x, theta6, zstash, gy = _f32_dev(x, "x"), _f32_dev(theta6, "theta6"), _f32_dev(zstash, "zstash"), _f32_dev(gy, "gy")
    zT, gzT = _f32_dev(zT, "zT"), _f32_dev(gzT, "gzT")
    B, T = x.shape
    if tuple(gy.shape) != (T, B) or tuple(zstash.shape) != (T, B) or zT is None or zT.numel() != B:
        raise WdfHipError(f"gy / zstash must be [T,B] = [{T},{B}], zT [{B}]")
    K = asym_chunks(T, n_chunks)
    need = lib().wdf_clipper_asym_bwd_tp_ws_bytes(B, K)
    if ws is None or ws.numel() < need:
        ws = torch.empty((need,), dtype=torch.uint8, device=x.device)
    g = torch.empty((6,), dtype=torch.float32, device=x.device)
    gz0 = torch.empty((B,), dtype=torch.float32, device=x.device) if want_gz0 else None
    rc, name = _asym_call("wdf_clipper_asym_bwd_tp", rseq, x, _ptr(theta6), float(fs), int(mode), _ptr(zstash), _ptr(zT), _ptr(gy),
                          _ptr(gzT), _ptr(ws), _ptr(g), _ptr(gz0), B, T, K, _stream())
    _check(rc, name)
    return (g, gz0) if want_gz0 else g


def asym_chunks(T, n_chunks):
    """The chunk count the asym kernels accept for T: n_chunks rounded to one that tiles T in 8-step units."""
    return chunk_geom(T, n_chunks, 8)[1]


def _asym_step_args(who, ws_bytes, x, theta6, mode, target, n_chunks, y, z0, want_zT, ws, status, opt, rseq, finish=True):
    """The checks and buffers the two one-pass steps of the two-different-diode clipper share
    -> x, theta6, target, z0, rseq, B, T, K, y, zT, ws, status, Adam tail."""
    rseq = _rseq_arg(rseq, x, mode, who)
    require_gpu()
    x, theta6, target, z0 = _f32_dev(x, "x"), _f32_dev(theta6, "theta6"), _f32_dev(target, "target"), _f32_dev(z0, "z0")
    if theta6.numel() != 6:
        raise WdfHipError("theta6 must hold {Is_up, nVt_up, Is_down, nVt_down, R, C}")
    B, T = x.shape
    if tuple(target.shape) != (T, B):
        raise WdfHipError(f"target must be [T,B] = [{T},{B}]")
    if z0 is not None and z0.numel() != B:
        raise WdfHipError(f"z0 must hold one state per sequence ({B})")
    adam = _adam_tail(opt, 6, who, "{Is_up, nVt_up, Is_down, nVt_down, R, C}", finish)
    K = asym_chunks(T, n_chunks)
    y, zT = _y_zT(y, want_zT, T, B, x)
    ws = _ws(ws, ws_bytes(B, K), x)
    if status is None:
        status = torch.empty((4,), dtype=torch.int32, device=x.device)
    return x, theta6, target, z0, rseq, B, T, K, y, zT, ws, status, adam


def clipper_asym_step_mse(x, theta6, fs, mode, target, gscale, n_chunks, warmup, tol=1e-12, max_iter=50, verify_tol=1e-6, y=None,
                          z0=None, want_zT=False, ws=None, status=None, out7=None, opt=None, rseq=None):
    """The MSE training step of the two-different-diode clipper in one pass over the data (wdf_clipper_asym_step_mse): forward,
    loss and d(gscale/2 sum (y - target)^2)/d{Is_up, nVt_up, Is_down, nVt_down, R, C}, x [B,T] and target [T,B] read once, y
    written once, no stash.  mode: ASYM_NEWTON_F32 or ASYM_NEWTON_F64.  n_chunks is rounded like asym_chunks(); y, ws, status,
    out7 can be preallocated; opt: a binding.Adam(6, ...) to update theta6 in the step's last launch.  rseq [B]: one pot
    resistance per sequence (wdf_clipper_asym_step_mse_rseq): theta6[4] is ignored, out7[5] (dR) is exactly 0 and opt never
    writes theta6[4].
    -> y [T,B], zT [B] | None, out7 = {sse, gtheta6}, status (int32[4]; read with mlp_tp_status())."""
    x, theta6, target, z0, rseq, B, T, K, y, zT, ws, status, adam = _asym_step_args(
        "clipper_asym_step_mse", lib().wdf_clipper_asym_step_mse_ws_bytes, x, theta6, mode, target, n_chunks, y, z0, want_zT, ws,
        status, opt, rseq)
    out7 = _out(out7, 7, "out7", "{sse, gtheta6}", x)
    rc, name = _asym_call(
        "wdf_clipper_asym_step_mse", rseq, x, _ptr(theta6), float(fs), int(mode), float(tol), int(max_iter), _ptr(target), float(gscale),
        _ptr(y), _ptr(z0), _ptr(zT), B, T, K, int(warmup), float(verify_tol), _ptr(ws), _ptr(status), _ptr(out7), *adam, _stream())
    _check(rc, name)
    return y, zT, out7, status


GN_TRI = tuple((q, r) for q in range(6) for r in range(q, 6))      # out28[7:28]: the upper triangle, row-major


def clipper_asym_step_gn(x, theta6, fs, mode, target, gscale, n_chunks, warmup, tol=1e-12, max_iter=50, verify_tol=1e-6, y=None,
                         z0=None, want_zT=False, ws=None, status=None, out28=None):
    """The Gauss-Newton form of clipper_asym_step_mse (wdf_clipper_asym_step_gn): the same one pass over the data, which also
    sums the products of the output's tangents.  out28 = {sse, g[6], H[21]}: g = gscale/2 d(sse)/d{Is_up, nVt_up, Is_down,
    nVt_down, R, C} (clipper_asym_step_mse's out7[1:7]) and H = gscale sum_t (dy_t/dtheta_q)(dy_t/dtheta_r) for q <= r, the
    upper triangle row-major (GN_TRI; gn_matrix() unpacks it) -- with gscale = 2/N the gradient of the mean squared error and
    (2/N) J^T J.  mode: ASYM_NEWTON_F32 or ASYM_NEWTON_F64.  n_chunks is rounded like asym_chunks(); y, ws, status, out28 can
    be preallocated.  theta6 is only read: a Levenberg-Marquardt optimizer (wdf_hip.lm) moves the parameters.
    -> y [T,B], zT [B] | None, out28, status (int32[4]; read with mlp_tp_status())."""
    x, theta6, target, z0, _, B, T, K, y, zT, ws, status, _ = _asym_step_args(
        "clipper_asym_step_gn", lib().wdf_clipper_asym_step_gn_ws_bytes, x, theta6, mode, target, n_chunks, y, z0, want_zT, ws,
        status, None, None)
    out28 = _out(out28, 28, "out28", "{sse, g[6], H[21]}", x)
    _check(lib().wdf_clipper_asym_step_gn(_ptr(x), _ptr(theta6), float(fs), int(mode), float(tol), int(max_iter), _ptr(target),
                                          float(gscale), _ptr(y), _ptr(z0), _ptr(zT), B, T, K, int(warmup), float(verify_tol), _ptr(ws),
                                          _ptr(status), _ptr(out28), _stream()), "wdf_clipper_asym_step_gn")
    return y, zT, out28, status


def gn_matrix(tri):
    """The 21 values of out28[7:28] (any float tensor on any device) -> the symmetric [6,6] matrix, float64, same device."""
    H = torch.zeros((6, 6), dtype=torch.float64, device=tri.device)
    q, r = (torch.tensor(i, device=tri.device) for i in zip(*GN_TRI))
    H[q, r] = tri.to(torch.float64)
    H[r, q] = tri.to(torch.float64)
    return H


def clipper_asym_step_esr(x, theta6, fs, mode, target, n_global, eps_energy, skip, n_chunks, warmup, tol=1e-12, max_iter=50,
                          verify_tol=1e-6, y=None, z0=None, want_zT=False, ws=None, status=None, sums14=None, gtheta6=None, loss3=None,
                          finish=True, opt=None, rseq=None):
    """The MSE + ESR training step of the two-different-diode clipper in one pass over the data (wdf_clipper_asym_step_esr):
    loss = S/n + sqrt(S / (E + eps_energy) / n) on the rows past `skip`, S = sum (y - target)^2, E = sum y^2, n = n_global.
    x [B,T] and target [T,B] read once, y written once, no stash.  mode: ASYM_NEWTON_F32 or ASYM_NEWTON_F64.  n_chunks is
    rounded like asym_chunks(); y, ws, status, sums14, gtheta6, loss3 can be preallocated.  finish=True: a single rank -- the
    kernel forms gtheta6 = dloss/d{Is_up, nVt_up, Is_down, nVt_down, R, C} and loss3 = {mse, esr, mse + esr} itself, and
    opt (a binding.Adam(6, ...)) updates theta6 in the same last launch.  finish=False: one shard of several -- only sums14 =
    {S, E, gP[6], gQ[6]} of this call comes back (gtheta6 and loss3 are None): all-reduce it and call asym_esr_finish().
    rseq [B]: one pot resistance per sequence (wdf_clipper_asym_step_esr_rseq): theta6[4] is ignored, component 4 of gP, gQ and
    gtheta6 is exactly 0 and opt never writes theta6[4].
    -> y [T,B], zT [B] | None, sums14, gtheta6, loss3, status (int32[4]; read with mlp_tp_status())."""
    x, theta6, target, z0, rseq, B, T, K, y, zT, ws, status, adam = _asym_step_args(
        "clipper_asym_step_esr", lib().wdf_clipper_asym_step_esr_ws_bytes, x, theta6, mode, target, n_chunks, y, z0, want_zT, ws,
        status, opt, rseq, finish)
    sums14 = _out(sums14, 14, "sums14", "{S, E, gP[6], gQ[6]}", x)
    gtheta6, loss3 = _esr_outs(finish, gtheta6, 6, "gtheta6", loss3, x)
    rc, name = _asym_call(
        "wdf_clipper_asym_step_esr", rseq, x, _ptr(theta6), float(fs), int(mode), float(tol), int(max_iter), _ptr(target), float(n_global),
        float(eps_energy), int(skip), _ptr(y), _ptr(z0), _ptr(zT), B, T, K, int(warmup), float(verify_tol), _ptr(ws), _ptr(status),
        _ptr(sums14), _ptr(gtheta6), _ptr(loss3), *adam, _stream())
    _check(rc, name)
    return y, zT, sums14, gtheta6, loss3, status


def asym_esr_finish(sums14, n_global, eps_energy, gtheta6=None, loss3=None):
    """Several ranks: sums14 = {S, E, gP[6], gQ[6]} summed over the ranks -> (gtheta6, loss3 = {mse, esr, mse + esr}), the
    global loss and its gradient (wdf_asym_esr_finish: the single-rank step's own formulas)."""
    return _esr_finish(lib().wdf_asym_esr_finish, sums14, "sums14", 6, (), n_global, eps_energy, gtheta6, "gtheta6", loss3)


def asym_root(a, theta6, fs, mode, tol=1e-12, max_iter=50):
    require_gpu()
    a = _f32_dev(a, "a")
    theta6 = _f32_dev(theta6, "theta6")
    b = torch.empty(a.shape, dtype=torch.float64, device=a.device)
    _check(lib().wdf_asym_root(_ptr(a), _ptr(theta6), float(fs), int(mode), float(tol), int(max_iter), _ptr(b),
                               a.numel(), _stream()), "wdf_asym_root")
    return b


ROOT_NONE, ROOT_DIODE_PAIR, ROOT_MLP = 0, 2, 3
ROOT_ASYM_PAIR = 4        # two different diodes, exact, fp32 Newton: ss_fwd / ss_bwd / ss_fwd_tp / ss_bwd_tp; rootp [5], groot [5]
#                           (ss_dyn_*: rootp [4] = {Is_up, nVt_up, Is_down, nVt_down}, groot float64 [4], R_port in the row)


def _ss_groot(root_kind, device):
    """The reverse sweeps' root-gradient buffer: [3] for the diode pair, [5] for two different diodes, None for a linear tree."""
    n = {ROOT_DIODE_PAIR: 3, ROOT_ASYM_PAIR: 5}.get(root_kind)
    return None if n is None else torch.empty((n,), dtype=torch.float32, device=device)


def _ss_check_shapes(who, x, coef, ns, ni, root_kind, rootp, z0=None, zstash=None, gy=None, sweep=False):
    """What the wdf_ss_* kernels index by (ns, ni, B, T) without the C ABI knowing the arrays' sizes -> (B, T): x holds B T ni values,
    coef wdf_ss_ncoef(ns, ni); z0 [ns,B]; for a reverse sweep (sweep=True) zstash [T,ns,B] (ns > 0) and gy [T,B]; rootp at least
    the 3 values the diode pair reads ({Is, nVt, R_port}) or the 5 of two different diodes, and there at all under either root."""
    ns, ni = int(ns), int(ni)
    if x.dim() < 2:
        raise WdfHipError(f"{who}: x must be [B,T,ni] (or [B,T] when ni == 1), got {tuple(x.shape)}")
    B, T = int(x.shape[0]), int(x.shape[1])
    if x.numel() != B * T * ni:
        raise WdfHipError(f"{who}: x has {x.numel()} elements, expected B*T*ni = {B * T * ni}")
    if coef.numel() != lib().wdf_ss_ncoef(ns, ni):
        raise WdfHipError(f"{who}: coef must hold {lib().wdf_ss_ncoef(ns, ni)} values for ns={ns}, ni={ni}, got {coef.numel()}")
    if z0 is not None and ns > 0 and tuple(z0.shape) != (ns, B):
        raise WdfHipError(f"{who}: z0 must be [ns,B] = [{ns},{B}], got {tuple(z0.shape)}")
    if sweep:
        if ns > 0 and (zstash is None or tuple(zstash.shape) != (T, ns, B)):
            raise WdfHipError(f"{who}: zstash must be [T,ns,B] = [{T},{ns},{B}], got {None if zstash is None else tuple(zstash.shape)}")
        if gy is None or tuple(gy.shape) != (T, B):
            raise WdfHipError(f"{who}: gy must be [T,B] = [{T},{B}], got {None if gy is None else tuple(gy.shape)}")
    need = {ROOT_DIODE_PAIR: 3, ROOT_ASYM_PAIR: 5}.get(int(root_kind), 0)
    if need and (rootp is None or rootp.numel() < need):
        raise WdfHipError(f"{who}: rootp must hold {need} values for root kind {int(root_kind)} "
                          f"({'Is, nVt, R_port' if need == 3 else 'Is_up, nVt_up, Is_down, nVt_down, R_port'}), "
                          f"got {None if rootp is None else rootp.numel()}")
    return B, T


def ss_fwd(x, coef, ns, ni, root_kind=ROOT_NONE, rootp=None, n_up=1, n_down=1, want_stash=True, z0=None,
           want_zT=False):
    """State-space recursion.  x [B,T,ni] (or [B,T] when ni == 1) -> y [T,B], zstash [T,ns,B] | None,
    zT [ns,B] | None."""
    require_gpu()
    x = _f32_dev(x, "x")
    coef = _f32_dev(coef, "coef")
    rootp = _f32_dev(rootp, "rootp")
    z0 = _f32_dev(z0, "z0")
    B, T = _ss_check_shapes("ss_fwd", x, coef, ns, ni, root_kind, rootp, z0=z0)
    y = torch.empty((T, B), dtype=torch.float32, device=x.device)
    zs = torch.empty((T, ns, B), dtype=torch.float32, device=x.device) if (want_stash and ns > 0) else None
    zT = torch.empty((ns, B), dtype=torch.float32, device=x.device) if want_zT else None
    rc = lib().wdf_ss_fwd(_ptr(x), _ptr(coef), _ptr(rootp), ns, ni, root_kind, int(n_up), int(n_down),
                          _ptr(y), _ptr(zs), _ptr(z0), _ptr(zT), B, T, 0, _stream())
    _check(rc, "wdf_ss_fwd")
    return y, zs, zT


def ss_fwd_lin_tp(x, coef, ns, ni, n_chunks, want_stash=True, z0=None, want_zT=False):
    """Exact chunked forward of a linear tree (root kind NONE); same returns as ss_fwd."""
    require_gpu()
    x, coef, z0 = _f32_dev(x, "x"), _f32_dev(coef, "coef"), _f32_dev(z0, "z0")
    B, T = _ss_check_shapes("ss_fwd_lin_tp", x, coef, ns, ni, ROOT_NONE, None, z0=z0)
    y = torch.empty((T, B), dtype=torch.float32, device=x.device)
    zs = torch.empty((T, ns, B), dtype=torch.float32, device=x.device) if want_stash else None
    zT = torch.empty((ns, B), dtype=torch.float32, device=x.device) if want_zT else None
    ws = torch.empty((lib().wdf_ss_fwd_lin_tp_ws_bytes(ns, B, int(n_chunks)),), dtype=torch.uint8, device=x.device)
    rc = lib().wdf_ss_fwd_lin_tp(_ptr(x), _ptr(coef), ns, ni, _ptr(y), _ptr(zs), _ptr(z0), _ptr(zT), B, T, int(n_chunks),
                                 _ptr(ws), _stream())
    _check(rc, "wdf_ss_fwd_lin_tp")
    return y, zs, zT


def ss_bwd(x, coef, ns, ni, zstash, gy, root_kind=ROOT_NONE, rootp=None, n_up=1, n_down=1, want_gz0=False):
    """Returns (gcoef [ncoef], groot [3] ([5] under ROOT_ASYM_PAIR) | None, gz0 [ns,B] | None)."""
    require_gpu()
    x = _f32_dev(x, "x")
    coef = _f32_dev(coef, "coef")
    rootp = _f32_dev(rootp, "rootp")
    zstash = _f32_dev(zstash, "zstash")
    gy = _f32_dev(gy, "gy")
    B, T = _ss_check_shapes("ss_bwd", x, coef, ns, ni, root_kind, rootp, zstash=zstash, gy=gy, sweep=True)
    ncoef = lib().wdf_ss_ncoef(ns, ni)
    ws = torch.empty((lib().wdf_ss_bwd_ws_bytes(ns, ni, B),), dtype=torch.uint8, device=x.device)
    gcoef = torch.empty((ncoef,), dtype=torch.float32, device=x.device)
    groot = _ss_groot(root_kind, x.device)
    gz0 = torch.empty((ns, B), dtype=torch.float32, device=x.device) if (want_gz0 and ns > 0) else None
    rc = lib().wdf_ss_bwd(_ptr(x), _ptr(coef), _ptr(rootp), ns, ni, root_kind, int(n_up), int(n_down),
                          _ptr(zstash), _ptr(gy), _ptr(ws), _ptr(gcoef), _ptr(groot), _ptr(gz0), B, T, 0, _stream())
    _check(rc, "wdf_ss_bwd")
    return gcoef, groot, gz0


def ss_tp_starts(T, n_chunks, warmup):
    """The sample every chunk's wave begins at (warm-up included) -> list of ints (rows of a stash to hand in as zinit)."""
    K = lib().wdf_ss_tp_chunks(int(T), int(n_chunks))
    out = (C.c_int64 * K)()
    _check(lib().wdf_ss_tp_starts(int(T), K, int(warmup), out), "wdf_ss_tp_starts")
    return list(out)


def ss_fwd_tp(x, coef, ns, ni, rootp, n_chunks, warmup, tol=1e-6, n_up=1, n_down=1, want_stash=True, z0=None, want_zT=False,
              zinit=None, root_kind=ROOT_DIODE_PAIR):
    """Time-parallel forward of a tree with a diode-pair root, or with root_kind=ROOT_ASYM_PAIR (rootp [5]) a pair of two
    different diodes (include/wdf_hip.h, wdf_ss_fwd_tp_root): chunks warmed up from
    z = 0 (or from zinit [chunks, ns, B]: states for the samples ss_tp_starts names), boundaries verified on the device,
    missed waves re-run sequentially behind a gate.
    -> y [T,B], zstash [T,ns,B] | None, zT [ns,B] | None, status (device int32[4]: read with ss_tp_status)."""
    require_gpu()
    x, coef, rootp, z0 = _f32_dev(x, "x"), _f32_dev(coef, "coef"), _f32_dev(rootp, "rootp"), _f32_dev(z0, "z0")
    zinit = _f32_dev(zinit, "zinit")
    B, T = _ss_check_shapes("ss_fwd_tp", x, coef, ns, ni, root_kind, rootp, z0=z0)
    K = lib().wdf_ss_tp_chunks(T, int(n_chunks))
    y = torch.empty((T, B), dtype=torch.float32, device=x.device)
    zs = torch.empty((T, ns, B), dtype=torch.float32, device=x.device) if want_stash else None
    zT = torch.empty((ns, B), dtype=torch.float32, device=x.device) if want_zT else None
    ws = torch.empty((lib().wdf_ss_fwd_tp_ws_bytes(ns, B, K),), dtype=torch.uint8, device=x.device)
    status = torch.empty((4,), dtype=torch.int32, device=x.device)
    if zinit is not None and tuple(zinit.shape) != (K, ns, B):
        raise WdfHipError(f"zinit: expected [chunks, ns, B] = [{K},{ns},{B}]")
    rc = lib().wdf_ss_fwd_tp_root(_ptr(x), _ptr(coef), _ptr(rootp), ns, ni, int(root_kind), int(n_up), int(n_down), _ptr(y),
                                  _ptr(zs), _ptr(z0), _ptr(zT), B, T, K, int(warmup), float(tol), _ptr(zinit), _ptr(ws),
                                  _ptr(status), _stream())
    _check(rc, "wdf_ss_fwd_tp_root")
    return y, zs, zT, status


def ss_tp_status(status):
    s = status.cpu()
    return {"n_bad": int(s[0]), "max_miss": float(s[1:2].view(torch.float32)[0]), "gated_waves": int(s[2])}


def ss_asym_step_built(ns, ni, loss="mse"):
    """Whether the one-pass step of a tree under ROOT_ASYM_PAIR is built for (ns, ni) and this loss ("mse" | "mse_esr"): the
    library answers a workspace size of 0 where it is not (no GPU needed)."""
    f = lib().wdf_ss_asym_step_esr_ws_bytes if loss == "mse_esr" else lib().wdf_ss_asym_step_ws_bytes
    return f(int(ns), int(ni), 64, 64, 1) > 0


def _ss_asym_step_args(who, x, coef, rootp, ns, ni, target, n_chunks, y, z0, want_zT, ws, status):
    require_gpu()
    x, coef, rootp, target, z0 = _f32_dev(x, "x"), _f32_dev(coef, "coef"), _f32_dev(rootp, "rootp"), _f32_dev(target, "target"), _f32_dev(z0, "z0")
    B, T = x.shape[0], x.shape[1]
    if x.numel() != B * T * ni or coef.numel() != lib().wdf_ss_ncoef(ns, ni):
        raise WdfHipError(f"{who}: x / coef do not match ns, ni")
    if rootp is None or rootp.numel() != 5:
        raise WdfHipError(f"{who}: rootp must hold {{Is_up, nVt_up, Is_down, nVt_down, R_port}}")
    if tuple(target.shape) != (T, B):
        raise WdfHipError(f"target must be [T,B] = [{T},{B}]")
    if z0 is not None and tuple(z0.shape) != (ns, B):
        raise WdfHipError(f"z0 must be [ns,B] = [{ns},{B}]")
    K = lib().wdf_ss_tp_chunks(T, int(n_chunks))
    y, zT = _y_zT(y, want_zT, T, B, x, ns)
    need = lib().wdf_ss_asym_step_ws_bytes(ns, ni, B, T, K)
    if need == 0:
        raise WdfHipError(f"{who}: no one-pass step is built for ns={ns}, ni={ni} (compose the loss from ss_fwd_tp and ss_bwd_tp)")
    if status is None:
        status = torch.empty((4,), dtype=torch.int32, device=x.device)
    return x, coef, rootp, target, z0, B, T, K, y, zT, _ws(ws, need, x), status


def ss_asym_step_mse(x, coef, rootp, ns, ni, target, gscale, n_chunks=1, warmup=0, tol=1e-6, y=None, z0=None, want_zT=False, ws=None,
                     status=None, out=None):
    """The MSE training step of a small tree under ROOT_ASYM_PAIR in one pass over the data (wdf_ss_asym_step_mse): forward,
    loss and d(gscale/2 sum (y - target)^2)/d{coef, rootp}; x [B,T,ni] and target [T,B] read once, y written once, no stash.
    n_chunks is rounded like ss_fwd_tp's (1: the exact sequential recursion); y, ws, status, out can be preallocated.
    -> y [T,B], zT [ns,B] | None, out = {sse, gcoef[ncoef], groot[5]}, status (int32[4]; read with ss_tp_status())."""
    x, coef, rootp, target, z0, B, T, K, y, zT, ws, status = _ss_asym_step_args("ss_asym_step_mse", x, coef, rootp, ns, ni, target,
                                                                               n_chunks, y, z0, want_zT, ws, status)
    n = 1 + coef.numel() + 5
    out = _out(out, n, "out", "{sse, gcoef, groot}", x)
    _check(lib().wdf_ss_asym_step_mse(_ptr(x), _ptr(coef), _ptr(rootp), int(ns), int(ni), _ptr(target), float(gscale), _ptr(y), _ptr(z0),
                                      _ptr(zT), B, T, K, int(warmup), float(tol), _ptr(ws), _ptr(status), _ptr(out), _stream()),
           "wdf_ss_asym_step_mse")
    return y, zT, out, status


def ss_asym_step_esr(x, coef, rootp, ns, ni, target, n_global, eps_energy, skip, n_chunks=1, warmup=0, tol=1e-6, y=None, z0=None,
                     want_zT=False, ws=None, status=None, sums=None, g=None, loss3=None, finish=True):
    """The MSE + ESR training step of a small tree under ROOT_ASYM_PAIR in one pass over the data (wdf_ss_asym_step_esr):
    loss = S/n + sqrt(S / (E + eps_energy) / n) on the rows past `skip`, S = sum (y - target)^2, E = sum y^2, n = n_global.
    finish=True: a single rank -- the kernel forms g = dloss/d{coef, rootp} and loss3 = {mse, esr, mse + esr} itself.
    finish=False: one shard of several -- only sums = {S, E, gP[ncoef + 5], gQ[ncoef + 5]} of this call comes back.
    -> y [T,B], zT [ns,B] | None, sums, g, loss3, status (int32[4]; read with ss_tp_status())."""
    x, coef, rootp, target, z0, B, T, K, y, zT, ws, status = _ss_asym_step_args("ss_asym_step_esr", x, coef, rootp, ns, ni, target,
                                                                               n_chunks, y, z0, want_zT, ws, status)
    if lib().wdf_ss_asym_step_esr_ws_bytes(ns, ni, B, T, K) == 0:
        raise WdfHipError(f"ss_asym_step_esr: no MSE + ESR step is built for ns={ns}, ni={ni}")
    ng = coef.numel() + 5
    sums = _out(sums, 2 + 2 * ng, "sums", "{S, E, gP, gQ}", x)
    g, loss3 = _esr_outs(finish, g, ng, "g", loss3, x)
    _check(lib().wdf_ss_asym_step_esr(_ptr(x), _ptr(coef), _ptr(rootp), int(ns), int(ni), _ptr(target), float(n_global), float(eps_energy),
                                      int(skip), _ptr(y), _ptr(z0), _ptr(zT), B, T, K, int(warmup), float(tol), _ptr(ws), _ptr(status),
                                      _ptr(sums), _ptr(g), _ptr(loss3), _stream()), "wdf_ss_asym_step_esr")
    return y, zT, sums, g, loss3, status


def _lin_step_call(name, store_y, lead, y, rest):
    """wdf_<name>(lead..., y, rest...) or, without the y store, wdf_<name>_noy(lead..., rest...): the twins share every other argument."""
    if store_y:
        _check(getattr(lib(), name)(*lead, _ptr(y), *rest), name)
    else:
        _check(getattr(lib(), name + "_noy")(*lead, *rest), name + "_noy")


def _lin_step_shape(x_tm, coef, what="ss_lin_step_mse"):
    """(ns, ni, B, T, ncoef) of a linear one-pass step from x_tm [T,ni,B] and coef ([ncoef], or the probe's [ncoef + 1] with the
    port resistance behind it): the ns in 0..2 whose wdf_ss_ncoef fits."""
    if x_tm.dim() != 3 or x_tm.shape[1] not in (1, 2) or x_tm.shape[0] < 1 or x_tm.shape[2] < 1:
        raise WdfHipError(f"{what}: x_tm must be [T,ni,B] with ni in 1..2, got {tuple(x_tm.shape)}")
    T, ni, B = (int(v) for v in x_tm.shape)
    for ns in (0, 1, 2):
        ncoef = lib().wdf_ss_ncoef(ns, ni)
        if coef.dim() == 1 and coef.numel() in (ncoef, ncoef + 1):
            return ns, ni, B, T, ncoef
    raise WdfHipError(f"{what}: coef {tuple(coef.shape)} is no coefficient vector of ns in 0..2 states and ni = {ni} inputs")


def _lin_step_args(what, ws_bytes, x_tm, coef, jac, target, n_chunks, z0, want_zT, ws, y, store_y=True):
    """The shape checks and buffers the two linear one-pass steps share -> x_tm, coef, target, z0, ns, ni, B, T, n_params, y, ws, zT."""
    _no_y(what, y, store_y)
    require_gpu()
    x_tm, coef, target, z0 = _f32_dev(x_tm, "x_tm"), _f32_dev(coef, "coef"), _f32_dev(target, "target"), _f32_dev(z0, "z0")
    ns, ni, B, T, ncoef = _lin_step_shape(x_tm, coef, what)
    if not (isinstance(jac, torch.Tensor) and jac.is_cuda and jac.dtype == torch.float64 and jac.is_contiguous() and jac.dim() == 2
            and jac.shape[0] in (ncoef, ncoef + 1) and 1 <= jac.shape[1] <= 15):
        raise WdfHipError(f"{what}: jac must be a contiguous float64 [{ncoef} (+1), 1..15] tensor on the GPU")
    n_params = int(jac.shape[1])
    if tuple(target.shape) != (T, B):
        raise WdfHipError(f"target must be [T,B] = [{T},{B}]")
    if ns > 0 and z0 is not None and tuple(z0.shape) != (ns, B):
        raise WdfHipError(f"z0 must be [ns,B] = [{ns},{B}]")
    y, zT = _y_zT(y, want_zT and ns > 0, T, B, x_tm, ns, store_y)
    need = ws_bytes(ns, ni, B, T, int(n_chunks))
    if need == 0:
        raise WdfHipError(f"{what}: no step for ns={ns}, ni={ni}, B={B}, T={T}, n_chunks={n_chunks}")
    return x_tm, coef, target, z0, ns, ni, B, T, n_params, y, _ws(ws, need, x_tm, zeroed=True), zT


def ss_lin_step_mse(x_tm, coef, jac, target, gscale, n_chunks, z0=None, want_zT=False, want_gcoef=False, ws=None, y=None,
                    store_y=True):
    """The MSE training step of a LINEAR tree in one pass (wdf_ss_lin_step_mse, csrc/wdf_ss_step.h): forward, the sum of squared
    errors, d(gscale/2 x that sum)/d{A, Bx, cy, dy} carried forward in time and its contraction with jac.  x_tm [T,ni,B] time-major,
    coef in SSCoef order (ns from its length), jac float64 [ncoef (+1), n_params] (ss_probe's), target [T,B]; z0 [ns,B] or None.
    ws: zeroed wdf_ss_lin_step_ws_bytes() bytes when not given (the step leaves it clean); y, ws and z0 are used as they are --
    the library pairs sequences up by their addresses.  store_y=False: wdf_ss_lin_step_mse_noy -- y is never stored or allocated
    (None in the dict), a y= handed in is refused; the same workspace serves both.
    -> dict: y [T,B] | None, out [1 + n_params] = {SSE, gradients}, loss (0-dim), gcoef [ns^2 + ns ni + ns + ni] | None, zT [ns,B] | None, ws."""
    x_tm, coef, target, z0, ns, ni, B, T, n_params, y, ws, zT = _lin_step_args("ss_lin_step_mse", lib().wdf_ss_lin_step_ws_bytes, x_tm, coef,
                                                                               jac, target, n_chunks, z0, want_zT, ws, y, store_y)
    out = torch.empty((1 + n_params,), dtype=torch.float32, device=x_tm.device)
    loss = torch.empty((), dtype=torch.float32, device=x_tm.device)
    gcoef = torch.empty((ns * ns + ns * ni + ns + ni,), dtype=torch.float32, device=x_tm.device) if want_gcoef else None
    _lin_step_call("wdf_ss_lin_step_mse", store_y, (_ptr(x_tm), _ptr(coef), _ptr(jac), n_params, ns, ni, _ptr(target), float(gscale)), y,
                   (_ptr(ws), _ptr(out), _ptr(loss), _ptr(gcoef), B, T, int(n_chunks), _ptr(z0), _ptr(zT), _stream()))
    return {"y": y, "out": out, "loss": loss, "gcoef": gcoef, "zT": zT, "ws": ws}


def sym_from_upper(tri, n):
    """The symmetric [n,n] matrix whose upper triangle, by rows, is tri [n (n + 1) / 2] (a device gather: no synchronisation)."""
    iu = torch.triu_indices(n, n, device=tri.device)
    H = tri.new_zeros((n, n))
    H[iu[0], iu[1]] = tri
    H[iu[1], iu[0]] = tri
    return H


def ss_lin_step_gn(x_tm, coef, jac, target, gscale, n_chunks, z0=None, want_zT=False, want_hcoef=False, ws=None, y=None):
    """The Gauss-Newton form of ss_lin_step_mse (wdf_ss_lin_step_gn, csrc/wdf_ss_lin_gn.h): the same pass also sums the products of
    the per-row dy/d{A, Bx, cy, dy} and contracts them twice with jac.  Arguments, shape checks and buffers as ss_lin_step_mse
    (always stores y); ws: zeroed wdf_ss_lin_step_gn_ws_bytes() bytes when not given.
    -> dict: y [T,B], out float64 [1 + P + P (P + 1) / 2] = {SSE, d(gscale/2 SSE)/d param [P], H's upper triangle by rows},
    H float64 [P,P] symmetric = gscale J^T J, loss (0-dim float32), hcoef float64 [kG (kG + 1) / 2] | None (sum d d^T over
    {A, Bx, cy, dy} before the Jacobian, upper triangle by rows), zT [ns,B] | None, ws."""
    x_tm, coef, target, z0, ns, ni, B, T, n_params, y, ws, zT = _lin_step_args("ss_lin_step_gn", lib().wdf_ss_lin_step_gn_ws_bytes, x_tm, coef,
                                                                               jac, target, n_chunks, z0, want_zT, ws, y)
    dev = x_tm.device
    out = torch.empty((1 + n_params + n_params * (n_params + 1) // 2,), dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    kG = ns * ns + ns * ni + ns + ni
    hcoef = torch.empty((kG * (kG + 1) // 2,), dtype=torch.float64, device=dev) if want_hcoef else None
    _check(lib().wdf_ss_lin_step_gn(_ptr(x_tm), _ptr(coef), _ptr(jac), n_params, ns, ni, _ptr(target), float(gscale), _ptr(y), _ptr(ws),
                                    _ptr(out), _ptr(loss), _ptr(hcoef), B, T, int(n_chunks), _ptr(z0), _ptr(zT), _stream()),
           "wdf_ss_lin_step_gn")
    return {"y": y, "out": out, "H": sym_from_upper(out[1 + n_params:], n_params), "loss": loss, "hcoef": hcoef, "zT": zT, "ws": ws}


ESR_EPS = 2.220446049250313e-16      # what the scripts' esr_loss adds to the energy (clipper_pot.py:146-156: float64 machine epsilon)


def ss_lin_step_esr(x_tm, coef, jac, target, skip, n_chunks, n_global=None, eps=ESR_EPS, z0=None, want_zT=False, want_gcoef=False,
                    ws=None, y=None, finish=True, store_y=True):
    """The MSE + ESR training step of a LINEAR tree in one pass (wdf_ss_lin_step_esr, csrc/wdf_ss_step.h): loss = S/n +
    sqrt(S / (E + eps) / n) on the rows t >= skip (0 <= skip < T), S = sum (y - target)^2, E = sum y^2, n = n_global (None: this
    call's own B (T - skip)).  Arguments, shape checks and buffers as ss_lin_step_mse; ws: zeroed wdf_ss_lin_step_esr_ws_bytes()
    bytes when not given.  finish=True: a single rank -- the kernel's last wave forms g = dloss/d params and loss3 itself;
    finish=False: one shard of several -- only sums comes back (g and loss3 None): add the shards' sums and call ss_lin_esr_finish().
    store_y=False: wdf_ss_lin_step_esr_noy, as ss_lin_step_mse's.
    -> dict: y [T,B] | None, sums [2 + 2 n_params] = {S, E, gP, gQ}, g [n_params] | None, loss3 [3] = {mse, esr, mse + esr} | None,
    gcoef [2 (ns^2 + ns ni + ns + ni)] = {GP, GQ} | None, zT [ns,B] | None, ws."""
    x_tm, coef, target, z0, ns, ni, B, T, n_params, y, ws, zT = _lin_step_args("ss_lin_step_esr", lib().wdf_ss_lin_step_esr_ws_bytes, x_tm,
                                                                               coef, jac, target, n_chunks, z0, want_zT, ws, y, store_y)
    skip = int(skip)
    if not 0 <= skip < T:
        raise WdfHipError(f"ss_lin_step_esr: skip must be in [0, T) = [0, {T}), got {skip}")
    n_global = float(B * (T - skip)) if n_global is None else float(n_global)
    if not n_global > 0.0 or not float(eps) >= 0.0:
        raise WdfHipError("ss_lin_step_esr: n_global > 0 and eps >= 0")
    dev = x_tm.device
    sums = torch.empty((2 + 2 * n_params,), dtype=torch.float32, device=dev)
    g, loss3 = _esr_outs(finish, None, n_params, "g", None, x_tm)
    gcoef = torch.empty((2 * (ns * ns + ns * ni + ns + ni),), dtype=torch.float32, device=dev) if want_gcoef else None
    _lin_step_call("wdf_ss_lin_step_esr", store_y, (_ptr(x_tm), _ptr(coef), _ptr(jac), n_params, ns, ni, _ptr(target), n_global, float(eps), skip),
                   y, (_ptr(ws), _ptr(sums), _ptr(g), _ptr(loss3), _ptr(gcoef), B, T, int(n_chunks), _ptr(z0), _ptr(zT), _stream()))
    return {"y": y, "sums": sums, "g": g, "loss3": loss3, "gcoef": gcoef, "zT": zT, "ws": ws}


NL_EVAL_SECANT = 12                  # wdf_ss_nl_eval_set: the secant switch, behind the step's fields 2..11


def ss_nl_eval_plan(ns, ni, B, T, n_chunks, cold_warmup, warm_warmup, w_min, w_max, tol, like):
    """A workspace of the diode-root evaluation pass (wdf_ss_nl_eval_ws_bytes), planned (wdf_ss_nl_eval_plan) on the device of
    `like`: the first call starts its chunks from z = 0 with cold_warmup, later ones from the snapshots the calls on THIS
    workspace took."""
    require_gpu()
    need = lib().wdf_ss_nl_eval_ws_bytes(int(ns), int(ni), int(B), int(T), int(n_chunks))
    if need == 0:
        raise WdfHipError(lib().wdf_last_error().decode() or "wdf_ss_nl_eval_ws_bytes: bad arguments")
    ws = torch.empty((need,), dtype=torch.uint8, device=like.device)
    _check(lib().wdf_ss_nl_eval_plan(_ptr(ws), int(ns), int(ni), int(B), int(T), int(n_chunks), int(cold_warmup), int(warm_warmup),
                                     int(w_min), int(w_max), float(tol), _stream()), "wdf_ss_nl_eval_plan")
    return ws


def ss_nl_eval_set(ws, field, value):
    """Field 2..11 of the control block (the step's), or NL_EVAL_SECANT (0: chunks start from the last snapshot as it is)."""
    _check(lib().wdf_ss_nl_eval_set(_ptr(ws), int(field), float(value), _stream()), "wdf_ss_nl_eval_set")


def ss_nl_eval_read(ws):
    """The control block as a dict (NlStepCtl: the step's 32 words, the step's meaning) -- synchronises."""
    raw = np.zeros(32, dtype=np.int32)
    _check(lib().wdf_ss_nl_eval_read(_ptr(ws), raw.ctypes.data, _stream()), "wdf_ss_nl_eval_read")
    f = raw.view(np.float32)
    return {"call": int(raw[0]), "parity": int(raw[1]), "have_snap": int(raw[2]), "w_cur": int(raw[3]), "w_snap": int(raw[4]),
            "w_min": int(raw[5]), "w_max": int(raw[6]), "cool": int(raw[7]), "tol": float(f[8]), "n_bad": int(raw[12]),
            "max_miss": float(f[13]), "gated_groups": int(raw[14]), "total_gated": int(raw[15]), "w_used": int(raw[19])}


def ss_nl_eval(x_tm, coef, params, n_tree, ns, ni, target, n_chunks, ws, skip=0, n_global=None, eps=ESR_EPS, n_up=1, n_down=1, y=None,
               store_y=True, sums=None, loss3=None):
    """The loss-only evaluation pass of a small tree with a diode-pair root (wdf_ss_nl_eval, csrc/wdf_ss_nl_eval.h): forward and
    the two loss sums past skip in one sweep, no gradient.  x_tm [T,ni,B] time-major, coef the probe's outputs (coefficients, then
    the port resistance), params the component values with Is, nVt at [n_tree], [n_tree + 1], target [T,B]; ws from
    ss_nl_eval_plan().  store_y=False: y is never stored or allocated (None in the dict), a y= handed in is refused.
    -> dict: y [T,B] | None, sums [2] float64 = {S, E}, loss3 [3] = {mse, esr, mse + esr} with n = n_global (None: B (T - skip)), ws."""
    _no_y("ss_nl_eval", y, store_y)
    require_gpu()
    x_tm, coef, params, target = _f32_dev(x_tm, "x"), _f32_dev(coef, "coef"), _f32_dev(params, "params"), _f32_dev(target, "target")
    ns, ni, n_tree, skip = int(ns), int(ni), int(n_tree), int(skip)
    if x_tm.dim() != 3 or x_tm.shape[1] != ni:
        raise WdfHipError(f"ss_nl_eval: x must be time-major [T,{ni},B], got {tuple(x_tm.shape)}")
    T, _, B = (int(v) for v in x_tm.shape)
    if tuple(target.shape) != (T, B):
        raise WdfHipError(f"target must be [T,B] = [{T},{B}]")
    if not 0 <= skip < T:
        raise WdfHipError(f"ss_nl_eval: skip must be in [0, T) = [0, {T}), got {skip}")
    n_global = float(B * (T - skip)) if n_global is None else float(n_global)
    if not n_global > 0.0 or not float(eps) >= 0.0:
        raise WdfHipError("ss_nl_eval: n_global > 0 and eps >= 0")
    y, _ = _y_zT(y, False, T, B, x_tm, None, store_y)
    need = lib().wdf_ss_nl_eval_ws_bytes(ns, ni, B, T, int(n_chunks))
    if need == 0:
        raise WdfHipError(lib().wdf_last_error().decode() or "wdf_ss_nl_eval_ws_bytes: bad arguments")
    if ws is None:
        raise WdfHipError("ss_nl_eval: ws must be a workspace planned by ss_nl_eval_plan()")
    ws = _ws(ws, need, x_tm)
    if sums is None:
        sums = torch.empty((2,), dtype=torch.float64, device=x_tm.device)
    elif not (isinstance(sums, torch.Tensor) and sums.is_cuda and sums.dtype == torch.float64 and sums.numel() == 2 and sums.is_contiguous()):
        raise WdfHipError("sums must hold {S, E} (2 doubles) on the GPU")
    loss3 = _out(loss3, 3, "loss3", "{mse, esr, mse + esr}", x_tm)
    _check(lib().wdf_ss_nl_eval(_ptr(x_tm), _ptr(coef), _ptr(params), n_tree, ns, ni, int(n_up), int(n_down), _ptr(target), skip, n_global,
                                float(eps), _ptr(y), _ptr(ws), _ptr(sums), _ptr(loss3), B, T, int(n_chunks), _stream()), "wdf_ss_nl_eval")
    return {"y": y, "sums": sums, "loss3": loss3, "ws": ws}


def ss_lin_eval(x_tm, coef, target, n_chunks, skip=0, n_global=None, eps=ESR_EPS, gscale=None, z0=None, want_zT=False, ws=None, y=None,
                store_y=True, sums=None, loss3=None, loss=None):
    """The loss-only evaluation pass of a LINEAR tree (wdf_ss_lin_eval, csrc/wdf_ss_lin_eval.h): forward and the two loss sums on
    the rows t >= skip, no gradient -- no jac, no out, no optimizer.  x_tm, coef, target, n_chunks, z0 / want_zT and the buffers as
    ss_lin_step_esr's (at the same n_chunks and addresses' alignment the results are that step's bit for bit); ws: zeroed
    wdf_ss_lin_eval_ws_bytes() bytes when not given (the pass leaves it clean; one workspace serves storing and no-y calls).
    gscale: None -> 2 / (B T), the mean squared error in `loss`.  store_y=False: y is never stored or allocated (None in the dict),
    a y= handed in is refused; a y of another shape than [T,B] or on another device than x_tm is refused here, before anything runs.
    -> dict: y [T,B] | None, sums [2] float64 = {S, E}, loss3 [3] = {mse, esr, mse + esr} with n = n_global (None: B (T - skip)),
    loss (0-dim) = gscale/2 x S, zT [ns,B] | None, ws."""
    _no_y("ss_lin_eval", y, store_y)
    if y is not None:
        want = (int(x_tm.shape[0]), int(x_tm.shape[2])) if isinstance(x_tm, torch.Tensor) and x_tm.dim() == 3 else None
        if not isinstance(y, torch.Tensor) or want is None or tuple(y.shape) != want or y.device != x_tm.device:
            raise WdfHipError(f"ss_lin_eval: y must be a [T,B] = {list(want) if want else '[T,B]'} tensor on x_tm's device, got "
                              f"{tuple(getattr(y, 'shape', ()))} on {getattr(y, 'device', None)}")
    require_gpu()
    x_tm, coef, target, z0 = _f32_dev(x_tm, "x_tm"), _f32_dev(coef, "coef"), _f32_dev(target, "target"), _f32_dev(z0, "z0")
    ns, ni, B, T, _ = _lin_step_shape(x_tm, coef, "ss_lin_eval")
    if tuple(target.shape) != (T, B):
        raise WdfHipError(f"target must be [T,B] = [{T},{B}]")
    if ns > 0 and z0 is not None and tuple(z0.shape) != (ns, B):
        raise WdfHipError(f"z0 must be [ns,B] = [{ns},{B}]")
    skip = int(skip)
    if not 0 <= skip < T:
        raise WdfHipError(f"ss_lin_eval: skip must be in [0, T) = [0, {T}), got {skip}")
    n_global = float(B * (T - skip)) if n_global is None else float(n_global)
    if not n_global > 0.0 or not float(eps) >= 0.0:
        raise WdfHipError("ss_lin_eval: n_global > 0 and eps >= 0")
    gscale = 2.0 / (B * T) if gscale is None else float(gscale)
    y, zT = _y_zT(y, want_zT and ns > 0, T, B, x_tm, ns, store_y)
    need = lib().wdf_ss_lin_eval_ws_bytes(ns, ni, B, T, int(n_chunks))
    if need == 0:
        raise WdfHipError(lib().wdf_last_error().decode() or "wdf_ss_lin_eval_ws_bytes: bad arguments")
    ws = _ws(ws, need, x_tm, zeroed=True)
    if sums is None:
        sums = torch.empty((2,), dtype=torch.float64, device=x_tm.device)
    elif not (isinstance(sums, torch.Tensor) and sums.is_cuda and sums.dtype == torch.float64 and sums.numel() == 2 and sums.is_contiguous()):
        raise WdfHipError("sums must hold {S, E} (2 doubles) on the GPU")
    loss3 = _out(loss3, 3, "loss3", "{mse, esr, mse + esr}", x_tm)
    loss = torch.empty((), dtype=torch.float32, device=x_tm.device) if loss is None else _out(loss, 1, "loss", "gscale/2 x S", x_tm)
    _check(lib().wdf_ss_lin_eval(_ptr(x_tm), _ptr(coef), ns, ni, _ptr(target), skip, n_global, float(eps), gscale, _ptr(y), _ptr(ws),
                                 _ptr(sums), _ptr(loss3), _ptr(loss), B, T, int(n_chunks), _ptr(z0), _ptr(zT), _stream()), "wdf_ss_lin_eval")
    return {"y": y, "sums": sums, "loss3": loss3, "loss": loss, "zT": zT, "ws": ws}


def ss_lin_esr_finish(sums, n_global, eps=ESR_EPS, g=None, loss3=None):
    """Several ranks: sums = {S, E, gP[n_params], gQ[n_params]} summed over the ranks -> (g [n_params], loss3 = {mse, esr,
    mse + esr}), the global loss and its gradient (wdf_ss_lin_esr_finish: the single-rank step's own formulas)."""
    require_gpu()
    n_params = (_f32_dev(sums, "sums").numel() - 2) // 2
    if sums.dim() != 1 or not 1 <= n_params <= 15:
        raise WdfHipError("sums must hold {S, E, gP[n_params], gQ[n_params]} with 1..15 parameters")
    if not float(n_global) > 0.0 or not float(eps) >= 0.0:
        raise WdfHipError("ss_lin_esr_finish: n_global > 0 and eps >= 0")
    return _esr_finish(lib().wdf_ss_lin_esr_finish, sums, "sums", n_params, (n_params,), n_global, eps, g, "g", loss3)


PROBE_MAX_OPS, PROBE_MAX_PARAMS = 384, 15                                            # csrc/wdf_ss_step.h


def _probe_tape(ops, consts, outs, n_params):
    """The host arrays of a probe tape, refused where the kernel would index its LDS arrays (or params / consts) out of range:
    an operand is an EARLIER node, a leaf's index lies inside consts / the parameter block, an output is a node."""
    ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 3)
    consts = np.ascontiguousarray(consts, dtype=np.float64).reshape(-1)
    outs = np.ascontiguousarray(outs, dtype=np.int32).reshape(-1)
    n = len(ops)
    if not 1 <= n <= PROBE_MAX_OPS or not 1 <= n_params <= PROBE_MAX_PARAMS or len(outs) < 1:
        raise WdfHipError(f"ss_probe: 1..{PROBE_MAX_OPS} operations on 1..{PROBE_MAX_PARAMS} parameters, at least one output "
                          f"(got {n}, {n_params}, {len(outs)})")
    op, a, b = ops[:, 0], ops[:, 1], ops[:, 2]
    i = np.arange(n)
    two, one = (op >= 2) & (op <= 5), (op == 6) | (op == 7)                           # ADD SUB MUL DIV / NEG RECIP (probe_tape.OP_*)
    bad = (op < 0) | (op > 7)
    bad |= (op == 0) & ((a < 0) | (a >= len(consts)))
    bad |= (op == 1) & ((a < 0) | (a >= n_params))
    bad |= (two | one) & ((a < 0) | (a >= i))
    bad |= two & ((b < 0) | (b >= i))
    if bad.any():
        k = int(np.argmax(bad))
        raise WdfHipError(f"ss_probe: operation {k} = {ops[k].tolist()} names a later node or an index outside the tape")
    if ((outs < 0) | (outs >= n)).any():
        raise WdfHipError(f"ss_probe: an output names a node outside the tape's {n}")
    return ops, consts, outs


def ss_probe(ops, consts, params, outs, jobs=None):
    """The probed step `ops` [n_ops,3] / `consts` (probe_tape.Tape.packed()) at the float32 parameter block `params` on the device,
    in float64 with forward tangents (wdf_ss_probe): -> coef float32 [n_out], coef64 [n_out], jac float64 [n_out, n_params] of the
    nodes `outs`.  jobs: [(Adam, theta, grad), ...] as for adam_jobs -- their updates are applied in the same launch BEFORE the
    probe reads the parameters (wdf_ss_probe_adam)."""
    require_gpu()
    params = _f32_dev(params, "params")
    n_params = int(params.numel())
    ops, consts, outs = _probe_tape(ops, consts, outs, n_params)
    jobs = list(jobs) if jobs else []
    if len(jobs) > ADAM_MULTI_MAX:
        raise WdfHipError(f"ss_probe: at most {ADAM_MULTI_MAX} jobs")
    dev = params.device
    tape_d = torch.as_tensor(ops, device=dev)
    consts_d = torch.as_tensor(consts if len(consts) else np.zeros(1), device=dev)
    outs_d = torch.as_tensor(outs, device=dev)
    n_out = len(outs)
    coef = torch.empty((n_out,), dtype=torch.float32, device=dev)
    coef64 = torch.empty((n_out,), dtype=torch.float64, device=dev)
    jac = torch.empty((n_out, n_params), dtype=torch.float64, device=dev)
    tail = (_ptr(tape_d), len(ops), _ptr(consts_d), _ptr(params), n_params, _ptr(outs_d), n_out, _ptr(coef), _ptr(coef64), _ptr(jac),
            _stream())
    if jobs:
        arr = adam_jobs(jobs)
        _check(lib().wdf_ss_probe_adam(C.cast(arr, C.c_void_p), len(jobs), *tail), "wdf_ss_probe_adam")
    else:
        _check(lib().wdf_ss_probe(*tail), "wdf_ss_probe")
    return coef, coef64, jac


def _dyn_rows_mode(rows, T, n, B, who):
    """per_sample argument of the wdf_ss_dyn_* entry points from the rows' shape: [n] -> 0 (one static row), [T,n,B] -> 1 (a row
    per sample), [1,n,B] with T > 1 -> 2 (a row per sequence: constant along the time axis)."""
    shp = tuple(rows.shape)
    if n and shp == (n,):
        return 0
    if n and shp == (T, n, B):
        return 1
    if n and shp == (1, n, B):
        return 2
    raise WdfHipError(f"{who}: rows [T,{n},B] (per sample), [1,{n},B] (per sequence) or [{n}] (static), got {shp}")


def _dyn_check_shapes(who, ns, B, T, root_kind, rootp, z0=None, zstash=None, gy=None, sweep=False):
    """What the wdf_ss_dyn_* kernels index by (ns, B, T) without the C ABI knowing the arrays' sizes: z0 [ns,B], and for the reverse
    sweep (sweep=True) zstash [T,ns,B] and gy [T,B]; rootp {Is, nVt} under the diode pair, {Is_up, nVt_up, Is_down, nVt_down} under
    two different diodes (a missing rootp is the C ABI's to refuse).  ns = 0 keeps one unread state slot, as ss_dyn_fwd allocates."""
    s1 = max(int(ns), 1)
    if z0 is not None and tuple(z0.shape) != (s1, B):
        raise WdfHipError(f"{who}: z0 must be [ns,B] = [{s1},{B}], got {tuple(z0.shape)}")
    if sweep:
        if zstash is None or tuple(zstash.shape) != (T, s1, B):
            raise WdfHipError(f"{who}: zstash must be [T,ns,B] = [{T},{s1},{B}], got {None if zstash is None else tuple(zstash.shape)}")
        if gy is None or tuple(gy.shape) != (T, B):
            raise WdfHipError(f"{who}: gy must be [T,B] = [{T},{B}], got {None if gy is None else tuple(gy.shape)}")
    need = {ROOT_DIODE_PAIR: 2, ROOT_ASYM_PAIR: 4}.get(int(root_kind), 0)
    if rootp is not None and rootp.numel() < need:
        raise WdfHipError(f"{who}: rootp must hold {need} values for root kind {int(root_kind)} "
                          f"({'Is, nVt' if need == 2 else 'Is_up, nVt_up, Is_down, nVt_down'}), got {rootp.numel()}")


def ss_dyn_fwd(x, rows, ns, ni, root_kind=ROOT_NONE, rootp=None, w=None, hidden=0, n_tanh=0, n_up=1, n_down=1, want_stash=True,
               z0=None, want_zT=False):
    """State-space recursion with streamed coefficient rows / the MLP root on any small tree (wdf_ss_dyn_fwd).
    x [B,T,ni]; rows [T,n,B] (per sample) or [n] (one static row), n = wdf_ss_dyn_row_len(ns, ni).
    -> y [T,B], zstash [T,ns,B] | None, zT [ns,B] | None."""
    require_gpu()
    x, rows, rootp, w, z0 = _f32_dev(x, "x"), _f32_dev(rows, "rows"), _f32_dev(rootp, "rootp"), _f32_dev(w, "w"), _f32_dev(z0, "z0")
    B, T = int(x.shape[0]), int(x.shape[1])
    n = lib().wdf_ss_dyn_row_len(int(ns), int(ni))
    if x.dim() != 3 or int(x.shape[2]) != ni:
        raise WdfHipError(f"ss_dyn_fwd: x [B,T,{ni}] (got {tuple(x.shape)})")
    per = _dyn_rows_mode(rows, T, n, B, "ss_dyn_fwd")
    _dyn_check_shapes("ss_dyn_fwd", ns, B, T, root_kind, rootp, z0=z0)
    y = torch.empty((T, B), dtype=torch.float32, device=x.device)
    zs = torch.empty((T, max(ns, 1), B), dtype=torch.float32, device=x.device) if (want_stash and ns > 0) else None
    zT = torch.empty((max(ns, 1), B), dtype=torch.float32, device=x.device) if want_zT else None
    rc = lib().wdf_ss_dyn_fwd(_ptr(x), _ptr(rows), per, int(ns), int(ni), int(root_kind), _ptr(rootp), _ptr(w), int(hidden),
                              int(n_tanh), int(n_up), int(n_down), _ptr(y), _ptr(zs), _ptr(z0), _ptr(zT), B, T, _stream())
    _check(rc, "wdf_ss_dyn_fwd")
    return y, zs, zT


def ss_dyn_bwd(x, rows, ns, ni, zstash, gy, root_kind=ROOT_NONE, rootp=None, w=None, hidden=0, n_tanh=0, n_up=1, n_down=1, want_gz0=False):
    """Reverse sweep of ss_dyn_fwd for dL/dy = gy [T,B] (wdf_ss_dyn_bwd).
    -> grows [T,n,B] (dL/d row entry of every sample; rows constant in time -- [n] or [1,n,B] -- : [1,n,B], summed over the steps by
    the kernel), groot (diode: float64 [2] = dL/d{Is, nVt}; two different diodes: float64 [4] = dL/d{Is_up, nVt_up, Is_down,
    nVt_down}, the sum over the waves with no chain rule; MLP: the flat weight gradient; else None), gz0 [ns,B] | None."""
    require_gpu()
    x, rows, rootp, w = _f32_dev(x, "x"), _f32_dev(rows, "rows"), _f32_dev(rootp, "rootp"), _f32_dev(w, "w")
    zstash, gy = _f32_dev(zstash, "zstash"), _f32_dev(gy, "gy")
    B, T = int(x.shape[0]), int(x.shape[1])
    n = lib().wdf_ss_dyn_row_len(int(ns), int(ni))
    per = _dyn_rows_mode(rows, T, n, B, "ss_dyn_bwd")
    _dyn_check_shapes("ss_dyn_bwd", ns, B, T, root_kind, rootp, zstash=zstash, gy=gy, sweep=True)
    dev = x.device
    # per sample: dL/d(row) of every sample [T,n,B]; rows constant in time: the kernel's own sum over the steps [1,n,B]
    grows = torch.empty((T if per == 1 else 1, n, B), dtype=torch.float32, device=dev)
    nsum = lib().wdf_ss_dyn_bwd_root_ws_bytes(int(root_kind), B) // (8 * ((B + 63) // 64))
    if nsum == 0:
        raise WdfHipError(f"ss_dyn_bwd: unknown root kind {root_kind}")
    ws = torch.zeros(((B + 63) // 64, nsum), dtype=torch.float64, device=dev)
    mlp = root_kind == ROOT_MLP
    gb, ain, lrin = (torch.empty((T, B), dtype=torch.float32, device=dev) for _ in range(3)) if mlp else (None, None, None)
    gz0 = torch.empty((max(ns, 1), B), dtype=torch.float32, device=dev) if want_gz0 else None
    rc = lib().wdf_ss_dyn_bwd(_ptr(x), _ptr(rows), per, int(ns), int(ni), int(root_kind), _ptr(rootp), _ptr(w), int(hidden),
                              int(n_tanh), int(n_up), int(n_down), _ptr(zstash), _ptr(gy), _ptr(grows), _ptr(ws), _ptr(gb), _ptr(ain),
                              _ptr(lrin), _ptr(gz0), B, T, _stream())
    _check(rc, "wdf_ss_dyn_bwd")
    groot = None
    if root_kind == ROOT_DIODE_PAIR:
        s = ws.sum(dim=0)
        rp = rootp.double()
        groot = torch.stack([s[0] / rp[0], s[1] - s[0] / rp[1]])
    elif root_kind == ROOT_ASYM_PAIR:
        groot = ws.sum(dim=0)
    elif mlp:
        groot = clipper_mlp_wgrad(ain.reshape(-1), lrin.reshape(-1), gb.reshape(-1), None, w, hidden, n_tanh, 1.0)
    return grows, groot, gz0


def dyn_chunks(T, n_chunks):
    """The chunk count wdf_ss_dyn_*_tp accept for a requested one: chunks are whole 8-step units."""
    return chunk_geom(T, n_chunks, 8)[1]


def dyn_chunk_len(T, n_chunks):
    return chunk_geom(T, n_chunks, 8)[0]


def ss_dyn_fwd_tp(x, rows, ns, ni, n_chunks, warmup, tol=1.0e-6, root_kind=ROOT_NONE, rootp=None, w=None, hidden=0, n_tanh=0, n_up=1,
                  n_down=1, want_stash=True, z0=None, want_zT=False, zinit=None):
    """ss_dyn_fwd in verified time chunks (wdf_ss_dyn_fwd_tp).  -> y, zstash | None, zT | None, status (int32 [4]: ss_tp_status)."""
    require_gpu()
    x, rows, rootp, w, z0 = _f32_dev(x, "x"), _f32_dev(rows, "rows"), _f32_dev(rootp, "rootp"), _f32_dev(w, "w"), _f32_dev(z0, "z0")
    zinit = _f32_dev(zinit, "zinit")
    B, T = int(x.shape[0]), int(x.shape[1])
    n = lib().wdf_ss_dyn_row_len(int(ns), int(ni))
    if x.dim() != 3 or int(x.shape[2]) != ni:
        raise WdfHipError(f"ss_dyn_fwd_tp: x [B,T,{ni}] (got {tuple(x.shape)})")
    per = _dyn_rows_mode(rows, T, n, B, "ss_dyn_fwd_tp")
    _dyn_check_shapes("ss_dyn_fwd_tp", ns, B, T, root_kind, rootp, z0=z0)
    K = dyn_chunks(T, n_chunks)
    if zinit is not None and tuple(zinit.shape) != (K, ns, B):
        raise WdfHipError(f"ss_dyn_fwd_tp: zinit must be [{K},{ns},{B}], got {tuple(zinit.shape)}")
    y = torch.empty((T, B), dtype=torch.float32, device=x.device)
    zs = torch.empty((T, ns, B), dtype=torch.float32, device=x.device) if want_stash else None
    zT = torch.empty((ns, B), dtype=torch.float32, device=x.device) if want_zT else None
    ws = torch.empty((lib().wdf_ss_dyn_fwd_tp_ws_bytes(int(ns), B, K),), dtype=torch.uint8, device=x.device)
    status = torch.zeros((4,), dtype=torch.int32, device=x.device)
    rc = lib().wdf_ss_dyn_fwd_tp(_ptr(x), _ptr(rows), per, int(ns), int(ni), int(root_kind), _ptr(rootp), _ptr(w), int(hidden),
                                 int(n_tanh), int(n_up), int(n_down), _ptr(y), _ptr(zs), _ptr(z0), _ptr(zT), B, T, K, int(warmup),
                                 float(tol), _ptr(zinit), _ptr(ws), _ptr(status), _stream())
    _check(rc, "wdf_ss_dyn_fwd_tp")
    return y, zs, zT, status


ROWS_MAX_OPS, ROWS_MAX_CONSTS, ROWS_MAX_OUT, ROWS_MAX_PARAMS = 192, 32, 48, 15      # csrc/wdf_ss_dyn_rows.h


class RowsTape:
    """A probe tape (probe_tape.Tape.packed()) and the nodes of the row entries, as the host arrays wdf_ss_dyn_rows takes."""

    def __init__(self, ops, consts, outs):
        self.ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 3)
        self.consts = np.ascontiguousarray(consts, dtype=np.float64).reshape(-1)
        self.outs = np.ascontiguousarray(outs, dtype=np.int32).reshape(-1)

    def fits(self, n_params):
        return (len(self.ops) <= ROWS_MAX_OPS and len(self.consts) <= ROWS_MAX_CONSTS and len(self.outs) <= ROWS_MAX_OUT
                and n_params <= ROWS_MAX_PARAMS)

    def args(self):
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        return (self.ops.ctypes.data_as(ip), len(self.ops), self.consts.ctypes.data_as(dp), len(self.consts),
                self.outs.ctypes.data_as(ip), len(self.outs))


def _rows_params(params, r):
    if params.dtype != torch.float64 or not params.is_cuda or not params.is_contiguous() or params.dim() != 1:
        raise WdfHipError("ss_dyn_rows: params is a contiguous 1-d float64 tensor on the GPU")
    if r is None:
        return None, 1, 1
    r = _f32_dev(r, "r")
    if r.dim() != 2:
        raise WdfHipError("ss_dyn_rows: r is [T, B]")
    return r, int(r.shape[1]), int(r.shape[0])


def ss_dyn_rows(tape, params, chan, r):
    """rows [T, n, B] float32 (r None: [1, n, 1]) of the probed step `tape` (RowsTape) at the component values `params` (float64
    [P], device), parameter `chan` taken per sample from r [T, B] (wdf_ss_dyn_rows)."""
    require_gpu()
    r, B, T = _rows_params(params, r)
    rows = torch.empty((T, len(tape.outs), B), dtype=torch.float32, device=params.device)
    rc = lib().wdf_ss_dyn_rows(*tape.args(), _ptr(params), int(params.numel()), int(chan), _ptr(r), _ptr(rows), B, T, _stream())
    _check(rc, "wdf_ss_dyn_rows")
    return rows


def ss_dyn_rows_bwd(tape, params, chan, r, grows):
    """dLoss/dparams float64 [P] from the rows' adjoint grows [T, n, B] (wdf_ss_dyn_rows_bwd); the channel's entry is 0."""
    require_gpu()
    r, B, T = _rows_params(params, r)
    grows = _f32_dev(grows, "grows")
    if tuple(grows.shape) != (T, len(tape.outs), B):
        raise WdfHipError(f"ss_dyn_rows_bwd: grows must be [{T}, {len(tape.outs)}, {B}]")
    P = int(params.numel())
    ws = torch.empty((lib().wdf_ss_dyn_rows_bwd_ws_bytes(P, B, T),), dtype=torch.uint8, device=params.device)
    gp = torch.empty((P,), dtype=torch.float64, device=params.device)
    rc = lib().wdf_ss_dyn_rows_bwd(*tape.args(), _ptr(params), P, int(chan), _ptr(r), _ptr(grows), _ptr(ws), _ptr(gp), B, T, _stream())
    _check(rc, "wdf_ss_dyn_rows_bwd")
    return gp


def ss_dyn_bwd_tp(x, rows, ns, ni, zstash, gy, n_chunks, root_kind=ROOT_NONE, rootp=None, w=None, hidden=0, n_tanh=0, n_up=1, n_down=1,
                  want_gz0=False):
    """ss_dyn_bwd in exact time chunks (wdf_ss_dyn_bwd_tp): same results up to fp32 summation order."""
    require_gpu()
    x, rows, rootp, w = _f32_dev(x, "x"), _f32_dev(rows, "rows"), _f32_dev(rootp, "rootp"), _f32_dev(w, "w")
    zstash, gy = _f32_dev(zstash, "zstash"), _f32_dev(gy, "gy")
    B, T = int(x.shape[0]), int(x.shape[1])
    n = lib().wdf_ss_dyn_row_len(int(ns), int(ni))
    per = _dyn_rows_mode(rows, T, n, B, "ss_dyn_bwd_tp")
    _dyn_check_shapes("ss_dyn_bwd_tp", ns, B, T, root_kind, rootp, zstash=zstash, gy=gy, sweep=True)
    dev = x.device
    K = dyn_chunks(T, n_chunks)
    # per sample: [T,n,B]; rows constant in time: one partial per chunk [K,n,B], added up below
    grows = torch.empty((T if per == 1 else K, n, B), dtype=torch.float32, device=dev)
    nws = lib().wdf_ss_dyn_bwd_tp_root_ws_bytes(int(root_kind), int(ns), B, T, K)
    if nws == 0:
        raise WdfHipError(f"ss_dyn_bwd_tp: no workspace for root kind {root_kind}, ns={ns}, B={B}, T={T}, {K} chunks")
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    mlp = root_kind == ROOT_MLP
    gb, ain, lrin = (torch.empty((T, B), dtype=torch.float32, device=dev) for _ in range(3)) if mlp else (None, None, None)
    gz0 = torch.empty((ns, B), dtype=torch.float32, device=dev) if want_gz0 else None
    rc = lib().wdf_ss_dyn_bwd_tp(_ptr(x), _ptr(rows), per, int(ns), int(ni), int(root_kind), _ptr(rootp), _ptr(w), int(hidden),
                                 int(n_tanh), int(n_up), int(n_down), _ptr(zstash), _ptr(gy), _ptr(grows), _ptr(ws), _ptr(gb), _ptr(ain),
                                 _ptr(lrin), _ptr(gz0), B, T, K, _stream())
    _check(rc, "wdf_ss_dyn_bwd_tp")
    groot = None
    if root_kind == ROOT_DIODE_PAIR:
        nparts = K * ((B + 63) // 64)
        s = ws[:nparts * 16].view(torch.float64).reshape(nparts, 2).sum(dim=0)
        rp = rootp.double()
        groot = torch.stack([s[0] / rp[0], s[1] - s[0] / rp[1]])
    elif root_kind == ROOT_ASYM_PAIR:
        nparts = K * ((B + 63) // 64)
        groot = ws[:nparts * 32].view(torch.float64).reshape(nparts, 4).sum(dim=0)
    elif mlp:
        groot = clipper_mlp_wgrad(ain.reshape(-1), lrin.reshape(-1), gb.reshape(-1), None, w, hidden, n_tanh, 1.0)
    if per != 1:
        grows = grows.sum(dim=0, keepdim=True, dtype=torch.float64).float() if K > 1 else grows      # [1,n,B]: the chunks in order
    return grows, groot, gz0


def ss_bwd_gx_built(ns, ni, root_kind):
    """Whether the input-gradient pass is built for (ns, ni, root_kind): the entry point itself answers, from the table its
    launch goes by, before it looks at anything but x, coef and the root arguments (no GPU needed: with gy and gx null the
    call ends in its argument checks, and no pointer is ever followed)."""
    one = (C.c_float * 8)()
    at = C.c_void_p(C.addressof(one))
    rc = lib().wdf_ss_bwd_gx(at, at, at, int(ns), int(ni), int(root_kind), 1, 1, None, None, None, None, None, 64, 64, 1, None)
    # (built: the call got as far as its null-pointer checks; not built, or no such ns / ni / root kind: it ended before them)
    return rc == -1 and lib().wdf_last_error().decode().startswith("null gy/gx")


def ss_bwd_gx(x, coef, ns, ni, zs, gy, root_kind=ROOT_NONE, rootp=None, n_up=1, n_down=1, n_chunks=1, ws_bwd_tp=None, gx=None,
              ws_gx=None):
    """The input gradient dL/dx of a reverse sweep (wdf_ss_bwd_gx) -> gx [T,ni,B], time-major: gx.permute(2, 0, 1) is a view in
    x's own [B,T,ni] layout.  x, coef, zs (the stash), gy, the root arguments: the sweep's.  n_chunks == 1: the sequential form.
    n_chunks > 1: behind ss_bwd_tp(..., n_chunks, return_ws=True) on the same stream, ws_bwd_tp the workspace that call handed
    back; ws_gx (or a fresh buffer) receives the chunks' entering adjoints, float [K, ns, B].  gx can be preallocated."""
    require_gpu()
    x, coef, rootp = _f32_dev(x, "x"), _f32_dev(coef, "coef"), _f32_dev(rootp, "rootp")
    zs, gy = _f32_dev(zs, "zstash"), _f32_dev(gy, "gy")
    B, T = _ss_check_shapes("ss_bwd_gx", x, coef, ns, ni, root_kind, rootp, zstash=zs, gy=gy, sweep=True)
    if not ss_bwd_gx_built(ns, ni, root_kind):
        raise WdfHipError(f"ss_bwd_gx: no input-gradient kernel is built for ns={ns}, ni={ni}, root kind {int(root_kind)}")
    n_chunks = int(n_chunks)
    if n_chunks < 1 or (n_chunks > 1 and ns < 1):
        raise WdfHipError(f"ss_bwd_gx: n_chunks >= 1, and 1 for a tree without states (got {n_chunks}, ns={ns})")
    K = lib().wdf_ss_tp_chunks(T, n_chunks)
    if K > 1:
        if ws_bwd_tp is None:
            raise WdfHipError("ss_bwd_gx: n_chunks > 1 needs ws_bwd_tp, the workspace ss_bwd_tp(..., return_ws=True) handed back")
        ws_bwd_tp = _ws(ws_bwd_tp, lib().wdf_ss_bwd_tp_ws_bytes(ns, ni, B, K), x)
        ws_gx = _ws(ws_gx, lib().wdf_ss_bwd_gx_ws_bytes(ns, B, K), x)
    else:
        ws_bwd_tp = ws_gx = None
    if gx is not None and tuple(getattr(gx, "shape", ())) != (T, ni, B):
        raise WdfHipError(f"gx must be [T,ni,B] = [{T},{ni},{B}], got {tuple(getattr(gx, 'shape', ()))}")
    gx = _out(gx, T * ni * B, "gx", "one value per sample and channel", x).view(T, ni, B)
    rc = lib().wdf_ss_bwd_gx(_ptr(x), _ptr(coef), _ptr(rootp), int(ns), int(ni), int(root_kind), int(n_up), int(n_down), _ptr(zs),
                             _ptr(gy), _ptr(ws_bwd_tp), _ptr(ws_gx), _ptr(gx), B, T, K, _stream())
    _check(rc, "wdf_ss_bwd_gx")
    return gx


def ss_bwd_tp(x, coef, ns, ni, zstash, gy, n_chunks, root_kind=ROOT_NONE, rootp=None, n_up=1, n_down=1, want_gz0=False,
              return_ws=False):
    """Exact chunked reverse sweep (wdf_ss_bwd_tp); same returns as ss_bwd.  return_ws: the workspace the call used comes back
    as a fourth value (ss_bwd_gx reads the chunk records in it)."""
    require_gpu()
    x, coef, rootp = _f32_dev(x, "x"), _f32_dev(coef, "coef"), _f32_dev(rootp, "rootp")
    zstash, gy = _f32_dev(zstash, "zstash"), _f32_dev(gy, "gy")
    B, T = _ss_check_shapes("ss_bwd_tp", x, coef, ns, ni, root_kind, rootp, zstash=zstash, gy=gy, sweep=True)
    K = lib().wdf_ss_tp_chunks(T, int(n_chunks))
    ncoef = lib().wdf_ss_ncoef(ns, ni)
    ws = torch.empty((lib().wdf_ss_bwd_tp_ws_bytes(ns, ni, B, K),), dtype=torch.uint8, device=x.device)
    gcoef = torch.empty((ncoef,), dtype=torch.float32, device=x.device)
    groot = _ss_groot(root_kind, x.device)
    gz0 = torch.empty((ns, B), dtype=torch.float32, device=x.device) if want_gz0 else None
    rc = lib().wdf_ss_bwd_tp(_ptr(x), _ptr(coef), _ptr(rootp), ns, ni, root_kind, int(n_up), int(n_down), _ptr(zstash),
                             _ptr(gy), _ptr(ws), _ptr(gcoef), _ptr(groot), _ptr(gz0), B, T, K, _stream())
    _check(rc, "wdf_ss_bwd_tp")
    return (gcoef, groot, gz0, ws) if return_ws else (gcoef, groot, gz0)


def omega(x, want_iters=False):
    require_gpu()
    x = _f32_dev(x, "x")
    w = torch.empty_like(x)
    it = torch.empty(x.shape, dtype=torch.int32, device=x.device) if want_iters else None
    _check(lib().wdf_omega_f32(_ptr(x), _ptr(w), _ptr(it), x.numel(), _stream()), "wdf_omega_f32")
    return (w, it) if want_iters else w


def diode_pair(a, R_port, Is, nVt, n_up=1, n_down=1):
    require_gpu()
    a = _f32_dev(a, "a")
    R_port = _f32_dev(R_port, "R_port")
    b = torch.empty_like(a)
    _check(lib().wdf_diode_pair_f32(_ptr(a), _ptr(R_port), float(Is), float(nVt), int(n_up), int(n_down),
                                    _ptr(b), a.numel(), _stream()), "wdf_diode_pair_f32")
    return b


class Adam:
    """Device-resident tf.keras.optimizers.Adam for a small float32 parameter vector (component
    values, flat MLP weights <= 1024): per-parameter learning rates and clip constraints
    (tf_wdf.py:74,104); one kernel launch per step, no host round trip."""

    def __init__(self, n, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7, lo=None, hi=None, device="cuda"):
        require_gpu()
        self.n = int(n)
        self.b1, self.b2, self.eps = float(beta_1), float(beta_2), float(epsilon)
        f = lambda a: torch.as_tensor(a, dtype=torch.float32).expand(self.n).contiguous().to(device)  # noqa: E731
        self.lr = f(lr)
        self.lr_scalar = float(lr) if np.ndim(lr) == 0 else None
        self.lo = None if lo is None else f(lo)
        self.hi = None if hi is None else f(hi)
        self.m = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.v = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.step = torch.zeros(1, dtype=torch.int32, device=device)

    def apply(self, theta, grad):
        """theta (in place) <- Adam update with grad, then the clip constraint."""
        theta = _f32_dev(theta, "theta")
        grad = _f32_dev(grad, "grad")
        if theta.numel() != self.n or grad.numel() != self.n:
            raise WdfHipError(f"Adam: expected {self.n} parameters")
        rc = lib().wdf_adam_step(_ptr(theta), _ptr(grad), *_adam_args(self), self.n, _stream())
        _check(rc, "wdf_adam_step")


class _AdamJob(C.Structure):                       # include/wdf_hip.h: wdf_adam_job
    _fields_ = [("theta", C.c_void_p), ("grad", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("step", C.c_void_p),
                ("lr", C.c_void_p), ("lo", C.c_void_p), ("hi", C.c_void_p), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("n", C.c_int)]


ADAM_MULTI_MAX = 8


def adam_jobs(jobs):
    """[(Adam, theta, grad), ...] -> the C array of wdf_adam_job."""
    arr = (_AdamJob * len(jobs))()
    for a, (opt, theta, grad) in zip(arr, jobs):
        theta, grad = _f32_dev(theta, "theta"), _f32_dev(grad, "grad")
        if theta.numel() != opt.n or grad.numel() != opt.n:
            raise WdfHipError(f"Adam: expected {opt.n} parameters")
        a.theta, a.grad, a.m, a.v, a.step, a.lr = _ptr(theta), _ptr(grad), _ptr(opt.m), _ptr(opt.v), _ptr(opt.step), _ptr(opt.lr)
        a.lo, a.hi, a.beta1, a.beta2, a.eps, a.n = _ptr(opt.lo), _ptr(opt.hi), opt.b1, opt.b2, opt.eps, opt.n
    return arr


def adam_step_multi(jobs):
    """jobs: [(Adam, theta, grad), ...] (at most ADAM_MULTI_MAX, distinct optimizers): every update in ONE launch."""
    if len(jobs) == 1:
        jobs[0][0].apply(jobs[0][1], jobs[0][2])
        return
    arr = adam_jobs(jobs)
    _check(lib().wdf_adam_step_multi(C.cast(arr, C.c_void_p), len(jobs), _stream()), "wdf_adam_step_multi")


def clock_stamp(out):
    """out: int64 device tensor [2] <- {shader clock counter, 100 MHz counter} when the stream gets here."""
    _check(lib().wdf_clock_stamp(_ptr(out), _stream()), "wdf_clock_stamp")


def device_info(device=0):
    buf = C.create_string_buffer(64)
    cus = lib().wdf_device_info(int(device), buf, 64)
    if cus < 0:
        raise WdfHipError(lib().wdf_last_error().decode())
    return buf.value.decode(), cus


class Event:
    """HIP event on the stream the kernels run on (bench.py roofline timing)."""

    def __init__(self):
        self.h = lib().wdf_event_create()
        if not self.h:
            raise WdfHipError("hipEventCreate failed")

    def record(self):
        _check(lib().wdf_event_record(self.h, _stream()), "wdf_event_record")

    def elapsed_ms(self, stop):
        ms = C.c_float(0.0)
        _check(lib().wdf_event_elapsed_ms(self.h, stop.h, C.byref(ms)), "wdf_event_elapsed_ms")
        return ms.value

    @staticmethod
    def bracket_next(start, stop):
        """Record start/stop right around the next recurrence kernel launched from this thread
        (excluding the verify / combine / reduce helpers of the same C call)."""
        lib().wdf_event_bracket_next(start.h, stop.h)

    def __del__(self):
        try:
            lib().wdf_event_destroy(self.h)
        except Exception:
            pass
