// wdf_capi_asym_checks.h -- the argument checks the two-different-diode clipper's translation units share (wdf_capi_asym.hip,
// wdf_capi_asym_gn.hip): one set of words in wdf_last_error() for one mistake, whichever entry point meets it.
#pragma once
#include "wdf_capi_common.h"

namespace wdfcapi {

constexpr int kAsymUnit = 8;                 // chunk lengths and warm-ups are multiples of 8 steps

inline int asym_check(int64_t B, int64_t T, float fs, int mode)
{
    if (B <= 0 || T <= 0 || !(fs > 0.0f)) return fail(WDF_EINVAL, "B, T, fs must be positive");
    if (mode < WDF_ASYM_OMEGA_F32 || mode > WDF_ASYM_NEWTON_F32) return fail(WDF_EINVAL, "unknown mode %d", mode);
    return WDF_OK;
}

inline int newton_check(double tol, int max_iter) { return (!(tol > 0.0) || max_iter < 1) ? fail(WDF_EINVAL, "tol > 0, max_iter >= 1") : WDF_OK; }

// what every one-pass step checks ahead of its own arguments and the tiling: sizes, a Newton mode, the solver's and the plan's
// numbers, the workspace's alignment, z0 / zT
inline int asym_step_check(int64_t B, int64_t T, float fs, int mode, double tol, int max_iter, int n_chunks, int warmup,
                           float verify_tol, const void* ws, const float* z0, const float* zT)
{
    int rc = asym_check(B, T, fs, mode);
    if (rc) return rc;
    if (mode == WDF_ASYM_OMEGA_F32)
        return fail(WDF_EINVAL, "mode 0 (the closed form) has no one-pass step: use wdf_clipper_asym_fwd_tp + wdf_clipper_asym_bwd_tp");
    if ((rc = newton_check(tol, max_iter))) return rc;
    if (n_chunks < 1 || n_chunks > 65535 || warmup < 0 || !(verify_tol >= 0.0f))
        return fail(WDF_EINVAL, "n_chunks in 1..65535, warmup >= 0, verify_tol >= 0");
    if (!aligned8(ws)) return fail(WDF_EINVAL, "ws must be 8-byte aligned");
    if (z0 && z0 == zT) return fail(WDF_EINVAL, "zT must not alias z0 (every chunk that starts at t = 0 reads z0)");
    return WDF_OK;
}

}  // namespace wdfcapi
