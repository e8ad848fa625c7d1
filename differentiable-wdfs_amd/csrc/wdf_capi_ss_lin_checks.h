// wdf_capi_ss_lin_checks.h -- what the translation units of the linear trees' one-pass steps share (wdf_capi_ss.hip: the MSE and
// MSE + ESR steps; wdf_capi_ss_lin_gn.hip: the Gauss-Newton step): the trees they serve, the workspace walk and the MSE step's
// argument checks -- one set of words in wdf_last_error() for one mistake, whichever entry point meets it.
#pragma once
#include "wdf_capi_common.h"
#include "wdf_ss_step.h"

namespace wdfcapi {

inline bool lin_step_ok(int ns, int ni) { return ns >= 0 && ns <= 2 && ni >= 1 && ni <= 2; }
inline int lin_step_d(int ns, int ni) { return ns * (1 + ns * ns + ns * ni); }
inline int lin_step_g(int ns, int ni) { return ns * ns + ns * ni + ns + ni; }
constexpr int kLinStepUnit = 32;

// the ticket's line, the chunks' zero-state ends, a line of slack for the alignment, the waves' partial sums: a row of
// `row_doubles` per wave (sized for one sequence per lane: a call that pairs them up uses half the waves)
inline size_t lin_step_ws_rows(int ns, int ni, int64_t B, int64_t T, int n_chunks, size_t row_doubles)
{
    if (!lin_step_ok(ns, ni) || B <= 0 || T <= 0 || n_chunks < 1) return 0;
    const int K = chunk_geom(T, n_chunks, kLinStepUnit).K;
    const size_t waves = waves64(B) * (size_t)K;
    return 256 + (size_t)K * (size_t)lin_step_d(ns, ni) * (size_t)B * sizeof(float) + 256 + waves * row_doubles * sizeof(double);
}

// the three parts of such a workspace, each on a 256-byte line of its own (by ADDRESS)
struct LinStepWs { unsigned* ticket; float* uend0; double* part; };
inline LinStepWs lin_step_ws(void* ws, int ns, int ni, int64_t B, int K)
{
    LinStepWs w;
    w.ticket = (unsigned*)ws;
    w.uend0 = (float*)((char*)ws + 256);
    w.part = (double*)round_up((uintptr_t)(w.uend0 + (size_t)K * (size_t)lin_step_d(ns, ni) * (size_t)B), 256);
    return w;
}

// two sequences per lane (8-byte loads and stores) when the rows of x, target, y and the workspace allow it
inline bool lin_step_pairs(int64_t B, const void* x, const void* target, const void* y, const void* ws, const void* z0, const void* zT)
{
    return (B % 2 == 0) && ((((uintptr_t)x | (uintptr_t)target | (uintptr_t)y | (uintptr_t)ws | (uintptr_t)z0 | (uintptr_t)zT) & 7u) == 0);
}

// the MSE step's argument checks (need_y = false: the _noy exports have no y to check)
inline int lin_step_mse_check(const char* what, const float* x, const float* coef, const double* jac, int n_params, int ns, int ni,
                              const float* target, bool need_y, const float* y, const void* ws, const void* out, int64_t B, int64_t T,
                              int n_chunks, const float* z0, const float* zT)
{
    if (z0 && z0 == zT) return fail(WDF_EINVAL, "%s: zT must not alias z0 (every chunk reads z0)", what);
    if (!x || !coef || !jac || !target || (need_y && !y) || !ws || !out) return fail(WDF_EINVAL, "null argument");
    if (!lin_step_ok(ns, ni)) return fail(WDF_EUNSUPPORTED, "%s: ns in 0..2, ni in 1..2 (got %d, %d)", what, ns, ni);
    if (B <= 0 || T <= 0 || n_chunks < 1 || n_params < 1 || n_params > wdf::kProbeMaxParams) return fail(WDF_EINVAL, "B, T, n_chunks >= 1, 1..%d parameters", wdf::kProbeMaxParams);
    return WDF_OK;
}

}  // namespace wdfcapi
