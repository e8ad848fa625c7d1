// wdf_capi_ss_lin_gn.hip -- C ABI of the Gauss-Newton form of the linear trees' one-pass MSE step (csrc/wdf_ss_lin_gn.h):
// argument checking (the MSE step's, wdf_capi_ss_lin_checks.h), the workspace layout, template dispatch and the two launches.
// A translation unit of its own: the kernels of wdf_capi_ss.hip stay as they are built.
#include "wdf_capi_ss_lin_checks.h"
#include "wdf_ss_lin_gn.h"
using namespace wdfcapi;

namespace {

size_t lin_gn_row(int ns, int ni)
{
    const int g = lin_step_g(ns, ni);
    return (size_t)(g + 1 + wdf::lin_gn_nh(g));
}

}  // namespace

extern "C" {

// The MSE step's layout with the larger partial rows: {gradient entries, sum of squares, Hc's upper triangle} per wave.
size_t wdf_ss_lin_step_gn_ws_bytes(int ns, int ni, int64_t B, int64_t T, int n_chunks)
{
    return lin_step_ok(ns, ni) ? lin_step_ws_rows(ns, ni, B, T, n_chunks, lin_gn_row(ns, ni)) : 0;
}

// x, coef, jac, target, y, n_chunks, z0 / zT as wdf_ss_lin_step_mse.  ws: wdf_ss_lin_step_gn_ws_bytes() bytes, ZERO before the first
// call (the step leaves it clean).  out: double [1 + P + P (P + 1) / 2], P = n_params = {sum of squared errors,
// d(gscale/2 x that sum)/d component value [P], H = gscale J^T J over the component values, upper triangle by rows};
// loss_out: (or NULL) float <- gscale/2 x that sum; hcoef_out: (or NULL) double [kG (kG + 1) / 2], kG = ns^2 + ns ni + ns + ni:
// sum d d^T over {A, Bx, cy, dy} before the Jacobian, upper triangle by rows.
int wdf_ss_lin_step_gn(const float* x, const float* coef, const double* jac, int n_params, int ns, int ni, const float* target,
                       float gscale, float* y, void* ws, double* out, float* loss_out, double* hcoef_out, int64_t B, int64_t T,
                       int n_chunks, const float* z0, float* zT, void* stream)
{
    const char* what = "wdf_ss_lin_step_gn";
    if (int rc = lin_step_mse_check(what, x, coef, jac, n_params, ns, ni, target, true, y, ws, out, B, T, n_chunks, z0, zT)) return rc;
    if (!aligned8(out) || !aligned8(hcoef_out) || !aligned8(ws)) return fail(WDF_EINVAL, "%s: out, hcoef_out and ws must be 8-byte aligned", what);
    const ChunkGeom g = chunk_geom(T, n_chunks, kLinStepUnit);
    const int K = g.K;
    const int64_t L = g.L;
    const LinStepWs w = lin_step_ws(ws, ns, ni, B, K);
    hipStream_t s = (hipStream_t)stream;
    // two sequences per lane by the MSE step's address rule, except on (2,2) (csrc/wdf_ss_lin_gn.h: LinGnPairs)
    const bool pair = lin_step_pairs(B, x, target, y, ws, z0, zT) && !(ns == 2 && ni == 2);
    const int64_t per_wave = pair ? 128 : 64;
    const dim3 grid((unsigned)((B + per_wave - 1) / per_wave), (unsigned)K);
    const bool ok = dispatch([&](auto NS, auto NI, auto PAIR) {
        if constexpr (PAIR() && !wdf::LinGnPairs<NS(), NI()>::ok) return false;
        else {
            using V = std::conditional_t<PAIR(), wdf::v2f, float>;
            if (NS() > 0 && K > 1) hipLaunchKernelGGL((wdf::ss_lin_step_zero_kernel<NS(), NI(), V>), grid, dim3(64), 0, s, x, coef, w.uend0, B, T, L);
            EventBracket bracket(s);
            hipLaunchKernelGGL((wdf::ss_lin_gn_kernel<NS(), NI(), V>), grid, dim3(64), 0, s, x, coef, (const float*)w.uend0, target, y, w.part,
                               w.ticket, jac, n_params, hcoef_out, B, T, L, z0, zT, gscale, out, loss_out);
            return true;
        }
    }, Values<int, 0, 1, 2>{ns}, Values<int, 1, 2>{ni}, Bools{pair});
    return ok ? check_launch(what) : no_kernel(what);
}

}  // extern "C"
