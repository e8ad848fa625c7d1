// wdf_capi_asym.hip -- C ABI of the two-different-diode (asymmetric) clipper (csrc/wdf_asym.h, csrc/wdf_asym_step.h): sequential and
// time-parallel forward / reverse sweep, the stand-alone root, the one-pass MSE and MSE + ESR steps.  Argument checking, workspace layouts,
// template dispatch and launches.
#include "wdf_capi_asym_checks.h"
#include "wdf_asym.h"
#include "wdf_asym_step.h"
using namespace wdfcapi;

namespace {

static_assert(WDF_ASYM_OMEGA_F32 == wdf::kAsymOmega && WDF_ASYM_NEWTON_F64 == wdf::kAsymNewton64 && WDF_ASYM_NEWTON_F32 == wdf::kAsymNewton32,
              "the header's mode numbers are the kernels'");
using AsymModes = Values<int, wdf::kAsymOmega, wdf::kAsymNewton64, wdf::kAsymNewton32>;
using NewtonModes = Values<int, wdf::kAsymNewton64, wdf::kAsymNewton32>;
constexpr int kUnit = kAsymUnit;             // chunk lengths and warm-ups are multiples of 8 steps (wdf_capi_asym_checks.h, with asym_check and newton_check)

// the sequential forward; with a gate: only the waves the verification flagged, the others leave at once
// rseq != nullptr: one pot resistance per sequence (the RSEQ instantiations; Newton modes only: no closed-form twin is built)
bool launch_asym_fwd(int mode, bool v4, const float* x, const float* theta6, float fs, float* y, float* zstash, const float* z0, float* zT,
                     double tol, int max_iter, long long* iters, int64_t B, int64_t T, const unsigned* gate, hipStream_t s,
                     const float* rseq = nullptr)
{
    return dispatch([&](auto m, auto v, auto rs) {
        if constexpr (rs() && m() == wdf::kAsymOmega) return false;
        else {
            hipLaunchKernelGGL((wdf::clipper_asym_fwd_kernel<m(), v(), rs()>), dim3(waves64(B)), dim3(64), 0, s, x, theta6, fs, y, zstash, z0, zT,
                               tol, max_iter, iters, B, T, gate, rseq);
            return true;
        }
    }, AsymModes{mode}, Bools{v4}, Bools{rseq != nullptr});
}

// what every *_rseq entry point checks on top of its static twin's checks
int rseq_check(const float* rseq, int mode, const char* what)
{
    if (!rseq) return fail(WDF_EINVAL, "%s: null rseq (one resistance per sequence, [B])", what);
    if (mode == WDF_ASYM_OMEGA_F32)
        return fail(WDF_EINVAL, "%s: mode 0 (the closed form, a model approximation kept for comparison) has no per-sequence pot: "
                                "use a Newton mode", what);
    return WDF_OK;
}

struct AsymFwdWs { float* zwarm; float* zend; unsigned* gate; size_t bytes; };
AsymFwdWs asym_fwd_ws(void* ws, int64_t B, int K)
{
    Carver c(ws);
    AsymFwdWs w;
    w.zwarm = c.take<float>((size_t)K * (size_t)B);
    w.zend = c.take<float>((size_t)K * (size_t)B);
    w.gate = c.take<unsigned>(waves64(B));
    w.bytes = c.off;
    return w;
}

struct AsymBwdWs { double* rec; double* part; size_t bytes; };
AsymBwdWs asym_bwd_ws(void* ws, int64_t B, int K)
{
    Carver c(ws);
    AsymBwdWs w;
    w.rec = c.take<double>((size_t)K * (size_t)wdf::kAsymRec * (size_t)B);
    w.part = c.take<double>(waves64(B) * 8);
    w.bytes = c.off;
    return w;
}

// [records double K x 15 x B][per-wave partials double waves x 8][zwarm, zend float K x B each][gate unsigned waves][ticket]
// (the MSE + ESR step: K x 23 x B and waves x 16)
struct AsymStepWs { double* rec; double* part; float* zwarm; float* zend; unsigned* gate; unsigned* ticket; size_t bytes; };
AsymStepWs asym_step_ws(void* ws, int64_t B, int K, bool esr = false)
{
    Carver c(ws);
    AsymStepWs w;
    w.rec = c.take<double>((size_t)K * (size_t)(esr ? wdf::kAsymStepRecEsr : wdf::kAsymStepRec) * (size_t)B);
    w.part = c.take<double>(waves64(B) * (size_t)(esr ? wdf::kAsymStepPartEsr : wdf::kAsymStepPart));
    w.zwarm = c.take<float>((size_t)K * (size_t)B);
    w.zend = c.take<float>((size_t)K * (size_t)B);
    w.gate = c.take<unsigned>(waves64(B));
    w.ticket = c.take<unsigned>(2);
    w.bytes = c.off;
    return w;
}

// The one-pass steps' common part: the checks both share, the chunked launch, the verification, the gated repair launch and
// the finish.  LOSS = 0: MSE (gscale, out7); LOSS = 1: MSE + ESR (skip, esr).
template <int LOSS>
int asym_step_common(const float* x, float* theta6, float fs, int mode, double tol, int max_iter, const float* target, float gscale,
                     int64_t skip, float* y, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup,
                     float verify_tol, void* ws, void* status, float* out7, const wdf::AsymStepEsrOut& esr, float* m, float* v,
                     int32_t* step, const float* lr, float beta1, float beta2, float eps, const float* lo, const float* hi, void* stream,
                     const char* what, const float* rseq = nullptr)
{
    int rc = asym_step_check(B, T, fs, mode, tol, max_iter, n_chunks, warmup, verify_tol, ws, z0, zT);
    if (rc) return rc;
    if (LOSS != 0 && (skip < 0 || skip >= T)) return fail(WDF_EINVAL, "skip must be in 0..T-1");
    if ((rc = adam_check(m, v, step, lr))) return rc;
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    if ((rc = check_tiles(g, n_chunks, T, kUnit, nullptr))) return rc;
    const int64_t W = round_up((int64_t)warmup, kUnit);
    const int64_t Lall = round_up(T, kUnit);                    // one chunk: the repair launch
    const AsymStepWs w = asym_step_ws(ws, B, g.K, LOSS != 0);
    const dim3 grid(waves64(B), (unsigned)g.K);
    hipStream_t s = (hipStream_t)stream;
    const bool v4 = (T % 4 == 0) && aligned16(x);
    const wdf::AsymStepAdam adam{m, v, step, lr, lo, hi, beta1, beta2, eps};
    const auto launch = [&](dim3 gr, const unsigned* gate, int64_t L) {
        return dispatch([&](auto md, auto vv, auto rs) {
            hipLaunchKernelGGL((wdf::clipper_asym_step_kernel<md(), vv(), LOSS, rs()>), gr, dim3(64), 0, s, x, (const float*)theta6, fs, target, y,
                               z0, zT, w.zwarm, w.zend, w.rec, tol, max_iter, (wdf::AsymTpStatus*)status, w.ticket, gate, B, T, L, W, skip, rseq);
        }, NewtonModes{mode}, Bools{v4}, Bools{rseq != nullptr});
    };
    bool ok;
    {
        EventBracket bracket(s);
        ok = launch(grid, nullptr, g.L);
    }
    if (ok && g.K > 1) {
        // every boundary checked on the device; the waves where one missed run again, exactly, as one chunk
        hipLaunchKernelGGL(wdf::asym_tp_verify_kernel, dim3(grid.x), dim3(64), 0, s, w.zwarm, w.zend, B, (int64_t)g.K, verify_tol, w.gate,
                           (wdf::AsymTpStatus*)status);
        ok = launch(dim3(grid.x), w.gate, Lall);
    }
    if (!ok) return no_kernel(what);
    const unsigned* fgate = g.K > 1 ? w.gate : nullptr;
    dispatch([&](auto rs) {
        hipLaunchKernelGGL((wdf::clipper_asym_step_finish_kernel<LOSS, rs()>), dim3(grid.x), dim3(64), 0, s, (const double*)w.rec, fgate, w.part,
                           w.ticket, theta6, fs, gscale, out7, esr, adam, B, (int64_t)g.K, rseq);
    }, Bools{rseq != nullptr});
    return check_launch(what);
}

// wdf_clipper_asym_fwd_tp and its _rseq twin
int asym_fwd_tp_common(const float* x, const float* theta6, float fs, int mode, double tol, int max_iter, float* y, float* zstash,
                       const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup, float verify_tol, void* ws, void* status,
                       void* stream, const char* what, const float* rseq)
{
    if (!x || !theta6 || !y || !ws || !status) return fail(WDF_EINVAL, "null x/theta6/y/ws/status");
    int rc = asym_check(B, T, fs, mode);
    if (rc) return rc;
    if (mode != WDF_ASYM_OMEGA_F32 && (rc = newton_check(tol, max_iter))) return rc;
    if (n_chunks < 1 || warmup < 0 || !(verify_tol >= 0.0f)) return fail(WDF_EINVAL, "n_chunks >= 1, warmup >= 0, verify_tol >= 0");
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    if ((rc = check_tiles(g, n_chunks, T, kUnit, nullptr))) return rc;
    const int64_t W = round_up((int64_t)warmup, kUnit);
    const AsymFwdWs w = asym_fwd_ws(ws, B, g.K);
    const dim3 grid(waves64(B), (unsigned)g.K);
    hipStream_t s = (hipStream_t)stream;
    const bool v4 = (T % 4 == 0) && aligned16(x);
    bool ok = dispatch([&](auto m, auto rs) {
        if constexpr (rs() && m() == wdf::kAsymOmega) return false;
        else {
            hipLaunchKernelGGL((wdf::clipper_asym_fwd_tp_kernel<m(), rs()>), grid, dim3(64), 0, s, x, theta6, fs, y, zstash, z0, zT, w.zwarm,
                               w.zend, tol, max_iter, (wdf::AsymTpStatus*)status, B, T, g.L, W, rseq);
            return true;
        }
    }, AsymModes{mode}, Bools{rseq != nullptr});
    if (ok && g.K > 1) {
        hipLaunchKernelGGL(wdf::asym_tp_verify_kernel, dim3(grid.x), dim3(64), 0, s, w.zwarm, w.zend, B, (int64_t)g.K, verify_tol, w.gate,
                           (wdf::AsymTpStatus*)status);
        ok = launch_asym_fwd(mode, v4, x, theta6, fs, y, zstash, z0, zT, tol, max_iter, nullptr, B, T, w.gate, s, rseq);
    }
    return ok ? check_launch(what) : no_kernel(what);
}

// wdf_clipper_asym_bwd_tp and its _rseq twin
int asym_bwd_tp_common(const float* x, const float* theta6, float fs, int mode, const float* zstash, const float* zT, const float* gy,
                       const float* gzT, void* ws, float* gtheta6, float* gz0, int64_t B, int64_t T, int n_chunks, void* stream,
                       const char* what, const float* rseq)
{
    if (!x || !theta6 || !zstash || !zT || !gy || !ws || !gtheta6) return fail(WDF_EINVAL, "null x/theta6/zstash/zT/gy/ws/gtheta6");
    int rc = asym_check(B, T, fs, mode);
    if (rc) return rc;
    if (n_chunks < 1) return fail(WDF_EINVAL, "n_chunks >= 1");
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    if ((rc = check_tiles(g, n_chunks, T, kUnit, nullptr))) return rc;
    const AsymBwdWs w = asym_bwd_ws(ws, B, g.K);
    const dim3 grid(waves64(B), (unsigned)g.K);
    hipStream_t s = (hipStream_t)stream;
    const bool v4 = (T % 4 == 0) && aligned16(x);
    // both Newton modes: the exact pair, differentiated at the root the forward stored (nothing is re-solved).  With a pot
    // per sequence the combine kernel applies the chain rule per lane and the reduce kernel skips its own.
    const bool ok = dispatch([&](auto newton, auto v, auto rs) {
        if constexpr (rs() && !newton()) return false;
        else {
            hipLaunchKernelGGL((wdf::clipper_asym_bwd_tp_kernel<newton(), v(), rs()>), grid, dim3(64), 0, s, x, theta6, fs, zstash, zT, gy, w.rec, B, T,
                               g.L, rseq);
            hipLaunchKernelGGL(wdf::clipper_asym_bwd_combine_kernel<rs()>, dim3(grid.x), dim3(64), 0, s, (const double*)w.rec, gzT, w.part, gz0, B,
                               (int64_t)g.K, theta6, fs, rseq);
            hipLaunchKernelGGL(wdf::clipper_asym_grad_reduce_kernel<rs()>, dim3(1), dim3(256), 0, s, (const double*)w.part, (int)grid.x, theta6, fs,
                               gtheta6);
            return true;
        }
    }, Bools{mode != WDF_ASYM_OMEGA_F32}, Bools{v4}, Bools{rseq != nullptr});
    if (!ok) return no_kernel(what);
    return check_launch(what);
}

}  // namespace

extern "C" {

int wdf_clipper_asym_fwd(const float* x, const float* theta6, float fs, int mode, double tol, int max_iter, float* y,
                         float* zstash, const float* z0, float* zT, long long* iters, int64_t B, int64_t T, void* stream)
{
    if (!x || !theta6 || !y) return fail(WDF_EINVAL, "null x/theta6/y");
    int rc = asym_check(B, T, fs, mode);
    if (rc) return rc;
    if (mode != WDF_ASYM_OMEGA_F32 && (rc = newton_check(tol, max_iter))) return rc;
    const bool v4 = (T % 4 == 0) && aligned16(x);
    if (!launch_asym_fwd(mode, v4, x, theta6, fs, y, zstash, z0, zT, tol, max_iter, iters, B, T, nullptr, (hipStream_t)stream))
        return no_kernel("wdf_clipper_asym_fwd");
    return check_launch("wdf_clipper_asym_fwd");
}

size_t wdf_clipper_asym_fwd_tp_ws_bytes(int64_t B, int n_chunks)
{
    return (B > 0 && n_chunks > 0) ? asym_fwd_ws(nullptr, B, n_chunks).bytes : 0;
}

int wdf_clipper_asym_fwd_tp(const float* x, const float* theta6, float fs, int mode, double tol, int max_iter, float* y,
                            float* zstash, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup,
                            float verify_tol, void* ws, void* status, void* stream)
{
    return asym_fwd_tp_common(x, theta6, fs, mode, tol, max_iter, y, zstash, z0, zT, B, T, n_chunks, warmup, verify_tol, ws, status, stream,
                              "wdf_clipper_asym_fwd_tp", nullptr);
}

size_t wdf_clipper_asym_bwd_ws_bytes(int64_t B) { return B > 0 ? waves64(B) * 8 * sizeof(double) : 0; }

int wdf_clipper_asym_bwd(const float* x, const float* theta6, float fs, double tol, int max_iter, const float* zstash,
                         const float* gy, void* ws, float* gtheta6, int64_t B, int64_t T, void* stream)
{
    if (!x || !theta6 || !zstash || !gy || !ws || !gtheta6) return fail(WDF_EINVAL, "null x/theta6/zstash/gy/ws/gtheta6");
    if (B <= 0 || T <= 0 || !(fs > 0.0f)) return fail(WDF_EINVAL, "B, T, fs must be positive");
    if (int rc = newton_check(tol, max_iter)) return rc;
    const unsigned grid = (unsigned)waves64(B);
    hipLaunchKernelGGL(wdf::clipper_asym_bwd_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, x, theta6, fs, zstash, gy, tol,
                       max_iter, (double*)ws, B, T);
    hipLaunchKernelGGL(wdf::clipper_asym_grad_reduce_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws,
                       (int)grid, theta6, fs, gtheta6);
    return check_launch("wdf_clipper_asym_bwd");
}

size_t wdf_clipper_asym_bwd_tp_ws_bytes(int64_t B, int n_chunks)
{
    return (B > 0 && n_chunks > 0) ? asym_bwd_ws(nullptr, B, n_chunks).bytes : 0;
}

int wdf_clipper_asym_bwd_tp(const float* x, const float* theta6, float fs, int mode, const float* zstash, const float* zT,
                            const float* gy, const float* gzT, void* ws, float* gtheta6, float* gz0, int64_t B, int64_t T,
                            int n_chunks, void* stream)
{
    return asym_bwd_tp_common(x, theta6, fs, mode, zstash, zT, gy, gzT, ws, gtheta6, gz0, B, T, n_chunks, stream, "wdf_clipper_asym_bwd_tp",
                              nullptr);
}

int wdf_asym_root(const float* a, const float* theta6, float fs, int mode, double tol, int max_iter, double* b, int64_t n,
                  void* stream)
{
    if (!a || !theta6 || !b || n <= 0) return fail(WDF_EINVAL, "wdf_asym_root: bad arguments");
    if (mode < WDF_ASYM_OMEGA_F32 || mode > WDF_ASYM_NEWTON_F32) return fail(WDF_EINVAL, "unknown mode %d", mode);
    if (mode == WDF_ASYM_NEWTON_F32) if (int rc = newton_check(tol, max_iter)) return rc;
    const unsigned grid = (unsigned)((n + 255) / 256);
    const bool ok = dispatch([&](auto m) {
        hipLaunchKernelGGL((wdf::asym_root_kernel<m()>), dim3(grid), dim3(256), 0, (hipStream_t)stream, a, theta6, fs, b, tol, max_iter, n);
    }, AsymModes{mode});
    return ok ? check_launch("wdf_asym_root") : no_kernel("wdf_asym_root");
}

// ---- the one-pass MSE and MSE + ESR steps (wdf_asym_step.h) -----------------------------------------------------------------
size_t wdf_clipper_asym_step_mse_ws_bytes(int64_t B, int n_chunks)
{
    return (B > 0 && n_chunks > 0) ? asym_step_ws(nullptr, B, n_chunks).bytes : 0;
}

int wdf_clipper_asym_step_mse(const float* x, float* theta6, float fs, int mode, double tol, int max_iter, const float* target,
                              float gscale, float* y, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup,
                              float verify_tol, void* ws, void* status, float* out7, float* m, float* v, int32_t* step,
                              const float* lr, float beta1, float beta2, float eps, const float* lo, const float* hi, void* stream)
{
    if (!x || !theta6 || !target || !y || !ws || !status || !out7) return fail(WDF_EINVAL, "null x/theta6/target/y/ws/status/out7");
    return asym_step_common<0>(x, theta6, fs, mode, tol, max_iter, target, gscale, 0, y, z0, zT, B, T, n_chunks, warmup, verify_tol, ws,
                               status, out7, wdf::AsymStepEsrOut{0.0, 0.0, nullptr, nullptr, nullptr}, m, v, step, lr, beta1, beta2, eps,
                               lo, hi, stream, "wdf_clipper_asym_step_mse");
}

size_t wdf_clipper_asym_step_esr_ws_bytes(int64_t B, int n_chunks)
{
    return (B > 0 && n_chunks > 0) ? asym_step_ws(nullptr, B, n_chunks, true).bytes : 0;
}

int wdf_clipper_asym_step_esr(const float* x, float* theta6, float fs, int mode, double tol, int max_iter, const float* target,
                              double n_global, double eps_energy, int64_t skip, float* y, const float* z0, float* zT, int64_t B,
                              int64_t T, int n_chunks, int warmup, float verify_tol, void* ws, void* status, float* sums14,
                              float* gtheta6, float* loss3, float* m, float* v, int32_t* step, const float* lr, float beta1,
                              float beta2, float eps, const float* lo, const float* hi, void* stream)
{
    if (!x || !theta6 || !target || !y || !ws || !status || !sums14) return fail(WDF_EINVAL, "null x/theta6/target/y/ws/status/sums14");
    if (!(n_global > 0.0)) return fail(WDF_EINVAL, "n_global must be positive");
    if (!(eps_energy >= 0.0)) return fail(WDF_EINVAL, "eps_energy must not be negative");
    if (m && !gtheta6) return fail(WDF_EINVAL, "Adam: the update reads the gradient from gtheta6");
    return asym_step_common<1>(x, theta6, fs, mode, tol, max_iter, target, 0.0f, skip, y, z0, zT, B, T, n_chunks, warmup, verify_tol, ws,
                               status, nullptr, wdf::AsymStepEsrOut{n_global, eps_energy, sums14, gtheta6, loss3}, m, v, step, lr, beta1,
                               beta2, eps, lo, hi, stream, "wdf_clipper_asym_step_esr");
}

int wdf_asym_esr_finish(const float* sums14, double n_global, double eps_energy, float* gtheta6, float* loss3, void* stream)
{
    if (!sums14 || !gtheta6 || !(n_global > 0.0) || !(eps_energy >= 0.0))
        return fail(WDF_EINVAL, "wdf_asym_esr_finish: null sums14/gtheta6, n_global <= 0 or eps_energy < 0");
    hipLaunchKernelGGL(wdf::esr_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums14, 6, n_global, eps_energy, gtheta6, loss3);
    return check_launch("wdf_asym_esr_finish");
}

// ---- one pot resistance per sequence: the static entry points' twins with rseq [B] behind x (Newton modes) --------------------
int wdf_clipper_asym_fwd_rseq(const float* x, const float* rseq, const float* theta6, float fs, int mode, double tol, int max_iter,
                              float* y, float* zstash, const float* z0, float* zT, long long* iters, int64_t B, int64_t T, void* stream)
{
    if (!x || !theta6 || !y) return fail(WDF_EINVAL, "null x/theta6/y");
    int rc = asym_check(B, T, fs, mode);
    if (rc) return rc;
    if ((rc = rseq_check(rseq, mode, "wdf_clipper_asym_fwd_rseq"))) return rc;
    if ((rc = newton_check(tol, max_iter))) return rc;
    const bool v4 = (T % 4 == 0) && aligned16(x);
    if (!launch_asym_fwd(mode, v4, x, theta6, fs, y, zstash, z0, zT, tol, max_iter, iters, B, T, nullptr, (hipStream_t)stream, rseq))
        return no_kernel("wdf_clipper_asym_fwd_rseq");
    return check_launch("wdf_clipper_asym_fwd_rseq");
}

int wdf_clipper_asym_fwd_tp_rseq(const float* x, const float* rseq, const float* theta6, float fs, int mode, double tol, int max_iter,
                                 float* y, float* zstash, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup,
                                 float verify_tol, void* ws, void* status, void* stream)
{
    if (int rc = rseq_check(rseq, mode, "wdf_clipper_asym_fwd_tp_rseq")) return rc;
    return asym_fwd_tp_common(x, theta6, fs, mode, tol, max_iter, y, zstash, z0, zT, B, T, n_chunks, warmup, verify_tol, ws, status, stream,
                              "wdf_clipper_asym_fwd_tp_rseq", rseq);
}

int wdf_clipper_asym_bwd_tp_rseq(const float* x, const float* rseq, const float* theta6, float fs, int mode, const float* zstash,
                                 const float* zT, const float* gy, const float* gzT, void* ws, float* gtheta6, float* gz0, int64_t B,
                                 int64_t T, int n_chunks, void* stream)
{
    if (int rc = rseq_check(rseq, mode, "wdf_clipper_asym_bwd_tp_rseq")) return rc;
    return asym_bwd_tp_common(x, theta6, fs, mode, zstash, zT, gy, gzT, ws, gtheta6, gz0, B, T, n_chunks, stream,
                              "wdf_clipper_asym_bwd_tp_rseq", rseq);
}

int wdf_clipper_asym_step_mse_rseq(const float* x, const float* rseq, float* theta6, float fs, int mode, double tol, int max_iter,
                                   const float* target, float gscale, float* y, const float* z0, float* zT, int64_t B, int64_t T,
                                   int n_chunks, int warmup, float verify_tol, void* ws, void* status, float* out7, float* m, float* v,
                                   int32_t* step, const float* lr, float beta1, float beta2, float eps, const float* lo, const float* hi,
                                   void* stream)
{
    if (!x || !theta6 || !target || !y || !ws || !status || !out7) return fail(WDF_EINVAL, "null x/theta6/target/y/ws/status/out7");
    if (int rc = rseq_check(rseq, mode, "wdf_clipper_asym_step_mse_rseq")) return rc;
    return asym_step_common<0>(x, theta6, fs, mode, tol, max_iter, target, gscale, 0, y, z0, zT, B, T, n_chunks, warmup, verify_tol, ws,
                               status, out7, wdf::AsymStepEsrOut{0.0, 0.0, nullptr, nullptr, nullptr}, m, v, step, lr, beta1, beta2, eps,
                               lo, hi, stream, "wdf_clipper_asym_step_mse_rseq", rseq);
}

int wdf_clipper_asym_step_esr_rseq(const float* x, const float* rseq, float* theta6, float fs, int mode, double tol, int max_iter,
                                   const float* target, double n_global, double eps_energy, int64_t skip, float* y, const float* z0,
                                   float* zT, int64_t B, int64_t T, int n_chunks, int warmup, float verify_tol, void* ws, void* status,
                                   float* sums14, float* gtheta6, float* loss3, float* m, float* v, int32_t* step, const float* lr,
                                   float beta1, float beta2, float eps, const float* lo, const float* hi, void* stream)
{
    if (!x || !theta6 || !target || !y || !ws || !status || !sums14) return fail(WDF_EINVAL, "null x/theta6/target/y/ws/status/sums14");
    if (int rc = rseq_check(rseq, mode, "wdf_clipper_asym_step_esr_rseq")) return rc;
    if (!(n_global > 0.0)) return fail(WDF_EINVAL, "n_global must be positive");
    if (!(eps_energy >= 0.0)) return fail(WDF_EINVAL, "eps_energy must not be negative");
    if (m && !gtheta6) return fail(WDF_EINVAL, "Adam: the update reads the gradient from gtheta6");
    return asym_step_common<1>(x, theta6, fs, mode, tol, max_iter, target, 0.0f, skip, y, z0, zT, B, T, n_chunks, warmup, verify_tol, ws,
                               status, nullptr, wdf::AsymStepEsrOut{n_global, eps_energy, sums14, gtheta6, loss3}, m, v, step, lr, beta1,
                               beta2, eps, lo, hi, stream, "wdf_clipper_asym_step_esr_rseq", rseq);
}

}  // extern "C"
