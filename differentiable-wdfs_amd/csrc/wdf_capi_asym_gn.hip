// wdf_capi_asym_gn.hip -- C ABI of the Gauss-Newton form of the two-different-diode clipper's one-pass MSE step
// (csrc/wdf_asym_gn.h): argument checking, the workspace layout, template dispatch and launches.  A translation unit of its
// own: the kernels of wdf_capi_asym.hip stay as they are built.
#include "wdf_capi_asym_checks.h"
#include "wdf_asym_gn.h"
using namespace wdfcapi;

namespace {

using NewtonModes = Values<int, wdf::kAsymNewton64, wdf::kAsymNewton32>;

// [records double K x 43 x B][per-wave partials double waves x 28][zwarm, zend float K x B each][gate unsigned waves][ticket]
struct AsymGnWs { double* rec; double* part; float* zwarm; float* zend; unsigned* gate; unsigned* ticket; size_t bytes; };
AsymGnWs asym_gn_ws(void* ws, int64_t B, int K)
{
    Carver c(ws);
    AsymGnWs w;
    w.rec = c.take<double>((size_t)K * (size_t)wdf::kAsymGnRec * (size_t)B);
    w.part = c.take<double>(waves64(B) * (size_t)wdf::kAsymGnPart);
    w.zwarm = c.take<float>((size_t)K * (size_t)B);
    w.zend = c.take<float>((size_t)K * (size_t)B);
    w.gate = c.take<unsigned>(waves64(B));
    w.ticket = c.take<unsigned>(2);
    w.bytes = c.off;
    return w;
}

}  // namespace

extern "C" {

size_t wdf_clipper_asym_step_gn_ws_bytes(int64_t B, int n_chunks)
{
    return (B > 0 && n_chunks > 0) ? asym_gn_ws(nullptr, B, n_chunks).bytes : 0;
}

int wdf_clipper_asym_step_gn(const float* x, const float* theta6, float fs, int mode, double tol, int max_iter, const float* target,
                             float gscale, float* y, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup,
                             float verify_tol, void* ws, void* status, float* out28, void* stream)
{
    const char* what = "wdf_clipper_asym_step_gn";
    if (!x || !theta6 || !target || !y || !ws || !status || !out28) return fail(WDF_EINVAL, "null x/theta6/target/y/ws/status/out28");
    int rc = asym_step_check(B, T, fs, mode, tol, max_iter, n_chunks, warmup, verify_tol, ws, z0, zT);
    if (rc) return rc;
    const ChunkGeom g = chunk_geom(T, n_chunks, kAsymUnit);
    if ((rc = check_tiles(g, n_chunks, T, kAsymUnit, nullptr))) return rc;
    const int64_t W = round_up((int64_t)warmup, kAsymUnit);
    const int64_t Lall = round_up(T, kAsymUnit);                // one chunk: the repair launch
    const AsymGnWs w = asym_gn_ws(ws, B, g.K);
    const dim3 grid(waves64(B), (unsigned)g.K);
    hipStream_t s = (hipStream_t)stream;
    const bool v4 = (T % 4 == 0) && aligned16(x);
    const auto launch = [&](dim3 gr, const unsigned* gate, int64_t L) {
        return dispatch([&](auto md, auto vv) {
            hipLaunchKernelGGL((wdf::clipper_asym_gn_kernel<md(), vv()>), gr, dim3(64), 0, s, x, theta6, fs, target, y, z0, zT, w.zwarm,
                               w.zend, w.rec, tol, max_iter, (wdf::AsymTpStatus*)status, w.ticket, gate, B, T, L, W);
        }, NewtonModes{mode}, Bools{v4});
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
    hipLaunchKernelGGL(wdf::clipper_asym_gn_finish_kernel, dim3(grid.x), dim3(64), 0, s, (const double*)w.rec, fgate, w.part, w.ticket,
                       theta6, fs, gscale, out28, B, (int64_t)g.K);
    return check_launch(what);
}

}  // extern "C"
