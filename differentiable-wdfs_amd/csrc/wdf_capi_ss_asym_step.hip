// wdf_capi_ss_asym_step.hip -- C ABI of the one-pass MSE and MSE + ESR steps of small state-space trees whose root is a pair of
// two different diodes (csrc/wdf_ss_asym_step.h): argument checking, the workspace layout, template dispatch and the launches
// of a step (chunks, verification, gated repair, finish).
#include "wdf_capi_common.h"
#include "wdf_ss_asym_step.h"
using namespace wdfcapi;

namespace {

constexpr int kUnit = 8;                     // chunk lengths and warm-ups: multiples of 8 steps (wdf_ss_tp_chunks' geometry)
using AsStates = Values<int, 1, 2, 3>;
using AsInputs = Values<int, 1, 2>;

// The instantiations that are built: every (ns, ni, loss) whose chunk and finish kernels fit a wave's registers without scratch
// (make asm TU=wdf_capi_ss_asym_step; profiles/r13_ss_asym_step_resources.txt): one and two states, both losses.  With three
// states the chunk kernel spills (MSE: 9 VGPRs at ni = 1, 2 at ni = 2; MSE + ESR: 103 and 59), so no ns = 3 kernel is built.
constexpr bool as_built(int ns, int ni, int loss) { return ns >= 1 && ns <= 2 && ni >= 1 && ni <= 2 && (loss == 0 || loss == 1); }
bool as_built_any(int ns, int ni) { return as_built(ns, ni, 0) || as_built(ns, ni, 1); }

int as_kn(int ns, int ni) { return ns * ns + ns * ni + ns + ns + ni + ns + ni + 1; }
int as_nt(int ns, int ni) { return ns * ns + ns * ni + ns + ns + ni + 5; }
// (the MSE + ESR step's record and sums, the larger of the two: ONE layout serves both losses)
int as_nrec(int ns, int ni) { return ns * ns + as_nt(ns, ni) * ns + 2 * ns; }
int as_nacc(int ns, int ni) { return 2 * (as_kn(ns, ni) + 5) + 2; }

struct AsWs { float* rec; double* gpart; double* part; float* zwarm; float* zend; unsigned* gate; unsigned* ticket; size_t bytes; };

// the one walk of the workspace: counts with ws = null (wdf_ss_asym_step_ws_bytes), carves otherwise
AsWs as_ws(void* ws, int ns, int ni, int64_t B, int K)
{
    Carver c(ws);
    AsWs w;
    w.gpart = c.take<double>((size_t)K * waves64(B) * (size_t)as_nacc(ns, ni));
    w.part = c.take<double>(waves64(B) * (size_t)as_nacc(ns, ni));
    w.rec = c.take<float>((size_t)K * (size_t)as_nrec(ns, ni) * (size_t)B);
    w.zwarm = c.take<float>((size_t)K * (size_t)ns * (size_t)B);
    w.zend = c.take<float>((size_t)K * (size_t)ns * (size_t)B);
    w.gate = c.take<unsigned>(waves64(B));
    w.ticket = c.take<unsigned>(2);
    w.bytes = c.off;
    return w;
}

// everything both entry points check, before any HIP call
int as_check(const char* what, int loss, const float* x, const float* coef, const float* rootp, int ns, int ni, const float* target,
             int64_t skip, float* y, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup, float tol, void* ws,
             void* status)
{
    if (!x || !coef || !rootp || !target || !y || !ws || !status) return fail(WDF_EINVAL, "%s: null x/coef/rootp/target/y/ws/status", what);
    if (ns < 1 || ns > 3 || ni < 1 || ni > 2)
        return fail(WDF_EUNSUPPORTED, "%s: the step covers ns in [1,3], ni in [1,2] (got ns=%d ni=%d)", what, ns, ni);
    if (!as_built(ns, ni, loss))
        return fail(WDF_EUNSUPPORTED, "%s: ns=%d ni=%d is not built for this loss (its kernels do not fit a wave's registers): compose "
                    "the loss from wdf_ss_fwd_tp_root and wdf_ss_bwd_tp", what, ns, ni);
    if (B <= 0 || T <= 0) return fail(WDF_EINVAL, "%s: B and T must be positive", what);
    if (n_chunks < 1 || n_chunks > 65535 || warmup < 0 || !(tol >= 0.0f))
        return fail(WDF_EINVAL, "%s: n_chunks in 1..65535, warmup >= 0, tol >= 0", what);
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    if (int rc = check_tiles(g, n_chunks, T, kUnit, "wdf_ss_tp_chunks")) return rc;
    if (g.K > 1 && round_up((int64_t)warmup, kUnit) > g.L)
        return fail(WDF_EINVAL, "%s: warmup = %d is longer than a chunk (%lld steps): fewer chunks, or one", what, warmup, (long long)g.L);
    if (loss != 0 && (skip < 0 || skip >= T)) return fail(WDF_EINVAL, "%s: skip must be in 0..T-1", what);
    if (!aligned8(ws)) return fail(WDF_EINVAL, "%s: ws must be 8-byte aligned", what);
    if (z0 && z0 == zT) return fail(WDF_EINVAL, "%s: zT must not alias z0 (every chunk that starts at t = 0 reads z0)", what);
    return WDF_OK;
}

template <int LOSS>
int as_step(const char* what, const float* x, const float* coef, const float* rootp, int ns, int ni, const float* target, int64_t skip,
            float* y, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup, float tol, void* ws, void* status,
            const wdf::SsAsymStepOut& out, void* stream)
{
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    const AsWs w = as_ws(ws, ns, ni, B, g.K);
    const dim3 grid(waves64(B), (unsigned)g.K);
    hipStream_t s = (hipStream_t)stream;
    const bool v4 = ((T * ni) % 4 == 0) && aligned16(x);
    wdf::SsAsymStepArgs a{x, coef, rootp, target, y, z0, zT, w.zwarm, w.zend, w.rec, w.gpart, (wdf::SsTpStatus*)status, w.ticket, nullptr,
                          B, T, g.L, round_up((int64_t)warmup, kUnit), skip};
    const auto launch = [&](dim3 gr) {
        return dispatch([&](auto NS, auto NI, auto V4) {
            if constexpr (!as_built(NS(), NI(), LOSS)) return false;
            else {
                hipLaunchKernelGGL((wdf::ss_asym_step_kernel<NS(), NI(), LOSS, V4()>), gr, dim3(64), 0, s, a);
                return true;
            }
        }, AsStates{ns}, AsInputs{ni}, Bools{v4});
    };
    bool ok;
    {
        EventBracket bracket(s);
        ok = launch(grid);
    }
    if (ok && g.K > 1) {
        // every boundary checked on the device; the waves where one missed run again, exactly, as one chunk
        hipLaunchKernelGGL(wdf::ss_tp_verify_kernel, dim3(grid.x), dim3(64), 0, s, (const float*)w.zwarm, (const float*)w.zend, ns, B,
                           (int64_t)g.K, tol, w.gate, (wdf::SsTpStatus*)status);
        a.gate = w.gate;
        a.L = round_up(T, kUnit);
        ok = launch(dim3(grid.x));
    }
    if (!ok) return no_kernel(what);
    const unsigned* fgate = g.K > 1 ? w.gate : nullptr;
    dispatch([&](auto NS, auto NI) {
        if constexpr (as_built(NS(), NI(), LOSS))
            hipLaunchKernelGGL((wdf::ss_asym_step_finish_kernel<NS(), NI(), LOSS>), dim3(grid.x), dim3(64), 0, s, (const float*)w.rec,
                               (const double*)w.gpart, fgate, w.part, w.ticket, out, B, (int64_t)g.K);
    }, AsStates{ns}, AsInputs{ni});
    return check_launch(what);
}

}  // namespace

extern "C" {

size_t wdf_ss_asym_step_ws_bytes(int ns, int ni, int64_t B, int64_t T, int n_chunks)
{
    if (!as_built_any(ns, ni) || B <= 0 || T <= 0 || n_chunks < 1) return 0;
    if (chunk_geom(T, n_chunks, kUnit).K != n_chunks) return 0;
    return as_ws(nullptr, ns, ni, B, n_chunks).bytes;
}

size_t wdf_ss_asym_step_esr_ws_bytes(int ns, int ni, int64_t B, int64_t T, int n_chunks)
{
    return as_built(ns, ni, 1) ? wdf_ss_asym_step_ws_bytes(ns, ni, B, T, n_chunks) : 0;
}

int wdf_ss_asym_step_mse(const float* x, const float* coef, const float* rootp, int ns, int ni, const float* target, float gscale,
                         float* y, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup, float tol, void* ws,
                         void* status, float* out, void* stream)
{
    const char* what = "wdf_ss_asym_step_mse";
    if (!out) return fail(WDF_EINVAL, "%s: null out", what);
    if (int rc = as_check(what, 0, x, coef, rootp, ns, ni, target, 0, y, z0, zT, B, T, n_chunks, warmup, tol, ws, status)) return rc;
    return as_step<0>(what, x, coef, rootp, ns, ni, target, 0, y, z0, zT, B, T, n_chunks, warmup, tol, ws, status,
                      wdf::SsAsymStepOut{gscale, out, 0.0, 0.0, nullptr, nullptr, nullptr}, stream);
}

int wdf_ss_asym_step_esr(const float* x, const float* coef, const float* rootp, int ns, int ni, const float* target, double n_global,
                         double eps_energy, int64_t skip, float* y, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks,
                         int warmup, float tol, void* ws, void* status, float* sums, float* g, float* loss3, void* stream)
{
    const char* what = "wdf_ss_asym_step_esr";
    if (!sums) return fail(WDF_EINVAL, "%s: null sums", what);
    if (!(n_global > 0.0)) return fail(WDF_EINVAL, "%s: n_global must be positive", what);
    if (!(eps_energy >= 0.0)) return fail(WDF_EINVAL, "%s: eps_energy must not be negative", what);
    if (loss3 && !g) return fail(WDF_EINVAL, "%s: loss3 comes with g (the single-rank finish)", what);
    if (int rc = as_check(what, 1, x, coef, rootp, ns, ni, target, skip, y, z0, zT, B, T, n_chunks, warmup, tol, ws, status)) return rc;
    return as_step<1>(what, x, coef, rootp, ns, ni, target, skip, y, z0, zT, B, T, n_chunks, warmup, tol, ws, status,
                      wdf::SsAsymStepOut{0.0f, nullptr, n_global, eps_energy, sums, g, loss3}, stream);
}

}  // extern "C"
