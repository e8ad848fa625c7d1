// wdf_capi_ss.hip -- C ABI of the generic state-space tree kernels (csrc/wdf_statespace.h: sequential, linear scan, time-parallel
// forward / reverse sweep) and of the probe and one-pass MSE step of linear trees (csrc/wdf_ss_step.h).  Argument checking,
// template dispatch and launches.
#include "wdf_capi_common.h"
#include "wdf_statespace.h"
#include "wdf_ss_step.h"
#include "wdf_capi_ss_lin_checks.h"
using namespace wdfcapi;

namespace {

// the shapes the kernels are instantiated for
using SsStates = Values<int, 0, 1, 2, 3, 4>;
using SsStates1 = Values<int, 1, 2, 3, 4>;        // the chunked kernels: at least one state to carry across a boundary
using SsInputs = Values<int, 1, 2>;
using SsRoots = Values<int, wdf::kRootNone, wdf::kRootDiode, wdf::kRootAsym>;
using SsNlRoots = Values<int, wdf::kRootDiode, wdf::kRootAsym>;      // the speculating forward: roots that are not folded into the matrices
// Two different diodes: up to three states.  The chunked reverse sweep's five root sums per run (1 + ns runs) do not fit a wave's
// registers at ns = 4 (kernel-resource-usage: 49 VGPR spills at ni = 1, 280 bytes of scratch at ni = 2), so that size is not built
// for this root in any of the four kernels: WDF_EUNSUPPORTED.
constexpr int kAsymMaxStates = 3;
template <class NS, class ROOT> constexpr bool ss_built(NS, ROOT) { return !(ROOT() == wdf::kRootAsym && NS() > kAsymMaxStates); }
// the instantiations of ss_bwd_gx_kernel: the family's (no instantiation uses scratch: profiles/ss_gx_resources.txt).  A linear
// tree takes SYM = true, two different diodes SYM = false, as in wdf_ss_bwd_tp.
template <class NS, class ROOT, class SYM> constexpr bool ss_gx_built(NS ns, ROOT root, SYM)
{
    return ss_built(ns, root) && !(ROOT() == wdf::kRootNone && !SYM()) && !(ROOT() == wdf::kRootAsym && SYM());
}
constexpr int kUnit = 8;                          // chunk lengths and warm-ups of the time-parallel kernels: multiples of 8 steps

int ss_check(const float* x, const float* coef, const float* rootp, int ns, int ni, int root, int n_up, int n_down,
             int64_t B, int64_t T, int flags)
{
    if (!x || !coef) return fail(WDF_EINVAL, "null x/coef");
    if (ns < 0 || ns > 4 || ni < 1 || ni > 2) return fail(WDF_EUNSUPPORTED, "state-space kernels cover ns in [0,4], ni in [1,2] (got ns=%d ni=%d)", ns, ni);
    if (root != wdf::kRootNone && root != wdf::kRootDiode && root != wdf::kRootAsym) return fail(WDF_EINVAL, "unknown root kind %d", root);
    if (root == wdf::kRootDiode && !rootp) return fail(WDF_EINVAL, "diode root needs rootp = {Is, nVt, R_port}");
    if (root == wdf::kRootAsym && ns > kAsymMaxStates)
        return fail(WDF_EUNSUPPORTED, "the two-different-diode root runs on trees of at most %d states (got ns=%d): its chunked reverse sweep "
                    "does not fit a wave's registers beyond", kAsymMaxStates, ns);
    if (root == wdf::kRootAsym && !rootp) return fail(WDF_EINVAL, "two-different-diode root needs rootp = {Is_up, nVt_up, Is_down, nVt_down, R_port}");
    if (root == wdf::kRootDiode && (n_up < 1 || n_down < 1 || n_up > 16 || n_down > 16)) return fail(WDF_EINVAL, "n_up/n_down must be in [1,16]");
    if (B <= 0 || T <= 0) return fail(WDF_EINVAL, "B and T must be positive");
    if (flags != 0) return fail(WDF_EINVAL, "state-space kernels take flags = 0");
    return WDF_OK;
}

bool ss_v4(const float* x, int64_t T, int ni) { return ((T * ni) % 4 == 0) && aligned16(x); }

// the sequential forward; with a gate: only the 64-sequence groups the verification flagged
bool launch_ss_fwd(int ns, int ni, int root, bool v4, const float* x, const float* coef, const float* rootp, int n_up, int n_down, float* y,
                   float* zstash, const float* z0, float* zT, int64_t B, int64_t T, const unsigned* gate, hipStream_t s)
{
    return dispatch([&](auto NS, auto NI, auto ROOT, auto V4) {
        if constexpr (!ss_built(NS, ROOT)) return false;
        else {
            hipLaunchKernelGGL((wdf::ss_fwd_kernel<NS(), NI(), ROOT(), false, V4()>), dim3(waves64(B)), dim3(64), 0, s, x, coef, rootp, n_up,
                               n_down, y, zstash, z0, zT, B, T, gate);
            return true;
        }
    }, SsStates{ns}, SsInputs{ni}, SsRoots{root}, Bools{v4});
}

void launch_ss_grad_reduce(const double* part, int ns, int ni, int root, const float* rootp, float* gcoef, float* groot, int64_t B, hipStream_t s)
{
    const int ncoef = wdf_ss_ncoef(ns, ni);
    if (root == wdf::kRootAsym) {
        hipLaunchKernelGGL(wdf::ss_grad_reduce_kernel<true>, dim3(1), dim3(64), 0, s, part, (int)waves64(B),
                           ncoef + wdf::kSsRootAcc<wdf::kRootAsym>, ncoef, rootp, gcoef, groot);
        return;
    }
    hipLaunchKernelGGL(wdf::ss_grad_reduce_kernel<false>, dim3(1), dim3(64), 0, s, part, (int)waves64(B), ncoef + 2, ncoef,
                       root == wdf::kRootDiode ? rootp : nullptr, gcoef, root == wdf::kRootDiode ? groot : nullptr);
}

// zwarm / zend [K][ns][B] (the linear scan: zero-state ends / chunk starts), then one gate word per 64 sequences
struct SsTpWs { float* za; float* zb; unsigned* gate; size_t bytes; };
SsTpWs ss_tp_ws(void* ws, int ns, int64_t B, int K)
{
    Carver c(ws);
    SsTpWs w;
    w.za = c.take<float>((size_t)K * (size_t)ns * (size_t)B);
    w.zb = c.take<float>((size_t)K * (size_t)ns * (size_t)B);
    w.gate = c.take<unsigned>(waves64(B));
    w.bytes = c.off;
    return w;
}

}  // namespace

extern "C" {

int wdf_ss_ncoef(int ns, int ni) { return ns * ns + ns * ni + ns + ns + ni + ns + ni + 1; }

size_t wdf_ss_bwd_ws_bytes(int ns, int ni, int64_t B)
{
    // (no root argument: rows of kN + 5 doubles, the two-different-diode root's, hold every root's)
    return B > 0 ? waves64(B) * (size_t)(wdf_ss_ncoef(ns, ni) + wdf::kSsRootAccMax) * sizeof(double) : 0;
}

int wdf_ss_fwd(const float* x, const float* coef, const float* rootp, int ns, int ni, int root, int n_up, int n_down,
               float* y, float* zstash, const float* z0, float* zT, int64_t B, int64_t T, int flags, void* stream)
{
    int rc = ss_check(x, coef, rootp, ns, ni, root, n_up, n_down, B, T, flags);
    if (rc) return rc;
    if (!y) return fail(WDF_EINVAL, "null y");
    if (!launch_ss_fwd(ns, ni, root, ss_v4(x, T, ni), x, coef, rootp, n_up, n_down, y, zstash, z0, zT, B, T, nullptr, (hipStream_t)stream))
        return no_kernel("wdf_ss_fwd");
    return check_launch("wdf_ss_fwd");
}

size_t wdf_ss_fwd_lin_tp_ws_bytes(int ns, int64_t B, int n_chunks)
{
    return (ns > 0 && B > 0 && n_chunks > 0) ? (size_t)2 * (size_t)n_chunks * (size_t)ns * (size_t)B * sizeof(float) : 0;
}

int wdf_ss_fwd_lin_tp(const float* x, const float* coef, int ns, int ni, float* y, float* zstash, const float* z0, float* zT,
                      int64_t B, int64_t T, int n_chunks, void* ws, void* stream)
{
    int rc = ss_check(x, coef, nullptr, ns, ni, wdf::kRootNone, 1, 1, B, T, 0);
    if (rc) return rc;
    if (!y || !ws) return fail(WDF_EINVAL, "null y/ws");
    if (ns < 1) return fail(WDF_EINVAL, "a tree without states has nothing to scan: use wdf_ss_fwd");
    if (n_chunks < 1) return fail(WDF_EINVAL, "n_chunks >= 1");
    const ChunkGeom g = chunk_geom(T, n_chunks, wdf::kLinBurst);      // chunks in whole bursts of the row loads
    const int K = g.K;
    const int64_t L = g.L;
    const SsTpWs w = ss_tp_ws(ws, ns, B, K);                          // (no gate: nothing to verify in a linear scan)
    float* zend0 = w.za;
    float* zstart = w.zb;
    const dim3 grid(waves64(B), (unsigned)K), one(waves64(B));
    hipStream_t s = (hipStream_t)stream;
    // (the last chunk's zero-state end is never used nor written)
    if (K > 1 && (rc = memset_async(zend0 + (size_t)(K - 1) * (size_t)ns * (size_t)B, 0, (size_t)ns * (size_t)B * sizeof(float), s))) return rc;
    const bool ok = dispatch([&](auto NS, auto NI, auto V4) {
        if (K > 1) hipLaunchKernelGGL((wdf::ss_lin_zero_state_kernel<NS(), NI(), V4()>), grid, dim3(64), 0, s, x, coef, zend0, B, T, L);
        hipLaunchKernelGGL((wdf::ss_lin_starts_kernel<NS()>), one, dim3(64), 0, s, coef, zend0, z0, zstart, B, (int64_t)K, L);
        EventBracket bracket(s);
        hipLaunchKernelGGL((wdf::ss_lin_chunk_kernel<NS(), NI(), V4()>), grid, dim3(64), 0, s, x, coef, zstart, y, zstash, zT, B, T, L);
    }, SsStates1{ns}, SsInputs{ni}, Bools{ss_v4(x, T, ni)});
    return ok ? check_launch("wdf_ss_fwd_lin_tp") : no_kernel("wdf_ss_fwd_lin_tp");
}

int wdf_ss_bwd(const float* x, const float* coef, const float* rootp, int ns, int ni, int root, int n_up, int n_down,
               const float* zstash, const float* gy, void* ws, float* gcoef, float* groot, float* gz0, int64_t B,
               int64_t T, int flags, void* stream)
{
    int rc = ss_check(x, coef, rootp, ns, ni, root, n_up, n_down, B, T, flags);
    if (rc) return rc;
    if (!gy || !ws || !gcoef) return fail(WDF_EINVAL, "null gy/ws/gcoef");
    if (ns > 0 && !zstash) return fail(WDF_EINVAL, "null zstash");
    if (root != wdf::kRootNone && !groot) return fail(WDF_EINVAL, "null groot");
    hipStream_t s = (hipStream_t)stream;
    const bool ok = dispatch([&](auto NS, auto NI, auto ROOT, auto V4) {
        if constexpr (!ss_built(NS, ROOT)) return false;
        else {
            hipLaunchKernelGGL((wdf::ss_bwd_kernel<NS(), NI(), ROOT(), false, V4()>), dim3(waves64(B)), dim3(64), 0, s, x, coef, rootp, n_up,
                               n_down, zstash, gy, (double*)ws, gz0, B, T);
            return true;
        }
    }, SsStates{ns}, SsInputs{ni}, SsRoots{root}, Bools{ss_v4(x, T, ni)});
    if (!ok) return no_kernel("wdf_ss_bwd");
    rc = check_launch("wdf_ss_bwd");
    if (rc) return rc;
    launch_ss_grad_reduce((const double*)ws, ns, ni, root, rootp, gcoef, groot, B, s);
    return check_launch("wdf_ss_grad_reduce");
}

// ---- time-parallel state-space kernels (wdf_statespace.h, second half) --------------------------------------
int wdf_ss_tp_chunks(int64_t T, int n_chunks) { return T > 0 ? chunk_geom(T, n_chunks, kUnit).K : 0; }

size_t wdf_ss_fwd_tp_ws_bytes(int ns, int64_t B, int n_chunks)
{
    return (ns < 1 || B <= 0 || n_chunks <= 0) ? 0 : ss_tp_ws(nullptr, ns, B, n_chunks).bytes;
}

int wdf_ss_tp_starts(int64_t T, int n_chunks, int warmup, int64_t* starts)
{
    if (T <= 0 || n_chunks < 1 || warmup < 0 || !starts) return fail(WDF_EINVAL, "T > 0, n_chunks >= 1, warmup >= 0, starts != NULL");
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    if (int rc = check_tiles(g, n_chunks, T, kUnit, "wdf_ss_tp_chunks")) return rc;
    const int64_t W = round_up((int64_t)warmup, kUnit);
    for (int k = 0; k < g.K; ++k) starts[k] = (k * g.L > W) ? k * g.L - W : 0;
    return WDF_OK;
}

int wdf_ss_fwd_tp(const float* x, const float* coef, const float* rootp, int ns, int ni, int n_up, int n_down, float* y,
                  float* zstash, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup, float tol,
                  const float* zinit, void* ws, void* status, void* stream)
{
    return wdf_ss_fwd_tp_root(x, coef, rootp, ns, ni, WDF_ROOT_DIODE_PAIR, n_up, n_down, y, zstash, z0, zT, B, T, n_chunks, warmup, tol,
                              zinit, ws, status, stream);
}

int wdf_ss_fwd_tp_root(const float* x, const float* coef, const float* rootp, int ns, int ni, int root_kind, int n_up, int n_down,
                       float* y, float* zstash, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup, float tol,
                       const float* zinit, void* ws, void* status, void* stream)
{
    if (root_kind != wdf::kRootDiode && root_kind != wdf::kRootAsym)
        return fail(WDF_EINVAL, "wdf_ss_fwd_tp_root: root kind %d has nothing to speculate about (a linear tree takes wdf_ss_fwd_lin_tp)", root_kind);
    int rc = ss_check(x, coef, rootp, ns, ni, root_kind, n_up, n_down, B, T, 0);
    if (rc) return rc;
    if (!y || !ws || !status) return fail(WDF_EINVAL, "null y/ws/status");
    if (ns < 1) return fail(WDF_EINVAL, "a tree without states has nothing to speculate about: use wdf_ss_fwd");
    if (n_chunks < 1 || warmup < 0 || !(tol >= 0.0f)) return fail(WDF_EINVAL, "n_chunks >= 1, warmup >= 0, tol >= 0");
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    if ((rc = check_tiles(g, n_chunks, T, kUnit, "wdf_ss_tp_chunks"))) return rc;
    const SsTpWs w = ss_tp_ws(ws, ns, B, g.K);
    float* zwarm = w.za;
    float* zend = w.zb;
    const dim3 grid(waves64(B), (unsigned)g.K);
    hipStream_t s = (hipStream_t)stream;
    const bool v4 = ss_v4(x, T, ni);
    const int64_t W = round_up((int64_t)warmup, kUnit);
    bool ok;
    {
        EventBracket bracket(s);
        // two different diodes have no symmetric case: they take the SYM = false instantiation
        ok = dispatch([&](auto NS, auto NI, auto ROOT, auto SYM, auto V4) {
            if constexpr ((ROOT() == wdf::kRootAsym && SYM()) || !ss_built(NS, ROOT)) return false;
            else {
                hipLaunchKernelGGL((wdf::ss_fwd_tp_kernel<NS(), NI(), ROOT(), SYM(), V4()>), grid, dim3(64), 0, s, x, coef, rootp, n_up,
                                   n_down, y, zstash, z0, zT, zwarm, zend, (wdf::SsTpStatus*)status, B, T, g.L, W, zinit);
                return true;
            }
        }, SsStates1{ns}, SsInputs{ni}, SsNlRoots{root_kind}, Bools{root_kind == wdf::kRootDiode && n_up == n_down}, Bools{v4});
    }
    if (ok && g.K > 1) {
        hipLaunchKernelGGL(wdf::ss_tp_verify_kernel, dim3(grid.x), dim3(64), 0, s, (const float*)zwarm, (const float*)zend, ns, B,
                           (int64_t)g.K, tol, w.gate, (wdf::SsTpStatus*)status);
        ok = launch_ss_fwd(ns, ni, root_kind, v4, x, coef, rootp, n_up, n_down, y, zstash, z0, zT, B, T, w.gate, s);
    }
    return ok ? check_launch("wdf_ss_fwd_tp") : no_kernel("wdf_ss_fwd_tp");
}

static int ss_tp_rec(int ns, int ni) { const int nacc = wdf_ss_ncoef(ns, ni) + wdf::kSsRootAccMax; return ns * ns + ns + nacc * (ns + 1); }

size_t wdf_ss_bwd_tp_ws_bytes(int ns, int ni, int64_t B, int n_chunks)
{
    if (ns < 1 || B <= 0 || n_chunks <= 0) return 0;
    return wdf_ss_bwd_ws_bytes(ns, ni, B) + (size_t)n_chunks * (size_t)ss_tp_rec(ns, ni) * (size_t)B * sizeof(float);
}

int wdf_ss_bwd_tp(const float* x, const float* coef, const float* rootp, int ns, int ni, int root, int n_up, int n_down,
                  const float* zstash, const float* gy, void* ws, float* gcoef, float* groot, float* gz0, int64_t B, int64_t T,
                  int n_chunks, void* stream)
{
    int rc = ss_check(x, coef, rootp, ns, ni, root, n_up, n_down, B, T, 0);
    if (rc) return rc;
    if (!gy || !ws || !gcoef || !zstash) return fail(WDF_EINVAL, "null gy/ws/gcoef/zstash");
    if (ns < 1) return fail(WDF_EINVAL, "a tree without states has no adjoint to scan: use wdf_ss_bwd");
    if (root != wdf::kRootNone && !groot) return fail(WDF_EINVAL, "null groot");
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    if ((rc = check_tiles(g, n_chunks, T, kUnit, "wdf_ss_tp_chunks"))) return rc;
    double* part = (double*)ws;
    float* rec = (float*)((char*)ws + wdf_ss_bwd_ws_bytes(ns, ni, B));
    const dim3 grid(waves64(B), (unsigned)g.K);
    hipStream_t s = (hipStream_t)stream;
    // a linear tree has no diode pair to be symmetric: it takes the SYM = true instantiation
    // (two different diodes have no symmetric case: SYM = false)
    const bool sym = root == wdf::kRootNone || (root == wdf::kRootDiode && n_up == n_down);
    const bool ok = dispatch([&](auto NS, auto NI, auto ROOT, auto SYM, auto V4) {
        if constexpr ((ROOT() == wdf::kRootNone && !SYM()) || (ROOT() == wdf::kRootAsym && SYM()) || !ss_built(NS, ROOT)) return false;
        else {
            {
                EventBracket bracket(s);
                hipLaunchKernelGGL((wdf::ss_bwd_tp_kernel<NS(), NI(), ROOT(), SYM(), V4()>), grid, dim3(64), 0, s, x, coef, rootp, n_up, n_down,
                                   zstash, gy, rec, B, T, g.L);
            }
            hipLaunchKernelGGL((wdf::ss_bwd_tp_combine_kernel<NS(), NI(), wdf::kSsRootAcc<ROOT()>>), dim3(grid.x), dim3(64), 0, s, (const float*)rec, part, gz0, B,
                               (int64_t)g.K);
            return true;
        }
    }, SsStates1{ns}, SsInputs{ni}, SsRoots{root}, Bools{sym}, Bools{ss_v4(x, T, ni)});
    if (!ok) return no_kernel("wdf_ss_bwd_tp");
    rc = check_launch("wdf_ss_bwd_tp");
    if (rc) return rc;
    launch_ss_grad_reduce(part, ns, ni, root, rootp, gcoef, groot, B, s);
    return check_launch("wdf_ss_grad_reduce");
}

// ---- the input gradient dL/dx (wdf_statespace.h: ss_bwd_gx_kernel, ss_bwd_gx_lamin_kernel) ------------------------------

size_t wdf_ss_bwd_gx_ws_bytes(int ns, int64_t B, int n_chunks)
{
    return (ns < 1 || B <= 0 || n_chunks <= 1) ? 0 : (size_t)n_chunks * (size_t)ns * (size_t)B * sizeof(float);
}

int wdf_ss_bwd_gx(const float* x, const float* coef, const float* rootp, int ns, int ni, int root, int n_up, int n_down,
                  const float* zstash, const float* gy, const void* ws_bwd_tp, void* ws_gx, float* gx, int64_t B, int64_t T,
                  int n_chunks, void* stream)
{
    int rc = ss_check(x, coef, rootp, ns, ni, root, n_up, n_down, B, T, 0);
    if (rc) return rc;
    const bool sym = root == wdf::kRootNone || (root == wdf::kRootDiode && n_up == n_down);
    // (the table the launch below goes by, asked before anything else: a combination that is not built says so whatever else is wrong)
    if (!dispatch([&](auto NS, auto ROOT, auto SYM) { return ss_gx_built(NS, ROOT, SYM); }, SsStates{ns}, SsRoots{root}, Bools{sym}))
        return no_kernel("wdf_ss_bwd_gx");
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    if ((rc = check_tiles(g, n_chunks, T, kUnit, "wdf_ss_tp_chunks"))) return rc;
    if (!gy || !gx) return fail(WDF_EINVAL, "null gy/gx");
    if (ns > 0 && !zstash) return fail(WDF_EINVAL, "null zstash");
    if (n_chunks > 1 && ns < 1) return fail(WDF_EINVAL, "a tree without states has no adjoint to carry across chunks: n_chunks = 1");
    if (n_chunks > 1 && (!ws_bwd_tp || !ws_gx)) return fail(WDF_EINVAL, "n_chunks > 1 needs wdf_ss_bwd_tp's workspace and ws_gx");
    hipStream_t s = (hipStream_t)stream;
    float* lamin = g.K > 1 ? (float*)ws_gx : nullptr;
    if (lamin) {
        const float* rec = (const float*)((const char*)ws_bwd_tp + wdf_ss_bwd_ws_bytes(ns, ni, B));
        const bool ok = dispatch([&](auto NS, auto NI, auto ROOT) {
            if constexpr (!ss_built(NS, ROOT)) return false;
            else {
                hipLaunchKernelGGL((wdf::ss_bwd_gx_lamin_kernel<NS(), NI(), wdf::kSsRootAcc<ROOT()>>), dim3(waves64(B)), dim3(64), 0, s, rec,
                                   lamin, B, (int64_t)g.K);
                return true;
            }
        }, SsStates1{ns}, SsInputs{ni}, SsRoots{root});
        if (!ok) return no_kernel("wdf_ss_bwd_gx");
        if ((rc = check_launch("wdf_ss_bwd_gx (entering adjoints)"))) return rc;
    }
    const dim3 grid(waves64(B), (unsigned)g.K);
    const bool ok = dispatch([&](auto NS, auto NI, auto ROOT, auto SYM, auto V4) {
        if constexpr (!ss_gx_built(NS, ROOT, SYM)) return false;
        else {
            EventBracket bracket(s);
            hipLaunchKernelGGL((wdf::ss_bwd_gx_kernel<NS(), NI(), ROOT(), SYM(), V4()>), grid, dim3(64), 0, s, x, coef, rootp, n_up, n_down,
                               zstash, gy, (const float*)lamin, gx, B, T, g.L);
            return true;
        }
    }, SsStates{ns}, SsInputs{ni}, SsRoots{root}, Bools{sym}, Bools{ss_v4(x, T, ni)});
    return ok ? check_launch("wdf_ss_bwd_gx") : no_kernel("wdf_ss_bwd_gx");
}

// ---- the one-pass MSE step of linear trees (wdf_ss_step.h) -------------------------------------------------------------
static int probe_launch(const wdf_adam_job* jobs, int n_jobs, const int32_t* tape, int n_ops, const double* consts, const float* params,
                        int n_params, const int32_t* outs, int n_out, float* coef, double* coef64, double* jac, void* stream, const char* what)
{
    if (!tape || !consts || !params || !outs || !coef || !coef64 || !jac) return fail(WDF_EINVAL, "null argument");
    if (n_ops < 1 || n_ops > wdf::kProbeMaxOps) return fail(WDF_EUNSUPPORTED, "%s: 1..%d operations (got %d)", what, wdf::kProbeMaxOps, n_ops);
    if (n_params < 1 || n_params > wdf::kProbeMaxParams) return fail(WDF_EUNSUPPORTED, "%s: 1..%d parameters (got %d)", what, wdf::kProbeMaxParams, n_params);
    if (n_out < 1) return fail(WDF_EINVAL, "n_out >= 1");
    if (n_jobs < 0 || n_jobs > WDF_ADAM_MULTI_MAX || (n_jobs > 0 && !jobs)) return fail(WDF_EINVAL, "%s: 0..%d jobs", what, WDF_ADAM_MULTI_MAX);
    wdf::AdamJobs a{};
    for (int i = 0; i < n_jobs; ++i) {
        const wdf_adam_job& j = jobs[i];
        if (!j.theta || !j.grad || !j.m || !j.v || !j.step || !j.lr) return fail(WDF_EINVAL, "job %d: null theta/grad/m/v/step/lr", i);
        if (j.n <= 0 || j.n > 1024) return fail(WDF_EINVAL, "job %d: n must be in 1..1024 (got %d)", i, j.n);
        a.j[i] = wdf::AdamJob{j.theta, j.grad, j.m, j.v, j.step, j.lr, j.lo, j.hi, j.beta1, j.beta2, j.eps, j.n};
    }
    hipLaunchKernelGGL(wdf::ss_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, tape, n_ops, consts, params, n_params, outs,
                       n_out, coef, coef64, jac, a, n_jobs);
    return check_launch(what);
}

int wdf_ss_probe(const int32_t* tape, int n_ops, const double* consts, const float* params, int n_params, const int32_t* outs,
                 int n_out, float* coef, double* coef64, double* jac, void* stream)
{
    return probe_launch(nullptr, 0, tape, n_ops, consts, params, n_params, outs, n_out, coef, coef64, jac, stream, "wdf_ss_probe");
}

// wdf_adam_step_multi(jobs) followed by wdf_ss_probe, in ONE launch: the jobs update (slices of) `params`.
int wdf_ss_probe_adam(const wdf_adam_job* jobs, int n_jobs, const int32_t* tape, int n_ops, const double* consts, const float* params,
                      int n_params, const int32_t* outs, int n_out, float* coef, double* coef64, double* jac, void* stream)
{
    return probe_launch(jobs, n_jobs, tape, n_ops, consts, params, n_params, outs, n_out, coef, coef64, jac, stream, "wdf_ss_probe_adam");
}

}  // extern "C"

// ---- the one-pass step of linear trees, MSE and MSE + ESR (wdf_ss_step.h) -----------------------------------------------
namespace {

// (the trees served, the workspace walk and the MSE step's argument checks: wdf_capi_ss_lin_checks.h, shared with the Gauss-Newton
//  step's translation unit)
// `families` rows of {gradient entries, sum of squares} per wave (1: MSE, 2: MSE + ESR)
size_t lin_step_ws_bytes(int ns, int ni, int64_t B, int64_t T, int n_chunks, int families)
{
    return lin_step_ws_rows(ns, ni, B, T, n_chunks, (size_t)(families * (lin_step_g(ns, ni) + 1)));
}

// Both losses' launches, arguments already checked: pass 1 where there is a state to carry across a chunk boundary, then pass 2
// (the bracketed one) with the loss's own scalars and outputs in `a`.  STORE_Y = false (the _noy exports): y is null and the
// instantiation without the y store runs.
template <int LOSS, bool STORE_Y = true>
int lin_step_launch(const char* what, const float* x, const float* coef, const double* jac, int n_params, int ns, int ni,
                    const float* target, float* y, void* ws, float* gcoef_out, int64_t B, int64_t T, int n_chunks, const float* z0,
                    float* zT, const typename wdf::LinLoss<LOSS>::type& a, hipStream_t s)
{
    const ChunkGeom g = chunk_geom(T, n_chunks, kLinStepUnit);
    const int K = g.K;
    const int64_t L = g.L;
    // the ticket, the chunks' zero-state ends and the waves' partial sums, each on a 256-byte line of its own (by ADDRESS)
    const LinStepWs w = lin_step_ws(ws, ns, ni, B, K);
    unsigned* ticket = w.ticket;
    float* uend0 = w.uend0;
    double* part = w.part;
    // two sequences per lane (8-byte loads and stores) when the rows of x, target, y and the workspace allow it, on every tree
    // and for both losses (no instantiation needs scratch for it: DESIGN.md's table)
    const bool pair = lin_step_pairs(B, x, target, y, ws, z0, zT);
    const int64_t per_wave = pair ? 128 : 64;
    const dim3 grid((unsigned)((B + per_wave - 1) / per_wave), (unsigned)K);
    const bool ok = dispatch([&](auto NS, auto NI, auto PAIR) {
        using V = std::conditional_t<PAIR(), wdf::v2f, float>;
        if (NS() > 0 && K > 1) hipLaunchKernelGGL((wdf::ss_lin_step_zero_kernel<NS(), NI(), V>), grid, dim3(64), 0, s, x, coef, uend0, B, T, L);
        EventBracket bracket(s);
        hipLaunchKernelGGL((wdf::ss_lin_step_kernel<NS(), NI(), V, LOSS, STORE_Y>), grid, dim3(64), 0, s, x, coef, (const float*)uend0, target, y,
                           part, ticket, jac, n_params, gcoef_out, B, T, L, z0, zT, a);
    }, Values<int, 0, 1, 2>{ns}, SsInputs{ni}, Bools{pair});
    return ok ? check_launch(what) : no_kernel(what);
}

// The two losses' argument checks, shared by an export and its _noy twin (STORE_Y = false: there is no y to check or pass).
template <bool STORE_Y>
int lin_step_mse(const char* what, const float* x, const float* coef, const double* jac, int n_params, int ns, int ni, const float* target,
                 float gscale, float* y, void* ws, float* out, float* loss_out, float* gcoef_out, int64_t B, int64_t T, int n_chunks,
                 const float* z0, float* zT, void* stream)
{
    if (int rc = lin_step_mse_check(what, x, coef, jac, n_params, ns, ni, target, STORE_Y, y, ws, out, B, T, n_chunks, z0, zT)) return rc;
    return lin_step_launch<0, STORE_Y>(what, x, coef, jac, n_params, ns, ni, target, y, ws, gcoef_out, B, T, n_chunks, z0, zT,
                                       wdf::LinMse{gscale, out, loss_out}, (hipStream_t)stream);
}

template <bool STORE_Y>
int lin_step_esr(const char* what, const float* x, const float* coef, const double* jac, int n_params, int ns, int ni, const float* target,
                 double n_global, double eps_energy, int64_t skip, float* y, void* ws, float* sums, float* g, float* loss3,
                 float* gcoef_out, int64_t B, int64_t T, int n_chunks, const float* z0, float* zT, void* stream)
{
    if (z0 && z0 == zT) return fail(WDF_EINVAL, "%s: zT must not alias z0 (every chunk reads z0)", what);
    if (!x || !coef || !jac || !target || (STORE_Y && !y) || !ws) return fail(WDF_EINVAL, "%s: null argument", what);
    if (!sums && !g) return fail(WDF_EINVAL, "%s: sums and g are both null (nothing to hand back)", what);
    if (!lin_step_ok(ns, ni)) return fail(WDF_EUNSUPPORTED, "%s: ns in 0..2, ni in 1..2 (got %d, %d)", what, ns, ni);
    if (B <= 0 || T <= 0 || n_chunks < 1 || n_params < 1 || n_params > wdf::kProbeMaxParams)
        return fail(WDF_EINVAL, "%s: B, T, n_chunks >= 1, 1..%d parameters", what, wdf::kProbeMaxParams);
    if (skip < 0 || skip >= T) return fail(WDF_EINVAL, "%s: skip must be in [0, T) (got %lld, T = %lld)", what, (long long)skip, (long long)T);
    if (!(n_global > 0.0) || !(eps_energy >= 0.0)) return fail(WDF_EINVAL, "%s: n_global > 0 and eps_energy >= 0", what);
    return lin_step_launch<1, STORE_Y>(what, x, coef, jac, n_params, ns, ni, target, y, ws, gcoef_out, B, T, n_chunks, z0, zT,
                                       wdf::LinEsr{skip, n_global, eps_energy, sums, g, loss3}, (hipStream_t)stream);
}

}  // namespace

extern "C" {

size_t wdf_ss_lin_step_ws_bytes(int ns, int ni, int64_t B, int64_t T, int n_chunks) { return lin_step_ws_bytes(ns, ni, B, T, n_chunks, 1); }

// x: [T][ni][B] time-major (the resident training set); coef / jac: wdf_ss_probe's outputs; target, y: [T][B].
// ws: wdf_ss_lin_step_ws_bytes() bytes, ZERO before the first call (the step leaves it clean).
// out: float [1 + n_params] = {sum of squared errors, d(gscale/2 x that sum)/d component value}; loss_out: (or NULL) <- gscale/2 x
// that sum; gcoef_out: float
// [ns^2 + ns ni + ns + ni] (dLoss/d{A, Bx, cy, dy}) or NULL.
// z0: float [ns][B] the capacitor states the call starts from, or NULL (zero); zT: float [ns][B] <- the states it ends in, or NULL
// (lpf.py:30-49 never resets C1: epoch n starts from epoch n - 1's final state).  z0 is a constant of the call (no gradient
// flows into the previous call, as in the reference, whose stored state belongs to the previous tape); zT must not alias z0.
int wdf_ss_lin_step_mse(const float* x, const float* coef, const double* jac, int n_params, int ns, int ni, const float* target,
                        float gscale, float* y, void* ws, float* out, float* loss_out, float* gcoef_out, int64_t B, int64_t T, int n_chunks,
                        const float* z0, float* zT, void* stream)
{
    return lin_step_mse<true>("wdf_ss_lin_step_mse", x, coef, jac, n_params, ns, ni, target, gscale, y, ws, out, loss_out, gcoef_out, B, T,
                              n_chunks, z0, zT, stream);
}

// wdf_ss_lin_step_mse without y: the same checks, workspace and results, the output never stored (12 B/sample instead of 16).
int wdf_ss_lin_step_mse_noy(const float* x, const float* coef, const double* jac, int n_params, int ns, int ni, const float* target,
                            float gscale, void* ws, float* out, float* loss_out, float* gcoef_out, int64_t B, int64_t T, int n_chunks,
                            const float* z0, float* zT, void* stream)
{
    return lin_step_mse<false>("wdf_ss_lin_step_mse_noy", x, coef, jac, n_params, ns, ni, target, gscale, nullptr, ws, out, loss_out,
                               gcoef_out, B, T, n_chunks, z0, zT, stream);
}

// The MSE + ESR step: the MSE step's layout with twice the partial sums per wave ({GP, S} and {GQ, E}).
size_t wdf_ss_lin_step_esr_ws_bytes(int ns, int ni, int64_t B, int64_t T, int n_chunks) { return lin_step_ws_bytes(ns, ni, B, T, n_chunks, 2); }

// x, coef, jac, target, y, z0 / zT, chunks as wdf_ss_lin_step_mse.  ws: wdf_ss_lin_step_esr_ws_bytes() bytes, ZERO before the first
// call (the step leaves it clean).  Loss on the rows t >= skip: S/n + sqrt(S / (E + eps_energy) / n), n = n_global.
// sums: float [2 + 2 n_params] = {S, E, gP, gQ} of this call, or NULL; g: float [n_params] (the step finished as a single rank), or
// NULL (then only sums is written); loss3: float [3] or NULL; gcoef_out: float [2 (ns^2 + ns ni + ns + ni)] = {GP, GQ} or NULL.
int wdf_ss_lin_step_esr(const float* x, const float* coef, const double* jac, int n_params, int ns, int ni, const float* target,
                        double n_global, double eps_energy, int64_t skip, float* y, void* ws, float* sums, float* g, float* loss3,
                        float* gcoef_out, int64_t B, int64_t T, int n_chunks, const float* z0, float* zT, void* stream)
{
    return lin_step_esr<true>("wdf_ss_lin_step_esr", x, coef, jac, n_params, ns, ni, target, n_global, eps_energy, skip, y, ws, sums, g,
                              loss3, gcoef_out, B, T, n_chunks, z0, zT, stream);
}

// wdf_ss_lin_step_esr without y (wdf_ss_lin_esr_finish serves both).
int wdf_ss_lin_step_esr_noy(const float* x, const float* coef, const double* jac, int n_params, int ns, int ni, const float* target,
                            double n_global, double eps_energy, int64_t skip, void* ws, float* sums, float* g, float* loss3,
                            float* gcoef_out, int64_t B, int64_t T, int n_chunks, const float* z0, float* zT, void* stream)
{
    return lin_step_esr<false>("wdf_ss_lin_step_esr_noy", x, coef, jac, n_params, ns, ni, target, n_global, eps_energy, skip, nullptr, ws,
                               sums, g, loss3, gcoef_out, B, T, n_chunks, z0, zT, stream);
}

// sums: {S, E, gP[n_params], gQ[n_params]} summed over the ranks -> g [n_params] and (optional) loss3, one small launch.
int wdf_ss_lin_esr_finish(const float* sums, int n_params, double n_global, double eps_energy, float* g, float* loss3, void* stream)
{
    if (!sums || !g) return fail(WDF_EINVAL, "wdf_ss_lin_esr_finish: null sums/g");
    if (n_params < 1 || n_params > wdf::kProbeMaxParams) return fail(WDF_EINVAL, "wdf_ss_lin_esr_finish: 1..%d parameters", wdf::kProbeMaxParams);
    if (!(n_global > 0.0) || !(eps_energy >= 0.0)) return fail(WDF_EINVAL, "wdf_ss_lin_esr_finish: n_global > 0 and eps_energy >= 0");
    hipLaunchKernelGGL(wdf::esr_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, n_params, n_global, eps_energy, g, loss3);
    return check_launch("wdf_ss_lin_esr_finish");
}

}  // extern "C"
