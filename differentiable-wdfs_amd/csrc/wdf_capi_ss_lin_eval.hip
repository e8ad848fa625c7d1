// wdf_capi_ss_lin_eval.hip -- C ABI of the loss-only evaluation pass of linear state-space trees (csrc/wdf_ss_lin_eval.h):
// workspace layout, argument checking, template dispatch and the two launches of a call.  A translation unit of its own: it
// compiles beside the training step's, whose code objects it leaves alone.
#include "wdf_capi_common.h"
#include "wdf_ss_lin_eval.h"
using namespace wdfcapi;

namespace {

constexpr int kUnit = 32;                    // chunk lengths: multiples of 32 steps, the step's rule (wdf_capi_ss.hip)

struct EvWs {
    unsigned* ticket;
    float* zend0;
    double* part;
    size_t total;
    int K;
    int64_t L;
};

// the one walk of the workspace: counts with ws = null (wdf_ss_lin_eval_ws_bytes), carves otherwise.  The ticket, the chunks'
// zero-state ends and the waves' partial sums, each on a 256-byte line of its own (sized for one sequence per lane: a call that
// pairs them up uses half the waves)
EvWs ev_ws(void* ws, int ns, int64_t B, int64_t T, int n_chunks)
{
    EvWs w{};
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    w.L = g.L;
    w.K = g.K;
    Carver c(ws);
    w.ticket = c.take<unsigned>(1);
    c.align(256);
    w.zend0 = c.take<float>((size_t)w.K * (size_t)ns * (size_t)B);
    c.align(256);
    w.part = c.take<double>(waves64(B) * (size_t)w.K * 2);
    c.align(256);
    w.total = c.off;
    return w;
}

int ev_check_shape(const char* who, int ns, int ni, int64_t B, int64_t T, int n_chunks)
{
    if (ns < 0 || ns > 2 || ni < 1 || ni > 2) return fail(WDF_EINVAL, "%s: ns in 0..2, ni in 1..2 (got %d, %d)", who, ns, ni);
    if (B <= 0 || T <= 0 || n_chunks < 1) return fail(WDF_EINVAL, "%s: B, T, n_chunks >= 1", who);
    return WDF_OK;
}

}  // namespace

extern "C" {

size_t wdf_ss_lin_eval_ws_bytes(int ns, int ni, int64_t B, int64_t T, int n_chunks)
{
    if (ev_check_shape("wdf_ss_lin_eval_ws_bytes", ns, ni, B, T, n_chunks)) return 0;
    return ev_ws(nullptr, ns, B, T, n_chunks).total;
}

int wdf_ss_lin_eval(const float* x, const float* coef, int ns, int ni, const float* target, int64_t skip, double n_global,
                    double eps_energy, float gscale, float* y, void* ws, double* sums, float* loss3, float* loss_out, int64_t B,
                    int64_t T, int n_chunks, const float* z0, float* zT, void* stream)
{
    const char* who = "wdf_ss_lin_eval";
    // every refusal before any HIP call
    if (!x || !coef || !target || !ws) return fail(WDF_EINVAL, "%s: null x/coef/target/ws", who);
    if (!sums && !loss3 && !loss_out) return fail(WDF_EINVAL, "%s: sums, loss3 and loss_out are all null (nothing to hand back)", who);
    if (int rc = ev_check_shape(who, ns, ni, B, T, n_chunks)) return rc;
    if (skip < 0 || skip >= T) return fail(WDF_EINVAL, "%s: skip must be in [0, T) (got %lld, T = %lld)", who, (long long)skip, (long long)T);
    if (!(n_global > 0.0)) return fail(WDF_EINVAL, "%s: n_global must be positive", who);
    if (!(eps_energy >= 0.0)) return fail(WDF_EINVAL, "%s: eps_energy must not be negative", who);
    if (z0 && z0 == zT) return fail(WDF_EINVAL, "%s: zT must not alias z0 (every chunk reads z0)", who);
    const EvWs l = ev_ws(ws, ns, B, T, n_chunks);
    // two sequences per lane (8-byte loads and stores) when the rows of x, target, y, the states and the workspace allow it
    const bool pair = (B % 2 == 0) && aligned8(x) && aligned8(target) && aligned8(y) && aligned8(ws) && aligned8(z0) && aligned8(zT);
    const int64_t per_wave = pair ? 128 : 64;
    const dim3 grid((unsigned)((B + per_wave - 1) / per_wave), (unsigned)l.K);
    const wdf::LinEval a{skip, n_global, eps_energy, gscale, sums, loss3, loss_out};
    hipStream_t s = (hipStream_t)stream;
    const bool ok = dispatch([&](auto NS, auto NI, auto PAIR, auto STORE_Y) {
        using V = std::conditional_t<PAIR(), wdf::v2f, float>;
        if constexpr (NS() > 0) {
            if (l.K > 1) hipLaunchKernelGGL((wdf::ss_lin_eval_zero_kernel<NS(), NI(), V>), grid, dim3(64), 0, s, x, coef, l.zend0, B, T, l.L);
        }
        EventBracket bracket(s);
        hipLaunchKernelGGL((wdf::ss_lin_eval_kernel<NS(), NI(), V, STORE_Y()>), grid, dim3(64), 0, s, x, coef, (const float*)l.zend0, target, y,
                           l.part, l.ticket, B, T, l.L, z0, zT, a);
    }, Values<int, 0, 1, 2>{ns}, Values<int, 1, 2>{ni}, Bools{pair}, Bools{y != nullptr});
    return ok ? check_launch(who) : no_kernel(who);
}

}  // extern "C"
