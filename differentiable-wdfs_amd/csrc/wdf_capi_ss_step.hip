// wdf_capi_ss_step.hip -- C ABI of the one-pass MSE and MSE + ESR steps of small state-space trees with a diode-pair root
// (csrc/wdf_ss_nl_step.h): workspace layout, plan, template dispatch and the two launches of a step.
#include "wdf_capi_common.h"
#include "wdf_ss_nl_step.h"
using namespace wdfcapi;

namespace {

bool nl_ok(int ns, int ni) { return ns >= 1 && ns <= 2 && ni >= 1 && ni <= 2; }
int nl_kn(int ns, int ni) { return ns * ns + ns * ni + ns + ns + ni + ns + ni + 1; }
int nl_nt(int ns, int ni) { return ns * ns + ns * ni + ns + ns + ni + 2; }
// (the MSE + ESR step's record and sums, the larger of the two: ONE layout serves both losses, so a workspace planned once
//  can go to either entry point)
int nl_nrec(int ns, int ni) { return 2 * ns + ns * ns + nl_nt(ns, ni) * ns + 2 * ns; }
int nl_nsnap(int ns, int ni) { return ns + nl_nt(ns, ni) * ns + ns * ns; }
int nl_nacc(int ns, int ni) { return 2 * (nl_kn(ns, ni) + 2) + 2; }

constexpr int kUnit = 32;                    // chunk lengths: multiples of 32 steps
constexpr size_t kCtlBytes = 512;            // control block at 0, ticket at 128, coef_prev at 256: what the plan zeroes

struct NlWs {
    wdf::NlStepCtl* ctl;
    unsigned* ticket;
    float *coef_prev, *rec, *snap;
    double *gpart, *part;
    size_t total;
    int K;
    int64_t L;
};

// the one walk of the workspace: counts with ws = null (wdf_ss_nl_step_ws_bytes, wdf_ss_nl_step_esr_ws_bytes), carves otherwise
// (sized for one sequence per lane: a call that pairs them up uses half the groups)
NlWs nl_ws(void* ws, int ns, int ni, int64_t B, int64_t T, int n_chunks)
{
    NlWs w{};
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    w.L = g.L;
    w.K = g.K;
    const size_t groups_max = waves64(B);
    Carver c(ws);
    w.ctl = c.take<wdf::NlStepCtl>(1);
    c.align(128);
    w.ticket = c.take<unsigned>(1);
    c.align(256);
    w.coef_prev = c.take<float>((size_t)nl_kn(ns, ni) + 2);
    c.align(kCtlBytes);
    w.rec = c.take<float>((size_t)w.K * nl_nrec(ns, ni) * (size_t)B);
    c.align(256);
    w.snap = c.take<float>((size_t)2 * w.K * nl_nsnap(ns, ni) * (size_t)B);
    c.align(256);
    w.gpart = c.take<double>((size_t)w.K * groups_max * nl_nacc(ns, ni));
    c.align(256);
    w.part = c.take<double>(groups_max * ((size_t)nl_nacc(ns, ni) + 2));          // (+ bad boundaries, largest miss)
    c.align(256);
    w.total = c.off;
    return w;
}

__global__ void nl_plan_kernel(wdf::NlStepCtl* ctl, unsigned* ticket, int cold, int warm, int w_min, int w_max, float tol)
{
    wdf::NlStepCtl c = {};
    c.w_cur = cold;
    c.w_snap = warm;
    c.w_min = w_min;
    c.w_max = w_max;
    c.tol = tol;
    c.grow_at = 0.5f;
    c.shrink_at = 0.125f;
    c.cool_miss = 32;
    *ctl = c;
    *ticket = 0u;
}

__global__ void nl_set_kernel(wdf::NlStepCtl* ctl, int field, double v)
{
    switch (field) {
    case 3: ctl->w_cur = (int)v; break;
    case 4: ctl->w_snap = (int)v; break;
    case 5: ctl->w_min = (int)v; break;
    case 6: ctl->w_max = (int)v; break;
    case 7: ctl->cool = (int)v; break;
    case 8: ctl->tol = (float)v; break;
    case 9: ctl->grow_at = (float)v; break;
    case 10: ctl->shrink_at = (float)v; break;
    case 11: ctl->cool_miss = (int)v; break;
    case 2: ctl->have_snap = (int)v; break;
    default: break;
    }
}

// the two launches of a step.  LOSS = 0: MSE (gscale, loss <- one float); LOSS = 1: MSE + ESR (skip, eps, loss <- three)
template <int LOSS>
int nl_step_launch(const char* who, const float* x, const float* coef, const float* params, const double* jac, int n_tree, int ns, int ni,
                   int n_up, int n_down, const float* target, float gscale, int64_t skip, double eps, float* y, void* ws, float* out,
                   float* loss, int64_t B, int64_t T, int n_chunks, void* stream)
{
    if (!x || !coef || !params || !jac || !target || !y || !ws || !out) return fail(WDF_EINVAL, "null argument");
    if (!nl_ok(ns, ni)) return fail(WDF_EUNSUPPORTED, "%s: ns in 1..2, ni in 1..2 (got %d, %d)", who, ns, ni);
    if (B <= 0 || T <= 0 || n_chunks < 1 || n_tree < 1 || n_tree > wdf::kProbeMaxParams || n_up < 1 || n_down < 1)
        return fail(WDF_EINVAL, "B, T, n_chunks, n_up, n_down >= 1, 1..7 component values");
    const NlWs l = nl_ws(ws, ns, ni, B, T, n_chunks);
    const bool pair = (B % 2 == 0) && aligned8(x) && aligned8(target) && aligned8(y) && aligned8(ws) && (LOSS == 0 || ns * ni == 1);
    const bool sym = n_up == n_down;
    typename wdf::NlArgs<LOSS>::type a{};
    a.x = x; a.coef = coef; a.pIs = params + n_tree; a.pV = params + n_tree + 1; a.pRp = coef + nl_kn(ns, ni);
    a.target = target; a.y = y;
    a.ctl = l.ctl;
    a.ticket = l.ticket;
    a.coef_prev = l.coef_prev;
    a.rec = l.rec;
    a.snap = l.snap;
    a.gpart = l.gpart;
    a.part = l.part;
    a.jac = jac; a.out = out;
    if constexpr (LOSS != 0) { a.loss3 = loss; a.skip = skip; a.eps = eps; }
    else a.loss = loss;
    a.B = B; a.T = T; a.L = l.L; a.K = l.K;
    a.groups = (int)((B + (pair ? 127 : 63)) / (pair ? 128 : 64));
    a.n_tree = n_tree; a.n_up = n_up; a.n_down = n_down; a.gscale = gscale;
    const int64_t units = (int64_t)a.groups * a.K;
    const dim3 grid((unsigned)((units + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    const bool ok = dispatch([&](auto NS, auto NI, auto SYM, auto PAIR) {
        if constexpr ((PAIR() && !wdf::NlPairs<NS(), NI(), LOSS>::ok) || !wdf::NlBuilt<NS(), NI(), LOSS>::ok) return false;
        else {
        using V = std::conditional_t<PAIR(), wdf::v2f, float>;
        constexpr int WD = PAIR() ? 2 : 1;
        {
            EventBracket bracket(s);
            hipLaunchKernelGGL((wdf::ss_nl_step_kernel<NS(), NI(), SYM(), V, LOSS>), grid, dim3(256), 0, s, a);
        }
        hipLaunchKernelGGL((wdf::ss_nl_step_finish_kernel<NS(), NI(), SYM(), WD, LOSS>), dim3(a.groups),
                           dim3(64 * WD * wdf::NlTile<NS(), WD, LOSS>::n), 0, s, a);
        return true;
        }
    }, Values<int, 1, 2>{ns}, Values<int, 1, 2>{ni}, Bools{sym}, Bools{pair});
    if (!ok) return no_kernel(who);
    return check_launch(who);
}

}  // namespace

extern "C" {

size_t wdf_ss_nl_step_ws_bytes(int ns, int ni, int64_t B, int64_t T, int n_chunks)
{
    if (!nl_ok(ns, ni)) { fail(WDF_EUNSUPPORTED, "wdf_ss_nl_step: ns in 1..2, ni in 1..2 (got %d, %d)", ns, ni); return 0; }
    if (B <= 0 || T <= 0 || n_chunks < 1) { fail(WDF_EINVAL, "B, T, n_chunks >= 1"); return 0; }
    return nl_ws(nullptr, ns, ni, B, T, n_chunks).total;
}

static bool esr_ok(int ns, int ni, const char* who)
{
    if (nl_ok(ns, ni) && ns * ni == 4) {
        fail(WDF_EUNSUPPORTED, "%s: the MSE + ESR step is built for ns * ni <= 2 (got ns = %d, ni = %d)", who, ns, ni);
        return false;
    }
    return true;
}

// (the same walk: the two steps share one layout, wdf_ss_nl_step_plan and the control block)
size_t wdf_ss_nl_step_esr_ws_bytes(int ns, int ni, int64_t B, int64_t T, int n_chunks)
{
    if (!esr_ok(ns, ni, "wdf_ss_nl_step_esr_ws_bytes")) return 0;
    return wdf_ss_nl_step_ws_bytes(ns, ni, B, T, n_chunks);
}

int wdf_ss_nl_step_chunk_len(int64_t T, int n_chunks)
{
    return (T > 0 && n_chunks >= 1) ? (int)chunk_geom(T, n_chunks, kUnit).L : 0;
}

// cold_warmup: the warm-up of the first call (chunks start from z = 0); warm_warmup: where that call takes the snapshots the
// second one starts from; afterwards the device steers it inside [w_min, min(w_max, chunk length)].  All multiples of 8.
int wdf_ss_nl_step_plan(void* ws, int ns, int ni, int64_t B, int64_t T, int n_chunks, int cold_warmup, int warm_warmup, int w_min,
                        int w_max, float tol, void* stream)
{
    if (!ws) return fail(WDF_EINVAL, "null argument");
    if (!nl_ok(ns, ni)) return fail(WDF_EUNSUPPORTED, "wdf_ss_nl_step_plan: ns in 1..2, ni in 1..2 (got %d, %d)", ns, ni);
    if (B <= 0 || T <= 0 || n_chunks < 1) return fail(WDF_EINVAL, "B, T, n_chunks >= 1");
    const NlWs l = nl_ws(ws, ns, ni, B, T, n_chunks);
    if (cold_warmup < 0 || cold_warmup % 8 || warm_warmup < 8 || warm_warmup % 8 || w_min < 8 || w_min % 8 || w_max < w_min ||
        w_max % 8 || warm_warmup > l.L || !(tol > 0.0f))
        return fail(WDF_EINVAL, "wdf_ss_nl_step_plan: warm-ups are multiples of 8, 8 <= w_min <= w_max, warm_warmup <= the chunk length %lld, tol > 0",
                    (long long)l.L);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = memset_async(ws, 0, kCtlBytes, s)) return rc;
    hipLaunchKernelGGL(nl_plan_kernel, dim3(1), dim3(1), 0, s, l.ctl, l.ticket, cold_warmup,
                       warm_warmup, w_min, w_max, tol);
    return check_launch("wdf_ss_nl_step_plan");
}

int wdf_ss_nl_step_set(void* ws, int field, double value, void* stream)
{
    if (!ws) return fail(WDF_EINVAL, "null argument");
    if (field < 2 || field > 11) return fail(WDF_EINVAL, "wdf_ss_nl_step_set: field 2..11");
    hipLaunchKernelGGL(nl_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (wdf::NlStepCtl*)ws, field, value);
    return check_launch("wdf_ss_nl_step_set");
}

// ctl_out: 32 words (NlStepCtl, csrc/wdf_ss_nl_step.h).  Synchronises the stream.
int wdf_ss_nl_step_read(const void* ws, int32_t* ctl_out, void* stream)
{
    if (!ws || !ctl_out) return fail(WDF_EINVAL, "null argument");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(ctl_out, ws, sizeof(wdf::NlStepCtl), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(WDF_ELAUNCH, "wdf_ss_nl_step_read: copy failed");
    return WDF_OK;
}

// x: [T][ni][B] time-major; coef: the probe's outputs (SSCoef order, then the port resistance the root sees); params: the
// component values on the device, the root's Is and nVt at [n_tree], [n_tree + 1]; jac: double [ncoef + 1][n_tree];
// target, y: [T][B]; ws: planned by wdf_ss_nl_step_plan.
// out: float [1 + n_tree + 2] = {sum of squared errors, d(gscale / 2 x that sum) / d{component values, Is, nVt}}; loss_out (or NULL)
// <- gscale / 2 x that sum.
int wdf_ss_nl_step_mse(const float* x, const float* coef, const float* params, const double* jac, int n_tree, int ns, int ni, int n_up,
                       int n_down, const float* target, float gscale, float* y, void* ws, float* out, float* loss_out, int64_t B, int64_t T,
                       int n_chunks, void* stream)
{
    return nl_step_launch<0>("wdf_ss_nl_step_mse", x, coef, params, jac, n_tree, ns, ni, n_up, n_down, target, gscale, 0, 0.0, y, ws, out,
                             loss_out, B, T, n_chunks, stream);
}

// The same pass with the loss of clipper_pot.py:141-177 on the rows t >= skip: out = {S = sum of squared errors past skip,
// d(mse + esr) / d{component values, Is, nVt}}, loss3_out = {mse, esr, mse + esr}, mse = S / n, esr = sqrt(S / (E + eps) / n),
// E = sum of y^2 past skip, n = B (T - skip).
int wdf_ss_nl_step_esr(const float* x, const float* coef, const float* params, const double* jac, int n_tree, int ns, int ni, int n_up,
                       int n_down, const float* target, int64_t skip, double eps, float* y, void* ws, float* out, float* loss3_out, int64_t B,
                       int64_t T, int n_chunks, void* stream)
{
    if (!loss3_out) return fail(WDF_EINVAL, "null argument");
    if (!esr_ok(ns, ni, "wdf_ss_nl_step_esr")) return WDF_EUNSUPPORTED;
    if (T > 0 && (skip < 0 || skip >= T)) return fail(WDF_EINVAL, "wdf_ss_nl_step_esr: skip must be in 0..T-1 (got %lld, T = %lld)", (long long)skip, (long long)T);
    if (!(eps >= 0.0)) return fail(WDF_EINVAL, "wdf_ss_nl_step_esr: eps >= 0");
    return nl_step_launch<1>("wdf_ss_nl_step_esr", x, coef, params, jac, n_tree, ns, ni, n_up, n_down, target, 0.0f, skip, eps, y, ws, out,
                             loss3_out, B, T, n_chunks, stream);
}

}  // extern "C"
