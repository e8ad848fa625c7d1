// wdf_capi_ss_nl_eval.hip -- C ABI of the loss-only evaluation pass of small state-space trees with a diode-pair root
// (csrc/wdf_ss_nl_eval.h): workspace layout, plan, argument checking, template dispatch and the two launches of a call.
// A translation unit of its own: it compiles beside the training step's.
#include "wdf_capi_common.h"
#include "wdf_ss_nl_eval.h"
using namespace wdfcapi;

namespace {

bool ev_ok(int ns, int ni) { return ns >= 1 && ns <= 2 && ni >= 1 && ni <= 2; }
int ev_kn(int ns, int ni) { return ns * ns + ns * ni + ns + ns + ni + ns + ni + 1; }

constexpr int kUnit = 32;                    // chunk lengths: multiples of 32 steps (wdf_ss_nl_step_chunk_len)
constexpr size_t kCtlBytes = 512;            // control block at 0, ticket and ring state at 128, the two coefficient vectors at 256
constexpr int kSecantField = 12;             // wdf_ss_nl_eval_set: the secant switch, behind the step's fields 2..11

struct EvWs {
    wdf::NlStepCtl* ctl;
    wdf::NlEvalAux* aux;
    float *coef_prev, *zwarm, *zend, *snap;
    double *gpart, *part;
    size_t total;
    int K;
    int64_t L, n_snap;
};

// the one walk of the workspace: counts with ws = null (wdf_ss_nl_eval_ws_bytes), carves otherwise
// (sized for one sequence per lane: a call that pairs them up uses half the groups)
EvWs ev_ws(void* ws, int ns, int ni, int64_t B, int64_t T, int n_chunks)
{
    EvWs w{};
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    w.L = g.L;
    w.K = g.K;
    w.n_snap = (T + wdf::kNlEvalSnap - 1) / wdf::kNlEvalSnap;
    const size_t groups_max = waves64(B);
    Carver c(ws);
    w.ctl = c.take<wdf::NlStepCtl>(1);
    c.align(128);
    w.aux = c.take<wdf::NlEvalAux>(1);
    c.align(256);
    w.coef_prev = c.take<float>(2 * ((size_t)ev_kn(ns, ni) + 2));
    c.align(kCtlBytes);
    w.zwarm = c.take<float>((size_t)w.K * ns * (size_t)B);
    c.align(256);
    w.zend = c.take<float>((size_t)w.K * ns * (size_t)B);
    c.align(256);
    w.snap = c.take<float>((size_t)wdf::kNlEvalRing * w.n_snap * ns * (size_t)B);
    c.align(256);
    w.gpart = c.take<double>((size_t)w.K * groups_max * 2);
    c.align(256);
    w.part = c.take<double>(groups_max * 4);
    c.align(256);
    w.total = c.off;
    return w;
}

// B, T and a chunk count that tiles T: (K - 1) L < T <= K L with L = wdf_ss_nl_step_chunk_len(T, K)
int ev_check_shape(const char* who, int ns, int ni, int64_t B, int64_t T, int n_chunks)
{
    if (!ev_ok(ns, ni)) return fail(WDF_EINVAL, "%s: ns in 1..2, ni in 1..2 (got %d, %d)", who, ns, ni);
    if (B <= 0 || T <= 0 || n_chunks < 1) return fail(WDF_EINVAL, "%s: B, T, n_chunks >= 1", who);
    return check_tiles(chunk_geom(T, n_chunks, kUnit), n_chunks, T, kUnit, nullptr);
}

__global__ void ev_plan_kernel(wdf::NlStepCtl* ctl, wdf::NlEvalAux* aux, int cold, int warm, int w_min, int w_max, float tol)
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
    *aux = wdf::NlEvalAux{0u, 0, 0, 1};
}

__global__ void ev_set_kernel(wdf::NlStepCtl* ctl, wdf::NlEvalAux* aux, int field, double v)
{
    switch (field) {
    case 2: ctl->have_snap = (int)v; break;
    case 3: ctl->w_cur = (int)v; break;
    case 4: ctl->w_snap = (int)v; break;
    case 5: ctl->w_min = (int)v; break;
    case 6: ctl->w_max = (int)v; break;
    case 7: ctl->cool = (int)v; break;
    case 8: ctl->tol = (float)v; break;
    case 9: ctl->grow_at = (float)v; break;
    case 10: ctl->shrink_at = (float)v; break;
    case 11: ctl->cool_miss = (int)v; break;
    case kSecantField: aux->secant = v != 0.0 ? 1 : 0; break;
    default: break;
    }
}

}  // namespace

extern "C" {

size_t wdf_ss_nl_eval_ws_bytes(int ns, int ni, int64_t B, int64_t T, int n_chunks)
{
    if (ev_check_shape("wdf_ss_nl_eval_ws_bytes", ns, ni, B, T, n_chunks)) return 0;
    return ev_ws(nullptr, ns, ni, B, T, n_chunks).total;
}

// cold_warmup: the warm-up of the first call (chunks start from z = 0); warm_warmup: the second call's, from the first one's
// snapshots; afterwards the device steers it inside [w_min, min(w_max, chunk length)] in multiples of 16.
int wdf_ss_nl_eval_plan(void* ws, int ns, int ni, int64_t B, int64_t T, int n_chunks, int cold_warmup, int warm_warmup, int w_min,
                        int w_max, float tol, void* stream)
{
    const char* who = "wdf_ss_nl_eval_plan";
    if (!ws) return fail(WDF_EINVAL, "%s: null ws", who);
    if (int rc = ev_check_shape(who, ns, ni, B, T, n_chunks)) return rc;
    const EvWs l = ev_ws(ws, ns, ni, B, T, n_chunks);
    if (cold_warmup < 0 || cold_warmup % 8 || warm_warmup < 16 || warm_warmup % 16 || w_min < 16 || w_min % 16 || w_max < w_min ||
        w_max % 16 || warm_warmup > l.L || !(tol > 0.0f))
        return fail(WDF_EINVAL, "%s: cold_warmup a multiple of 8, the others of 16, 16 <= w_min <= w_max, warm_warmup <= the chunk length %lld, tol > 0",
                    who, (long long)l.L);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = memset_async(ws, 0, kCtlBytes, s)) return rc;
    hipLaunchKernelGGL(ev_plan_kernel, dim3(1), dim3(1), 0, s, l.ctl, l.aux, cold_warmup, warm_warmup, w_min, w_max, tol);
    return check_launch(who);
}

int wdf_ss_nl_eval_set(void* ws, int field, double value, void* stream)
{
    if (!ws) return fail(WDF_EINVAL, "wdf_ss_nl_eval_set: null ws");
    if (field < 2 || field > kSecantField) return fail(WDF_EINVAL, "wdf_ss_nl_eval_set: field 2..11 (the step's), or 12 (the secant switch)");
    Carver c(ws);
    wdf::NlStepCtl* ctl = c.take<wdf::NlStepCtl>(1);
    c.align(128);
    hipLaunchKernelGGL(ev_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, ctl, c.take<wdf::NlEvalAux>(1), field, value);
    return check_launch("wdf_ss_nl_eval_set");
}

// ctl_out: 32 words (NlStepCtl, csrc/wdf_ss_nl_step.h).  Synchronises the stream.
int wdf_ss_nl_eval_read(const void* ws, int32_t* ctl_out, void* stream)
{
    if (!ws || !ctl_out) return fail(WDF_EINVAL, "wdf_ss_nl_eval_read: null argument");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(ctl_out, ws, sizeof(wdf::NlStepCtl), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(WDF_ELAUNCH, "wdf_ss_nl_eval_read: copy failed");
    return WDF_OK;
}

int wdf_ss_nl_eval(const float* x, const float* coef, const float* params, int n_tree, int ns, int ni, int n_up, int n_down,
                   const float* target, int64_t skip, double n_global, double eps, float* y, void* ws, double* sums, float* loss3,
                   int64_t B, int64_t T, int n_chunks, void* stream)
{
    const char* who = "wdf_ss_nl_eval";
    // every refusal before any HIP call
    if (!x || !coef || !params || !target || !ws || !sums) return fail(WDF_EINVAL, "%s: null x/coef/params/target/ws/sums", who);
    if (int rc = ev_check_shape(who, ns, ni, B, T, n_chunks)) return rc;
    if (skip < 0 || skip >= T) return fail(WDF_EINVAL, "%s: skip must be in 0..T-1 (got %lld, T = %lld)", who, (long long)skip, (long long)T);
    if (!(n_global > 0.0)) return fail(WDF_EINVAL, "%s: n_global must be positive", who);
    if (!(eps >= 0.0)) return fail(WDF_EINVAL, "%s: eps must not be negative", who);
    if (n_tree < 1 || n_tree > wdf::kProbeMaxParams || n_up < 1 || n_down < 1)
        return fail(WDF_EINVAL, "%s: n_up, n_down >= 1, 1..%d component values", who, wdf::kProbeMaxParams);
    const EvWs l = ev_ws(ws, ns, ni, B, T, n_chunks);
    const bool pair = (B % 2 == 0) && aligned8(x) && aligned8(target) && (!y || aligned8(y)) && aligned8(ws);
    const bool sym = n_up == n_down;
    wdf::NlEvalArgs a{};
    a.x = x; a.coef = coef; a.pIs = params + n_tree; a.pV = params + n_tree + 1; a.pRp = coef + ev_kn(ns, ni);
    a.target = target; a.y = y;
    a.ctl = l.ctl; a.aux = l.aux; a.coef_prev = l.coef_prev;
    a.zwarm = l.zwarm; a.zend = l.zend; a.snap = l.snap; a.gpart = l.gpart; a.part = l.part;
    a.sums = sums; a.loss3 = loss3; a.n_global = n_global; a.eps = eps;
    a.B = B; a.T = T; a.L = l.L; a.skip = skip; a.n_snap = l.n_snap;
    a.K = l.K;
    a.groups = (int)((B + (pair ? 127 : 63)) / (pair ? 128 : 64));
    a.n_up = n_up; a.n_down = n_down;
    const int64_t units = (int64_t)a.groups * a.K;
    const dim3 grid((unsigned)((units + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    const bool ok = dispatch([&](auto NS, auto NI, auto SYM, auto PAIR, auto STORE_Y) {
        using V = std::conditional_t<PAIR(), wdf::v2f, float>;
        constexpr int WD = PAIR() ? 2 : 1;
        {
            EventBracket bracket(s);
            hipLaunchKernelGGL((wdf::ss_nl_eval_kernel<NS(), NI(), SYM(), V, STORE_Y()>), grid, dim3(256), 0, s, a);
        }
        hipLaunchKernelGGL((wdf::ss_nl_eval_finish_kernel<NS(), NI(), SYM(), WD, STORE_Y()>), dim3(a.groups), dim3(64), 0, s, a);
    }, Values<int, 1, 2>{ns}, Values<int, 1, 2>{ni}, Bools{sym}, Bools{pair}, Bools{y != nullptr});
    return ok ? check_launch(who) : no_kernel(who);
}

}  // extern "C"
