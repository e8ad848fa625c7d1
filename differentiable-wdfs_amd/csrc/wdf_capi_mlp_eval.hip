// wdf_capi_mlp_eval.hip -- C ABI of the MLP-root pot clipper's loss-only evaluation pass (csrc/wdf_mlp_eval.h): argument
// checking, template dispatch and the four launches of wdf_clipper_mlp_eval (three of the step's forward kernel under the pass's
// tag, MlpEvalPass<STORE_Y>, then the finish).  The state block is the training step's
// (wdf_capi_mlp_step_layout.h: one layout walk for both).  A translation unit of its own: it compiles beside the step's.
#include "wdf_capi_mlp_step_layout.h"
#include "wdf_mlp_eval.h"
using namespace wdfcapi;

namespace {

template <int NL, bool DYN_R, int ACT, bool STORE_Y>
void launch_mlp_eval(const wdf::MlpStepArgs& A, int n_items, int n_cols, double n_global, double eps_energy, double* sums, float* loss3,
                     hipStream_t s)
{
    const dim3 items((unsigned)((n_items + 3) / 4)), cols((unsigned)((n_cols + 3) / 4));
    {
        EventBracket bracket(s);
        hipLaunchKernelGGL((wdf::mlp_step_fwd_kernel<NL, DYN_R, ACT, 0, wdf::MlpEvalPass<STORE_Y>>), items, dim3(256), 0, s, A);
    }
    hipLaunchKernelGGL((wdf::mlp_step_fwd_kernel<NL, DYN_R, ACT, 1, wdf::MlpEvalPass<STORE_Y>>), items, dim3(256), 0, s, A);
    hipLaunchKernelGGL((wdf::mlp_step_fwd_kernel<NL, DYN_R, ACT, 2, wdf::MlpEvalPass<STORE_Y>>), cols, dim3(256), 0, s, A);
    hipLaunchKernelGGL(wdf::mlp_eval_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)A.colsum, n_cols, n_global, eps_energy, sums,
                       loss3, A.ctl);
}

}  // namespace

extern "C" {

// One evaluation call on the resident set: the forward in verified chunks, the two repair launches, the finish.  The state
// is the step's (wdf_clipper_mlp_step_state_bytes / _plan with wgrad_chunks = 1); its block maps and weight-gradient
// partials are not touched.  y NULL: no y store.
int wdf_clipper_mlp_eval(const float* x, const float* p, const float* lr, const float* theta2, const float* w, int hidden, int n_layers,
                         int activation, float fs, const float* target, int64_t skip, double n_global, double eps_energy, float* y,
                         void* state, int64_t B, int64_t T, int n_items, double* sums, float* loss3, void* stream)
{
    const char* what = "wdf_clipper_mlp_eval";
    // every refusal before any HIP call
    if (!x || !w || !target || !state || !sums) return fail(WDF_EINVAL, "%s: null x/w/target/state/sums", what);
    if ((p == nullptr) != (lr == nullptr)) return fail(WDF_EINVAL, "%s: p and lr go together", what);
    if (!p && !theta2) return fail(WDF_EINVAL, "%s: static R needs theta2", what);
    if (!(fs > 0.0f)) return fail(WDF_EINVAL, "%s: fs must be positive", what);
    if (skip < 0) return fail(WDF_EINVAL, "%s: skip must not be negative", what);
    if (!(n_global > 0.0)) return fail(WDF_EINVAL, "%s: n_global must be positive", what);
    if (!(eps_energy >= 0.0)) return fail(WDF_EINVAL, "%s: eps_energy must not be negative", what);
    if (!aligned16(x) || (p && (!aligned16(p) || !aligned16(lr)))) return fail(WDF_EINVAL, "%s: x, p, lr must be 16-byte aligned", what);
    if (step_check_shape(hidden, n_layers, activation, B, T, n_items, 1)) return WDF_EINVAL;      // (its message stands)
    const StepLayout L = step_layout(hidden, n_layers, B, T, n_items, 1);
    wdf::MlpStepArgs A = step_state_args(state, L, hidden, B, T, skip, n_items, fs);
    A.x = x; A.p = p; A.lr = lr; A.theta2 = theta2; A.w = w; A.target = target;
    A.y = y;
    A.zstash = nullptr; A.kappa = nullptr; A.maps = nullptr;    // the pass has no reverse sweep to feed
    hipStream_t s = (hipStream_t)stream;
    const bool ok = dispatch([&](auto NL, auto DYN, auto ACT, auto STORE_Y) {
        launch_mlp_eval<NL(), DYN(), ACT(), STORE_Y()>(A, n_items, L.n_cols, n_global, eps_energy, sums, loss3, s);
    }, Values<int, 3, 4, 5>{n_layers}, Bools{p != nullptr}, Values<int, 0, 1>{activation}, Bools{y != nullptr});
    return ok ? check_launch(what) : no_kernel(what);
}

}  // extern "C"
