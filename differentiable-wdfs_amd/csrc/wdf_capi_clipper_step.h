// wdf_capi_clipper_step.h -- what wdf_capi_clipper.hip, wdf_capi_clipper_noy.hip and wdf_capi_clipper_eval.hip share: the dispatcher
// of the clipper kernels' four leading template parameters, the layout of the caller's warm-start state, and the hand-over of a
// checked one-pass step to the translation unit that holds the instantiations WITHOUT the y store (a unit of its own: the storing
// step's unit is the longest compile of the library, and the two compile side by side).
#pragma once
#include "wdf_capi_common.h"
#include "wdf_clipper_fused.h"

namespace wdfcapi {

// The kernels' four leading template parameters from runtime values: dyn is Bools{r != nullptr} or, where a kernel also has the
// one-value-per-sequence form, Values<int, 0, 1, 2>.  TM && V4 is never built: a time-major x has no 4-step rows to load.
template <class Dyn, class F> bool dispatch4(F&& f, Dyn dyn, bool sym, bool tm, bool v4)
{
    return dispatch([&](auto DYN, auto SYM, auto TM, auto V4) {
        if constexpr (TM() && V4()) return false;
        else return dispatch([&] { return f(DYN, SYM, TM, V4); });
    }, dyn, Bools{sym}, Bools{tm}, Bools{v4});
}

// state: nullptr (stateless, cold every call) or the caller's persistent warm-start buffer
// [TpCtl][tile tickets + accumulators][snapshot ring kTpRing x J x K x B floats]
struct TpWarm { wdf::TpCtl* ctl; float* snap; int J; };

// per-tile tickets, 4 accumulator words, per-tile repair flags
inline size_t tp_ticket_bytes(int64_t B) { return round_up((2 * waves64(B) + 4) * sizeof(unsigned), 64); }

// the caller's persistent warm-start state: [TpCtl][tile tickets + accumulators][snapshot ring]
struct TpState { wdf::TpCtl* ctl; unsigned* tickets; float* snap; size_t bytes; };
inline TpState tp_state(void* state, int64_t B, size_t ring_floats)
{
    Carver c(state);
    TpState w;
    w.ctl = c.take<wdf::TpCtl>(1);
    w.tickets = c.take<unsigned>(tp_ticket_bytes(B) / sizeof(unsigned));
    w.snap = c.take<float>(ring_floats);
    w.bytes = c.off;
    return w;
}

// A one-pass step without y, arguments checked and workspace carved (step_tp_common): everything launch_fused takes but y.
// form: kFusedFinishLater, or kFusedInKernel for a single chunk (no boundary, no second launch) -- no other form is built.
struct FusedNoYLaunch {
    const float* x; const float* r; const float* theta; float fs; int n_up, n_down; const float* target; float hgs; int64_t skip;
    const float* z0; float* zT; float* zwarm; float* zend; float* rec; double* part; double* wpart; unsigned* tickets; unsigned* gticket;
    wdf::FusedGroupWs grp; wdf::TpStatus* status; wdf::TpCtl* ctl; float* snap; int J; float tol; int64_t B, T; int K; int64_t L, W;
    int general; bool pairs, esr; wdf::FusedOut out; int64_t skew; int form; hipStream_t s;
};

// dyn: 0 static R, 1 per-sample r, 2 one r per sequence.  false: no kernel for the combination.
bool launch_fused_noy(int dyn, bool sym, bool tm, bool v4, const FusedNoYLaunch& a);

}  // namespace wdfcapi
