// wdf_capi_clipper_noy.hip -- the one-pass clipper step WITHOUT the y store (WDF_NO_Y_STORE on wdf_clipper_step_mse_tp / _esr_tp):
// the STORE_Y = false instantiations of clipper_fused_tp_kernel and clipper_fused_finish_kernel (csrc/wdf_clipper_fused.h) and
// their launches.  The entry points, their checks and the workspace layout stay in wdf_capi_clipper.hip (step_tp_common).
#include <algorithm>

#include "wdf_capi_clipper_step.h"

namespace wdfcapi {

namespace {

// launch_fused's default form with y = nullptr: one chunk wave to a workgroup, then -- more than one chunk -- the finish launch
// with several waves per tile, whose wave 0 also runs the repair walk (without the y store as well).
template <int DYN_R, bool SYM, bool TM, bool V4>
void launch_noy(const FusedNoYLaunch& a)
{
    const int per_tile = a.pairs ? 128 : 64;
    const dim3 grid((unsigned)((a.B + per_tile - 1) / per_tile), (unsigned)a.K);
    const int fin_waves = (int)std::min<int64_t>(wdf::kFinMaxWaves, (a.K + wdf::kFinMinSeg - 1) / wdf::kFinMinSeg);
    hipStream_t s = a.s;
    dispatch([&](auto PAIRS, auto LOSS) {                      // LOSS 1: MSE, 2: MSE + ESR
        using V = std::conditional_t<PAIRS(), wdf::v2f, float>;
        constexpr int N = PAIRS() ? 2 : 1;                     // sequences per lane
        {
            EventBracket bracket(s);
            hipLaunchKernelGGL((wdf::clipper_fused_tp_kernel<DYN_R, SYM, TM, V4, V, LOSS(), false>), grid, dim3(64), 0, s, a.x, a.r, a.theta, a.fs,
                               a.n_up, a.n_down, a.target, a.hgs, a.skip, (float*)nullptr, a.z0, a.zT, a.zwarm, a.zend, a.rec, a.status, a.ctl,
                               a.snap, a.J, a.tickets, a.gticket, a.tol, a.B, a.T, (int64_t)a.K, a.L, a.W, a.general, a.part, a.out, a.skew,
                               a.wpart, a.form, a.grp);
        }
        if (a.form == wdf::kFusedFinishLater)
            hipLaunchKernelGGL((wdf::clipper_fused_finish_kernel<DYN_R, SYM, TM, N, LOSS(), false>), dim3(grid.x), dim3(64 * fin_waves), 0, s, a.x,
                               a.r, a.theta, a.fs, a.n_up, a.n_down, a.target, a.hgs, a.skip, (float*)nullptr, a.zT, a.zwarm, a.zend, a.rec, a.B,
                               a.T, (int64_t)a.K, a.L, a.tol, a.status, a.ctl, a.snap, a.J, a.tickets, a.gticket, a.general, a.part, a.out,
                               a.skew, a.wpart, a.W);
    }, Bools{a.pairs}, Values<int, 1, 2>{a.esr ? 2 : 1});
}

}  // namespace

bool launch_fused_noy(int dyn, bool sym, bool tm, bool v4, const FusedNoYLaunch& a)
{
    if (a.form != wdf::kFusedFinishLater && !(a.form == wdf::kFusedInKernel && a.K < 2)) return false;
    return dispatch4([&](auto DYN, auto SYM, auto TM, auto V4) { launch_noy<DYN(), SYM(), TM(), V4()>(a); }, Values<int, 0, 1, 2>{dyn}, sym,
                     tm, v4);
}

}  // namespace wdfcapi
