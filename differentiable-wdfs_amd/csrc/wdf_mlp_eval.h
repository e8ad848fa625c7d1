// wdf_mlp_eval.h -- the LOSS-ONLY evaluation pass of the resident MLP-root pot clipper (clipper_pot.py:251-262: the validation
// line of every epoch -- ClipperModel.forward over val_X, MSE + ESR past skip_samples, never differentiated), gfx950.
//
// wdf_mlp_step.h's forward is the TRAINING forward: beside every owned step it runs the kappa chain (dz'/dz through the network),
// carries the block's adjoint map and stores zstash, kappa and the maps for a reverse sweep -- and the call is committed (call
// count, snapshot parity, have_snap) by the reverse sweep's last launch only, so a pair that is only evaluated through that
// forward starts every chunk cold, every call.  Here the step's own chunked, verified, device-steered forward (mlp_step_fwd_kernel:
// its work items, tickets, flags, zwarm / zend / zpre, snapshot ping-pong, verification, per-column warm-up controller and
// repair loop; the step's own state block, its MlpStepArgs with zstash = kappa = maps = null) runs an evaluation block, and the
// last launch commits the call.  This header holds what the pass adds to that kernel:
//
//   mlp_step_block(MlpEvalPass<STORE_Y>, ...)   the evaluation block: owned steps produce y (stored or not) and the two loss sums.
//   MlpEvalPass<STORE_Y>   the pass's tag: mlp_step_fwd_kernel<NL, DYN_R, ACT, MODE, MlpEvalPass<STORE_Y>> runs that block, and its
//         repair (MODE 1) reads the old trajectory from the snapshot rows MODE 0 of THIS call published (the state before every
//         owned 16-step block: the number the step reads from zstash).
//   mlp_eval_finish_kernel   the column sums in fixed order -> sums[2], the three loss values, the call's bookkeeping.
//
// Four launches (MODE 0, 1, 2, finish), every buffer fixed: capturable as a HIP graph like the step.  No wave waits on another
// workgroup.
#pragma once

#include "wdf_mlp_step.h"

namespace wdf {

// The evaluation pass's tag (MlpTrainPass's counterpart, wdf_mlp_step.h).  The old state before step tb + 16 is row (tb + 16) / 16
// of the snapshot set this call writes (the repair loop's comment says why it still is the old one when it is read).
template <bool STORE_Y>
struct MlpEvalPass {
    static __device__ __forceinline__ float old_state(const MlpStepArgs& A, const float* snap_w, int64_t tb, int64_t b)
    { return step_published(snap_w + ((tb + 16) >> 4) * A.B + b); }
};

// One block of 16 steps of the evaluation pass.  OWNED: y (STORE_Y) and the block's two loss sums; otherwise a warm-up block:
// state only.  a, zn, yv, sS, sE are the training block's expressions, letter for letter: y and the sums agree with the step's.
template <int NL, bool DYN_R, int ACT, bool OWNED, bool PASS_STORE_Y>
__device__ __forceinline__ void mlp_step_block(MlpEvalPass<PASS_STORE_Y>, const MlpStepArgs& A, const StepWeights<NL>& Wt,
                                               const MlpClipConsts& c, int64_t tb, int col, int64_t b, bool live, int g,
                                               const float* __restrict__ xp, const float* __restrict__ pp,
                                               const float* __restrict__ lp, StepSpan& sp)
{
    constexpr bool STORE_Y = OWNED && PASS_STORE_Y;
    const int64_t B = A.B;
    float xs[16], ps[16], ls[16];
    step_load_inputs<DYN_R>(xp, pp, lp, tb, xs, ps, ls);
    float tt[4] = {0.0f, 0.0f, 0.0f, 0.0f};                     // group g looks after the steps i = g (mod 4)
    if constexpr (OWNED) {
#pragma unroll
        for (int q = 0; q < 4; ++q) tt[q] = A.target[(tb + 4 * q + g) * B + b];
    }
    float z = sp.z;
    float yk = 0.0f, sS = 0.0f, sE = 0.0f;
    mfma_v4f act[NL];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float p = DYN_R ? ps[i] : c.p, lr = DYN_R ? ls[i] : c.lr;
        const float b_diff = z - xs[i];
        const float b_temp = -p * b_diff;
        const float a = z + b_temp;
        const float zn = b_temp - step_mlp_fwd<NL, ACT>(Wt, a, lr, act);     // b_root = -MLP (clipper_pot.py:121)
        if constexpr (OWNED) {
            const float yv = 0.5f * (zn + z);
            if ((i & 3) == g) {
                yk = yv;
                const float msk = (tb + i >= A.skip) ? 1.0f : 0.0f;
                const float d = yv - tt[i >> 2];
                sS = fmaf(msk * d, d, sS);
                sE = fmaf(msk * yv, yv, sE);
            }
            if constexpr (STORE_Y) {
                if ((i & 3) == 3 && live) A.y[(tb + (i - 3 + g)) * B + b] = yk;
            }
        }
        z = zn;
    }
    sp.z = z;
    if constexpr (OWNED) {
        // the block's two loss sums, published: the column's last finisher of this launch adds the blocks up
        const float bS = wave_sum_f32(live ? sS : 0.0f), bE = wave_sum_f32(live ? sE : 0.0f);
        if ((threadIdx.x & 63) == 0) {
            float* __restrict__ lb = A.lossblk + ((tb >> 4) * A.n_cols + col) * 2;
            step_publish(lb, bS);
            step_publish(lb + 1, bE);
        }
    }
}

// ---- (4) the column sums in mlp_step_sums_kernel's order -> sums[2]; the three loss values with the reduce kernel's
// expressions; the call is committed (what mlp_step_reduce_adam_kernel does for a training step).  One wave.
static __global__ __launch_bounds__(64) void mlp_eval_finish_kernel(const double* __restrict__ colsum, int n_cols, double n_global,
                                                                    double eps_energy, double* __restrict__ sums,
                                                                    float* __restrict__ loss3, MlpStepCtl* ctl)
{
    double s = 0.0, e = 0.0;
    for (int cc = threadIdx.x; cc < n_cols; cc += 64) { s += colsum[2 * cc]; e += colsum[2 * cc + 1]; }
    const double S = wave_sum_dpp(s), E = wave_sum_dpp(e);
    if (threadIdx.x == 0) {
        sums[0] = S; sums[1] = E;
        const double mse = S / n_global, esr = sqrt(S / (E + eps_energy) / n_global);
        if (loss3) { loss3[0] = (float)mse; loss3[1] = (float)esr; loss3[2] = (float)(mse + esr); }
        ctl->call += 1;
        ctl->parity ^= 1;
        ctl->have_snap = 1;
    }
}

}  // namespace wdf
