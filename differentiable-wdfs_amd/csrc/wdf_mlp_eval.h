// wdf_mlp_eval.h -- the LOSS-ONLY evaluation pass of the resident MLP-root pot clipper (clipper_pot.py:251-262: the validation
// line of every epoch -- ClipperModel.forward over val_X, MSE + ESR past skip_samples, never differentiated), gfx950.
//
// wdf_mlp_step.h's forward is the TRAINING forward: beside every owned step it runs the kappa chain (dz'/dz through the network),
// carries the block's adjoint map and stores zstash, kappa and the maps for a reverse sweep -- and the call is committed (call
// count, snapshot parity, have_snap) by the reverse sweep's last launch only, so a pair that is only evaluated through that
// forward starts every chunk cold, every call.  Here the same chunked, verified, device-steered forward (the step's work items,
// tickets, flags, zwarm / zend / zpre, snapshot ping-pong, verification, per-column warm-up controller: the step's own state
// block, its MlpStepArgs with zstash = kappa = maps = null) runs an evaluation block, and the last launch commits the call:
//
//   (1) mlp_eval_fwd_kernel<MODE 0>   the chunked forward; owned steps produce y (stored or not) and the two loss sums.
//   (2) <MODE 1>  flagged chunks again from their predecessors' end states, until they meet the old trajectory -- which the step
//         reads from zstash and this pass from the snapshot rows MODE 0 of THIS call published (the state before every owned
//         16-step block: the same number).
//   (3) <MODE 2>  what still fails: the whole column sequentially.
//   (4) mlp_eval_finish_kernel   the column sums in fixed order -> sums[2], the three loss values, the call's bookkeeping.
//
// Four launches, every buffer fixed: capturable as a HIP graph like the step.  No wave waits on another workgroup.
#pragma once

#include "wdf_mlp_step.h"

namespace wdf {

// One block of 16 steps of the evaluation pass.  OWNED: y (STORE_Y) and the block's two loss sums; otherwise a warm-up block:
// state only.  a, zn, yv, sS, sE are mlp_step_block's expressions, letter for letter: y and the sums agree with the step's.
template <int NL, bool DYN_R, int ACT, bool OWNED, bool STORE_Y>
__device__ __forceinline__ void mlp_eval_block(const MlpStepArgs& A, const StepWeights<NL>& Wt, const MlpClipConsts& c, int64_t tb,
                                               int col, int64_t b, bool live, int g, const float* __restrict__ xp,
                                               const float* __restrict__ pp, const float* __restrict__ lp, float& zio)
{
    const int64_t B = A.B;
    float xs[16], ps[16], ls[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 xv = *reinterpret_cast<const float4*>(xp + tb + 4 * q);
        xs[4 * q] = xv.x; xs[4 * q + 1] = xv.y; xs[4 * q + 2] = xv.z; xs[4 * q + 3] = xv.w;
        if constexpr (DYN_R) {
            const float4 pv = *reinterpret_cast<const float4*>(pp + tb + 4 * q);
            const float4 lv = *reinterpret_cast<const float4*>(lp + tb + 4 * q);
            ps[4 * q] = pv.x; ps[4 * q + 1] = pv.y; ps[4 * q + 2] = pv.z; ps[4 * q + 3] = pv.w;
            ls[4 * q] = lv.x; ls[4 * q + 1] = lv.y; ls[4 * q + 2] = lv.z; ls[4 * q + 3] = lv.w;
        }
    }
    float tt[4] = {0.0f, 0.0f, 0.0f, 0.0f};                     // group g looks after the steps i = g (mod 4)
    if constexpr (OWNED) {
#pragma unroll
        for (int q = 0; q < 4; ++q) tt[q] = A.target[(tb + 4 * q + g) * B + b];
    }
    float z = zio;
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
    zio = z;
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

// One span of one column: steps [tw, t0) warm up, [t0, t1) are owned.  Returns the end state.  (mlp_step_span with the
// evaluation block.)
template <int NL, bool DYN_R, int ACT, bool PUBLISH, bool STORE_Y>
__device__ __forceinline__ float mlp_eval_span(const MlpStepArgs& A, const StepWeights<NL>& Wt, const MlpClipConsts& c,
                                               int item, int col, int64_t tw, int64_t t0, int64_t t1, float z,
                                               float* __restrict__ snap_w)
{
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const int64_t B = A.B, T = A.T;
    const int64_t b_raw = (int64_t)col * 16 + n;
    const bool live = b_raw < B;
    const int64_t b = live ? b_raw : B - 1;
    const float* __restrict__ xp = A.x + b * T;
    const float* __restrict__ pp = DYN_R ? A.p + b * T : nullptr;
    const float* __restrict__ lp = DYN_R ? A.lr + b * T : nullptr;
    for (int64_t tb = tw; tb < t0; tb += 16) {                   // ---- warm-up blocks
        const int64_t j = (t0 - tb) >> 4;                        // 16-step units before the first owned step
        if (g == 0 && j <= kStepPre) step_publish(A.zpre + ((int64_t)item * kStepPre + (j - 1)) * 16 + n, z);
        mlp_eval_block<NL, DYN_R, ACT, false, false>(A, Wt, c, tb, col, b, live, g, xp, pp, lp, z);
    }
    if (g == 0) {
        if constexpr (PUBLISH) step_publish(A.zwarm + (int64_t)item * 16 + n, z);
        else A.zwarm[(int64_t)item * 16 + n] = z;
    }
    for (int64_t tb = t0; tb < t1; tb += 16) {                   // ---- owned blocks
        // the state a later call may start from; this call's verifier compares shorter warm-ups against it, and this call's
        // MODE 1 holds a re-run chunk against it
        if (g == 0 && live) step_publish(snap_w + (tb >> 4) * B + b, z);
        mlp_eval_block<NL, DYN_R, ACT, true, STORE_Y>(A, Wt, c, tb, col, b, live, g, xp, pp, lp, z);
    }
    return z;
}

// MODE 0 / 1 / 2 and the grid as mlp_step_fwd_kernel's (four-wave workgroups: one wave per SIMD).  A.zstash, A.kappa and A.maps
// are null and never looked at; A.y is null when !STORE_Y.
template <int NL, bool DYN_R, int ACT, int MODE, bool STORE_Y>
__global__ __launch_bounds__(256) void mlp_eval_fwd_kernel(const MlpStepArgs A)
{
    const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4;
    const int unit = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);   // item (MODE 0, 1) or column (MODE 2) of this wave
    if (unit >= (MODE == 2 ? A.n_cols : A.n_items)) return;
    // the two repair launches leave at once unless their item / column is flagged: ONE load decides
    if constexpr (MODE == 1) { if (A.flag[unit] == 0u) return; }
    if constexpr (MODE == 2) { if (A.colseq[unit] == 0u) return; }
    MlpStepCtl* ctl = A.ctl;
    const int par = ctl->parity;                                   // this call reads set `par`, writes the other
    const int64_t nblk = A.T >> 4;
    float* snap_w = A.snap + (int64_t)(par ^ 1) * nblk * A.B;
    const float* snap_r = A.snap + (int64_t)par * nblk * A.B;
    int* st = ctl->status[ctl->call & 1];
    if constexpr (MODE == 2) {
        const int col = unit;
        const MlpStepCol cinfo = A.cols[col];
        const MlpClipConsts c = DYN_R ? MlpClipConsts{} : mlp_load_consts(A.theta2, A.fs);
        const StepWeights<NL> Wt = step_load_weights<NL, ACT>(A.w, A.H, lane);
        // one item after the other, each from the state the previous one ended in
        float z = 0.0f;                                            // reset(): clipper_pot.py:110-111
        for (int k = 0; k < cinfo.K; ++k) {
            const MlpStepItem it = A.items[cinfo.first + k];
            z = mlp_eval_span<NL, DYN_R, ACT, false, STORE_Y>(A, Wt, c, cinfo.first + k, col, it.t0, it.t0, it.t1, z, snap_w);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        mlp_step_column_loss(A, col);
        if (lane == 0) {
            A.colseq[col] = 0u;
            atomicAdd(&st[3], 1);
            atomicAdd(&ctl->total_sequential, 1);
        }
        return;
    } else {
        const int item = unit;
        const MlpStepItem it = A.items[item];
        const MlpStepCol cinfo = A.cols[it.col];
        if constexpr (MODE == 0) {
            if (item == 0 && lane == 0) {                          // the NEXT call's verdict words start clean
                int* nx = ctl->status[(ctl->call + 1) & 1];
                nx[0] = 0; nx[1] = 0; nx[2] = 0; nx[3] = 0;
            }
            if (lane == 0) {
                A.hwid[2 * item] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));       // HW_REG_HW_ID
                A.hwid[2 * item + 1] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11));  // HW_REG_XCC_ID
            }
        }
        const MlpClipConsts c = DYN_R ? MlpClipConsts{} : mlp_load_consts(A.theta2, A.fs);
        const StepWeights<NL> Wt = step_load_weights<NL, ACT>(A.w, A.H, lane);
        const int64_t b_raw = (int64_t)it.col * 16 + n;
        const bool live = b_raw < A.B;
        const int64_t b = live ? b_raw : A.B - 1;
        int64_t tw = it.t0;
        float z = 0.0f;
        if constexpr (MODE == 0) {
            if (it.k > 0) {
                const int warm = ctl->have_snap;
                const int64_t W = 16 * (int64_t)(warm ? A.wcol[it.col] : ctl->cold16);
                tw = it.t0 > W ? it.t0 - W : 0;
                z = (warm && tw > 0) ? snap_r[(tw >> 4) * A.B + b] : 0.0f;
            }
            z = mlp_eval_span<NL, DYN_R, ACT, true, STORE_Y>(A, Wt, c, item, it.col, tw, it.t0, it.t1, z, snap_w);
            if (g == 0) step_publish(A.zend + (int64_t)item * 16 + n, z);
        } else {
            // The repair, as the step's: the flagged chunk again from the state its predecessor ended in, block by block until
            // the new state meets the OLD trajectory.  The step reads the old state before step tb + 16 from its stash; here it is
            // row (tb + 16) / 16 of the snapshot set this call writes: MODE 0 published the state before every owned block there.
            // The row is read BEFORE this loop publishes over it (row tb now, row tb + 16 in the next iteration), and nobody else
            // writes it: the chunk that owns it is either not flagged (it does not run in this launch) or, if it is, this wave stops
            // at its boundary (the column goes sequential).  At a chunk's end the reference is the recorded end state, as in the step.
            const float* __restrict__ xp = A.x + b * A.T;
            const float* __restrict__ pp = DYN_R ? A.p + b * A.T : nullptr;
            const float* __restrict__ lp = DYN_R ? A.lr + b * A.T : nullptr;
            z = A.zend[(int64_t)(item - 1) * 16 + n];             // (k > 0: only boundaries are flagged)
            const float eps_c = ctl->repair_at * ctl->tol;
            int cur = item;                                       // the item whose steps are being rewritten
            int64_t t_end = it.t1;
            for (int64_t tb = it.t0; tb < A.T; tb += 16) {
                if (tb == t_end) {                                // ran through a whole chunk without meeting the old trajectory
                    const bool last = cur + 1 >= cinfo.first + cinfo.K;
                    if (!last && A.flag[cur + 1] != 0u) { if (lane == 0) A.colseq[it.col] = 1u; break; }
                    cur += 1;
                    t_end = A.items[cur].t1;
                }
                if (g == 0 && live) step_publish(snap_w + (tb >> 4) * A.B + b, z);
                const float z_old_next = (tb + 16 < A.T) ? step_published(snap_w + ((tb + 16) >> 4) * A.B + b) : z;
                const float z_end_old = A.zend[(int64_t)cur * 16 + n];
                mlp_eval_block<NL, DYN_R, ACT, true, STORE_Y>(A, Wt, c, tb, it.col, b, live, g, xp, pp, lp, z);
                const float ref = (tb + 16 == t_end) ? z_end_old : z_old_next;
                const bool off = live && !(fabsf(z - ref) <= eps_c);
                if (tb + 16 < A.T && __ballot(off) == 0ull) break;
            }
        }
        // ---- the column's last finisher (mlp_step_fwd_kernel's, word for word)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's outputs and boundary states have landed
        unsigned* tk = (MODE == 0 ? A.ticket : A.ticket2) + it.col;
        const unsigned expect = MODE == 0 ? (unsigned)cinfo.K : A.nflag[it.col];
        unsigned old = 0;
        if (lane == 0) old = atomicAdd(tk, 1u);
        old = __builtin_amdgcn_readfirstlane(old);
        if (old != expect - 1u) return;
        if (lane == 0) *tk = 0u;                                   // left clean for the next launch
        mlp_step_column_loss(A, it.col);
        const float tol = ctl->tol;
        if constexpr (MODE == 0) {
            // every boundary of the column: lane (q, n) takes the boundaries k = 1 + q, 5 + q, ...
            float m0 = 0.0f, mp[kStepPre] = {0.0f, 0.0f, 0.0f};
            int nbad = 0;
            const int warm = ctl->have_snap;
            const int wc = warm ? A.wcol[it.col] : ctl->cold16;
            for (int k = 1 + g; k < cinfo.K; k += 4) {
                const int64_t ik = cinfo.first + k;
                const float zw = step_published(A.zwarm + ik * 16 + n);
                const float ze = step_published(A.zend + (ik - 1) * 16 + n);
                const float m = live ? fabsf(zw - ze) : 0.0f;
                const bool bad = !(m <= tol);
                const unsigned long long any = __ballot(bad) >> (16 * g) & 0xffffull;   // (the 16 lanes of this boundary)
                if (n == 0) A.flag[ik] = any ? 1u : 0u;
                nbad += (any && n == 0) ? 1 : 0;
                m0 = fmaxf(m0, m);
                const int64_t t0k = A.items[ik].t0;
#pragma unroll
                for (int j = 1; j <= kStepPre; ++j) {
                    // the miss a warm-up j units shorter would have arrived with (needs j <= W and the sample to exist)
                    float mj = j <= wc ? 0.0f : 3.0e38f;         // (a warm-up that reaches back to t = 0 is exact)
                    if (j <= wc && t0k - 16 * j > 0) {
                        const float zp = step_published(A.zpre + (ik * kStepPre + (j - 1)) * 16 + n);
                        const float zt = step_published(snap_w + ((t0k >> 4) - j) * A.B + b);
                        mj = live ? fabsf(zp - zt) : 0.0f;
                    }
                    mp[j - 1] = fmaxf(mp[j - 1], mj);
                }
            }
            m0 = wave_max_dpp(m0);
#pragma unroll
            for (int j = 0; j < kStepPre; ++j) mp[j] = wave_max_dpp(mp[j]);
            nbad = wave_sum_dpp(nbad);
            if (lane == 0) {
                if (cinfo.K > 0) A.flag[cinfo.first] = 0u;
                A.nflag[it.col] = (unsigned)nbad;
                A.colmiss[4 * it.col] = m0;
#pragma unroll
                for (int j = 0; j < kStepPre; ++j) A.colmiss[4 * it.col + 1 + j] = mp[j];
                if (nbad) { atomicAdd(&st[0], nbad); atomicAdd(&st[2], 1); atomicAdd(&ctl->total_flagged, nbad); }
                if (m0 > 0.0f) atomicMax(&st[1], __float_as_int(m0));
                // ---- steer the column's warm-up for the next call
                if (warm && !ctl->freeze && cinfo.K > 1) {
                    int W = A.wcol[it.col], cl = A.cool[it.col];
                    const float ms = mp[ctl->slack - 1];
                    if (nbad) { W += 2; cl = ctl->cool_miss; }
                    else if (m0 > ctl->grow_at * tol || mp[1] > tol) { W += 1; cl = cl > ctl->cool_shrink ? cl : ctl->cool_shrink; }
                    else if (cl > 0) { cl -= 1; }
                    else if (mp[kStepPre - 1] <= ctl->shrink_at * tol && W - 2 >= ctl->w_min) { W -= 2; cl = ctl->cool_shrink; }   // ample slack
                    else if (ms <= ctl->shrink_at * tol && W > ctl->w_min) { W -= 1; cl = ctl->cool_shrink; }
                    W = W > ctl->w_max ? ctl->w_max : W;
                    if (wc > A.wpeak[it.col]) A.wpeak[it.col] = wc;
                    A.wcol[it.col] = W;
                    A.cool[it.col] = cl;
                }
            }
        } else {
            if (lane == 0) {
                for (int k = 1; k < cinfo.K; ++k) A.flag[cinfo.first + k] = 0u;
                A.nflag[it.col] = 0u;
            }
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
