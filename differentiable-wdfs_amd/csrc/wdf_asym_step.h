// wdf_asym_step.h -- the training step of the two-different-diode clipper (wdf_asym.h) in ONE pass over the data, for the
// MSE loss (LOSS = 0) and for the scripts' MSE + ESR loss past `skip` samples (LOSS = 1):
// forward, loss and gradient with x and the target read once and y written once, no state stash, one root solve per sample.
// Both Newton modes; the closed form (mode 0) is a model approximation and keeps the kernel pair.
//
// The gradient is carried FORWARD in time as the state's tangent.  With the local partials of wdf_asym.h's reverse sweep
// (Da = d b / d a, c_i = d b / d{Is1, V1, Is2, V2, Rp} at the root the step just solved, c_p = -(1 + Da)(z - x),
// kappa = Da - p (1 + Da)) the state's tangent to each of the six parameters {Is1, V1, Is2, V2, Rp, p} obeys
//     tau_i' = kappa tau_i + c_i ,   dy_i = (tau_i' + tau_i) / 2 ,
// and with the residual e = y - target the step adds  S += e^2 ,  G_i += e dy_i  (G = d(S/2)/d parameter).
//
// Time chunks (grid.y) start from a warmed-up state exactly as clipper_asym_fwd_tp_kernel's do and are verified by the same
// asym_tp_verify_kernel.  The tangent entering a chunk is unknown, but the recurrence is linear in it with the SAME factor
// for every parameter, so a chunk runs with zero entering tangent and records per sequence
//     P = prod kappa                       its leaving tangent  = P tau_in + q_i
//     A = sum_t e_t (m_t' + m_t) / 2       its gradient sums    = A tau_in + beta_i      (m_t: the product of kappa before step t)
// and S.  clipper_asym_step_finish_kernel walks a sequence's K records first to last (tau = 0 enters chunk 0: z0 is a
// constant of the call) -- the forward-time twin of the reverse sweep's {P, q, alpha, beta}, exact: no truncation, no tangent
// warm-up.  A chunk whose start state missed the verification never reaches the gradient: the flagged waves are re-run by a
// gated launch of the same kernel with one chunk, whose record (slot 0) replaces the wave's K chunked ones.
//
// MSE + ESR (clipper_pot.py:146-156,177,232,248): loss = S/n + sqrt(S / (E + eps) / n), S = sum e^2, E = sum y^2 over the rows
// t >= skip.  dLoss/dy = ga e + gb y with ga, gb functions of the GLOBAL S and E (esr_coef_kernel's formulas), so the pass
// carries BOTH tangent-weighted sums, gP_i = sum e dy_i = d(S/2)/d parameter and gQ_i = sum y dy_i = d(E/2)/d parameter; a
// chunk records, next to the above,
//     A_Q = sum_t y_t (m_t' + m_t) / 2     gQ's sums = A_Q tau_in + betaQ_i
// and E.  Rows before skip add nothing to S, E, A, A_Q, beta, betaQ (e and y enter the sums as zero: a wave-uniform select);
// state, y, tau and m advance on them as on any other row.  The finish kernel hands back {S, E, gP[6], gQ[6]} of this call
// in theta-space (the chain rule is linear: applied to gP and gQ separately), which is what several ranks all-reduce, and
// finishes the step itself as a single rank when asked.
//
// One pot resistance per sequence (RSEQ, rseq [B]; wdf_clipper_asym_step_{mse,esr}_rseq): the port constants are the lane's own
// (asym_load_seq), the tangents and records are unchanged, and the chain rule Rp, p -> C moves from the last wave into every
// lane of the finish kernel, ahead of the wave sum.  The R component of every gradient is exactly 0 and theta6[4] is never
// read or written, by Adam either.
//
// Precision as the reverse sweep's: partials in fp32 (their inputs are fp32), recurrence and sums in fp64.
// rec, LOSS = 0: double [K][15][B] = {P, A, S, q[6], beta[6]};
//      LOSS = 1: double [K][23][B] = {P, A, S, q[6], beta[6], A_Q, E, betaQ[6]} (rows 0..14 as LOSS = 0).
// L and W are multiples of 8.
#pragma once

#include "wdf_asym.h"
#include "wdf_optim.h"
#include "wdf_esr.h"

namespace wdf {

constexpr int kAsymStepRec = 15;
constexpr int kAsymStepRecEsr = 23;
constexpr int kAsymStepPart = 8;                 // doubles per wave partial, LOSS = 0: {S, G[6], 0}
constexpr int kAsymStepPartEsr = 16;             //                           LOSS = 1: {S, E, gP[6], gQ[6], 0, 0}

// gate == nullptr: the chunked launch, grid = (waves, K); it also clears status and the finish kernel's ticket.
// gate != nullptr: the repair launch, grid = (waves, 1) with L >= T: flagged waves only.
// skip: LOSS = 1 only (rows before it count for nothing); anywhere in 0..T-1, inside a block or a later chunk.
// RSEQ (last template parameter) and rseq [B] (last argument): one pot resistance per sequence (wdf_asym.h asym_load_seq) -- the
// constants are then this lane's; the six tangents stay {Is1, V1, Is2, V2, Rp, p}, the records keep their layout.
template <int MODE, bool VEC4, int LOSS = 0, bool RSEQ = false>
__global__ __launch_bounds__(64) void clipper_asym_step_kernel(const float* __restrict__ x, const float* __restrict__ theta6, float fs,
                                                               const float* __restrict__ target, float* __restrict__ y,
                                                               const float* __restrict__ z0, float* __restrict__ zT,
                                                               float* __restrict__ zwarm, float* __restrict__ zend,
                                                               double* __restrict__ rec, double tol, int max_iter,
                                                               AsymTpStatus* __restrict__ status, unsigned* __restrict__ ticket,
                                                               const unsigned* __restrict__ gate, int64_t B, int64_t T, int64_t L,
                                                               int64_t W, int64_t skip = 0, const float* __restrict__ rseq = nullptr)
{
    using S = typename AsymStep<MODE>::S;
    if (gate != nullptr) {
        if (gate[blockIdx.x] == 0u) return;
    } else if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        *status = AsymTpStatus{0, 0.0f, 0, 0};                   // the verify kernel adds
        *ticket = 0u;                                            // the finish kernel counts its waves in
    }
    const int64_t b_raw = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int64_t b = b_raw < B ? b_raw : B - 1;
    const int64_t k = blockIdx.y;
    const int64_t t0 = k * L, t1 = (t0 + L < T) ? t0 + L : T;
    const int64_t tw = (k > 0 && t0 > W) ? t0 - W : 0;
    const AsymConsts c = RSEQ ? asym_load_seq(theta6, fs, rseq[b]) : asym_load(theta6, fs);
    const double p = c.p;
    const float* __restrict__ xp = x + b * T;
    int iters = 0;
    S z = (tw == 0 && z0) ? (S)z0[b] : (S)0;
    double tau[6] = {0, 0, 0, 0, 0, 0}, be[6] = {0, 0, 0, 0, 0, 0};
    double m = 1.0, A = 0.0, sse = 0.0;
    double bq[LOSS ? 6 : 1] = {}, AQ = 0.0, en = 0.0;            // LOSS = 1: betaQ, A_Q, E
    constexpr int kB = 8;
    float xc[kB], xn[kB], tc[kB], tn[kB];
    auto load_x = [&](int64_t t, float(&v)[kB]) {                // [B][T]: two float4 per lane where the block is whole
        if constexpr (VEC4) {
            if (t + kB <= T) {
                const float4* q4 = reinterpret_cast<const float4*>(xp + t);
                const float4 u0 = q4[0], u1 = q4[1];
                v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < kB; ++i) v[i] = xp[t + i < T ? t + i : T - 1];
    };
    auto load_t = [&](int64_t t, float(&v)[kB]) {                // [T][B]: coalesced rows
#pragma unroll
        for (int i = 0; i < kB; ++i) v[i] = target[(t + i < T ? t + i : T - 1) * B + b];
    };
#pragma unroll
    for (int i = 0; i < kB; ++i) tn[i] = 0.0f;
    load_x(tw, xn);
    if (tw == t0) load_t(t0, tn);
    for (int64_t tb = tw; tb < t1; tb += kB) {
        if (tb == t0) zwarm[k * B + b] = (float)z;              // the state this chunk arrives with
#pragma unroll
        for (int i = 0; i < kB; ++i) { xc[i] = xn[i]; tc[i] = tn[i]; }
        if (tb + kB < t1) {                                      // one block ahead of the recursion
            load_x(tb + kB, xn);
            if (tb + kB >= t0) load_t(tb + kB, tn);
        }
        const bool owned = tb >= t0;                             // (t0 - tw is a multiple of 8: a block is warm-up or owned, whole)
#pragma unroll
        for (int i = 0; i < kB; ++i) {
            if (tb + i < t1) {                                   // wave-uniform (the last chunk's ragged end)
                const S zb = z;
                AsymRootAt at;
                const float yv = AsymStep<MODE>::run_at(c, xc[i], z, tol, max_iter, iters, at);
                if (owned) {                                     // wave-uniform; behind the Newton loop, whose ballot exit it leaves alone
                    y[(tb + i) * B + b] = yv;
                    const double bd = (double)(zb - (S)xc[i]);
                    float Daf, cf[5];
                    asym_newton_partials(c, at.v, at.e1, at.e2, Daf, cf);
                    const double Da = (double)Daf;
                    const double kap = Da - p * (1.0 + Da);
                    double cth[6];
#pragma unroll
                    for (int q = 0; q < 5; ++q) cth[q] = (double)cf[q];
                    cth[5] = -(1.0 + Da) * bd;
                    if constexpr (LOSS == 0) {
                        const double e = (double)yv - (double)tc[i], eh = 0.5 * e;
                        sse = fma(e, e, sse);
#pragma unroll
                        for (int q = 0; q < 6; ++q) {
                            const double t_new = fma(kap, tau[q], cth[q]);
                            be[q] = fma(eh, t_new + tau[q], be[q]);
                            tau[q] = t_new;
                        }
                        const double m_new = kap * m;
                        A = fma(eh, m_new + m, A);
                        m = m_new;
                    } else {
                        const bool counted = tb + i >= skip;     // wave-uniform: a select, no branch
                        const double yd = counted ? (double)yv : 0.0;
                        const double e = counted ? (double)yv - (double)tc[i] : 0.0;
                        const double eh = 0.5 * e, yh = 0.5 * yd;
                        sse = fma(e, e, sse);
                        en = fma(yd, yd, en);
#pragma unroll
                        for (int q = 0; q < 6; ++q) {
                            const double t_new = fma(kap, tau[q], cth[q]);
                            const double dy2 = t_new + tau[q];
                            be[q] = fma(eh, dy2, be[q]);
                            bq[q] = fma(yh, dy2, bq[q]);
                            tau[q] = t_new;
                        }
                        const double m_new = kap * m, dm2 = m_new + m;
                        A = fma(eh, dm2, A);
                        AQ = fma(yh, dm2, AQ);
                        m = m_new;
                    }
                }
            }
        }
    }
    zend[k * B + b] = (float)z;
    if (zT && t1 == T) zT[b] = (float)z;
    double* __restrict__ r = rec + (k * (LOSS ? kAsymStepRecEsr : kAsymStepRec)) * B + b;
    r[0] = m;
    r[B] = A;
    r[2 * B] = sse;
#pragma unroll
    for (int q = 0; q < 6; ++q) { r[(3 + q) * B] = tau[q]; r[(9 + q) * B] = be[q]; }
    if constexpr (LOSS != 0) {
        r[15 * B] = AQ;
        r[16 * B] = en;
#pragma unroll
        for (int q = 0; q < 6; ++q) r[(17 + q) * B] = bq[q];
    }
}

// Adam with clip bounds on theta6 in the finish kernel's last wave (adam_clip_kernel's rule, wdf_optim.h); m == nullptr: none
struct AsymStepAdam {
    float* m; float* v; int32_t* step; const float* lr; const float* lo; const float* hi;
    float b1, b2, eps;
};

__device__ __forceinline__ double asym_wave_sum_all(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// What the MSE + ESR finish hands back (LOSS = 1): sums14 = {S, E, gP[6], gQ[6]} of THIS call in theta-space; gtheta6 != nullptr:
// the step finished as a single rank -- ga, gb, mse, esr from S, E, n_global and eps (esr_coef_kernel's formulas),
// gtheta6 = ga gP + gb gQ, loss3 = {mse, esr, mse + esr} (optional), then Adam, if asked for.
struct AsymStepEsrOut {
    double n_global, eps; float* sums14; float* gtheta6; float* loss3;
};

// the chain rule Rp, p -> R, C of a pair of sums (clipper_asym_grad_reduce_kernel's formulas)
__device__ __forceinline__ void asym_step_chain_rule(double SRp, double Sp, double R, double C, float fs, double& gR, double& gC)
{
    const double G1 = 1.0 / R, G2 = C * (2.0 * (double)fs), Rp = 1.0 / (G1 + G2), p = G1 * Rp;
    gR = SRp * Rp * Rp * G1 * G1 - Sp * G1 * G1 * Rp * (1.0 - p);
    gC = -2.0 * (double)fs * (SRp * Rp * Rp + Sp * p * Rp);
}

// One lane per sequence: the K records first to last (one record where the wave was repaired), the wave's sums -> part[wave][8]
// = {S, G[6], 0} (LOSS = 1: part[wave][16] = {S, E, gP[6], gQ[6], 0, 0}, both families walked with the same tangent:
// gP_i += A tau_i + beta_i, gQ_i += A_Q tau_i + betaQ_i, tau_i <- P tau_i + q_i); the wave that finishes LAST sums the
// partials in a fixed order (lane i takes waves i, i + 64, ...; then the shuffle tree), applies the chain rule Rp, p -> R, C
// and, LOSS = 0, gscale: out7 = {sse, d(gscale/2 sse)/d{Is1, V1, Is2, V2, R, C}}; LOSS = 1: AsymStepEsrOut; then Adam, if asked for.
// RSEQ: one pot per sequence.  Rp and p differ from lane to lane, so their sums over sequences mean nothing: each lane applies
// the chain rule to its own {S_Rp, S_p} with its own R_b (asym_seq_chain_rule) behind its record walk and ahead of the wave sum,
// for gP and, LOSS = 1, gQ alike.  Slot 5 then carries dC, slot 4 exactly 0 (the pot is data, not a parameter), and the last
// wave skips its own chain rule: out7, sums14 and gtheta6 keep their layouts with component 4 equal to 0.0f.  Adam leaves
// theta6[4] bit-for-bit as it was: a zero gradient on zero moments moves nothing, and so that a clip bound, a moment left by
// static steps or eps = 0 cannot either, its lane leaves before it touches value or moments.
template <int LOSS, bool RSEQ = false>
__global__ __launch_bounds__(64) void clipper_asym_step_finish_kernel(const double* __restrict__ rec, const unsigned* __restrict__ gate,
                                                                      double* part, unsigned* ticket, float* theta6, float fs,
                                                                      float gscale, float* __restrict__ out7, AsymStepEsrOut esr,
                                                                      AsymStepAdam adam, int64_t B, int64_t K,
                                                                      const float* __restrict__ rseq = nullptr)
{
    constexpr int NREC = LOSS ? kAsymStepRecEsr : kAsymStepRec, NP = LOSS ? kAsymStepPartEsr : kAsymStepPart;
    constexpr int NS = LOSS ? 14 : 7, GP = LOSS ? 2 : 1, GQ = 8;            // sums; where gP (and, LOSS = 1, gQ) start in them
    const int64_t b_raw = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = b_raw < B;
    const int64_t b = live ? b_raw : B - 1;
    const int64_t kn = (gate != nullptr && gate[blockIdx.x] != 0u) ? 1 : K;
    double tau[6] = {0, 0, 0, 0, 0, 0}, s[NS] = {};
    for (int64_t k = 0; k < kn; ++k) {
        const double* __restrict__ r = rec + (k * NREC) * B + b;
        const double P = r[0], A = r[B];
        s[0] += r[2 * B];
        double AQ = 0.0;
        if constexpr (LOSS != 0) { AQ = r[15 * B]; s[1] += r[16 * B]; }
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            s[GP + q] += fma(A, tau[q], r[(9 + q) * B]);
            if constexpr (LOSS != 0) s[GQ + q] += fma(AQ, tau[q], r[(17 + q) * B]);
            tau[q] = fma(P, tau[q], r[(3 + q) * B]);
        }
    }
    if constexpr (RSEQ) {
        const double Rb = (double)rseq[b], Cb = (double)theta6[5];
        s[GP + 5] = asym_seq_chain_rule(s[GP + 4], s[GP + 5], Rb, Cb, fs);
        s[GP + 4] = 0.0;
        if constexpr (LOSS != 0) {
            s[GQ + 5] = asym_seq_chain_rule(s[GQ + 4], s[GQ + 5], Rb, Cb, fs);
            s[GQ + 4] = 0.0;
        }
    }
    const unsigned nwaves = gridDim.x;
    double w[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) w[i] = asym_wave_sum_all(live ? s[i] : 0.0);
    unsigned done = 0;
    if (threadIdx.x == 0) {
        double* o = part + (int64_t)blockIdx.x * NP;
#pragma unroll
        for (int i = 0; i < NS; ++i) __hip_atomic_store(o + i, w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the partial has landed before the count moves
        done = atomicAdd(ticket, 1u);
    }
    done = __builtin_amdgcn_readfirstlane(done);
    if (done != nwaves - 1) return;
    double t[NS] = {};
    for (unsigned i = threadIdx.x; i < nwaves; i += 64)
#pragma unroll
        for (int j = 0; j < NS; ++j) t[j] += __hip_atomic_load(part + (int64_t)i * NP + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int j = 0; j < NS; ++j) t[j] = asym_wave_sum_all(t[j]);
    // every lane forms the chain rule, lanes 0..5 keep their component
    const double R = theta6[4], C = theta6[5];
    double gR, gC;
    if constexpr (RSEQ) { gR = 0.0; gC = t[GP + 5]; }
    else asym_step_chain_rule(t[GP + 4], t[GP + 5], R, C, fs, gR, gC);
    const int i = threadIdx.x < 6 ? threadIdx.x : 5;
    const double gi = i == 0 ? t[GP] : (i == 1 ? t[GP + 1] : (i == 2 ? t[GP + 2] : (i == 3 ? t[GP + 3] : (i == 4 ? gR : gC))));
    float g;
    if constexpr (LOSS == 0) {
        g = (float)((double)gscale * gi);
        if (threadIdx.x == 0) out7[0] = (float)t[0];
        if (threadIdx.x < 6) out7[1 + threadIdx.x] = g;
    } else {
        double qR, qC;
        if constexpr (RSEQ) { qR = 0.0; qC = t[GQ + 5]; }
        else asym_step_chain_rule(t[GQ + 4], t[GQ + 5], R, C, fs, qR, qC);
        const double qi = i == 0 ? t[GQ] : (i == 1 ? t[GQ + 1] : (i == 2 ? t[GQ + 2] : (i == 3 ? t[GQ + 3] : (i == 4 ? qR : qC))));
        if (threadIdx.x == 0) { esr.sums14[0] = (float)t[0]; esr.sums14[1] = (float)t[1]; }
        if (threadIdx.x < 6) { esr.sums14[2 + threadIdx.x] = (float)gi; esr.sums14[8 + threadIdx.x] = (float)qi; }
        if (esr.gtheta6 == nullptr) return;
        const EsrTerms lt = esr_terms(t[0], t[1] + esr.eps, esr.n_global);
        const double mse = lt.mse, er = lt.esr, ga = lt.ga, gb = lt.gb;
        g = (float)(ga * gi + gb * qi);
        if (threadIdx.x < 6) esr.gtheta6[threadIdx.x] = g;
        if (threadIdx.x == 0 && esr.loss3) { esr.loss3[0] = (float)mse; esr.loss3[1] = (float)er; esr.loss3[2] = (float)(mse + er); }
    }
    if (adam.m == nullptr) return;
    const int n = *adam.step + 1;                                // (one wave: every lane has read it before lane 0 writes)
    if (threadIdx.x == 0) *adam.step = n;
    if (threadIdx.x >= 6) return;
    if (RSEQ && threadIdx.x == 4) return;                        // theta6[4] is not a parameter of this call: never written
    const double c1 = 1.0 - ipow((double)adam.b1, n), c2 = 1.0 - ipow((double)adam.b2, n);
    const float mi = adam.b1 * adam.m[i] + (1.0f - adam.b1) * g;
    const float vi = adam.b2 * adam.v[i] + (1.0f - adam.b2) * g * g;
    adam.m[i] = mi;
    adam.v[i] = vi;
    const float lr_t = (float)((double)adam.lr[i] * sqrt(c2) / c1);
    float th = theta6[i] - lr_t * mi / (sqrtf(vi) + adam.eps);
    if (adam.lo) th = fmaxf(th, adam.lo[i]);
    if (adam.hi) th = fminf(th, adam.hi[i]);
    theta6[i] = th;
}

// (several ranks: sums14 summed over the ranks -> the global loss and gradient: esr_finish_kernel, wdf_esr.h, six entries)

}  // namespace wdf
