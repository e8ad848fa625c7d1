// wdf_asym_step.h -- the MSE training step of the two-different-diode clipper (wdf_asym.h) in ONE pass over the data:
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
// Precision as the reverse sweep's: partials in fp32 (their inputs are fp32), recurrence and sums in fp64.
// rec: double [K][15][B] = {P, A, S, q[6], beta[6]}.   L and W are multiples of 8.
#pragma once

#include "wdf_asym.h"
#include "wdf_optim.h"

namespace wdf {

constexpr int kAsymStepRec = 15;

// gate == nullptr: the chunked launch, grid = (waves, K); it also clears status and the finish kernel's ticket.
// gate != nullptr: the repair launch, grid = (waves, 1) with L >= T: flagged waves only.
template <int MODE, bool VEC4>
__global__ __launch_bounds__(64) void clipper_asym_step_kernel(const float* __restrict__ x, const float* __restrict__ theta6, float fs,
                                                               const float* __restrict__ target, float* __restrict__ y,
                                                               const float* __restrict__ z0, float* __restrict__ zT,
                                                               float* __restrict__ zwarm, float* __restrict__ zend,
                                                               double* __restrict__ rec, double tol, int max_iter,
                                                               AsymTpStatus* __restrict__ status, unsigned* __restrict__ ticket,
                                                               const unsigned* __restrict__ gate, int64_t B, int64_t T, int64_t L,
                                                               int64_t W)
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
    const AsymConsts c = asym_load(theta6, fs);
    const double p = c.p;
    const float* __restrict__ xp = x + b * T;
    int iters = 0;
    S z = (tw == 0 && z0) ? (S)z0[b] : (S)0;
    double tau[6] = {0, 0, 0, 0, 0, 0}, be[6] = {0, 0, 0, 0, 0, 0};
    double m = 1.0, A = 0.0, sse = 0.0;
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
                }
            }
        }
    }
    zend[k * B + b] = (float)z;
    if (zT && t1 == T) zT[b] = (float)z;
    double* __restrict__ r = rec + (k * kAsymStepRec) * B + b;
    r[0] = m;
    r[B] = A;
    r[2 * B] = sse;
#pragma unroll
    for (int q = 0; q < 6; ++q) { r[(3 + q) * B] = tau[q]; r[(9 + q) * B] = be[q]; }
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

// One lane per sequence: the K records first to last (one record where the wave was repaired), the wave's sums -> part[wave][8]
// = {S, G[6], 0}; the wave that finishes LAST sums the partials in a fixed order (lane i takes waves i, i + 64, ...; then
// the shuffle tree), applies the chain rule Rp, p -> R, C (clipper_asym_grad_reduce_kernel's formulas) and gscale:
// out7 = {sse, d(gscale/2 sse)/d{Is1, V1, Is2, V2, R, C}}; then Adam, if asked for.
static __global__ __launch_bounds__(64) void clipper_asym_step_finish_kernel(const double* __restrict__ rec, const unsigned* __restrict__ gate,
                                                                             double* part, unsigned* ticket, float* theta6, float fs,
                                                                             float gscale, float* __restrict__ out7, AsymStepAdam adam,
                                                                             int64_t B, int64_t K)
{
    const int64_t b_raw = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = b_raw < B;
    const int64_t b = live ? b_raw : B - 1;
    const int64_t kn = (gate != nullptr && gate[blockIdx.x] != 0u) ? 1 : K;
    double tau[6] = {0, 0, 0, 0, 0, 0}, s[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int64_t k = 0; k < kn; ++k) {
        const double* __restrict__ r = rec + (k * kAsymStepRec) * B + b;
        const double P = r[0], A = r[B];
        s[0] += r[2 * B];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            s[1 + q] += fma(A, tau[q], r[(9 + q) * B]);
            tau[q] = fma(P, tau[q], r[(3 + q) * B]);
        }
    }
    const unsigned nwaves = gridDim.x;
    double w[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) w[i] = asym_wave_sum_all(live ? s[i] : 0.0);
    unsigned done = 0;
    if (threadIdx.x == 0) {
        double* o = part + (int64_t)blockIdx.x * 8;
#pragma unroll
        for (int i = 0; i < 7; ++i) __hip_atomic_store(o + i, w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the partial has landed before the count moves
        done = atomicAdd(ticket, 1u);
    }
    done = __builtin_amdgcn_readfirstlane(done);
    if (done != nwaves - 1) return;
    double t[7] = {0, 0, 0, 0, 0, 0, 0};
    for (unsigned i = threadIdx.x; i < nwaves; i += 64)
#pragma unroll
        for (int j = 0; j < 7; ++j) t[j] += __hip_atomic_load(part + (int64_t)i * 8 + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int j = 0; j < 7; ++j) t[j] = asym_wave_sum_all(t[j]);
    // every lane forms the chain rule, lanes 0..5 keep their component
    const double R = theta6[4], C = theta6[5];
    const double G1 = 1.0 / R, G2 = C * (2.0 * (double)fs), Rp = 1.0 / (G1 + G2), p = G1 * Rp;
    const double SRp = t[5], Sp = t[6];
    const double gR = SRp * Rp * Rp * G1 * G1 - Sp * G1 * G1 * Rp * (1.0 - p);
    const double gC = -2.0 * (double)fs * (SRp * Rp * Rp + Sp * p * Rp);
    const int i = threadIdx.x < 6 ? threadIdx.x : 5;
    const double gi = i == 0 ? t[1] : (i == 1 ? t[2] : (i == 2 ? t[3] : (i == 3 ? t[4] : (i == 4 ? gR : gC))));
    const float g = (float)((double)gscale * gi);
    if (threadIdx.x == 0) out7[0] = (float)t[0];
    if (threadIdx.x < 6) out7[1 + threadIdx.x] = g;
    if (adam.m == nullptr) return;
    const int n = *adam.step + 1;                                // (one wave: every lane has read it before lane 0 writes)
    if (threadIdx.x == 0) *adam.step = n;
    if (threadIdx.x >= 6) return;
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

}  // namespace wdf
