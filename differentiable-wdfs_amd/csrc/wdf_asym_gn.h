// wdf_asym_gn.h -- the Gauss-Newton form of the one-pass MSE step of the two-different-diode clipper (wdf_asym_step.h): the same
// pass over the data -- x and the target read once, y written once, warm-up, zwarm / zend, the gated repair launch, every
// expression of the MSE step in its order -- and, next to S = sum e^2 and G_i = sum e dy_i, the Gauss-Newton matrix
//     H_qr = sum_t dy_q(t) dy_r(t)          (q <= r: 21 values)
// from the tangents the step already holds in registers at every sample.  No second sweep, no stored Jacobian.  A
// Levenberg-Marquardt optimizer on the host (lib/wdf_hip/lm.py) moves the parameters: there is no Adam in this launch.
//
// A chunk runs with zero entering tangent (tau0), m the running product of kappa.  With
//     u_q = (tau0_q' + tau0_q) / 2     dy_q for a zero entering tangent
//     w   = (m' + m) / 2
// the output's tangent for an entering tangent tau_in is  dy_q(t) = w_t tau_in,q + u_q(t)  -- the same kappa for all six
// parameters -- so the product dy_q dy_r expands into four sums that do not depend on tau_in.  Next to the MSE step's
// {P, A, S, q[6], beta[6]} a chunk records, in fp64,
//     M2 = sum w^2      N_q = sum w u_q (6)      H0_qr = sum u_q u_r (q <= r: 21)
// rec: double [K][43][B] = {P, A, S, q[6], beta[6], M2, N[6], H0[21]}; rows 0..14 are the MSE step's.
//
// clipper_asym_gn_finish_kernel walks a sequence's records first to last (tau = 0 enters chunk 0; one record where the wave
// was repaired):
//     G_q  += A tau_q + beta_q
//     H_qr += M2 tau_q tau_r + tau_q N_r + tau_r N_q + H0_qr
//     tau_q <- P tau_q + q_q
// exact: no truncation.  Per-wave partials {S, G[6], H[21]} (28 doubles), the MSE finish's counted ticket and fixed summation
// order; the last wave applies the chain rule {Rp, p} -> {R, C} to G (asym_step_chain_rule) and to H as C^T H C with the same
// 6 x 6 Jacobian C (identity on the four diode entries, asym_step_chain_rule's four partials elsewhere) and writes
//     out28 = {sse, gscale G[6], gscale H[21]}     H: the upper triangle, row-major, in theta order
// With gscale = 2 / (B T): the gradient of the mean squared error and (2/n) J^T J.
// L and W are multiples of 8.  Both Newton modes; no per-sequence pot.
#pragma once

#include "wdf_asym_step.h"

namespace wdf {

constexpr int kAsymGnTri = 21;                   // the upper triangle of a 6 x 6 matrix
constexpr int kAsymGnRec = kAsymStepRec + 1 + 6 + kAsymGnTri;      // 43
constexpr int kAsymGnPart = 1 + 6 + kAsymGnTri;  // doubles per wave partial and floats of out28: {S, G[6], H[21]}

// row-major index of (q, r), q <= r, in the upper triangle
__host__ __device__ constexpr int asym_gn_tri(int q, int r) { return q * 6 - q * (q - 1) / 2 + (r - q); }

// gate == nullptr: the chunked launch, grid = (waves, K); it also clears status and the finish kernel's ticket.
// gate != nullptr: the repair launch, grid = (waves, 1) with L >= T: flagged waves only.
template <int MODE, bool VEC4>
__global__ __launch_bounds__(64) void clipper_asym_gn_kernel(const float* __restrict__ x, const float* __restrict__ theta6, float fs,
                                                             const float* __restrict__ target, float* __restrict__ y,
                                                             const float* __restrict__ z0, float* __restrict__ zT,
                                                             float* __restrict__ zwarm, float* __restrict__ zend,
                                                             double* __restrict__ rec, double tol, int max_iter,
                                                             AsymTpStatus* __restrict__ status, unsigned* __restrict__ ticket,
                                                             const unsigned* __restrict__ gate, int64_t B, int64_t T, int64_t L, int64_t W)
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
    double M2 = 0.0, N[6] = {0, 0, 0, 0, 0, 0}, H0[kAsymGnTri] = {};
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
                    double u[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        const double t_new = fma(kap, tau[q], cth[q]);
                        const double dy2 = t_new + tau[q];
                        be[q] = fma(eh, dy2, be[q]);
                        u[q] = 0.5 * dy2;
                        tau[q] = t_new;
                    }
                    const double m_new = kap * m, dm2 = m_new + m;
                    A = fma(eh, dm2, A);
                    m = m_new;
                    const double w = 0.5 * dm2;
                    M2 = fma(w, w, M2);
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        N[q] = fma(w, u[q], N[q]);
#pragma unroll
                        for (int r = q; r < 6; ++r) H0[asym_gn_tri(q, r)] = fma(u[q], u[r], H0[asym_gn_tri(q, r)]);
                    }
                }
            }
        }
    }
    zend[k * B + b] = (float)z;
    if (zT && t1 == T) zT[b] = (float)z;
    double* __restrict__ r = rec + (k * kAsymGnRec) * B + b;
    r[0] = m;
    r[B] = A;
    r[2 * B] = sse;
#pragma unroll
    for (int q = 0; q < 6; ++q) { r[(3 + q) * B] = tau[q]; r[(9 + q) * B] = be[q]; r[(16 + q) * B] = N[q]; }
    r[15 * B] = M2;
#pragma unroll
    for (int j = 0; j < kAsymGnTri; ++j) r[(22 + j) * B] = H0[j];
}

// One lane per sequence: the K records first to last (one record where the wave was repaired), the wave's sums ->
// part[wave][28] = {S, G[6], H[21]}; the wave that finishes LAST sums the partials in a fixed order (lane i takes waves i,
// i + 64, ...; then the shuffle tree), applies the chain rule Rp, p -> R, C to G and, as C^T H C, to H, and lane 0 writes
// out28 = {sse, gscale G, gscale H}.
__global__ __launch_bounds__(64) void clipper_asym_gn_finish_kernel(const double* __restrict__ rec, const unsigned* __restrict__ gate,
                                                                    double* part, unsigned* ticket, const float* __restrict__ theta6,
                                                                    float fs, float gscale, float* __restrict__ out28, int64_t B,
                                                                    int64_t K)
{
    constexpr int NS = kAsymGnPart, GP = 1, HP = 7;
    const int64_t b_raw = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = b_raw < B;
    const int64_t b = live ? b_raw : B - 1;
    const int64_t kn = (gate != nullptr && gate[blockIdx.x] != 0u) ? 1 : K;
    double tau[6] = {0, 0, 0, 0, 0, 0}, s[NS] = {};
    for (int64_t k = 0; k < kn; ++k) {
        const double* __restrict__ r = rec + (k * kAsymGnRec) * B + b;
        const double P = r[0], A = r[B], M2 = r[15 * B];
        s[0] += r[2 * B];
        double N[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) N[q] = r[(16 + q) * B];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
#pragma unroll
            for (int j = q; j < 6; ++j) {
                const double cross = fma(tau[q], N[j], tau[j] * N[q]);
                s[HP + asym_gn_tri(q, j)] += fma(M2 * tau[q], tau[j], cross) + r[(22 + asym_gn_tri(q, j)) * B];
            }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            s[GP + q] += fma(A, tau[q], r[(9 + q) * B]);
            tau[q] = fma(P, tau[q], r[(3 + q) * B]);
        }
    }
    const unsigned nwaves = gridDim.x;
    double w[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) w[i] = asym_wave_sum_all(live ? s[i] : 0.0);
    unsigned done = 0;
    if (threadIdx.x == 0) {
        double* o = part + (int64_t)blockIdx.x * NS;
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
        for (int j = 0; j < NS; ++j) t[j] += __hip_atomic_load(part + (int64_t)i * NS + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int j = 0; j < NS; ++j) t[j] = asym_wave_sum_all(t[j]);
    // every lane forms the chain rule, lane 0 writes
    const double R = theta6[4], C = theta6[5];
    double gR, gC;
    asym_step_chain_rule(t[GP + 4], t[GP + 5], R, C, fs, gR, gC);
    // the Jacobian's lower right block from the same function: J44 = dRp/dR, J54 = dp/dR, J45 = dRp/dC, J55 = dp/dC
    double J44, J45, J54, J55;
    asym_step_chain_rule(1.0, 0.0, R, C, fs, J44, J45);
    asym_step_chain_rule(0.0, 1.0, R, C, fs, J54, J55);
    double Ht[kAsymGnTri];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int j = q; j < 4; ++j) Ht[asym_gn_tri(q, j)] = t[HP + asym_gn_tri(q, j)];
        const double h4 = t[HP + asym_gn_tri(q, 4)], h5 = t[HP + asym_gn_tri(q, 5)];
        Ht[asym_gn_tri(q, 4)] = h4 * J44 + h5 * J54;
        Ht[asym_gn_tri(q, 5)] = h4 * J45 + h5 * J55;
    }
    {
        const double h44 = t[HP + asym_gn_tri(4, 4)], h45 = t[HP + asym_gn_tri(4, 5)], h55 = t[HP + asym_gn_tri(5, 5)];
        const double a4 = h44 * J44 + h45 * J54, a5 = h45 * J44 + h55 * J54;      // (H J)[4..5][4]
        const double c4 = h44 * J45 + h45 * J55, c5 = h45 * J45 + h55 * J55;      // (H J)[4..5][5]
        Ht[asym_gn_tri(4, 4)] = J44 * a4 + J54 * a5;
        Ht[asym_gn_tri(4, 5)] = J44 * c4 + J54 * c5;
        Ht[asym_gn_tri(5, 5)] = J45 * c4 + J55 * c5;
    }
    if (threadIdx.x != 0) return;
    const double gs = (double)gscale;
    out28[0] = (float)t[0];
#pragma unroll
    for (int q = 0; q < 4; ++q) out28[1 + q] = (float)(gs * t[GP + q]);
    out28[5] = (float)(gs * gR);
    out28[6] = (float)(gs * gC);
#pragma unroll
    for (int j = 0; j < kAsymGnTri; ++j) out28[HP + j] = (float)(gs * Ht[j]);
}

}  // namespace wdf
