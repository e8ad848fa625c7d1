// wdf_ss_lin_gn.h -- the Gauss-Newton form of the one-pass MSE step of LINEAR state-space trees (csrc/wdf_ss_step.h), gfx950.
//
// Pass 2 of the MSE step forms, at every row and from an EXACT chunk start, d_i = dy/d coefficient_i for every entry of
// {A, Bx, cy, dy} (kG of them) and sums g d_i.  The Gauss-Newton matrix of the mean squared error in coefficient space is a
// plain sum beside those:
//
//     Hc_ij = sum_rows d_i d_j ,  i <= j                       (kG (kG + 1) / 2 sums: no record has to compose)
//
// and the chain rule to the component values is the finishing wave's, used twice:  H = gscale J^T Hc J  with the probe's
// float64 Jacobian.  One pass returns {SSE, d(gscale/2 SSE)/d theta, H}: what wdf_hip/lm.py takes.  There is no optimizer here.
//
// Pass 1 is ss_lin_step_zero_kernel, unchanged.  Every expression of the MSE step keeps its place in pass 2 (y, e, SSE, the
// weighted tangent sums, lin_u_step, z0 / zT): y and zT are the MSE step's bits, and so are SSE and the gradient where both ran
// at the same lane width.
#pragma once

#include "wdf_ss_step.h"

namespace wdf {

// Two sequences per lane wherever the MSE step pairs them up, except on the largest tree: (2,2) would hold 78 + 13 sums twice
// over and spill (profiles/lin_gn_resources.txt); it runs one per lane.
template <int NS, int NI> struct LinGnPairs { static constexpr bool ok = !(NS == 2 && NI == 2); };

constexpr int lin_gn_nh(int kG) { return kG * (kG + 1) / 2; }
// entry (i, j), i <= j, of an upper triangle of order n stored by rows
__host__ __device__ constexpr int lin_gn_tri(int n, int i, int j) { return i * n - i * (i - 1) / 2 + (j - i); }

// part: double [waves][kG + 1 + kH] = {gA.., gBx.., gcy.., gdy.., SSE, Hc upper triangle by rows}.
// out: double [1 + P + P (P + 1) / 2] = {SSE, d(gscale/2 SSE)/d param, H upper triangle by rows}, P = n_params;
// loss_out: (or NULL) float <- gscale/2 x SSE; hcoef_out: (or NULL) double [kH], Hc before the Jacobian.
template <int NS, int NI, typename V>
__global__ __launch_bounds__(64) void ss_lin_gn_kernel(const float* __restrict__ x, const float* __restrict__ coef,
                                                       const float* __restrict__ uend0, const float* __restrict__ target,
                                                       float* __restrict__ y, double* __restrict__ part,
                                                       unsigned* __restrict__ ticket, const double* __restrict__ jac, int n_params,
                                                       double* __restrict__ hcoef_out, int64_t B, int64_t T, int64_t L,
                                                       const float* __restrict__ z0, float* __restrict__ zT, float gscale,
                                                       double* __restrict__ out, float* __restrict__ loss_out)
{
    using U = LinU<NS, NI, V>;
    using C = SSCoef<NS, NI>;
    constexpr int W = LinWidth<V>::w;
    constexpr int kG = U::kG, kH = lin_gn_nh(kG), oH = kG + 1, kP = oH + kH;   // accumulators: {G[kG], SSE, Hc[kH]}
    const V zero = vsplat<V>(0.0f);
    const int64_t b_raw = ((int64_t)blockIdx.x * 64 + threadIdx.x) * W;
    const bool live = b_raw < B;
    const int64_t b = live ? b_raw : B - W;
    const int64_t k = blockIdx.y, t0 = k * L, t1 = (t0 + L < T) ? t0 + L : T;
    SSCoef<NS, NI> c;
    c.load(coef);
    U u;
    u.zero();
    if (NS > 0 && z0) {                                           // (a constant of the call: the tangents start at 0)
#pragma unroll
        for (int s = 0; s < NS; ++s) u.z[s] = lin_ld<V>(z0 + s * B + b);
    }
    if (NS > 0 && k > 0) lin_walk_to<NS, NI, V>(c, uend0, B, b, k, L, u);
    const float lv = live ? 1.0f : 0.0f;
    const float gs = live ? gscale : 0.0f;
    double acc[kP];
#pragma unroll
    for (int i = 0; i < kP; ++i) acc[i] = 0.0;
    V xn[kLinBlk2][NI], tn[kLinBlk2];
    lin_load_blk<NI, V>(x, target, B, b, t0, t1, xn, tn);
    for (int64_t tb = t0; tb < t1; tb += 32) {                     // fp32 sums within 32 steps, fp64 across
        V f[kP];
#pragma unroll
        for (int i = 0; i < kP; ++i) f[i] = zero;
#pragma unroll 1
        for (int64_t ts = tb; ts < tb + 32 && ts < t1; ts += kLinBlk2) {
            const int n = t1 - ts < kLinBlk2 ? (int)(t1 - ts) : kLinBlk2;
            V xs[kLinBlk2][NI], tg[kLinBlk2];
#pragma unroll
            for (int i = 0; i < kLinBlk2; ++i) {
                tg[i] = tn[i];
#pragma unroll
                for (int j = 0; j < NI; ++j) xs[i][j] = xn[i][j];
            }
            if (ts + kLinBlk2 < t1) lin_load_blk<NI, V>(x, target, B, b, ts + kLinBlk2, t1, xn, tn);
#pragma unroll
            for (int i = 0; i < kLinBlk2; ++i) {
                if (i >= n) break;
                V yv = zero;
#pragma unroll
                for (int j = 0; j < NI; ++j) yv = vfma(c.v[C::oDy + j], xs[i][j], yv);
#pragma unroll
                for (int s = 0; s < NS; ++s) yv = vfma(c.v[C::oCy + s], u.z[s], yv);
                const V e = yv - tg[i];
                if (live) lin_st_nt<V>(y + (ts + i) * B + b, yv);
                const V w = e * gs;
                f[kG] = vfma(e * lv, e, f[kG]);
                // d[r] = dy/d coefficient r of this row, each formed once: the two inner products with cy, the states, the inputs
                V d[kG];
#pragma unroll
                for (int cc = 0; cc < U::nA; ++cc) {
                    V a = zero;
#pragma unroll
                    for (int s = 0; s < NS; ++s) a = vfma(c.v[C::oCy + s], u.SA[cc][s], a);
                    d[cc] = a;
                }
#pragma unroll
                for (int cc = 0; cc < U::nB; ++cc) {
                    V a = zero;
#pragma unroll
                    for (int s = 0; s < NS; ++s) a = vfma(c.v[C::oCy + s], u.SB[cc][s], a);
                    d[U::nA + cc] = a;
                }
#pragma unroll
                for (int s = 0; s < NS; ++s) d[U::nA + U::nB + s] = u.z[s];
#pragma unroll
                for (int j = 0; j < NI; ++j) d[U::nA + U::nB + NS + j] = xs[i][j];
#pragma unroll
                for (int r = 0; r < kG; ++r) f[r] = vfma(w, d[r], f[r]);
                // Hc: row r of the triangle carries the dead lanes' weight 0 once
#pragma unroll
                for (int r = 0; r < kG; ++r) {
                    const V dl = d[r] * lv;
#pragma unroll
                    for (int q = r; q < kG; ++q) f[oH + lin_gn_tri(kG, r, q)] = vfma(dl, d[q], f[oH + lin_gn_tri(kG, r, q)]);
                }
                lin_u_step<NS, NI, V>(c, xs[i], u);
            }
        }
#pragma unroll
        for (int i = 0; i < kP; ++i) acc[i] += lin_hsum(f[i]);
    }
    if (NS > 0 && zT && t1 == T && live) {                          // the states the call ends in [NS][B] (never the z0 buffer)
#pragma unroll
        for (int s = 0; s < NS; ++s) lin_st<V>(zT + s * B + b, u.z[s]);
    }
    // ---- this wave's partial; the last wave of the launch adds them up in wave order and finishes the step (the MSE step's
    // ticket and order)
    const int64_t wave = (int64_t)blockIdx.y * gridDim.x + blockIdx.x, nwaves = (int64_t)gridDim.x * gridDim.y;
#pragma unroll
    for (int i = 0; i < kP; ++i) {
        const double s = wave_sum_dpp(acc[i]);
        if (threadIdx.x == 0) __hip_atomic_store(part + wave * kP + i, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned old = 0;
    if (threadIdx.x == 0) old = atomicAdd(ticket, 1u);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != (unsigned)(nwaves - 1)) return;
    if (threadIdx.x == 0) *ticket = 0u;
    // the totals cannot be indexed dynamically in registers: they go through LDS, and so does the kG x n_params slice of jac
    __shared__ double s_tot[kP];
    __shared__ double s_jac[kG][kProbeMaxParams];
    const int p = threadIdx.x;
    double gp = 0.0;
    {
        double tot[oH];                                           // {G, SSE}: the MSE step's registers and order
#pragma unroll
        for (int i = 0; i < oH; ++i) tot[i] = 0.0;
        for (int64_t w = threadIdx.x; w < nwaves; w += 64) {
#pragma unroll
            for (int i = 0; i < oH; ++i) tot[i] += __hip_atomic_load(part + w * kP + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int i = 0; i < oH; ++i) tot[i] = wave_sum_dpp(tot[i]);
        if (p < n_params) {
#pragma unroll
            for (int i = 0; i < kG; ++i) {
                const int row = i < U::nA ? C::oA + i : (i < U::nA + U::nB ? C::oB + (i - U::nA)
                                                         : (i < U::nA + U::nB + NS ? C::oCy + (i - U::nA - U::nB) : C::oDy + (i - U::nA - U::nB - NS)));
                const double j = jac[row * n_params + p];
                s_jac[i][p] = j;
                gp += tot[i] * j;
            }
        }
        if (p == 0) s_tot[kG] = tot[kG];
    }
    // Hc: eight entries at a time (a wave's row segment per trip: the loads are in flight together), every entry its waves in order
    constexpr int kSeg = 8;
#pragma unroll 1
    for (int h0 = 0; h0 < kH; h0 += kSeg) {
        double tot[kSeg];
#pragma unroll
        for (int i = 0; i < kSeg; ++i) tot[i] = 0.0;
        for (int64_t w = threadIdx.x; w < nwaves; w += 64) {
#pragma unroll
            for (int i = 0; i < kSeg; ++i)
                if (h0 + i < kH) tot[i] += __hip_atomic_load(part + w * kP + oH + h0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int i = 0; i < kSeg; ++i) {
            const double s = wave_sum_dpp(tot[i]);
            if (p == 0 && h0 + i < kH) s_tot[oH + h0 + i] = s;
        }
    }
    __syncthreads();
    const double sse = s_tot[kG];
    if (p < n_params) out[1 + p] = gp;
    if (p == 0) {
        out[0] = sse;
        if (loss_out) *loss_out = (float)(0.5 * (double)gscale * sse);          // the mean squared error when gscale = 2 / (B T)
    }
    // H_qr = gscale sum_ij jac[row_i][q] Hc_ij jac[row_j][r], q <= r: up to 120 entries, lane by lane and trip by trip
    const int nH = n_params * (n_params + 1) / 2;
    for (int e = p; e < nH; e += 64) {
        int q = 0, rem = e;
        while (rem >= n_params - q) { rem -= n_params - q; ++q; }
        const int r = q + rem;
        double h = 0.0;
        for (int i = 0; i < kG; ++i) {
            double a = 0.0;                                       // (Hc J)_ir
            for (int j = 0; j < kG; ++j) a += s_tot[oH + (i <= j ? lin_gn_tri(kG, i, j) : lin_gn_tri(kG, j, i))] * s_jac[j][r];
            h += s_jac[i][q] * a;
        }
        out[1 + n_params + e] = (double)gscale * h;
    }
    if (hcoef_out) {
        for (int e = p; e < kH; e += 64) hcoef_out[e] = s_tot[oH + e];
    }
}

}  // namespace wdf
