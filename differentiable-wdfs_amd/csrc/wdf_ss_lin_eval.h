// wdf_ss_lin_eval.h -- the LOSS-ONLY evaluation pass of LINEAR state-space trees (the validation line of every epoch of lpf.py /
// voltage_divider.py: the model's output and its loss on a set nobody takes a gradient of), gfx950.
//
//     z' = A z + Bx x ;  y = cy . z + dy . x ;  S = sum (y - target)^2 ,  E = sum y^2  on the rows t >= skip
//
// The sibling of wdf_ss_step.h's one-pass training step without everything a gradient needs: no tangents S_c = dz/dc, no
// weighted tangent sums, no Jacobian, no optimizer.  What is left of the joint recursion u = (z, S_A, S_B) is z alone, and the z
// part of the step does not depend on the rest, so every expression below is the step's own, in the step's order: at the same
// chunk count, lane width and alignment y, zT, S, E and the losses are the step's BIT FOR BIT (a validation call and a training
// step that report the same parameters report the same numbers).
//
//   * pass 1 (ss_lin_eval_zero_kernel): every chunk but the last from z = 0 -> zend0 [K][NS][B];
//   * pass 2 (ss_lin_eval_kernel): the wave builds A^L from L homogeneous steps, walks the earlier chunks' ends to its exact
//     start, runs its chunk with the two sums, publishes them behind the step's counted ticket; the last wave adds the partials
//     in wave order and writes the losses.
// 16 B per sample through HBM (x twice, target, y), 12 without y; NS = 0 or one chunk: x once.
#pragma once

#include "wdf_ss_step.h"      // SSCoef, lin_ld / lin_st / lin_st_nt, lin_load_x, lin_load_blk, lin_hsum, LinWidth, wave_sum_dpp, esr_terms

namespace wdf {

// one step of z with input x: lin_u_step's z row
template <int NS, int NI, typename V>
__device__ __forceinline__ void lin_z_step(const SSCoef<NS, NI>& c, const V (&x)[NI], V (&z)[NS > 0 ? NS : 1])
{
    using C = SSCoef<NS, NI>;
    const V zero = vsplat<V>(0.0f);
    V zn[NS > 0 ? NS : 1];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        V a = zero;
#pragma unroll
        for (int i = 0; i < NI; ++i) a = vfma(c.v[C::oB + s * NI + i], x[i], a);
#pragma unroll
        for (int q = 0; q < NS; ++q) a = vfma(c.v[C::oA + s * NS + q], z[q], a);
        zn[s] = a;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) z[s] = zn[s];
}

// ---- pass 1: every chunk from z = 0 -> zend0 [K][NS][B] (not launched when NS = 0 or K = 1) --------------------------------
template <int NS, int NI, typename V>
__global__ __launch_bounds__(64) void ss_lin_eval_zero_kernel(const float* __restrict__ x, const float* __restrict__ coef,
                                                              float* __restrict__ zend0, int64_t B, int64_t T, int64_t L)
{
    constexpr int W = LinWidth<V>::w;
    const int64_t b_raw = ((int64_t)blockIdx.x * 64 + threadIdx.x) * W;
    const int64_t b = b_raw < B ? b_raw : B - W;
    const int64_t k = blockIdx.y, t0 = k * L, t1 = (t0 + L < T) ? t0 + L : T;
    if (t1 == T) return;                                          // (nothing comes after the last chunk)
    SSCoef<NS, NI> c;
    c.load(coef);
    V z[NS > 0 ? NS : 1];
#pragma unroll
    for (int s = 0; s < NS; ++s) z[s] = vsplat<V>(0.0f);
    for (int64_t tb = t0; tb < t1; tb += kLinBlk) {
        const int n = t1 - tb < kLinBlk ? (int)(t1 - tb) : kLinBlk;
        V xs[kLinBlk][NI];
        lin_load_x(x, B, b, tb, n, xs);
#pragma unroll
        for (int i = 0; i < kLinBlk; ++i)
            if (i < n) lin_z_step<NS, NI, V>(c, xs[i], z);
    }
    if (b_raw < B) {
#pragma unroll
        for (int s = 0; s < NS; ++s) lin_st<V>(zend0 + (k * NS + s) * B + b, z[s]);
    }
}

// z <- the exact state at the start of chunk k, from the zero-state chunk ends zend0 [K][NS][B]: lin_walk_to's z part
template <int NS, int NI, typename V>
__device__ __forceinline__ void lin_eval_walk_to(const SSCoef<NS, NI>& c, const float* __restrict__ zend0, int64_t B, int64_t b,
                                                 int64_t k, int64_t L, V (&z)[NS > 0 ? NS : 1])
{
    float AL[NS > 0 ? NS : 1][NS > 0 ? NS : 1];
    const float zero_x[NI] = {};
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        float h[NS > 0 ? NS : 1];
#pragma unroll
        for (int s = 0; s < NS; ++s) h[s] = 0.0f;
        h[j] = 1.0f;
        for (int64_t t = 0; t < L; ++t) lin_z_step<NS, NI, float>(c, zero_x, h);
#pragma unroll
        for (int s = 0; s < NS; ++s) AL[s][j] = h[s];
    }
    V p[NS > 0 ? NS : 1], pn[NS > 0 ? NS : 1], n[NS > 0 ? NS : 1];
#pragma unroll
    for (int s = 0; s < NS; ++s) p[s] = lin_ld<V>(zend0 + s * B + b);
    for (int64_t q = 0; q < k; ++q) {
#pragma unroll
        for (int s = 0; s < NS; ++s) pn[s] = p[s];
        if (q + 1 < k) {                                           // (the next chunk's end is on its way while this one is applied)
#pragma unroll
            for (int s = 0; s < NS; ++s) pn[s] = lin_ld<V>(zend0 + ((q + 1) * NS + s) * B + b);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            V a = p[s];
#pragma unroll
            for (int r = 0; r < NS; ++r) a = vfma(AL[s][r], z[r], a);
            n[s] = a;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            z[s] = n[s];
            p[s] = pn[s];
        }
    }
}

// what the finishing wave needs: the loss's scalars and where the results go (each output may be NULL)
//   sums: double [2] = {S, E} (E without eps); loss3: float [3] = {mse, esr, mse + esr} by esr_terms(S, E + eps, n_global);
//   loss_out: <- (float)(0.5 gscale S), the MSE step's formula.
struct LinEval { int64_t skip; double n_global, eps; float gscale; double* sums; float* loss3; float* loss_out; };

// ---- pass 2: every chunk from its exact start: y (STORE_Y) and the two sums; the last wave finishes -------------------------
// The step's geometry: 64-thread workgroups, blockIdx.y = chunk, dead lanes shadow sequence B - W with weight 0.
// part: double [waves][2] = {S, E}.  ticket: one word, left 0.  z0 / zT: float [NS][B] or NULL, as the step's.
// STORE_Y = false: the one store of y is compiled out and no address is formed from y.
template <int NS, int NI, typename V, bool STORE_Y>
__global__ __launch_bounds__(64) void ss_lin_eval_kernel(const float* __restrict__ x, const float* __restrict__ coef,
                                                         const float* __restrict__ zend0, const float* __restrict__ target,
                                                         float* __restrict__ y, double* __restrict__ part,
                                                         unsigned* __restrict__ ticket, int64_t B, int64_t T, int64_t L,
                                                         const float* __restrict__ z0, float* __restrict__ zT, const LinEval a)
{
    using C = SSCoef<NS, NI>;
    constexpr int W = LinWidth<V>::w;
    const V zero = vsplat<V>(0.0f);
    const int64_t b_raw = ((int64_t)blockIdx.x * 64 + threadIdx.x) * W;
    const bool live = b_raw < B;
    const int64_t b = live ? b_raw : B - W;
    const int64_t k = blockIdx.y, t0 = k * L, t1 = (t0 + L < T) ? t0 + L : T;
    SSCoef<NS, NI> c;
    c.load(coef);
    V z[NS > 0 ? NS : 1];
#pragma unroll
    for (int s = 0; s < NS; ++s) z[s] = zero;
    if (NS > 0 && z0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) z[s] = lin_ld<V>(z0 + s * B + b);
    }
    if (NS > 0 && k > 0) lin_eval_walk_to<NS, NI, V>(c, zend0, B, b, k, L, z);
    const float lv = live ? 1.0f : 0.0f;
    double accS = 0.0, accE = 0.0;
    // 8-step blocks, the next one's loads in flight under this one's arithmetic
    V xn[kLinBlk2][NI], tn[kLinBlk2];
    lin_load_blk<NI, V>(x, target, B, b, t0, t1, xn, tn);
    for (int64_t tb = t0; tb < t1; tb += 32) {                     // fp32 sums within 32 steps, fp64 across
        V fS = zero, fE = zero;
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
                for (int s = 0; s < NS; ++s) yv = vfma(c.v[C::oCy + s], z[s], yv);
                const V e = yv - tg[i];
                if constexpr (STORE_Y) { if (live) lin_st_nt<V>(y + (ts + i) * B + b, yv); }
                // rows before skip: the weights themselves are 0, by a select (ts, i, skip are the same in every lane) -- not
                // 0 x e, which would let a NaN or Inf in a skipped row of target (padding) into a sum
                const bool on = ts + i >= a.skip;
                const V es = on ? e : zero;
                const V w0 = es * lv;
                const V w1 = on ? yv * lv : zero;
                fS = vfma(w0, es, fS);
                fE = vfma(w1, yv, fE);
                lin_z_step<NS, NI, V>(c, xs[i], z);
            }
        }
        accS += lin_hsum(fS);
        accE += lin_hsum(fE);
    }
    if (NS > 0 && zT && t1 == T && live) {                          // the states the call ends in [NS][B] (never the z0 buffer)
#pragma unroll
        for (int s = 0; s < NS; ++s) lin_st<V>(zT + s * B + b, z[s]);
    }
    // ---- this wave's partial; the last wave of the launch (a counted ticket: no wait on anything) adds them up in wave order
    const int64_t wave = (int64_t)blockIdx.y * gridDim.x + blockIdx.x, nwaves = (int64_t)gridDim.x * gridDim.y;
    const double sS = wave_sum_dpp(accS), sE = wave_sum_dpp(accE);
    if (threadIdx.x == 0) {
        __hip_atomic_store(part + wave * 2, sS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part + wave * 2 + 1, sE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned old = 0;
    if (threadIdx.x == 0) old = atomicAdd(ticket, 1u);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != (unsigned)(nwaves - 1)) return;
    if (threadIdx.x == 0) *ticket = 0u;
    double totS = 0.0, totE = 0.0;
    for (int64_t w = threadIdx.x; w < nwaves; w += 64) {
        totS += __hip_atomic_load(part + w * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        totE += __hip_atomic_load(part + w * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const double S = wave_sum_dpp(totS), E = wave_sum_dpp(totE);
    if (threadIdx.x != 0) return;
    if (a.sums) {
        a.sums[0] = S;
        a.sums[1] = E;
    }
    if (a.loss3) {
        const EsrTerms lt = esr_terms(S, E + a.eps, a.n_global);
        a.loss3[0] = (float)lt.mse;
        a.loss3[1] = (float)lt.esr;
        a.loss3[2] = (float)(lt.mse + lt.esr);
    }
    if (a.loss_out) *a.loss_out = (float)(0.5 * (double)a.gscale * S);
}

}  // namespace wdf
