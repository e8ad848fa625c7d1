// wdf_elementwise.h -- kernels without a time recursion: the MSE + ESR loss sums and coefficients, the weighted loss family
// (MSE, ESR, pre-emphasised ESR, mean),
// and the element-wise Wright omega / diode-pair evaluations the parity tests and the pre-training
// table use.  gfx950.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wdf_omega.h"
#include "wdf_esr.h"

namespace wdf {

// ---- MSE + ESR loss (clipper_pot.py:146-156,177) ---------------------------------------------
// Sums over the samples past skip_samples of one rank's [T][B] arrays: S = sum (y - t)^2 and
// E = sum y^2 (the script passes (outs, target) as (target_y, predicted_y), :248, so the energy is
// the model output's).  Grid-stride, per-block partials in double, fixed-order finish.
static __global__ __launch_bounds__(256) void loss_sums_kernel(const float* __restrict__ y, const float* __restrict__ target,
                                                        int64_t n0, int64_t n1, double* __restrict__ part)
{
    __shared__ double sh[256][2];
    double s = 0.0, e = 0.0;
    for (int64_t i = n0 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n1; i += (int64_t)gridDim.x * 256) {
        const float yv = y[i], d = yv - target[i];
        s += (double)(d * d);
        e += (double)(yv * yv);
    }
    sh[threadIdx.x][0] = s; sh[threadIdx.x][1] = e;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { sh[threadIdx.x][0] += sh[threadIdx.x + off][0]; sh[threadIdx.x][1] += sh[threadIdx.x + off][1]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = sh[0][0]; part[2 * blockIdx.x + 1] = sh[0][1]; }
}

static __global__ __launch_bounds__(256) void loss_sums_finish_kernel(const double* __restrict__ part, int nblk,
                                                               double* __restrict__ sums)
{
    __shared__ double sh[256][2];
    double s = 0.0, e = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) { s += part[2 * i]; e += part[2 * i + 1]; }
    sh[threadIdx.x][0] = s; sh[threadIdx.x][1] = e;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { sh[threadIdx.x][0] += sh[threadIdx.x + off][0]; sh[threadIdx.x][1] += sh[threadIdx.x + off][1]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { sums[0] = sh[0][0]; sums[1] = sh[0][1]; }
}

// From the (global) sums: the loss and the coefficients of its derivative w.r.t. y, dL/dy_i = ga (y_i - t_i) + gb y_i
// (esr_terms, wdf_esr.h).
static __global__ void esr_coef_kernel(const double* __restrict__ sums, double n, double eps, float* __restrict__ gcoef,
                                float* __restrict__ loss)
{
    const EsrTerms lt = esr_terms(sums[0], sums[1] + eps, n);
    gcoef[0] = (float)lt.ga;
    gcoef[1] = (float)lt.gb;
    loss[0] = (float)lt.mse; loss[1] = (float)lt.esr; loss[2] = (float)(lt.mse + lt.esr);
}

// dL/dy [T][B] of that loss for a reverse sweep that takes an upstream gradient (the MLP-root sweep): zero before
// skip, ga (y - t) + gb y after, with {ga, gb} read from the device (esr_coef_kernel's output).
static __global__ __launch_bounds__(256) void loss_esr_grad_kernel(const float* __restrict__ y, const float* __restrict__ target,
                                                                   const float* __restrict__ gcoef, int64_t n0, int64_t n1,
                                                                   float* __restrict__ gy)
{
    const float ga = gcoef[0], gb = gcoef[1];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n1; i += (int64_t)gridDim.x * 256) {
        const float yv = y[i];
        gy[i] = i < n0 ? 0.0f : fmaf(ga, yv - target[i], gb * yv);
    }
}

// ---- the weighted loss family: MSE, ESR, pre-emphasised ESR, mean (clipper_pot.py:141-165) ------------------------------
// loss = w_mse S/n + w_esr sqrt(S/(E+eps)/n) + w_emph sqrt(Sp/(Ep+eps)/n) + w_avg |So - St|/n over the rows past skip of one
// rank's [T][B] arrays, o = y[skip:], t = target[skip:]:  S = sum (o-t)^2, E = sum o^2, So = sum o, St = sum t, and Sp, Ep the
// same two sums behind the pre-emphasis filter f(v)[0] = v[0], f(v)[k] = v[k] - c v[k-1] along TIME inside the kept rows (the
// previous row of [T][B] is the same lane B elements back, so every access is a row access).  (outs, target) are passed as
// (target_y, predicted_y) as for the MSE + ESR loss above: both energies are the model output's.
//
// One kept element's six addends: e, ep = fmaf(-c, e_prev, e), op and the squares in fp32 (as loss_sums_kernel forms d * d),
// accumulated in double.  A first kept row passes a zero previous row: fmaf(-c, 0, e) is e.
static __device__ __forceinline__ void loss_terms_acc(double (&a)[6], float yv, float tv, float yp, float tp, float c)
{
    const float e = yv - tv, ep = fmaf(-c, yp - tp, e), op = fmaf(-c, yp, yv);
    a[0] += (double)(e * e);
    a[1] += (double)(yv * yv);
    a[2] += (double)(ep * ep);
    a[3] += (double)(op * op);
    a[4] += (double)yv;
    a[5] += (double)tv;
}

// Block sum of six doubles per thread in fixed order -> out[6] (thread 0 writes).
static __device__ __forceinline__ void loss_terms_block_sum(const double (&a)[6], double* __restrict__ out)
{
    __shared__ double sh[256][6];
    for (int k = 0; k < 6; ++k) sh[threadIdx.x][k] = a[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            for (int k = 0; k < 6; ++k) sh[threadIdx.x][k] += sh[threadIdx.x + off][k];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; ++k) out[k] = sh[0][k];
}

// Grid-stride over the kept elements n0 .. n1-1, per-block partials part[block][6].  VEC: B % 4 == 0 and both pointers 16-byte
// aligned (the host checks), so n0, n1 and every i - B are multiples of 4 and a lane takes four elements per 16-byte load.
template <bool VEC>
static __global__ __launch_bounds__(256) void loss_terms_sums_kernel(const float* __restrict__ y, const float* __restrict__ target,
                                                                     int64_t n0, int64_t n1, int64_t B, float c,
                                                                     double* __restrict__ part)
{
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if constexpr (VEC) {
        const int64_t ng = (n1 - n0) >> 2;
        for (int64_t g = first; g < ng; g += stride) {
            const int64_t i = n0 + 4 * g;
            const float4 yv = *reinterpret_cast<const float4*>(y + i), tv = *reinterpret_cast<const float4*>(target + i);
            float4 yp = make_float4(0.0f, 0.0f, 0.0f, 0.0f), tp = yp;
            if (i - B >= n0) {
                yp = *reinterpret_cast<const float4*>(y + (i - B));
                tp = *reinterpret_cast<const float4*>(target + (i - B));
            }
            loss_terms_acc(a, yv.x, tv.x, yp.x, tp.x, c);
            loss_terms_acc(a, yv.y, tv.y, yp.y, tp.y, c);
            loss_terms_acc(a, yv.z, tv.z, yp.z, tp.z, c);
            loss_terms_acc(a, yv.w, tv.w, yp.w, tp.w, c);
        }
    } else {
        for (int64_t i = n0 + first; i < n1; i += stride) {
            const bool prev = i - B >= n0;
            loss_terms_acc(a, y[i], target[i], prev ? y[i - B] : 0.0f, prev ? target[i - B] : 0.0f, c);
        }
    }
    loss_terms_block_sum(a, part + 6 * (int64_t)blockIdx.x);
}

static __global__ __launch_bounds__(256) void loss_terms_finish_kernel(const double* __restrict__ part, int nblk,
                                                                       double* __restrict__ sums6)
{
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += 256)
        for (int k = 0; k < 6; ++k) a[k] += part[6 * i + k];
    loss_terms_block_sum(a, sums6);
}

// From the (global) sums6 = {S, E, Sp, Ep, So, St}, all in fp64: terms[5] = {mse, esr, esr_emph, avg, loss} and the
// coefficients of
//   dL/dy[k] = ga e[k] + gb o[k] + al (ep[k] - c ep[k+1]) + be (op[k] - c op[k+1]) + gm ,   u[T'] := 0 ,
//   ga = w_mse 2/n + w_esr / (esr (E+eps) n) ,  gb = -w_esr esr / (E+eps) ,
//   al = w_emph / (esr_emph (Ep+eps) n) ,       be = -w_emph esr_emph / (Ep+eps) ,   gm = w_avg sign(So - St) / n
// as gcoef[6] = {ga, gb, al, be, gm, c}.  An ESR that is 0 contributes 0 (esr_coef_kernel's rule); sign(0) = 0.
struct LossWeights { double mse, esr, emph, avg; };

static __global__ void loss_terms_coef_kernel(const double* __restrict__ sums6, double n, double eps, LossWeights w, double c,
                                              float* __restrict__ gcoef, float* __restrict__ terms)
{
    const double S = sums6[0], E = sums6[1] + eps, Sp = sums6[2], Ep = sums6[3] + eps, d = sums6[4] - sums6[5];
    const double mse = S / n, esr = sqrt(S / E / n), emph = sqrt(Sp / Ep / n), avg = fabs(d) / n;
    gcoef[0] = (float)(w.mse * 2.0 / n + (esr > 0.0 ? w.esr / (esr * E * n) : 0.0));
    gcoef[1] = (float)(-w.esr * esr / E);
    gcoef[2] = (float)(emph > 0.0 ? w.emph / (emph * Ep * n) : 0.0);
    gcoef[3] = (float)(-w.emph * emph / Ep);
    gcoef[4] = (float)(w.avg * (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0)) / n);
    gcoef[5] = (float)c;
    terms[0] = (float)mse; terms[1] = (float)esr; terms[2] = (float)emph; terms[3] = (float)avg;
    terms[4] = (float)(w.mse * mse + w.esr * esr + w.emph * emph + w.avg * avg);
}

// One element of dL/dy from its own, the previous and the next kept row (zeros where there is none; `next` says whether the
// next row exists: u[T'] := 0 drops ep[k+1] and op[k+1] whole, not only their next-row part).  Differences and filter in fp64
// from the fp32 data -- y - t and e - c e_prev are then exact up to fp64 rounding, so where e[k] ~ c e[k-1] cancels the result
// still carries the rounding of the five fp32 coefficients only -- with c the caller's double (gcoef[5] is its fp32 copy).
static __device__ __forceinline__ float loss_terms_gy(float yv, float tv, float yp, float tp, float yn, float tn, bool next,
                                                      double ga, double gb, double al, double be, double gm, double c)
{
    const double o = (double)yv, e = o - (double)tv, em = (double)yp - (double)tp;
    double fe = e - c * em, fo = o - c * (double)yp;
    if (next) {
        fe -= c * (((double)yn - (double)tn) - c * e);
        fo -= c * ((double)yn - c * o);
    }
    return (float)(ga * e + gb * o + al * fe + be * fo + gm);
}

// gy [T][B]: exactly 0 on the rows before skip (i < n0), the expression above after.  VEC as in loss_terms_sums_kernel, gy
// 16-byte aligned too.
template <bool VEC>
static __global__ __launch_bounds__(256) void loss_terms_grad_kernel(const float* __restrict__ y, const float* __restrict__ target,
                                                                     const float* __restrict__ gcoef, double c, int64_t n0,
                                                                     int64_t n1, int64_t B, float* __restrict__ gy)
{
    const double ga = gcoef[0], gb = gcoef[1], al = gcoef[2], be = gcoef[3], gm = gcoef[4];
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if constexpr (VEC) {
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int64_t i = 4 * first; i < n1; i += 4 * stride) {
            float4 g = zero;
            if (i >= n0) {
                const float4 yv = *reinterpret_cast<const float4*>(y + i), tv = *reinterpret_cast<const float4*>(target + i);
                float4 yp = zero, tp = zero, yn = zero, tn = zero;
                const bool next = i + B < n1;
                if (i - B >= n0) {
                    yp = *reinterpret_cast<const float4*>(y + (i - B));
                    tp = *reinterpret_cast<const float4*>(target + (i - B));
                }
                if (next) {
                    yn = *reinterpret_cast<const float4*>(y + (i + B));
                    tn = *reinterpret_cast<const float4*>(target + (i + B));
                }
                g.x = loss_terms_gy(yv.x, tv.x, yp.x, tp.x, yn.x, tn.x, next, ga, gb, al, be, gm, c);
                g.y = loss_terms_gy(yv.y, tv.y, yp.y, tp.y, yn.y, tn.y, next, ga, gb, al, be, gm, c);
                g.z = loss_terms_gy(yv.z, tv.z, yp.z, tp.z, yn.z, tn.z, next, ga, gb, al, be, gm, c);
                g.w = loss_terms_gy(yv.w, tv.w, yp.w, tp.w, yn.w, tn.w, next, ga, gb, al, be, gm, c);
            }
            *reinterpret_cast<float4*>(gy + i) = g;
        }
    } else {
        for (int64_t i = first; i < n1; i += stride) {
            float g = 0.0f;
            if (i >= n0) {
                const bool prev = i - B >= n0, next = i + B < n1;
                g = loss_terms_gy(y[i], target[i], prev ? y[i - B] : 0.0f, prev ? target[i - B] : 0.0f, next ? y[i + B] : 0.0f,
                                  next ? target[i + B] : 0.0f, next, ga, gb, al, be, gm, c);
            }
            gy[i] = g;
        }
    }
}

// ---- element-wise building blocks (parity tests) ----------------------------------------
static __global__ void omega_kernel(const float* __restrict__ x, float* __restrict__ w, int32_t* __restrict__ iters, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float xi = x[i < n ? i : n - 1];
    int it = 0;
    const float wi = wright_omega<true>(xi, &it);
    if (i < n) { w[i] = wi; if (iters) iters[i] = it; }
}

static __global__ void diode_pair_kernel(const float* __restrict__ a, const float* __restrict__ Rp, float Is, float nVt,
                                  int n_up, int n_down, float* __restrict__ b, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t j = i < n ? i : n - 1;
    const DiodeStatic d = make_diode_static(nVt, n_up, n_down);
    const float L = logf(Rp[j] * Is / nVt);
    const DiodeOut o = diode_pair<false, float>(a[j], L, d);
    if (i < n) b[i] = o.b;
}

}  // namespace wdf
