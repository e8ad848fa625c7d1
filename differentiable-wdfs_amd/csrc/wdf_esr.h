// wdf_esr.h -- the scripts' training loss (clipper_pot.py:146-156,177) from its two global sums, once for every kernel family:
//     loss = mse + esr ,  mse = S / n ,  esr = sqrt(S / (E + eps) / n) ,  S = sum (y - target)^2 ,  E = sum y^2
//     dLoss/dy_i = ga (y_i - target_i) + gb y_i ,  ga = 2/n + 1/(esr (E + eps) n) ,  gb = -esr / (E + eps)
// in fp64, in exactly this operation order (the host mirror is dist.esr_coefficients).  An ESR of 0 contributes 0 to ga, not a
// division by zero.  gfx950.
#pragma once

#include <hip/hip_runtime.h>

namespace wdf {

struct EsrTerms { double mse, esr, ga, gb; };

// E_plus_eps: the energy sum with eps already added
__host__ __device__ inline EsrTerms esr_terms(double S, double E_plus_eps, double n)
{
    const double E = E_plus_eps;
    const double mse = S / n, esr = sqrt(S / E / n);
    const double ga = 2.0 / n + (esr > 0.0 ? 1.0 / (esr * E * n) : 0.0), gb = -esr / E;
    return EsrTerms{mse, esr, ga, gb};
}

// Several ranks: sums = {S, E, gP[n_params], gQ[n_params]} summed over the ranks -> the global loss and its gradient
// g = ga gP + gb gQ (the single-rank finishes' formulas, on the floats); loss3: (or NULL) {mse, esr, mse + esr}.
// One wave, lane p owns entry p (n_params <= 64).
static __global__ __launch_bounds__(64) void esr_finish_kernel(const float* __restrict__ sums, int n_params, double n, double eps,
                                                               float* __restrict__ g, float* __restrict__ loss3)
{
    const EsrTerms lt = esr_terms((double)sums[0], (double)sums[1] + eps, n);
    const double ga = lt.ga, gb = lt.gb;
    const int p = threadIdx.x;
    if (p < n_params) g[p] = (float)(ga * (double)sums[2 + p] + gb * (double)sums[2 + n_params + p]);
    if (p == 0 && loss3) { loss3[0] = (float)lt.mse; loss3[1] = (float)lt.esr; loss3[2] = (float)(lt.mse + lt.esr); }
}

}  // namespace wdf
