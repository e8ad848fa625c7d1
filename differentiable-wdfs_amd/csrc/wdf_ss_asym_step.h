// wdf_ss_asym_step.h -- the one-pass training step of small state-space trees whose root is a pair of two DIFFERENT diodes
// (root kind kRootAsym of wdf_statespace.h: the exact Shockley pair of wdf_asym.h, solved by Newton in fp32 at every step):
// forward, loss and the gradient of every coefficient and of the root's five values in ONE sweep over the data -- x and the
// target read once, y written once, no state stash, one root solve per sample -- for the MSE loss (LOSS = 0) and for the
// scripts' MSE + ESR loss on the rows t >= skip (LOSS = 1).
//
//   a = ca.z + da.x      (b, v, e1, e2) = asym_newton32_solve(a)      y = fy b + cy.z + dy.x      z' = A z + Bx x + E b
//
// Tangents: wdf_ss_nl_step.h's construction (nl_step) with five root tangents where it has two.  With Da = db/da and
// cf = db/d{Is_up, nVt_up, Is_down, nVt_down, R_port} from asym_newton_partials at the root the step just solved, and
// M = A + E (Da ca)^T, every tangent S_c = dz/d theta_c (theta: the entries of A, Bx, E, ca, da, then the five root values)
// does   S_c' = M S_c + E beta_c + direct   and   G_c += gw.S_c + gf beta_c,   gw = g (cy + fy Da ca), gf = g fy,
// beta = Da z_s for ca_s, Da x_i for da_i, cf[i] for the root's own values (the values themselves: no L, V re-parametrisation),
// direct = z_j / x_j / b into row i for A_ij / Bx_ij / E_i.  cy, dy, fy enter y only: G += g {z, x, b}.
// LOSS = 0: g = e = y - target (the finish launch scales the sums by gscale).  LOSS = 1: two families, P with weight e and Q
// with weight y, next to S = sum e^2 and E = sum y^2; a row before skip has weight 0 in every sum (t is the same for a whole
// wave: a scalar select), while state, tangents, Psi and y advance over it as over any row.
//
// Time chunks follow wdf_asym_step.h's model.  Grid = (waves, K).  Chunk 0 starts from z0 (or 0) with zero tangent (z0 is a
// constant of the call); chunk k > 0 starts W steps early from z = 0 and runs the state only.  The tangents' recursion is
// linear given the state trajectory, S_t = S0_t + Psi_t S_start, so a chunk runs from S = 0, carries Psi (P[j] = Psi e_j)
// and H = sum gw Psi (HQ for the Q family) and records per sequence {z arriving, z_end, Psi_end, S0_end, H (, HQ)} and, per
// wave, its own sums.  ss_tp_verify_kernel (wdf_statespace.h) compares the boundaries at tol per state and fills the same status
// words as the chunked forward; a wave with a missed boundary is re-run by a gated launch of the SAME kernel as one chunk,
// whose record (slot 0) replaces the wave's K records: a wrong start state never reaches y, the loss or the gradient.
// ss_asym_step_finish_kernel walks a sequence's records in time order in double -- G += H.S_start, S_start <- Psi_end
// S_start + S0_end -- sums per wave, and the wave that finishes last (a counted ticket, no spin) adds the waves in index order.
//
// Precision: state and tangents fp32; sums leave fp32 for double every 32 steps; everything composed across chunks is double.
// One lane per sequence.  The solver's stop rule is a wavefront ballot: dead lanes shadow sequence B - 1 and waves leave whole.
// zwarm / zend [K][NS][B] float; rec [K][nRec][B] float; gpart [K][waves][nAcc] double; part [waves][nAcc] double.
#pragma once

#include "wdf_statespace.h"

namespace wdf {

template <int NS, int NI, int LOSS = 0>
struct AsStepDims {
    using C = SSCoef<NS, NI>;
    static constexpr int nT = C::oCy + 5;                        // tangents: A, Bx, E, ca, da entries, then the root's five values
    static constexpr int nG = C::kN + 5;                         // gradient entries: every coefficient, then the root's five
    static constexpr int oPsi = 0, oS = NS * NS, oH = oS + nT * NS, oHQ = oH + NS;
    static constexpr int nRec = oH + NS + (LOSS ? NS : 0);       // Psi_end, S0_end, H (, HQ)
    static constexpr int nQ = LOSS ? nG : 1, nHQ = LOSS ? NS : 1;
    static constexpr int nAcc = LOSS ? 2 * nG + 2 : nG + 1;      // {GP[nG], S} (, GQ[nG], E)
    static constexpr int oQ = nG + 1;
    __host__ __device__ static constexpr int gidx(int c) { return c < C::oCy ? c : C::kN + (c - C::oCy); }
};

struct SsAsymStepArgs {
    const float* x;            // [B][T][NI]
    const float* coef;         // SSCoef order
    const float* rootp;        // {Is_up, nVt_up, Is_down, nVt_down, R_port}
    const float* target;       // [T][B]
    float* y;                  // [T][B]
    const float* z0;           // [NS][B] or null
    float* zT;                 // [NS][B] or null
    float* zwarm;              // [K][NS][B]
    float* zend;               // [K][NS][B]
    float* rec;                // [K][nRec][B]
    double* gpart;             // [K][waves][nAcc]
    SsTpStatus* status;
    unsigned* ticket;
    const unsigned* gate;      // null: the chunked launch; else the repair launch (one chunk, flagged waves only)
    int64_t B, T, L, W, skip;
};

// one owned step: y; state, tangents, Psi and the fp32 sums advance.  on: the row's weight (LOSS = 1: 0 before skip).
template <int NS, int NI, int LOSS>
__device__ __forceinline__ float ss_asym_step_one(const SSCoef<NS, NI>& c, const SSAsym& dp, const float (&x)[NI], float tgt, float on,
                                                  float (&z)[NS], float (&S)[AsStepDims<NS, NI>::nT][NS], float (&P)[NS][NS],
                                                  float (&G)[AsStepDims<NS, NI>::nG], float (&H)[NS], float& sse,
                                                  float (&GQ)[AsStepDims<NS, NI, LOSS>::nQ], float (&HQ)[AsStepDims<NS, NI, LOSS>::nHQ],
                                                  float& see)
{
    using C = SSCoef<NS, NI>;
    float a = 0.0f;
#pragma unroll
    for (int s = 0; s < NS; ++s) a = fmaf(c.v[C::oCa + s], z[s], a);
#pragma unroll
    for (int i = 0; i < NI; ++i) a = fmaf(c.v[C::oDa + i], x[i], a);
    int iters = 0;
    float v, e1, e2, Da, cf[5];
    const float b = asym_newton32_solve(dp.c, a, kSsAsymTol, kSsAsymMaxIter, iters, v, e1, e2);
    asym_newton_partials(dp.c, v, e1, e2, Da, cf);
    float yv = c.v[C::oFy] * b;
#pragma unroll
    for (int s = 0; s < NS; ++s) yv = fmaf(c.v[C::oCy + s], z[s], yv);
#pragma unroll
    for (int i = 0; i < NI; ++i) yv = fmaf(c.v[C::oDy + i], x[i], yv);
    const float e = yv - tgt;
    const float g = LOSS ? e * on : e;
    sse = fmaf(g, e, sse);
    const float gf = g * c.v[C::oFy];
    float gq = 0.0f, gfq = 0.0f, gwq[NS];
    if constexpr (LOSS != 0) {
        gq = yv * on;
        gfq = gq * c.v[C::oFy];
        see = fmaf(gq, yv, see);
    }
    // M = A + E (Da ca)^T: the step's Jacobian; gw = g (cy + fy Da ca): dLoss/dz through y
    float M[NS][NS], gw[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const float dq = Da * c.v[C::oCa + q];
        gw[q] = fmaf(gf, dq, g * c.v[C::oCy + q]);
        if constexpr (LOSS != 0) gwq[q] = fmaf(gfq, dq, gq * c.v[C::oCy + q]);
#pragma unroll
        for (int s = 0; s < NS; ++s) M[s][q] = fmaf(dq, c.v[C::oE + s], c.v[C::oA + s * NS + q]);
    }
    // every tangent: G += gw.S + gf beta;  S' = M S + E beta + direct
    auto advance = [&](float (&Sc)[NS], float& Gc, float& Qc, float beta, bool has_beta, int di, float dv) {
        float acc = Gc;
#pragma unroll
        for (int s = 0; s < NS; ++s) acc = fmaf(gw[s], Sc[s], acc);
        if (has_beta) acc = fmaf(gf, beta, acc);
        Gc = acc;
        if constexpr (LOSS != 0) {
            float aq = Qc;
#pragma unroll
            for (int s = 0; s < NS; ++s) aq = fmaf(gwq[s], Sc[s], aq);
            if (has_beta) aq = fmaf(gfq, beta, aq);
            Qc = aq;
        }
        float sn[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float w = (s == di) ? dv : 0.0f;
            if (has_beta) w = fmaf(beta, c.v[C::oE + s], w);
#pragma unroll
            for (int q = 0; q < NS; ++q) w = fmaf(M[s][q], Sc[q], w);
            sn[s] = w;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) Sc[s] = sn[s];
    };
    auto Q = [&](int i) -> float& { return GQ[LOSS ? i : 0]; };  // (the Q accumulator beside G[i]; a placeholder without the family)
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j) advance(S[C::oA + i * NS + j], G[C::oA + i * NS + j], Q(C::oA + i * NS + j), 0.0f, false, i, z[j]);
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) advance(S[C::oB + i * NI + j], G[C::oB + i * NI + j], Q(C::oB + i * NI + j), 0.0f, false, i, x[j]);
#pragma unroll
    for (int i = 0; i < NS; ++i) advance(S[C::oE + i], G[C::oE + i], Q(C::oE + i), 0.0f, false, i, b);
#pragma unroll
    for (int s = 0; s < NS; ++s) advance(S[C::oCa + s], G[C::oCa + s], Q(C::oCa + s), Da * z[s], true, -1, 0.0f);
#pragma unroll
    for (int i = 0; i < NI; ++i) advance(S[C::oDa + i], G[C::oDa + i], Q(C::oDa + i), Da * x[i], true, -1, 0.0f);
#pragma unroll
    for (int r = 0; r < 5; ++r) advance(S[C::oCy + r], G[C::kN + r], Q(C::kN + r), cf[r], true, -1, 0.0f);
#pragma unroll
    for (int j = 0; j < NS; ++j) advance(P[j], H[j], HQ[LOSS ? j : 0], 0.0f, false, -1, 0.0f);
    // the coefficients y sees directly
#pragma unroll
    for (int s = 0; s < NS; ++s) G[C::oCy + s] = fmaf(g, z[s], G[C::oCy + s]);
#pragma unroll
    for (int i = 0; i < NI; ++i) G[C::oDy + i] = fmaf(g, x[i], G[C::oDy + i]);
    G[C::oFy] = fmaf(g, b, G[C::oFy]);
    if constexpr (LOSS != 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) GQ[C::oCy + s] = fmaf(gq, z[s], GQ[C::oCy + s]);
#pragma unroll
        for (int i = 0; i < NI; ++i) GQ[C::oDy + i] = fmaf(gq, x[i], GQ[C::oDy + i]);
        GQ[C::oFy] = fmaf(gq, b, GQ[C::oFy]);
    }
    // the state (ss_fwd_step's order of operations)
    float zn[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float w = c.v[C::oE + s] * b;
#pragma unroll
        for (int q = 0; q < NS; ++q) w = fmaf(c.v[C::oA + s * NS + q], z[q], w);
#pragma unroll
        for (int i = 0; i < NI; ++i) w = fmaf(c.v[C::oB + s * NI + i], x[i], w);
        zn[s] = w;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) z[s] = zn[s];
    return yv;
}

__device__ __forceinline__ double ss_asym_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int NS, int NI, int LOSS, bool VEC4>
__global__ __launch_bounds__(64) void ss_asym_step_kernel(const SsAsymStepArgs a)
{
    using C = SSCoef<NS, NI>;
    using D = AsStepDims<NS, NI, LOSS>;
    if (a.gate != nullptr) {
        if (a.gate[blockIdx.x] == 0u) return;
    } else if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        *a.status = SsTpStatus{0, 0.0f, 0, 0};                  // the verify kernel adds
        *a.ticket = 0u;                                          // the finish kernel counts its waves in
    }
    const int64_t B = a.B, T = a.T;
    const int64_t b_raw = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = b_raw < B;
    const int64_t b = live ? b_raw : B - 1;
    const int64_t k = blockIdx.y, t0 = k * a.L, t1 = (t0 + a.L < T) ? t0 + a.L : T;
    const int64_t tw = (k > 0 && t0 > a.W) ? t0 - a.W : 0;
    C c;
    c.load(a.coef);
    SSAsym dp = {};
    dp.load(a.rootp, 0, 0);
    float z[NS], S[D::nT][NS], P[NS][NS], G[D::nG], H[NS], sse = 0.0f;
    float GQ[D::nQ], HQ[D::nHQ], see = 0.0f;
    // the double sums live in LDS, one column per lane (touched every 32 steps: 2 nAcc registers a lane would not have otherwise;
    // a lane reads and writes its own column only: no barrier)
    __shared__ double accs[D::nAcc][64];
    double (*acc)[64] = reinterpret_cast<double (*)[64]>(&accs[0][threadIdx.x]);
#pragma unroll
    for (int s = 0; s < NS; ++s) z[s] = (tw == 0 && a.z0) ? a.z0[s * B + b] : 0.0f;
#pragma unroll
    for (int cc = 0; cc < D::nT; ++cc)
#pragma unroll
        for (int s = 0; s < NS; ++s) S[cc][s] = 0.0f;
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int s = 0; s < NS; ++s) P[j][s] = j == s ? 1.0f : 0.0f;
#pragma unroll
    for (int i = 0; i < D::nG; ++i) G[i] = 0.0f;
#pragma unroll
    for (int s = 0; s < NS; ++s) H[s] = 0.0f;
#pragma unroll
    for (int i = 0; i < D::nQ; ++i) GQ[i] = 0.0f;
#pragma unroll
    for (int s = 0; s < D::nHQ; ++s) HQ[s] = 0.0f;
#pragma unroll
    for (int i = 0; i < D::nAcc; ++i) acc[i][0] = 0.0;
    constexpr int kB = kBlkSS;
    float xc[kB][NI], xn[kB][NI], tc[kB], tn[kB];
    const float* __restrict__ xp = a.x + b * T * NI;
    auto load_x = [&](int64_t t, float (&v)[kB][NI]) {           // the lane's own row: 16-byte loads where the block is whole
        if (t + kB <= T) {
            ss_load_block<NI, VEC4>(a.x, b, T, t, v);
            return;
        }
#pragma unroll
        for (int i = 0; i < kB; ++i) {
            const int64_t tt = t + i < T ? t + i : T - 1;
#pragma unroll
            for (int j = 0; j < NI; ++j) v[i][j] = xp[tt * NI + j];
        }
    };
    auto load_t = [&](int64_t t, float (&v)[kB]) {               // [T][B]: coalesced rows
#pragma unroll
        for (int i = 0; i < kB; ++i) v[i] = a.target[(t + i < T ? t + i : T - 1) * B + b];
    };
#pragma unroll
    for (int i = 0; i < kB; ++i) tn[i] = 0.0f;
    load_x(tw, xn);
    if (tw == t0) load_t(t0, tn);
    int since = 0;
    for (int64_t tb = tw; tb < t1; tb += kB) {                   // (t0 - tw is a multiple of 8: a block is warm-up or owned, whole)
#pragma unroll
        for (int i = 0; i < kB; ++i) {
            tc[i] = tn[i];
#pragma unroll
            for (int j = 0; j < NI; ++j) xc[i][j] = xn[i][j];
        }
        if (tb + kB < t1) {                                      // one block ahead of the recursion
            load_x(tb + kB, xn);
            if (tb + kB >= t0) load_t(tb + kB, tn);
        }
        if (tb < t0) {                                           // warm-up: the state alone
#pragma unroll
            for (int i = 0; i < kB; ++i) (void)ss_fwd_step<NS, NI, kRootAsym, false>(c, dp, xc[i], z);
            continue;
        }
        if (tb == t0) {                                          // the state this chunk arrives with
#pragma unroll
            for (int s = 0; s < NS; ++s) a.zwarm[(k * NS + s) * B + b] = z[s];
        }
#pragma unroll
        for (int i = 0; i < kB; ++i) {
            if (tb + i < t1) {                                   // wave-uniform (the last chunk's ragged end)
                const float on = (LOSS != 0 && tb + i < a.skip) ? 0.0f : 1.0f;      // wave-uniform: a select
                a.y[(tb + i) * B + b] = ss_asym_step_one<NS, NI, LOSS>(c, dp, xc[i], tc[i], on, z, S, P, G, H, sse, GQ, HQ, see);
            }
        }
        if (++since == 4) {                                      // fp32 sums within 32 steps, fp64 across
            since = 0;
#pragma unroll
            for (int i = 0; i < D::nG; ++i) { acc[i][0] += (double)G[i]; G[i] = 0.0f; }
            acc[D::nG][0] += (double)sse;
            sse = 0.0f;
            if constexpr (LOSS != 0) {
#pragma unroll
                for (int i = 0; i < D::nG; ++i) { acc[D::oQ + i][0] += (double)GQ[i]; GQ[i] = 0.0f; }
                acc[D::oQ + D::nG][0] += (double)see;
                see = 0.0f;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < D::nG; ++i) acc[i][0] += (double)G[i];
    acc[D::nG][0] += (double)sse;
    if constexpr (LOSS != 0) {
#pragma unroll
        for (int i = 0; i < D::nG; ++i) acc[D::oQ + i][0] += (double)GQ[i];
        acc[D::oQ + D::nG][0] += (double)see;
    }
    // (a dead lane repeats sequence B - 1: its stores write the same values again, its sums count for nothing)
#pragma unroll
    for (int s = 0; s < NS; ++s) a.zend[(k * NS + s) * B + b] = z[s];
    if (a.zT && t1 == T) {
#pragma unroll
        for (int s = 0; s < NS; ++s) a.zT[s * B + b] = z[s];
    }
    float* __restrict__ rk = a.rec + ((size_t)k * D::nRec) * B + b;
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int s = 0; s < NS; ++s) rk[(size_t)(D::oPsi + j * NS + s) * B] = P[j][s];
#pragma unroll
    for (int cc = 0; cc < D::nT; ++cc)
#pragma unroll
        for (int s = 0; s < NS; ++s) rk[(size_t)(D::oS + cc * NS + s) * B] = S[cc][s];
#pragma unroll
    for (int s = 0; s < NS; ++s) rk[(size_t)(D::oH + s) * B] = H[s];
    if constexpr (LOSS != 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) rk[(size_t)(D::oHQ + s) * B] = HQ[s];
    }
    double* gp = a.gpart + ((size_t)k * gridDim.x + blockIdx.x) * D::nAcc;
#pragma unroll
    for (int i = 0; i < D::nAcc; ++i) {
        const double s = ss_asym_wave_sum(live ? acc[i][0] : 0.0);
        if (threadIdx.x == 0) gp[i] = s;
    }
}

// What the finish hands back.  LOSS = 0: out = {sse, gscale G[kN], gscale G_root[5]}.  LOSS = 1: sums = {S, E, gP[kN + 5],
// gQ[kN + 5]} of THIS call (what several ranks all-reduce); g != nullptr: the step finished as a single rank -- ga, gb, mse, esr
// from S, E, n_global and eps (esr_coef_kernel's formulas, fp64), g = ga gP + gb gQ, loss3 = {mse, esr, mse + esr} (optional).
struct SsAsymStepOut {
    float gscale; float* out;
    double n_global, eps; float* sums; float* g; float* loss3;
};

// One lane per sequence: the K records first to last (one record where the wave was repaired) in double, the wave's sums ->
// part[wave][nAcc]; the wave that finishes LAST adds the partials in wave order (lane i owns accumulator i, and i + 64).
template <int NS, int NI, int LOSS>
__global__ __launch_bounds__(64) void ss_asym_step_finish_kernel(const float* __restrict__ rec, const double* __restrict__ gpart,
                                                                 const unsigned* __restrict__ gate, double* part, unsigned* ticket,
                                                                 SsAsymStepOut o, int64_t B, int64_t K)
{
    using D = AsStepDims<NS, NI, LOSS>;
    static_assert(D::nG <= 64, "one lane per gradient entry in the last wave");
    const int64_t b_raw = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = b_raw < B;
    const int64_t b = live ? b_raw : B - 1;
    const int64_t kn = (gate != nullptr && gate[blockIdx.x] != 0u) ? 1 : K;
    double Ss[D::nT][NS], tot[D::nAcc];
#pragma unroll
    for (int cc = 0; cc < D::nT; ++cc)
#pragma unroll
        for (int s = 0; s < NS; ++s) Ss[cc][s] = 0.0;
#pragma unroll
    for (int i = 0; i < D::nAcc; ++i) tot[i] = 0.0;
    for (int64_t k = 0; k < kn; ++k) {
        const float* __restrict__ r = rec + ((size_t)k * D::nRec) * B + b;
        double Hh[NS], HQh[D::nHQ], Psi[NS][NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) Hh[s] = (double)r[(size_t)(D::oH + s) * B];
        if constexpr (LOSS != 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) HQh[s] = (double)r[(size_t)(D::oHQ + s) * B];
        }
#pragma unroll
        for (int j = 0; j < NS; ++j)
#pragma unroll
            for (int s = 0; s < NS; ++s) Psi[j][s] = (double)r[(size_t)(D::oPsi + j * NS + s) * B];
#pragma unroll
        for (int cc = 0; cc < D::nT; ++cc) {
            double d = 0.0, dq = 0.0, sn[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                d = fma(Hh[s], Ss[cc][s], d);
                if constexpr (LOSS != 0) dq = fma(HQh[s], Ss[cc][s], dq);
            }
            tot[D::gidx(cc)] += d;
            if constexpr (LOSS != 0) tot[D::oQ + D::gidx(cc)] += dq;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                double w = (double)r[(size_t)(D::oS + cc * NS + s) * B];
#pragma unroll
                for (int j = 0; j < NS; ++j) w = fma(Psi[j][s], Ss[cc][j], w);
                sn[s] = w;
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) Ss[cc][s] = sn[s];
        }
    }
    const unsigned nwaves = gridDim.x;
    __shared__ double tt[D::nAcc];                                // (one wave per workgroup)
#pragma unroll
    for (int i = 0; i < D::nAcc; ++i) {
        const double w = ss_asym_wave_sum(live ? tot[i] : 0.0);
        if (threadIdx.x == 0) tt[i] = w;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < D::nAcc; i += 64) {             // lane i keeps the wave's accumulator i (and i + 64)
        double mine = tt[i];
        for (int64_t k = 0; k < kn; ++k) mine += gpart[((size_t)k * nwaves + blockIdx.x) * D::nAcc + i];    // the chunks' own sums, in time order
        __hip_atomic_store(part + (size_t)blockIdx.x * D::nAcc + i, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the partial has landed before the count moves
    __syncthreads();
    unsigned done = 0;
    if (threadIdx.x == 0) done = atomicAdd(ticket, 1u);
    done = __builtin_amdgcn_readfirstlane(done);
    if (done != nwaves - 1) return;
    for (int i = threadIdx.x; i < D::nAcc; i += 64) {
        double t = 0.0;
        for (unsigned w = 0; w < nwaves; ++w) t += __hip_atomic_load(part + (size_t)w * D::nAcc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tt[i] = t;
    }
    __syncthreads();
    const int i = (int)threadIdx.x;
    if constexpr (LOSS == 0) {
        if (i < D::nG) o.out[1 + i] = (float)((double)o.gscale * tt[i]);
        if (i == 0) o.out[0] = (float)tt[D::nG];
    } else {
        const double Ssum = tt[D::nG], Esum = tt[D::oQ + D::nG];
        const double t = tt[i < D::nG ? i : 0], q = tt[D::oQ + (i < D::nG ? i : 0)];      // gP_i and gQ_i
        if (i == 0) { o.sums[0] = (float)Ssum; o.sums[1] = (float)Esum; }
        if (i < D::nG) { o.sums[2 + i] = (float)t; o.sums[2 + D::nG + i] = (float)q; }
        if (o.g == nullptr) return;
        // (esr_terms' expressions, wdf_esr.h, by hand: calling it reorders this kernel's instructions)
        const double n = o.n_global, En = Esum + o.eps;
        const double mse = Ssum / n, er = sqrt(Ssum / En / n);
        const double ga = 2.0 / n + (er > 0.0 ? 1.0 / (er * En * n) : 0.0), gb = -er / En;
        if (i < D::nG) o.g[i] = (float)(ga * t + gb * q);
        if (i == 0 && o.loss3) { o.loss3[0] = (float)mse; o.loss3[1] = (float)er; o.loss3[2] = (float)(mse + er); }
    }
}

}  // namespace wdf
