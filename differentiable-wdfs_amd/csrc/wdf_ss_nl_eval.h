// wdf_ss_nl_eval.h -- the LOSS-ONLY evaluation pass of small state-space trees with a diode-pair root (gfx950): forward and
//     S = sum (y - target)^2 ,  E = sum y^2      over the rows t >= skip
// in one sweep over the resident set, for a loss nobody differentiates (the validation half of the scripts' epoch,
// clipper_pot.py:245-269).  The training step (wdf_ss_nl_step.h) carries 7+ tangents per state, Psi, H, the chunk records, the
// record walk and the chain rule for a gradient such a call throws away; this pass keeps its GEOMETRY -- unit -> (chunk k, group),
// 256-thread workgroups of four chunk waves, dead lanes shadowing sequence B - WD, 8-step blocks with the next block in flight,
// the root tier chosen once per launch -- and runs per step the state update (nl_z_step's) plus y and two fp32 running sums,
// flushed into fp64 every 32 steps.  A chunk wave publishes zwarm[k] (the state it arrives with at t0), zend[k] and its {S, E}
// as two doubles per (chunk, group); STORE_Y = false compiles the y store out (8 B/sample: x and the target in, nothing out).
//
// Warm start.  Without tangents the step's Taylor prediction is not available.  The pass takes SNAPSHOTS by absolute time
// instead: the state in front of every 16th step, [3][ceil(T / 16)][NS][B], a ring over the last three calls (0.25 B per sample
// and state).  A warm-up of any multiple of 16 can then start from an earlier call's state at that very sample: the last
// snapshot when one call is valid, the secant (1 + lam) z1 - lam z2 along the coefficient path when two are (tp_extrapolation's
// rule, wdf_clipper.h, on the vector {coefficients, L, V}).  Correctness never rests on the start: every boundary is verified.
//
// ss_nl_eval_finish_kernel, a launch of its own (also when K = 1), one wave per group: verifies |zwarm[k] - zend[k - 1]| <= tol,
// re-runs a group that missed from its first missed boundary to T (exact from there: y, snapshots, zend, the {S, E} slots of
// those chunks), sums the group's slots in chunk order and takes a counted ticket; the last group reduces over the groups in a
// fixed order, writes sums[2] and loss3, steers the warm-up (NlStepCtl: the step's layout and rule) and advances the ring.
// No wave waits on another workgroup, no float atomics: the same calls on the same state history give the same bits.
#pragma once
#include "wdf_esr.h"
#include "wdf_ss_nl_step.h"

namespace wdf {

#ifndef WDF_NL_EVAL_WAVES
// waves per SIMD the chunk kernel's register allocation is held to.  1, the step's bound: the eight-step block with the next
// block's loads in flight, their addresses and the x terms of eight steps want up to ~270 registers with two states, two sources
// and two sequences per lane; held to 2 waves (256 registers) six instantiations spill
#define WDF_NL_EVAL_WAVES 1
#endif
constexpr int kNlEvalSnap = 16;      // a snapshot in front of every 16th step
constexpr int kNlEvalRing = 3;       // the slot being written, and the two the secant reads

// what the pass keeps beside NlStepCtl (at +128 in the workspace): the ticket, and the snapshot ring's state
struct NlEvalAux {
    unsigned ticket;
    int head;                        // the ring slot of the last call's snapshots
    int valid;                       // calls whose snapshots (and coefficients) are there: 0..2
    int secant;                      // 0: always start from the last snapshot
};

struct NlEvalArgs {
    const float* x;                  // [T][NI][B]
    const float* coef;               // SSCoef order (the probe's output)
    const float* pIs;
    const float* pV;
    const float* pRp;
    const float* target;             // [T][B]
    float* y;                        // [T][B] (STORE_Y)
    NlStepCtl* ctl;
    NlEvalAux* aux;
    float* coef_prev;                // [2][kN + 2]: {coefficients, L, V} of the last call, and of the one before
    float* zwarm;                    // [K][NS][B]
    float* zend;                     // [K][NS][B]
    float* snap;                     // [3][n_snap][NS][B]
    double* gpart;                   // [K][groups][2]
    double* part;                    // [groups][4]: {S, E, bad boundaries, largest miss}
    double* sums;                    // <- {S, E}
    float* loss3;                    // (or null) <- {mse, esr, mse + esr}
    double n_global, eps;
    int64_t B, T, L, skip, n_snap;
    int K, groups, n_up, n_down;
};

__device__ __forceinline__ void nl_eval_load_diode(const NlEvalArgs& a, SSDiode& dp)
{
    NlStepArgs s{};
    s.pIs = a.pIs; s.pV = a.pV; s.pRp = a.pRp; s.n_up = a.n_up; s.n_down = a.n_down;
    nl_load_diode(s, dp);
}

// entry i of {coefficients, L, V}
template <int NS, int NI>
__device__ __forceinline__ float nl_eval_coef(const SSCoef<NS, NI>& c, const SSDiode& dp, int i)
{
    return i < SSCoef<NS, NI>::kN ? c.v[i] : (i == SSCoef<NS, NI>::kN ? dp.L : dp.V);
}

// the secant's factor: the projection of the coefficients' relative change since the last call onto the change before it,
// clamped to [-1, 2]; 0 (the last snapshot) when the earlier change has no length or the projection is NaN (a coefficient that
// is 0 has no relative change)
template <int NS, int NI>
__device__ __forceinline__ float nl_eval_lambda(const SSCoef<NS, NI>& c, const SSDiode& dp, const float* __restrict__ prev)
{
    constexpr int n = SSCoef<NS, NI>::kN + 2;
    float n10 = 0.0f, n00 = 0.0f;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        const float p1 = prev[i], p2 = prev[n + i];
        const float d1 = p1 != 0.0f ? nl_eval_coef(c, dp, i) / p1 - 1.0f : 0.0f;
        const float d0 = p2 != 0.0f ? p1 / p2 - 1.0f : 0.0f;
        n10 = fmaf(d1, d0, n10);
        n00 = fmaf(d0, d0, n00);
    }
    if (!(n00 > 1.0e-30f)) return 0.0f;
    const float q = n10 / n00;
    if (!(q == q)) return 0.0f;                               // (before the clamp: fmaxf would turn a NaN into -1)
    return fminf(fmaxf(q, -1.0f), 2.0f);
}

// one owned step: y and the state (nl_step's forward half, its expressions)
template <int NS, int NI, bool SYM, typename V, int FAST>
__device__ __forceinline__ V nl_eval_step(const SSCoef<NS, NI>& c, const SSDiode& dp, const V (&x)[NI], V (&z)[NS])
{
    using C = SSCoef<NS, NI>;
    V a = vsplat<V>(0.0f);
#pragma unroll
    for (int s = 0; s < NS; ++s) a = vfma(c.v[C::oCa + s], z[s], a);
#pragma unroll
    for (int i = 0; i < NI; ++i) a = vfma(c.v[C::oDa + i], x[i], a);
    const V b = diode_pair<SYM, V, FAST>(a, vsplat<V>(dp.L), dp.d).b;
    V yv = b * c.v[C::oFy];
#pragma unroll
    for (int s = 0; s < NS; ++s) yv = vfma(c.v[C::oCy + s], z[s], yv);
#pragma unroll
    for (int i = 0; i < NI; ++i) yv = vfma(c.v[C::oDy + i], x[i], yv);
    V zn[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        V v = b * c.v[C::oE + s];
#pragma unroll
        for (int q = 0; q < NS; ++q) v = vfma(c.v[C::oA + s * NS + q], z[q], v);
#pragma unroll
        for (int i = 0; i < NI; ++i) v = vfma(c.v[C::oB + s * NI + i], x[i], v);
        zn[s] = v;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) z[s] = zn[s];
    return yv;
}

// Chunk k of the lane's sequences b: the steps [tw, t1) from the state z, of which [t0, t1) are owned (tw < t0: warm-up, a
// multiple of 8 steps; then zwarm[k] is published).  Writes y (STORE_Y), the snapshots of ring slot `slot`, zend[k] and the
// chunk's {S, E} slot.  The chunk kernel runs it once per wave; the finish kernel's repair once per chunk from k* on (tw = t0).
template <int NS, int NI, bool SYM, typename V, int FAST, bool STORE_Y>
__device__ __forceinline__ void nl_eval_span(const NlEvalArgs& a, const SSCoef<NS, NI>& c, const SSDiode& dp, V (&z)[NS], int64_t b,
                                             bool live, int lane, int64_t grp, int64_t k, int64_t tw, int64_t t0, int64_t t1, int slot,
                                             bool publish_warm)
{
    const V zero = vsplat<V>(0.0f);
    const int64_t B = a.B;
    const float lv = live ? 1.0f : 0.0f;
    V s = zero, e = zero;
    double S = 0.0, E = 0.0;
    float* __restrict__ sp = a.snap + (size_t)slot * a.n_snap * NS * B + b;
    V xn[kLinBlk][NI], tn[kLinBlk];
    auto load_blk = [&](int64_t ts) {
        const int n = t1 - ts < kLinBlk ? (int)(t1 - ts) : kLinBlk;
        lin_load_x<NI, V>(a.x, B, b, ts, n, xn);
#pragma unroll
        for (int i = 0; i < kLinBlk; ++i) tn[i] = (i < n && ts >= t0) ? lin_ld<V>(a.target + (ts + i) * B + b) : zero;
    };
    load_blk(tw);
    int since = 0;
    for (int64_t ts = tw; ts < t1; ts += kLinBlk) {               // 8-step blocks, the next one in flight
        const int n = t1 - ts < kLinBlk ? (int)(t1 - ts) : kLinBlk;
        V xc[kLinBlk][NI], tc[kLinBlk];
#pragma unroll
        for (int i = 0; i < kLinBlk; ++i) {
            tc[i] = tn[i];
#pragma unroll
            for (int j = 0; j < NI; ++j) xc[i][j] = xn[i][j];
        }
        if (ts + kLinBlk < t1) load_blk(ts + kLinBlk);
        if (ts < t0) {                                            // warm-up (t0 - tw is a multiple of 8)
#pragma unroll
            for (int i = 0; i < kLinBlk; ++i) nl_z_step<NS, NI, SYM, V, FAST>(c, dp, xc[i], z);
            continue;
        }
        if (ts == t0 && publish_warm && live) {
#pragma unroll
            for (int q = 0; q < NS; ++q) lin_st<V>(a.zwarm + ((size_t)k * NS + q) * B + b, z[q]);
        }
        if (ts % kNlEvalSnap == 0 && live) {                      // (t0 is a multiple of 32: every second block)
#pragma unroll
            for (int q = 0; q < NS; ++q) lin_st<V>(sp + ((size_t)(ts / kNlEvalSnap) * NS + q) * B, z[q]);
        }
        if (n == kLinBlk) {
#pragma unroll
            for (int i = 0; i < kLinBlk; ++i) {
                const float w = (ts + i < a.skip) ? 0.0f : lv;    // (the same for a whole wave: a scalar select)
                const V yv = nl_eval_step<NS, NI, SYM, V, FAST>(c, dp, xc[i], z);
                if constexpr (STORE_Y) lin_st_nt<V>(a.y + (ts + i) * B + b, yv);     // (a dead lane repeats the last sequence's values)
                const V d = yv - tc[i];
                s = vfma(d * w, d, s);
                e = vfma(yv * w, yv, e);
            }
        } else {
#pragma unroll
            for (int i = 0; i < kLinBlk; ++i) {
                if (i >= n) break;
                const float w = (ts + i < a.skip) ? 0.0f : lv;
                const V yv = nl_eval_step<NS, NI, SYM, V, FAST>(c, dp, xc[i], z);
                if constexpr (STORE_Y) { if (live) lin_st_nt<V>(a.y + (ts + i) * B + b, yv); }
                const V d = yv - tc[i];
                s = vfma(d * w, d, s);
                e = vfma(yv * w, yv, e);
            }
        }
        if (++since == 4) {                                       // fp32 sums within 32 steps, fp64 across
            since = 0;
            S += lin_hsum(s); E += lin_hsum(e);
            s = zero; e = zero;
        }
    }
    S += lin_hsum(s); E += lin_hsum(e);
    if (live) {
#pragma unroll
        for (int q = 0; q < NS; ++q) lin_st<V>(a.zend + ((size_t)k * NS + q) * B + b, z[q]);
    }
    double* gp = a.gpart + ((size_t)k * a.groups + grp) * 2;
    const double Sw = wave_sum_dpp(S), Ew = wave_sum_dpp(E);
    if (lane == 0) {
        __hip_atomic_store(gp + 0, Sw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(gp + 1, Ew, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int NS, int NI, bool SYM, typename V, int FAST, bool STORE_Y>
__device__ __forceinline__ void nl_eval_chunk(const NlEvalArgs& a, const SSCoef<NS, NI>& c, const SSDiode& dp)
{
    constexpr int WD = LinWidth<V>::w;
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= (int64_t)a.groups * a.K) return;
    const int64_t k = unit / a.groups, grp = unit % a.groups;
    const int64_t B = a.B, b_raw = (grp * 64 + lane) * WD;
    const bool live = b_raw < B;
    const int64_t b = live ? b_raw : B - WD;
    const int64_t t0 = k * a.L, t1 = (t0 + a.L < a.T) ? t0 + a.L : a.T;
    const NlEvalAux aux = *a.aux;
    const int valid = a.ctl->have_snap ? aux.valid : 0;
    // a start from snapshots lies on a multiple of 16 (the controller keeps w there; a cold warm-up or a value set by hand is rounded up)
    const int w_cur = (a.ctl->w_cur + kNlEvalSnap - 1) / kNlEvalSnap * kNlEvalSnap;
    const int64_t tw = t0 > w_cur ? t0 - w_cur : 0;
    V z[NS];
    if (tw == 0 || !valid) {
#pragma unroll
        for (int q = 0; q < NS; ++q) z[q] = vsplat<V>(0.0f);
    } else {
        const size_t per = (size_t)a.n_snap * NS * B, at = (size_t)(tw / kNlEvalSnap) * NS * B + b;
        const int h2 = valid > 1 ? (aux.head + kNlEvalRing - 1) % kNlEvalRing : aux.head;     // (one call valid: aliases the newest, unused)
        V z2[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            z[q] = lin_ld<V>(a.snap + aux.head * per + at + (size_t)q * B);
            z2[q] = lin_ld<V>(a.snap + h2 * per + at + (size_t)q * B);
        }
        if (valid > 1 && aux.secant) {
            const float lam = nl_eval_lambda(c, dp, a.coef_prev);
#pragma unroll
            for (int q = 0; q < NS; ++q) z[q] = vfma(vsplat<V>(lam), z[q] - z2[q], z[q]);
        }
    }
    nl_eval_span<NS, NI, SYM, V, FAST, STORE_Y>(a, c, dp, z, b, live, lane, grp, k, tw, t0, t1, (aux.head + 1) % kNlEvalRing, true);
}

template <int NS, int NI, bool SYM, typename V, bool STORE_Y>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WDF_NL_EVAL_WAVES, WDF_NL_EVAL_WAVES))) void ss_nl_eval_kernel(const NlEvalArgs a)
{
    SSCoef<NS, NI> c;
    c.load(a.coef);
    SSDiode dp = {};
    nl_eval_load_diode(a, dp);
    if constexpr (SYM) {
        // the root tier, once per launch, as ss_nl_step_kernel chooses it
        const float l0 = dp.L - dp.d.l_dn;
        if (l0 <= -7.5f && l0 >= -80.0f) {
            nl_eval_chunk<NS, NI, SYM, V, kRootLean, STORE_Y>(a, c, dp);
            return;
        }
        if (l0 <= kSeriesOnlyBelow) {
            nl_eval_chunk<NS, NI, SYM, V, kRootFast, STORE_Y>(a, c, dp);
            return;
        }
    }
    nl_eval_chunk<NS, NI, SYM, V, kRootGeneral, STORE_Y>(a, c, dp);
}

// One wave per group of 64 WD sequences (the chunk kernel's groups).
template <int NS, int NI, bool SYM, int WD, bool STORE_Y>
__global__ __launch_bounds__(64) void ss_nl_eval_finish_kernel(const NlEvalArgs a)
{
    using V = std::conditional_t<WD == 2, v2f, float>;
    using C = SSCoef<NS, NI>;
    const int lane = threadIdx.x;
    const int64_t grp = blockIdx.x, B = a.B;
    const int K = a.K;
    const NlStepCtl c0 = *a.ctl;                                  // (only the launch's last wave writes these, after everyone has read)
    const NlEvalAux x0 = *a.aux;
    const float tol = c0.tol;
    const int64_t b_raw = (grp * 64 + lane) * WD;
    const bool live = b_raw < B;
    const int64_t b = live ? b_raw : B - WD;
    // ---- the group's boundaries, eight in flight together; k*: the first one that any sequence of the group missed
    float miss = 0.0f;
    int nbad = 0, kstar = K;
    constexpr int kBatch = 8;
    for (int k0 = 1; k0 < K; k0 += kBatch) {
        V zw[kBatch][NS], ze[kBatch][NS];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int k = k0 + j < K ? k0 + j : K - 1;            // clamped: re-reads the last boundary
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                zw[j][q] = lin_ld<V>(a.zwarm + ((size_t)k * NS + q) * B + b);
                ze[j][q] = lin_ld<V>(a.zend + ((size_t)(k - 1) * NS + q) * B + b);
            }
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            bool bad = false;
            if (k0 + j < K) {
#pragma unroll
                for (int q = 0; q < NS; ++q)
#pragma unroll
                    for (int h = 0; h < WD; ++h) {
                        const float m = fabsf(vget(zw[j][q], h) - vget(ze[j][q], h));
                        if (live) {
                            miss = fmaxf(miss, m);
                            if (!(m <= tol)) { ++nbad; bad = true; }      // NaN counts as bad
                        }
                    }
            }
            if (__builtin_amdgcn_ballot_w64(bad) != 0 && k0 + j < kstar) kstar = k0 + j;
        }
    }
    const float wmiss = wave_max_dpp(miss);
    const int wbad = wave_sum_dpp(nbad);
    if (wbad != 0) {
        // a boundary missed: this group again from k*, sequentially from its predecessor's end -- exact from there on
        C c;
        c.load(a.coef);
        SSDiode dp = {};
        nl_eval_load_diode(a, dp);
        V z[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) z[q] = lin_ld<V>(a.zend + ((size_t)(kstar - 1) * NS + q) * B + b);
        const int slot = (x0.head + 1) % kNlEvalRing;
        for (int k = kstar; k < K; ++k) {
            const int64_t t0 = (int64_t)k * a.L, t1 = (t0 + a.L < a.T) ? t0 + a.L : a.T;
            nl_eval_span<NS, NI, SYM, V, kRootGeneral, STORE_Y>(a, c, dp, z, b, live, lane, grp, k, t0, t0, t1, slot, false);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the rewritten slots have landed
    }
    // ---- the group's slots in chunk order (lane i: chunks i, i + 64, ...), then the wave's tree
    double S = 0.0, E = 0.0;
    for (int k = lane; k < K; k += 64) {
        const double* gp = a.gpart + ((size_t)k * a.groups + grp) * 2;
        S += __hip_atomic_load(gp + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        E += __hip_atomic_load(gp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    S = wave_sum_dpp(S);
    E = wave_sum_dpp(E);
    // ---- this group's partial; the last wave adds them up in a fixed order
    if (lane == 0) {
        double* o = a.part + (size_t)grp * 4;
        __hip_atomic_store(o + 0, S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 1, E, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 2, (double)wbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 3, (double)wmiss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned old = 0;
    if (lane == 0) old = atomicAdd(&a.aux->ticket, 1u);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != (unsigned)(a.groups - 1)) return;
    if (lane == 0) a.aux->ticket = 0u;
    double s0 = 0.0, s1 = 0.0, nbd = 0.0, ggd = 0.0;
    float mm = 0.0f;
    for (int64_t w = lane; w < a.groups; w += 64) {
        double v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = __hip_atomic_load(a.part + (size_t)w * 4 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s0 += v[0];
        s1 += v[1];
        nbd += v[2];
        ggd += v[2] > 0.0 ? 1.0 : 0.0;
        mm = fmaxf(mm, (float)v[3]);
    }
    s0 = wave_sum_dpp(s0);
    s1 = wave_sum_dpp(s1);
    const int nb = (int)wave_sum_dpp(nbd), gg = (int)wave_sum_dpp(ggd);
    mm = wave_max_dpp(mm);
    // what this call's snapshots were taken with: lane i moves entry i of the two coefficient vectors
    {
        constexpr int n = C::kN + 2;
        static_assert(n <= 64, "one lane per entry");
        C c;
        c.load(a.coef);
        SSDiode dp = {};
        nl_eval_load_diode(a, dp);
        float now = 0.0f;
#pragma unroll
        for (int i = 0; i < n; ++i) now = lane == i ? nl_eval_coef(c, dp, i) : now;
        if (lane < n) {
            a.coef_prev[n + lane] = a.coef_prev[lane];
            a.coef_prev[lane] = now;
        }
    }
    if (lane != 0) return;
    a.sums[0] = s0;
    a.sums[1] = s1;
    if (a.loss3 != nullptr) {
        const EsrTerms lt = esr_terms(s0, s1 + a.eps, a.n_global);
        a.loss3[0] = (float)lt.mse; a.loss3[1] = (float)lt.esr; a.loss3[2] = (float)(lt.mse + lt.esr);
    }
    // the verdict, and the next call's warm-up by the step's rule: x2 on a miss, +16 above grow_at tol, -16 below shrink_at tol
    // after the cool-down.  (Snapshots lie at every 16th sample: the new warm-up holds from the very next call.)
    NlStepCtl* ctl = a.ctl;
    ctl->n_bad = nb;
    ctl->max_miss = mm;
    ctl->gated_groups = gg;
    // (what the chunk kernel ran with: w_cur rounded up to a multiple of 16)
    const int w_used = (c0.w_cur + kNlEvalSnap - 1) / kNlEvalSnap * kNlEvalSnap, ws = c0.w_snap;
    int w = ws, cool = c0.cool;
    if (c0.have_snap && x0.valid) {                              // (a cold call says nothing about the starts from snapshots)
        const int base = w_used > ws ? w_used : ws;
        if (nb) { w = base * 2; cool = c0.cool_miss; }
        else if (mm > c0.grow_at * tol) { w = base + kNlEvalSnap; if (cool < 2) cool = 2; }
        else if (cool > 0) --cool;
        else if (mm <= c0.shrink_at * tol && w_used <= ws) w = ws - kNlEvalSnap;
    }
    int wmax = c0.w_max < (int)a.L ? c0.w_max : (int)a.L;
    wmax = wmax / kNlEvalSnap * kNlEvalSnap;
    w = (w + kNlEvalSnap - 1) / kNlEvalSnap * kNlEvalSnap;
    if (w > wmax) w = wmax;
    if (w < c0.w_min) w = c0.w_min;
    ctl->w_used = w_used;
    ctl->w_cur = w;
    ctl->w_snap = w;
    ctl->cool = cool;
    ctl->have_snap = 1;
    ctl->parity = c0.parity ^ 1;
    ctl->call = c0.call + 1;
    ctl->total_gated = c0.total_gated + gg;
    NlEvalAux* aux = a.aux;
    aux->head = (x0.head + 1) % kNlEvalRing;
    aux->valid = x0.valid < 2 ? x0.valid + 1 : 2;
}

}  // namespace wdf
