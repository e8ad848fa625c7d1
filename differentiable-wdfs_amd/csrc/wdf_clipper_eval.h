// wdf_clipper_eval.h -- the diode clipper's LOSS-ONLY evaluation pass (gfx950): forward and the two loss sums
//     S = sum (y - target)^2 ,  E = sum y^2      over the steps >= skip
// in one pass over the data, for a loss that nobody differentiates -- the validation half of every epoch of the scripts'
// training loop (clipper_pot.py:245-269: val_loss / val_mse / val_esr; every fifth epoch a plot also reads val_outs).
//
// The one-pass training step (wdf_clipper_fused.h) carries the state's tangent, the chunk records, the record walk and the
// chain rule for a gradient such a call throws away, and it is bound by VALU issue, not by HBM.  This pass keeps the step's
// STRUCTURE -- chunk_span, the controller and the snapshots in one flight of loads, the warm start from the TpCtl / snapshot
// ring with tp_extrapolation, the cold warm-up, buffer-descriptor rows, tiles of FusedTile<V, DYN_R>::NR steps prefetched a
// tile ahead, the XWindow path for batch-major x, the wait on the back edge, the snapshot stores, zwarm / zend / zT -- and per
// step runs fwd_step (wdf_clipper.h: the expressions the step's forward half uses) plus two fp32 running sums, flushed into
// fp64 every kFlushSteps steps.  No tangent, no record: what a chunk hands over is {S, E} per (tile, chunk, sequence slot),
// two doubles summed over the wave by the chunk wave itself (fused_publish_record's wpart with NP = 2).  STORE_Y = false
// compiles the stores of y out (8 B/sample: x and the target in, nothing out).
//
// clipper_eval_finish_kernel, a launch of its own behind the chunk kernel (the kFusedFinishLater form; one chunk has no boundary
// and no second launch), one wave per tile: verifies the tile's chunk boundaries as tp_verify_tile<..., DEFER> does, repairs a
// tile that missed (fused_repair_tile's walk without the record: the failing chunks again from the exact state with the
// forward-only step -- y, snapshots and that chunk's {S, E} slot rewritten), sums the tile's slots over the chunks in a fixed
// order and writes the tile's partial; the last tile, found by a counted ticket that is left at zero, reduces over the tiles in
// a fixed order, writes sums[2] (doubles: what several ranks all-reduce before wdf_esr_coef) and, when asked, loss3 =
// {S/n, sqrt(S/(E + eps)/n), their sum} (esr_terms), publishes the status and steers the warm start.  No wave waits on another
// workgroup, no float atomics: the same call on the same inputs gives the same bits.
#pragma once

#include "wdf_clipper_fused.h"

namespace wdf {

#ifndef WDF_EVAL_WAVES
#define WDF_EVAL_WAVES 2            // waves per SIMD the evaluation kernel's register allocation is held to
#endif
constexpr int kEvalNP = 2;          // {S, E}

// What the pass hands back: sums[2] = {S, E} of this call's batch; loss3 (or null) from them with n_global and eps.
struct EvalOut { double* sums; float* loss3; double n_global, eps; };

// The running sums of the lane's sequences since the last flush, and their fp64 totals
template <typename V>
struct EvalSums {
    static constexpr int N = VT<V>::N;
    V s, e;
    double S[N], E[N];
    __device__ __forceinline__ void init()
    {
        s = e = vsplat<V>(0.0f);
#pragma unroll
        for (int j = 0; j < N; ++j) S[j] = E[j] = 0.0;
    }
    __device__ __forceinline__ void flush()
    {
#pragma unroll
        for (int j = 0; j < N; ++j) { S[j] += (double)vget(s, j); E[j] += (double)vget(e, j); }
        s = e = vsplat<V>(0.0f);
    }
    // w: 1 on the steps that carry loss, 0 below skip
    __device__ __forceinline__ void add(V y, V tgt, float w)
    {
        const V d = y - tgt;
        s = vfma(w * d, d, s);
        e = vfma(w * y, y, e);
    }
};

// The chunk's hand-over: wpart double [tiles][K][NSEQ][2]; `slot0`: the first sequence slot this call covers (the repair re-runs
// one slot of 64 sequences at a time with V = float).  Dead lanes (past the end of the batch) contribute 0.
template <typename V, int NSEQ>
__device__ __forceinline__ void eval_publish(double* wpart, int64_t k, int64_t K, bool live, int slot0, const EvalSums<V>& d)
{
#pragma unroll
    for (int j = 0; j < VT<V>::N; ++j) {
        double* w = wpart + (((int64_t)blockIdx.x * K + k) * NSEQ + slot0 + j) * kEvalNP;
        const double S = wave_sum_dpp(live ? d.S[j] : 0.0), E = wave_sum_dpp(live ? d.E[j] : 0.0);
        if ((threadIdx.x & 63u) == 0) {
            __hip_atomic_store(w + 0, S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(w + 1, E, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// A tile's totals {S, E} (the same in every lane) -> its slot of `part` ([tiles][2] doubles); the LAST tile to arrive (gticket,
// left at zero) reduces over the tiles in a fixed order -- lane i takes tiles i, i + 64, ..., then the wave's tree --, writes
// sums and loss3, publishes the status and steers the warm start.  One wave.
__device__ __forceinline__ void eval_tile_partial_and_finish(double S, double E, double* part, unsigned* gticket, const float* theta,
                                                             const EvalOut& out, const TpFinishCtx& fc)
{
    const unsigned ntiles = gridDim.x;
    unsigned done = 0;
    if (threadIdx.x == 0) {
        double* o = part + (int64_t)blockIdx.x * kEvalNP;
        __hip_atomic_store(o + 0, S, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 1, E, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the partial (and the verification's atomics) have landed before the count moves
        done = atomicAdd(&gticket[0], 1u);
    }
    done = __builtin_amdgcn_readfirstlane(done);
    if (done != ntiles - 1) return;
    if (threadIdx.x == 0) gticket[0] = 0u;
    double t0 = 0.0, t1 = 0.0;
    for (unsigned i = threadIdx.x; i < ntiles; i += 64) {
        t0 += __hip_atomic_load(part + (int64_t)i * kEvalNP + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t1 += __hip_atomic_load(part + (int64_t)i * kEvalNP + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const TpFinishFetched ff = tp_finish_fetch(fc);
    t0 = wave_sum_dpp(t0);
    t1 = wave_sum_dpp(t1);
    if (threadIdx.x == 0) {
        out.sums[0] = t0;
        out.sums[1] = t1;
        if (out.loss3 != nullptr) {
            const EsrTerms lt = esr_terms(t0, t1 + out.eps, out.n_global);
            out.loss3[0] = (float)lt.mse; out.loss3[1] = (float)lt.esr; out.loss3[2] = (float)(lt.mse + lt.esr);
        }
    }
    tp_finish_deferred(fc, ff, theta);
}

// Chunk geometry, warm start and load schedule as clipper_fused_body (wdf_clipper_fused.h); k of K: the wave's chunk.
template <int DYN_R, bool SYM, bool TM, bool VEC4, int FAST, typename V, bool STORE_Y>
__device__ __forceinline__ void clipper_eval_body(
    const ClipConsts& c_in, const float* __restrict__ x, const float* __restrict__ r, const float* __restrict__ target,
    float* __restrict__ y, const float* __restrict__ z0, float* __restrict__ zT, float* __restrict__ zwarm, float* __restrict__ zend,
    const float* __restrict__ theta, const TpCtl* __restrict__ ctl, float* __restrict__ snap, int J, int64_t B, int64_t T, int64_t L,
    int64_t W, int64_t skip, int64_t k, int64_t K, int64_t skew, double* wpart, double (&tot)[kEvalNP])
{
    constexpr int NR = FusedTile<V, DYN_R>::NR;
    const LaneOwn<V> q(B);
    const ClipConstsSeq<V> c = make_seq_consts<DYN_R, V>(c_in, DYN_R == 2 ? load_step<V, TM>(r, q, B, T, 0) : vsplat<V>(1.0f));
    int64_t t0, t1;
    chunk_span(k, K, L, skew, T, t0, t1);
    int64_t tw = 0;
    V z = vsplat<V>(0.0f);
    // the controller in one flight of loads; then everything the wave needs to take its first step in a second one
    TpCtl c0 = {};
    if (ctl != nullptr) c0 = *ctl;
    __builtin_amdgcn_sched_barrier(0);
    const bool stateful = ctl != nullptr && c0.geom == tp_geom_tag(K, J, tp_span_scheme(skew));
    const int valid = stateful ? c0.valid : 0;
    const int head = stateful ? c0.head : 0;
    const bool warm_start = k > 0 && valid > 0 && !(stateful && c0.cold_hold > 0);   // (cold_hold: tp_publish_status_and_steer)
    const int jw = warm_start ? c0.j_next : 0;
    if (warm_start) tw = t0 - (int64_t)kWarmStep * jw;
    else tw = (t0 > W) ? t0 - W : 0;
    float* __restrict__ snapw = (snap != nullptr && k + 1 < K) ? snap + ((int64_t)((head + 1) % kTpRing) * J * K + k) * B : nullptr;

    const uint32_t rowb = (uint32_t)B * 4u;
    const uint32_t boff = q.boff;
    V xc[NR], xn[NR], rc[NR], rn[NR], gc[NR], gn[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) { xc[i] = xn[i] = gc[i] = gn[i] = vsplat<V>(0.0f); rc[i] = rn[i] = vsplat<V>(1.0f); }
    const int64_t nfull_end = t1 - (t1 - tw) % NR;
    constexpr bool WIN = fused_x_window<DYN_R, TM, VEC4>();   // batch-major x: whole lines through LDS (XWindow)
    XWindow<V, WIN> xw(x, q, B, T);
    if constexpr (WIN) static_assert(NR == XWindow<V, true>::NR, "a window is N tiles");
    if (tw < nfull_end) {
        if constexpr (WIN) xw.first_issue(tw);
        else load_x_tile<V, TM, VEC4, NR>(x, q, B, T, tw, rowb, xn);
        if constexpr (DYN_R == 1) load_x_tile<V, TM, VEC4, NR>(r, q, B, T, tw, rowb, rn);
        if (tw >= t0) load_rows<V, NR>(target + tw * B, boff, rowb, gn);
    }
    if (warm_start) {
        // (valid = 1: one snapshot, taken as it is; 2: secant; 3: + parabola -- the missing ones alias the newest, unused)
        const int h2 = valid > 1 ? (head + kTpRing - 1) % kTpRing : head;
        const int h3 = valid > 2 ? (head + kTpRing - 2) % kTpRing : h2;
        z = load_own<V>(snap + (((int64_t)head * J + jw) * K + (k - 1)) * B, q);
        const V z2 = load_own<V>(snap + (((int64_t)h2 * J + jw) * K + (k - 1)) * B, q);
        const V z3 = load_own<V>(snap + (((int64_t)h3 * J + jw) * K + (k - 1)) * B, q);
        __builtin_amdgcn_sched_barrier(0);                  // (the tile's loads stay above: one flight)
        if (valid > 1) {                                    // extrapolated along the parameter path (tp_extrapolation)
            const TpExtrap e = tp_extrapolation(theta, c0, valid);
            const V zs = vfma(vsplat<V>(e.lam), z - z2, z);                       // secant
            if (e.quad) {
                const V zq = vfma(vsplat<V>(e.w3), z3 - z, vfma(vsplat<V>(e.w2), z2 - z, z));
                const V cq = zq - zs;                                             // what the parabola adds: kept where it is signal
                z = zs + vsel(vgt_c(vabs(cq), 4.0e-7f), cq, vsplat<V>(0.0f));
            } else {
                z = zs;
            }
        }
    } else if (tw == 0 && z0) {
        z = load_own<V>(z0, q);
    }
    int64_t t = tw;
    if constexpr (WIN) { if (tw < nfull_end) xw.first(tw, nfull_end, xn); }
    for (; t < t0 && t < nfull_end; t += NR) {              // ---- warm-up tiles: nothing summed, nothing stored
#pragma unroll
        for (int i = 0; i < NR; ++i) { xc[i] = xn[i]; if constexpr (DYN_R == 1) rc[i] = rn[i]; }
        if (t + NR < nfull_end) {
            if constexpr (WIN) xw.next(t + NR, nfull_end, xn);
            else load_x_tile<V, TM, VEC4, NR>(x, q, B, T, t + NR, rowb, xn);
            if constexpr (DYN_R == 1) load_x_tile<V, TM, VEC4, NR>(r, q, B, T, t + NR, rowb, rn);
            if (t + NR >= t0) load_rows<V, NR>(target + (t + NR) * B, boff, rowb, gn);   // the first owned tile's target
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) (void)fwd_step<DYN_R, SYM, V, FAST>(c, xc[i], rc[i], z);
    }
    publish_own<V>(zwarm + k * B, q, z);
    wait_vmcnt<0>();
    EvalSums<V> d;
    d.init();
    for (; t < nfull_end; t += NR) {                        // ---- owned tiles
#pragma unroll
        for (int i = 0; i < NR; ++i) { xc[i] = xn[i]; gc[i] = gn[i]; if constexpr (DYN_R == 1) rc[i] = rn[i]; }
        const bool more = t + NR < nfull_end;
        if (snapw != nullptr && t1 - t <= (int64_t)kWarmStep * (J - 1) && (t1 - t) % kWarmStep == 0)
            store_own<V>(snapw + ((t1 - t) / kWarmStep) * K * B, q, z);   // snapshot kWarmStep j steps before the chunk's end
        // (STORE_Y = false: y is null and no address is formed from it)
        [[maybe_unused]] const __amdgpu_buffer_rsrc_t ry = row_rsrc(STORE_Y ? y + t * B : nullptr);
        // steps of this tile below `skip` carry no loss: their number, a scalar
        const int64_t below = skip - t;
        const int n_masked = __builtin_amdgcn_readfirstlane((int)(below < 0 ? 0 : (below > NR ? NR : below)));
        // the next tile's loads at the TOP of this tile, a whole tile before their first use (vmcnt is one in-order counter)
        __builtin_amdgcn_sched_barrier(0);
        if (more) {
            if constexpr (WIN) xw.next(t + NR, nfull_end, xn);
            else load_x_tile<V, TM, VEC4, NR>(x, q, B, T, t + NR, rowb, xn);
            if constexpr (DYN_R == 1) load_x_tile<V, TM, VEC4, NR>(r, q, B, T, t + NR, rowb, rn);
            load_rows<V, NR>(target + (t + NR) * B, boff, rowb, gn);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const V yv = fwd_step<DYN_R, SYM, V, FAST>(c, xc[i], rc[i], z);
            if constexpr (STORE_Y) buf_store_nt(yv, ry, boff, i * rowb);
            d.add(yv, gc[i], step_loss_scale(i, n_masked, 1.0f));
        }
        // everything but this tile's NR stores has returned (clipper_fused_body: the wait on the back edge)
        wait_vmcnt<STORE_Y ? NR : 0>();
        if ((t + NR - t0) % kFlushSteps == 0) d.flush();
    }
    for (int64_t tt = nfull_end; tt < t1; ++tt) {           // tail of the last chunk (T % NR)
        const V xin = load_step<V, TM>(x, q, B, T, tt);
        const V rin = DYN_R == 1 ? load_step<V, TM>(r, q, B, T, tt) : vsplat<V>(1.0f);
        const V tg = load_own<V>(target + tt * B, q);
        const V yv = fwd_step<DYN_R, SYM, V, FAST>(c, xin, rin, z);
        if constexpr (STORE_Y) store_own<V>(y + tt * B, q, yv);
        d.add(yv, tg, tt >= skip ? 1.0f : 0.0f);
    }
    d.flush();
    publish_own<V>(zend + k * B, q, z);
    if (snapw != nullptr) store_own<V>(snapw, q, z);
    if (zT && t1 == T) store_own<V>(zT, q, z);
    eval_publish<V, VT<V>::N>(wpart, k, K, q.live, 0, d);
    // (one chunk: the tile's totals, for the finish inside this kernel)
    tot[0] = tot[1] = 0.0;
#pragma unroll
    for (int j = 0; j < VT<V>::N; ++j) { tot[0] += wave_sum_dpp(q.live ? d.S[j] : 0.0); tot[1] += wave_sum_dpp(q.live ? d.E[j] : 0.0); }
}

// tickets: [TpAcc (the verification's totals)][...]; gticket: the count of tiles through the finish -- zero before the first
// launch (wdf_clipper_eval_tp_ws_init) and left zero by every call.  A tile is the 64 * VT<V>::N sequences of one wave;
// grid (tiles, K), one chunk wave to a workgroup.  K > 1: the waves are done after their body, clipper_eval_finish_kernel
// follows.  K == 1: no boundary to verify -- the wave hands its tile's totals on itself.
template <int DYN_R, bool SYM, bool TM, bool VEC4, typename V, bool STORE_Y>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WDF_EVAL_WAVES, WDF_EVAL_WAVES))) void clipper_eval_tp_kernel(
    const float* __restrict__ x, const float* __restrict__ r, const float* theta, float fs, int n_up, int n_down,
    const float* __restrict__ target, int64_t skip, float* __restrict__ y, const float* __restrict__ z0, float* __restrict__ zT,
    float* zwarm, float* zend, TpStatus* __restrict__ status, TpCtl* ctl, float* snap, int J, unsigned* tickets, unsigned* gticket,
    float tol, int64_t B, int64_t T, int64_t K, int64_t L, int64_t W, int general, double* part, double* wpart, EvalOut out, int64_t skew)
{
    static_assert(!(TM && VEC4), "a time-major x has no 4-step rows to load");
    const int64_t k = blockIdx.y;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { status->fallback_ran = 0; status->pad = 0u; }   // (the finish launch counts)
    const ClipConsts c = load_consts(theta, fs, n_up, n_down);
    const int tier = root_tier<DYN_R, SYM>(c, general);     // wave-uniform, once per launch
    double tot[kEvalNP];
    bool ran = false;
    if constexpr (SYM && DYN_R != 1) {
        if (tier == kRootLean) {
            clipper_eval_body<DYN_R, SYM, TM, VEC4, kRootLean, V, STORE_Y>(c, x, r, target, y, z0, zT, zwarm, zend, theta, ctl, snap, J, B, T, L, W,
                                                                           skip, k, K, skew, wpart, tot);
            ran = true;
        }
    }
    if (!ran) {
        if (tier != kRootGeneral)
            clipper_eval_body<DYN_R, SYM, TM, VEC4, kRootFast, V, STORE_Y>(c, x, r, target, y, z0, zT, zwarm, zend, theta, ctl, snap, J, B, T, L, W,
                                                                           skip, k, K, skew, wpart, tot);
        else
            clipper_eval_body<DYN_R, SYM, TM, VEC4, kRootGeneral, V, STORE_Y>(c, x, r, target, y, z0, zT, zwarm, zend, theta, ctl, snap, J, B, T, L,
                                                                              W, skip, k, K, skew, wpart, tot);
    }
    if (K > 1) return;
    const TpFinishCtx fc{status, ctl, J, tickets, tol, K, L, W, tp_span_scheme(skew)};
    eval_tile_partial_and_finish(tot[0], tot[1], part, gticket, theta, out, fc);
}

// Re-run of chunk [t0, t1) for 64 sequences (one per lane, index b) from the exact state z: outputs, snapshots, the {S, E} slot
// (fused_rerun_chunk without the record).
template <int DYN_R, bool SYM, bool TM, int FAST, int NSEQ, bool STORE_Y>
__device__ __forceinline__ void eval_rerun_chunk(const ClipConsts& c_in, const float* __restrict__ x, const float* __restrict__ r,
                                                 const float* __restrict__ target, float* __restrict__ y, double* wpart,
                                                 float* __restrict__ snapw, int J, int64_t K, int64_t k, int64_t b, int64_t B, bool live,
                                                 int slot, int64_t T, int64_t t0, int64_t t1, int64_t skip, float& z)
{
    const ClipConstsSeq<float> c = make_seq_consts<DYN_R, float>(c_in, DYN_R == 2 ? load_one<TM>(r, b, B, T, 0) : 1.0f);
    EvalSums<float> d;
    d.init();
    for (int64_t t = t0; t < t1; t += kBlk) {
        if ((t - t0) % kWarmStep == 0) {
            d.flush();
            if (snapw != nullptr && t1 - t <= (int64_t)kWarmStep * (J - 1) && (t1 - t) % kWarmStep == 0)
                snapw[((t1 - t) / kWarmStep) * K * B + b] = z;
        }
        float xv[kBlk], rv[kBlk], gv[kBlk];
#pragma unroll
        for (int i = 0; i < kBlk; ++i) {
            const int64_t tt = (t + i < t1) ? t + i : t1 - 1;
            xv[i] = load_one<TM>(x, b, B, T, tt);
            rv[i] = DYN_R == 1 ? load_one<TM>(r, b, B, T, tt) : 1.0f;
            gv[i] = target[tt * B + b];
        }
#pragma unroll
        for (int i = 0; i < kBlk; ++i) {
            if (t + i < t1) {                                    // wave-uniform
                const float yv = fwd_step<DYN_R, SYM, float, FAST>(c, xv[i], rv[i], z);
                if constexpr (STORE_Y) y[(t + i) * B + b] = yv;
                d.add(yv, gv[i], (t + i >= skip) ? 1.0f : 0.0f);
            }
        }
    }
    d.flush();
    if (snapw != nullptr) snapw[b] = z;
    eval_publish<float, NSEQ>(wpart, k, K, live, slot, d);
}

// The rare path of the finish launch: the wave re-runs, in time order, every chunk of its tile that was entered more than tol
// off (fused_repair_tile's walk), behind the kernel boundary: the re-run rewrites rows that waves on another XCD wrote.
template <int DYN_R, bool SYM, bool TM, int NSEQ, bool STORE_Y>
__device__ __forceinline__ void eval_repair_tile(
    const float* __restrict__ x, const float* __restrict__ r, const float* theta, float fs, int n_up, int n_down,
    const float* __restrict__ target, int64_t skip, float* __restrict__ y, float* __restrict__ zT, const float* zwarm, float* zend,
    int64_t B, int64_t T, int64_t K, int64_t L, float tol, TpStatus* __restrict__ status, TpCtl* ctl, float* __restrict__ snap, int J,
    int general, int64_t skew, double* wpart, int64_t b_first, bool live, int lane)
{
    const ClipConsts c = load_consts(theta, fs, n_up, n_down);
    const int tier = root_tier<DYN_R, SYM>(c, general);
    // the ring slot the pass wrote its snapshots to (the control block is advanced by the wave that finishes the call: the last
    // of this launch's tiles through the ticket -- after every tile has read this)
    int slot = 0;
    if (ctl != nullptr && snap != nullptr) slot = ((ctl->geom == tp_geom_tag(K, J, tp_span_scheme(skew)) ? ctl->head : 0) + 1) % kTpRing;
    int nrep = 0;
#pragma unroll 1
    for (int h = 0; h < NSEQ; ++h) {
        const int64_t b = b_first + h;
        bool fixed_prev = false;
        float ze_fix = 0.0f;
        for (int64_t k = 1; k < K; ++k) {
            const float e = fixed_prev ? ze_fix : load_published(zend + (k - 1) * B + b);
            const float m = fabsf(load_published(zwarm + k * B + b) - e);
            fixed_prev = false;
            if (__builtin_amdgcn_ballot_w64(!(m <= tol)) == 0) continue;
            int64_t t0, t1;
            chunk_span(k, K, L, skew, T, t0, t1);
            float* __restrict__ snapw = (snap != nullptr && k + 1 < K) ? snap + ((int64_t)slot * J * K + k) * B : nullptr;
            float z = e;
            bool ran = false;
            if constexpr (SYM && DYN_R != 1) {
                if (tier == kRootLean) {
                    eval_rerun_chunk<DYN_R, SYM, TM, kRootLean, NSEQ, STORE_Y>(c, x, r, target, y, wpart, snapw, J, K, k, b, B, live, h, T, t0, t1, skip, z);
                    ran = true;
                }
            }
            if (!ran) {
                if (tier != kRootGeneral) eval_rerun_chunk<DYN_R, SYM, TM, kRootFast, NSEQ, STORE_Y>(c, x, r, target, y, wpart, snapw, J, K, k, b, B, live, h, T, t0, t1, skip, z);
                else eval_rerun_chunk<DYN_R, SYM, TM, kRootGeneral, NSEQ, STORE_Y>(c, x, r, target, y, wpart, snapw, J, K, k, b, B, live, h, T, t0, t1, skip, z);
            }
            __hip_atomic_store(zend + k * B + b, z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (zT && t1 == T) zT[b] = z;
            ze_fix = z;
            fixed_prev = true;
            ++nrep;
        }
    }
    if (lane == 0 && nrep) atomicAdd(&status->fallback_ran, nrep);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the re-written slots have landed (write-through)
}

// One wave per tile, grid (tiles), behind clipper_eval_tp_kernel with K > 1.
template <int DYN_R, bool SYM, bool TM, int NSEQ, bool STORE_Y>
__global__ __launch_bounds__(64) void clipper_eval_finish_kernel(
    const float* __restrict__ x, const float* __restrict__ r, const float* theta, float fs, int n_up, int n_down,
    const float* __restrict__ target, int64_t skip, float* __restrict__ y, float* __restrict__ zT, const float* zwarm, float* zend,
    int64_t B, int64_t T, int64_t K, int64_t L, float tol, TpStatus* __restrict__ status, TpCtl* ctl, float* __restrict__ snap, int J,
    unsigned* tickets, unsigned* gticket, int general, double* part, double* wpart, EvalOut out, int64_t skew, int64_t W)
{
    const int lane = threadIdx.x;
    const int64_t raw = ((int64_t)blockIdx.x * 64 + lane) * NSEQ;
    const bool live = raw < B;
    const int64_t b_first = live ? raw : B - NSEQ;
    // ---- the tile's chunk boundaries, |zwarm[k] - zend[k - 1]| <= tol: tp_verify_tile<DYN_R, NSEQ, DEFER>'s check with K an
    // argument (this launch has no chunk axis): 31 boundaries' loads in flight together
    float miss = 0.0f;
    int nbad = 0;
    constexpr int kBatch = 31;
    for (int64_t k0 = 1; k0 < K; k0 += kBatch) {
        float zw[kBatch][NSEQ], ze[kBatch][NSEQ];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int64_t k = (k0 + j < K) ? k0 + j : K - 1;   // clamped: re-reads the last boundary
            load_published_row<NSEQ>(zwarm + k * B, (uint32_t)b_first * 4u, zw[j]);
            load_published_row<NSEQ>(zend + (k - 1) * B, (uint32_t)b_first * 4u, ze[j]);
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j)
#pragma unroll
            for (int h = 0; h < NSEQ; ++h) {
                const float m = fabsf(zw[j][h] - ze[j][h]);
                if (k0 + j < K) {
                    miss = fmaxf(miss, m);
                    nbad += !(m <= tol) ? 1 : 0;                // NaN counts as bad
                }
            }
    }
    const float tile_miss = wave_max_dpp(miss);
    const int tile_bad_pairs = wave_sum_dpp(nbad);
    if (lane == 0) {                                         // the tile's share of the verification totals
        TpAcc* acc = reinterpret_cast<TpAcc*>(tickets);
        if (tile_miss > 0.0f) (void)atomicMax(&acc->max_miss_bits, __float_as_int(tile_miss));
        if (tile_bad_pairs) (void)atomicAdd(&acc->n_bad, (unsigned)tile_bad_pairs);
    }
    if (tile_bad_pairs != 0)
        eval_repair_tile<DYN_R, SYM, TM, NSEQ, STORE_Y>(x, r, theta, fs, n_up, n_down, target, skip, y, zT, zwarm, zend, B, T, K, L, tol, status,
                                                        ctl, snap, J, general, skew, wpart, b_first, live, lane);
    // ---- the tile's slots over the chunks, in a fixed order: lane i takes chunks i, i + 64, ... (slots in order), then the wave's tree
    const double* w = wpart + (int64_t)blockIdx.x * K * NSEQ * kEvalNP;
    double S = 0.0, E = 0.0;
    for (int64_t kk = lane; kk < K; kk += 64)
#pragma unroll
        for (int h = 0; h < NSEQ; ++h) {
            S += __hip_atomic_load(w + (kk * NSEQ + h) * kEvalNP + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            E += __hip_atomic_load(w + (kk * NSEQ + h) * kEvalNP + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    S = wave_sum_dpp(S);
    E = wave_sum_dpp(E);
    const TpFinishCtx fc{status, ctl, J, tickets, tol, K, L, W, tp_span_scheme(skew)};
    eval_tile_partial_and_finish(S, E, part, gticket, theta, out, fc);
}

}  // namespace wdf
