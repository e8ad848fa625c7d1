// wdf_capi_clipper.hip -- C ABI of the diode-clipper sequence kernels (csrc/wdf_clipper.h, csrc/wdf_clipper_fused.h): sequential and
// time-parallel forward / reverse sweep, the one-pass training step.  Argument checking, workspace layouts, template dispatch
// and launches.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <cstddef>
#include "wdf_capi_common.h"
#include "wdf_clipper.h"
#include "wdf_clipper_fused.h"
#include "wdf_capi_clipper_step.h"
#include "wdf_omega64.h"
using namespace wdfcapi;

namespace {

template <bool DYN_R, bool SYM, bool TM, bool V4>
void launch_fwd(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down, float* y,
                float* zstash, const float* z0, float* zT, int64_t B, int64_t T, int general, hipStream_t s)
{
    EventBracket bracket(s);
    dispatch([&](auto STASH) {
        hipLaunchKernelGGL((wdf::clipper_fwd_kernel<DYN_R, SYM, TM, V4, STASH()>), dim3(waves64(B)), dim3(64), 0, s, x, r, theta,
                           fs, n_up, n_down, y, zstash, z0, zT, B, T, general);
    }, Bools{zstash != nullptr});
}

template <bool DYN_R, bool SYM, bool TM, bool V4>
void launch_bwd(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down,
                const float* zstash, const float* gy, double* ws, float* gz0, const float* gzT, int64_t B, int64_t T,
                hipStream_t s)
{
    EventBracket bracket(s);
    hipLaunchKernelGGL((wdf::clipper_bwd_kernel<DYN_R, SYM, TM, V4>), dim3(waves64(B)), dim3(64), 0, s, x, r, theta, fs,
                       n_up, n_down, zstash, gy, ws, gz0, gzT, B, T);
}

int check_common(const float* x, const float* theta, int n_up, int n_down, int64_t B, int64_t T, int flags)
{
    if (!x || !theta) return fail(WDF_EINVAL, "null x/theta");
    if (B <= 0 || T <= 0) return fail(WDF_EINVAL, "B and T must be positive (got B=%lld T=%lld)", (long long)B, (long long)T);
    if (B > (int64_t)64 * 0x7fffffff) return fail(WDF_EINVAL, "B too large");
    if (n_up < 1 || n_down < 1 || n_up > 16 || n_down > 16) return fail(WDF_EINVAL, "n_up/n_down must be in [1,16]");
    if (flags & ~(WDF_X_TIME_MAJOR | WDF_PREC_F64 | WDF_GENERAL_ROOT)) return fail(WDF_EINVAL, "unknown flag bits 0x%x", flags);
    return WDF_OK;
}

// ---- time-parallel clipper (chunk lengths and warm-ups: multiples of wdf::kTile steps) ------------

// (TpWarm, tp_ticket_bytes, tp_state: wdf_capi_clipper_step.h -- the evaluation pass takes the same warm-start state)

// the forward's workspace: zwarm [K][B], zend [K][B], then (stateless calls) the tile tickets
struct TpFwdWs { float* zwarm; float* zend; unsigned* tickets; size_t bytes; };
inline TpFwdWs tp_fwd_ws(void* ws, int64_t B, int K)
{
    Carver c(ws);
    TpFwdWs w;
    w.zwarm = c.take<float>((size_t)K * (size_t)B);
    w.zend = c.take<float>((size_t)K * (size_t)B);
    w.tickets = c.take<unsigned>(tp_ticket_bytes(B) / sizeof(unsigned));
    w.bytes = c.off;
    return w;
}

template <bool DYN_R, bool SYM, bool TM, bool V4>
void launch_fwd_tp(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down, float* y,
                   float* zstash, const float* z0, float* zT, float* zwarm, float* zend, wdf::TpStatus* status,
                   float tol, int64_t B, int64_t T, ChunkGeom g, int64_t W, TpWarm warm, unsigned* tickets, int general,
                   hipStream_t s)
{
    const dim3 grid(waves64(B), (unsigned)g.K);
    // a stateless call (no warm-start block to steer): the chunk boundaries are verified by the launch behind the forward
    const int later = (warm.ctl == nullptr && g.K > 1) ? 1 : 0;
    dispatch([&](auto STASH) {
        {
            EventBracket bracket(s);
            hipLaunchKernelGGL((wdf::clipper_fwd_tp_kernel<DYN_R, SYM, TM, V4, STASH(), float>), grid, dim3(64), 0, s, x, r, theta, fs, n_up,
                               n_down, y, zstash, z0, zT, zwarm, zend, status, warm.ctl, warm.snap, warm.J, tickets, tol, B, B, T, g.L, W,
                               general, later);
        }
        if (g.K > 1)                            // blocks of unflagged tiles (normally all of them) leave at once
            hipLaunchKernelGGL((wdf::clipper_tp_repair_kernel<DYN_R, SYM, TM, STASH()>), dim3(grid.x), dim3(64), 0, s, x, r, theta, fs, n_up,
                               n_down, y, zstash, zT, zwarm, zend, B, T, (int64_t)g.K, g.L, tol, status, warm.ctl, warm.snap, warm.J,
                               tickets, general, later);
    }, Bools{zstash != nullptr});
}

template <bool DYN_R, bool SYM, bool TM, bool V4>
void launch_bwd_tp(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down,
                   const float* zstash, const float* gy, const float* target, const float* zT, float gscale,
                   float* part, double* ws, float* gz0, int64_t B, int64_t T, ChunkGeom g, const float* gcoef,
                   int64_t skip, unsigned* tickets, float* gtheta, int accumulate, float* sse_out, wdf::AdamTail adam,
                   int general, hipStream_t s)
{
    const dim3 grid(waves64(B), (unsigned)g.K);
    // ONE launch: the sweep; the last chunk wave of every tile combines the tile's chunk records, the last
    // tile reduces, applies the chain rule and (optionally) Adam
    EventBracket bracket(s);
    dispatch([&](auto LOSS) {                                  // 0: gy given, 1: MSE, 2: MSE + ESR
        hipLaunchKernelGGL((wdf::clipper_bwd_tp_kernel<DYN_R, SYM, TM, V4, LOSS(), float>), grid, dim3(64), 0, s, x, r, theta, fs, n_up, n_down,
                           zstash, gy, target, zT, gscale, part, B, B, T, g.L, gcoef, skip, tickets, ws, gz0, gtheta, accumulate, sse_out,
                           adam, general);
    }, Values<int, 0, 1, 2>{gcoef ? 2 : (target ? 1 : 0)});
}

inline size_t bwd_ticket_bytes(int64_t B) { return round_up((waves64(B) + 4) * sizeof(unsigned), 64); }

// the reverse sweep's workspace: [tiles][4] doubles, [K][9][B] floats, then -- on a 64-byte line -- the tickets (tiles done + one per tile)
struct TpBwdWs { double* sums; float* part; unsigned* tickets; size_t bytes; };
inline TpBwdWs tp_bwd_ws(void* ws, int64_t B, int K)
{
    Carver c(ws);
    TpBwdWs w;
    w.sums = c.take<double>(waves64(B) * 4);
    w.part = c.take<float>((size_t)K * wdf::kTpOut * (size_t)B);
    c.align(64);
    w.tickets = c.take<unsigned>(bwd_ticket_bytes(B) / sizeof(unsigned));
    w.bytes = c.off;
    return w;
}

// ---- the one-pass training step (wdf_clipper_fused.h) --------------------------------------------
struct FusedWs { double* part; double* wpart; float* zwarm; float* zend; float* rec; unsigned* tickets; unsigned* gticket; size_t clear_bytes;
                 wdf::FusedGroupWs grp; size_t bytes; };

// chunk waves per workgroup of the group form, and the groups a tile then has
inline int fused_group_waves(int K) { return std::min(wdf::kGroupWaves, K); }
inline int fused_groups(int K) { return (K + fused_group_waves(K) - 1) / fused_group_waves(K); }

// ONE layout for both losses (sized for the larger, MSE + ESR; a workspace may serve either from call to call):
// [tiles][8] doubles (the tiles' sums; MSE uses 4 of them), [tiles][K][slots][8] doubles (the chunk waves' own sums, one set
// per sequence slot of a lane), zwarm / zend [K][B], the records (16-byte granules [K][3][lanes], lanes <= 64 x ceil(B / 64)),
// then -- on a 64-byte line: wdf_clipper_step_mse_tp_ws_init clears these -- the tile tickets and the step's ticket line.
// Behind them what the group form's workgroups hand to their finish launch, per group of chunks as the areas above are per
// chunk: the group records, the groups' own sums, their verdicts (8 bytes per tile and group).
inline FusedWs fused_ws(void* ws, int64_t B, int K)
{
    const size_t tiles = waves64(B) + 1;                       // >= tiles x slots for either lane form
    Carver c(ws);
    FusedWs w;
    w.part = c.take<double>(tiles * 8);
    w.wpart = c.take<double>(tiles * (size_t)K * wdf::kFsPartEsr);
    w.zwarm = c.take<float>((size_t)K * (size_t)B);
    w.zend = c.take<float>((size_t)K * (size_t)B);
    w.rec = c.take<float>((size_t)K * wdf::kFsQuads * (waves64(B) * 64) * 4);
    c.align(64);
    const size_t tickets_at = c.off;
    w.tickets = c.take<unsigned>(tp_ticket_bytes(B) / sizeof(unsigned));
    w.gticket = c.take<unsigned>(16);
    w.clear_bytes = c.off - tickets_at;
    c.align(16);
    const size_t Kg = (size_t)fused_groups(K);
    w.grp.rec = c.take<float>(Kg * wdf::kFsQuads * (waves64(B) * 64) * 4);
    w.grp.part = c.take<double>(tiles * Kg * wdf::kFsPartEsr);
    w.grp.verdict = c.take<unsigned long long>(tiles * Kg);
    w.bytes = c.off;
    return w;
}

// The form of the one-pass step's launches (launch_fused).  window: x goes through a per-workgroup window in LDS (those launches
// keep one chunk wave to a workgroup); n_waves: chunk waves of the launch.  WDF_FUSED_FINISH = group | launch | inkernel names the
// form (read at every call: tests and A/B runs switch it inside one process).  Unset: the finish launch of round 6.  The group
// form is opt-in: at the headline shape it was measured 0.3 - 0.8 us ahead of that form on the same build, inside the spread
// (profiles/README.md), and in workgroups of eight a launch of fewer than two chunk waves per SIMD leaves CUs idle.
inline int fused_form(int K, bool window)
{
    if (K < 2) return wdf::kFusedInKernel;                   // one chunk: no boundary, no record walk, no second launch
    const char* e = getenv("WDF_FUSED_FINISH");
    if (e == nullptr) return wdf::kFusedFinishLater;
    if (strcmp(e, "inkernel") == 0) return wdf::kFusedInKernel;
    return (strcmp(e, "group") == 0 && !window) ? wdf::kFusedGroup : wdf::kFusedFinishLater;
}

// Skewed chunk spans (wdf_clipper_fused.h, chunk_span): only when the launch puts about two chunk waves on every SIMD --
// that is the situation the skew answers -- the chunk count is even, the ragged last chunk keeps more than `skew` steps and
// the shorter chunks still hold the warm-start snapshots.  WDF_FUSED_SKEW=0 switches it off, =force applies it whenever
// the geometry allows (tests).  grouped (the group form, whole groups only): the long and the short spans alternate by half
// groups, returned as a negative skew.
inline int64_t fused_skew(int64_t n_waves, int K, int64_t L, int64_t T, int max_warm_tiles, bool grouped)
{
    static const int mode = []() { const char* e = getenv("WDF_FUSED_SKEW"); return !e ? 1 : (strcmp(e, "force") == 0 ? 2 : atoi(e) != 0); }();
    if (mode == 0 || K < 2 || (K & 1)) return 0;
    if (grouped && K % wdf::kGroupWaves != 0) return 0;
    if (mode == 1) {
        static const int n_simd = []() { int dev = 0, cus = 256; (void)hipGetDevice(&dev);
                                         (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev); return 4 * cus; }();
        if (2 * n_waves <= 3 * (int64_t)n_simd || 2 * n_waves > 5 * (int64_t)n_simd) return 0;
    }
    static const int64_t steps = []() { const char* e = getenv("WDF_FUSED_SKEW_STEPS"); return e ? (int64_t)atoi(e) : (int64_t)-1; }();   // (A/B runs)
    const int64_t skew = (steps >= 0 ? steps : L / 4) / wdf::kTile * wdf::kTile;
    if (skew <= 0 || skew >= L) return 0;
    if (T - (int64_t)(K - 1) * L <= skew) return 0;                                   // the last chunk would be empty
    if ((int64_t)max_warm_tiles * wdf::kWarmStep > L - skew) return 0;                      // snapshots reach further back than the short chunks
    return grouped ? -skew : skew;
}

template <int DYN_R, bool SYM, bool TM, bool V4>
void launch_fused(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down, const float* target,
                  float hgs, int64_t skip, float* y, const float* z0, float* zT, FusedWs w, wdf::TpStatus* status, float tol,
                  int64_t B, int64_t T, ChunkGeom g, int64_t W, TpWarm warm, int general, bool pairs, bool esr, wdf::FusedOut out,
                  int64_t skew, int form, hipStream_t s)
{
    // pairs: two adjacent sequences per lane, packed fp32 arithmetic (wdf_clipper_fused.h); a tile is then 128 sequences
    const int per_tile = pairs ? 128 : 64;
    // The step's tail (verification, walk over the chunk records, reduction, chain rule, warm-start steering, Adam) and the repair
    // of missed tiles are ONE launch behind the chunk kernel.  WDF_FUSED_FINISH picks the form:
    //   group    G = min(8, K) chunk waves to a workgroup, which combine in LDS (wdf_clipper_fused.h, fused_group_compose); the finish
    //            launch walks ceil(K / G) group records per tile with one wave (clipper_fused_group_finish_kernel).  Opt-in;
    //            not where x goes through a per-workgroup window in LDS (batch-major x in 16-byte rows): those launches
    //            take the next form.
    //   launch   round 6, the default: one chunk wave to a workgroup, several finishing waves per tile (clipper_fused_finish_kernel).
    //   inkernel round 5: the tile's last chunk wave does the tail, an idle repair launch follows.
    // (fused_form above reads it.)
    const int G = form == wdf::kFusedGroup ? fused_group_waves(g.K) : 1;
    const dim3 grid((unsigned)((B + per_tile - 1) / per_tile), (unsigned)((g.K + G - 1) / G));
    // waves per tile of the finish launch: the chunks spread over as many of the kFinMaxWaves as leaves each at least kFinMinSeg
    // records (32 chunks: 8 waves of 4; 128: 8 waves of 16 in two register batches)
    const int fin_waves = (int)std::min<int64_t>(wdf::kFinMaxWaves, (g.K + wdf::kFinMinSeg - 1) / wdf::kFinMinSeg);
    dispatch([&](auto PAIRS, auto LOSS) {                      // LOSS 1: MSE, 2: MSE + ESR
        using V = std::conditional_t<PAIRS(), wdf::v2f, float>;
        constexpr int N = PAIRS() ? 2 : 1;                     // sequences per lane
        const size_t lds = form == wdf::kFusedGroup ? (size_t)G * sizeof(wdf::GroupStage<N, LOSS()>) : 0;
        {
            EventBracket bracket(s);
            hipLaunchKernelGGL((wdf::clipper_fused_tp_kernel<DYN_R, SYM, TM, V4, V, LOSS()>), grid, dim3(64 * G), lds, s, x, r, theta, fs, n_up,
                               n_down, target, hgs, skip, y, z0, zT, w.zwarm, w.zend, w.rec, status, warm.ctl, warm.snap, warm.J, w.tickets,
                               w.gticket, tol, B, T, (int64_t)g.K, g.L, W, general, w.part, out, skew, w.wpart, form, w.grp);
        }
        if (form == wdf::kFusedGroup)
            hipLaunchKernelGGL((wdf::clipper_fused_group_finish_kernel<DYN_R, SYM, TM, N, LOSS()>), dim3(grid.x), dim3(64), 0, s, x, r, theta, fs,
                               n_up, n_down, target, hgs, skip, y, zT, w.zwarm, w.zend, w.rec, B, T, (int64_t)g.K, g.L, tol, status, warm.ctl,
                               warm.snap, warm.J, w.tickets, w.gticket, general, w.part, out, skew, w.wpart, W, G, w.grp);
        else if (form == wdf::kFusedFinishLater)
            hipLaunchKernelGGL((wdf::clipper_fused_finish_kernel<DYN_R, SYM, TM, N, LOSS()>), dim3(grid.x), dim3(64 * fin_waves), 0, s, x, r,
                               theta, fs, n_up, n_down, target, hgs, skip, y, zT, w.zwarm, w.zend, w.rec, B, T, (int64_t)g.K, g.L, tol,
                               status, warm.ctl, warm.snap, warm.J, w.tickets, w.gticket, general, w.part, out, skew, w.wpart, W);
        else if (g.K > 1)                       // blocks of unflagged tiles (normally all of them) leave at once
            hipLaunchKernelGGL((wdf::clipper_fused_repair_kernel<DYN_R, SYM, TM, N, LOSS()>), dim3(grid.x), dim3(64), 0, s, x, r, theta, fs,
                               n_up, n_down, target, hgs, skip, y, zT, w.zwarm, w.zend, w.rec, B, T, (int64_t)g.K, g.L, tol, status,
                               warm.ctl, warm.snap, warm.J, w.tickets, w.gticket, general, w.part, out, skew, w.wpart, W);
    }, Bools{pairs}, Values<int, 1, 2>{esr ? 2 : 1});
}

// theta: the parameters the step's last wave updates in place when the caller passed Adam's m (adam_check: with v, step and lr)
wdf::AdamTail adam_tail(float* theta, float* m, float* v, int32_t* step, const float* lr, float beta1, float beta2, float eps, const float* lo,
                        const float* hi)
{
    return wdf::AdamTail{m ? theta : nullptr, m, v, step, lr, beta1, beta2, eps, lo, hi};
}

}  // namespace

extern "C" {
#ifdef WDF_DBG_TIMES
__attribute__((visibility("default"))) int wdf_debug_set_times(void* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(wdf::g_dbg_times), &p, sizeof(p)); }
#endif

int wdf_clipper_fwd(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down, float* y,
                    float* zstash, const float* z0, float* zT, int64_t B, int64_t T, int flags, void* stream)
{
    int rc = check_common(x, theta, n_up, n_down, B, T, flags);
    if (rc) return rc;
    if (!y) return fail(WDF_EINVAL, "null y");
    if (!(fs > 0.0f)) return fail(WDF_EINVAL, "fs must be positive");
    const bool tm = flags & WDF_X_TIME_MAJOR;
    if (flags & WDF_PREC_F64) {                  // tree and root in fp64 (csrc/wdf_omega64.h): the on-device accuracy reference
        dispatch([&](auto DYN, auto TM) {
            hipLaunchKernelGGL((wdf::clipper_fwd_f64_kernel<DYN(), TM()>), dim3(waves64(B)), dim3(64), 0, (hipStream_t)stream, x, r, theta, fs, n_up, n_down, y, zstash, z0, zT, B, T);
        }, Bools{r != nullptr}, Bools{tm});
        return check_launch("wdf_clipper_fwd (fp64)");
    }
    const bool v4 = !tm && (T % 4 == 0) && aligned16(x) && (!r || aligned16(r));
    const bool ok = dispatch4([&](auto DYN, auto SYM, auto TM, auto V4) {
        launch_fwd<DYN(), SYM(), TM(), V4()>(x, r, theta, fs, n_up, n_down, y, zstash, z0, zT, B, T, (flags & WDF_GENERAL_ROOT) ? 1 : 0,
                                             (hipStream_t)stream);
    }, Bools{r != nullptr}, n_up == n_down, tm, v4);
    return ok ? check_launch("wdf_clipper_fwd") : no_kernel("wdf_clipper_fwd");
}

size_t wdf_clipper_bwd_ws_bytes(int64_t B) { return B > 0 ? waves64(B) * 4 * sizeof(double) : 0; }

int wdf_clipper_bwd(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down,
                    const float* zstash, const float* gy, void* ws, float* gtheta, float* gz0, const float* gzT,
                    int accumulate, int64_t B, int64_t T, int flags, void* stream)
{
    int rc = check_common(x, theta, n_up, n_down, B, T, flags);
    if (rc) return rc;
    if (!zstash || !gy || !ws || !gtheta) return fail(WDF_EINVAL, "null zstash/gy/ws/gtheta");
    if (!(fs > 0.0f)) return fail(WDF_EINVAL, "fs must be positive");
    const bool tm = flags & WDF_X_TIME_MAJOR;
    if (flags & WDF_PREC_F64) {                  // the adjoint in fp64 (csrc/wdf_omega64.h): the on-device accuracy reference
        dispatch([&](auto DYN, auto TM) {
            hipLaunchKernelGGL((wdf::clipper_bwd_f64_kernel<DYN(), TM()>), dim3(waves64(B)), dim3(64), 0, (hipStream_t)stream, x, r, theta, fs, n_up, n_down, zstash, gy, (double*)ws, gz0, gzT, B, T);
        }, Bools{r != nullptr}, Bools{tm});
    } else {
        const bool v4 = !tm && (T % 4 == 0) && aligned16(x) && (!r || aligned16(r));
        const bool ok = dispatch4([&](auto DYN, auto SYM, auto TM, auto V4) {
            launch_bwd<DYN(), SYM(), TM(), V4()>(x, r, theta, fs, n_up, n_down, zstash, gy, (double*)ws, gz0, gzT, B, T, (hipStream_t)stream);
        }, Bools{r != nullptr}, n_up == n_down, tm, v4);
        if (!ok) return no_kernel("wdf_clipper_bwd");
    }
    rc = check_launch("wdf_clipper_bwd");
    if (rc) return rc;
    const int nparts = (int)waves64(B);
    hipLaunchKernelGGL(wdf::clipper_grad_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream,
                       (const double*)ws, nparts, theta, fs, r != nullptr ? 1 : 0, gtheta, accumulate,
                       (float*)nullptr);
    return check_launch("wdf_clipper_grad_reduce");
}

int wdf_clipper_tp_chunks(int64_t T, int n_chunks) { return T > 0 ? chunk_geom(T, n_chunks, wdf::kTile).K : 0; }
int wdf_clipper_tp_warm_unit(void) { return wdf::kWarmStep; }

size_t wdf_clipper_fwd_tp_ws_bytes(int64_t B, int n_chunks)
{
    return (B > 0 && n_chunks > 0) ? tp_fwd_ws(nullptr, B, n_chunks).bytes : 0;
}

static int fwd_tp_common(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down, float* y,
                         float* zstash, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup,
                         float tol, void* ws, void* status, void* state, int max_warm_tiles, int flags, void* stream)
{
    int rc = check_common(x, theta, n_up, n_down, B, T, flags);
    if (rc) return rc;
    if (!y || !ws || !status) return fail(WDF_EINVAL, "null y/ws/status");
    if (!(fs > 0.0f)) return fail(WDF_EINVAL, "fs must be positive");
    if (n_chunks < 1 || warmup < 0 || !(tol >= 0.0f)) return fail(WDF_EINVAL, "n_chunks >= 1, warmup >= 0, tol >= 0");
    if (B >= ((int64_t)1 << 24)) return fail(WDF_EINVAL, "the time-parallel forward addresses a 16-row tile with 32-bit offsets: B < 2^24");
    if (flags & WDF_PREC_F64) return fail(WDF_EUNSUPPORTED, "WDF_PREC_F64 applies to wdf_clipper_fwd and wdf_omega_f64 only");
    const ChunkGeom g = chunk_geom(T, n_chunks, wdf::kTile);
    const int64_t W = round_up((int64_t)warmup, wdf::kTile);
    const TpFwdWs w = tp_fwd_ws(ws, B, g.K);
    TpWarm warm{nullptr, nullptr, 1};
    unsigned* tickets = w.tickets;
    if (state) {
        if (max_warm_tiles < 1 || max_warm_tiles > wdf::kTpMaxWarmTiles)
            return fail(WDF_EINVAL, "max_warm_tiles must be in 1..%d", wdf::kTpMaxWarmTiles);
        if (g.K >= (1 << 20)) return fail(WDF_EINVAL, "too many chunks for a warm-start state");
        const TpState st = tp_state(state, B, 0);
        tickets = st.tickets;                                                // zeroed by the reset, left clean by every launch
        warm = TpWarm{st.ctl, st.snap, max_warm_tiles + 1};
    } else if (g.K <= 1) {                  // (stateless: verified by the launch behind the forward, no tickets; one chunk: no boundaries --
        if ((rc = memset_async(tickets, 0, tp_ticket_bytes(B), (hipStream_t)stream))) return rc;   //  the last tile's ticket still counts the tiles)
    }
    const bool tm = (flags & WDF_X_TIME_MAJOR) != 0;
    const bool v4 = !tm && (T % 4 == 0) && T < (1 << 23) && aligned16(x) && (!r || aligned16(r));
    const bool ok = dispatch4([&](auto DYN, auto SYM, auto TM, auto V4) {
        launch_fwd_tp<DYN(), SYM(), TM(), V4()>(x, r, theta, fs, n_up, n_down, y, zstash, z0, zT, w.zwarm, w.zend, (wdf::TpStatus*)status, tol, B,
                                                T, g, W, warm, tickets, (flags & WDF_GENERAL_ROOT) ? 1 : 0, (hipStream_t)stream);
    }, Bools{r != nullptr}, n_up == n_down, tm, v4);
    return ok ? check_launch("wdf_clipper_fwd_tp") : no_kernel("wdf_clipper_fwd_tp");
}

int wdf_clipper_fwd_tp(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down, float* y,
                       float* zstash, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup,
                       float tol, void* ws, void* status, int flags, void* stream)
{
    return fwd_tp_common(x, r, theta, fs, n_up, n_down, y, zstash, z0, zT, B, T, n_chunks, warmup, tol, ws, status,
                         nullptr, 0, flags, stream);
}

size_t wdf_clipper_fwd_tp_state_bytes(int64_t B, int n_chunks, int max_warm_tiles)
{
    if (B <= 0 || n_chunks <= 0 || max_warm_tiles < 1 || max_warm_tiles > wdf::kTpMaxWarmTiles) return 0;
    return tp_state(nullptr, B, (size_t)wdf::kTpRing * (size_t)(max_warm_tiles + 1) * (size_t)n_chunks * (size_t)B).bytes;
}

int wdf_clipper_fwd_tp_state_reset(void* state, int64_t B, int min_warm_tiles, void* stream)
{
    if (!state || B <= 0) return fail(WDF_EINVAL, "null state / bad B");
    if (min_warm_tiles < 0 || min_warm_tiles > wdf::kTpMaxWarmTiles) return fail(WDF_EINVAL, "min_warm_tiles must be in 0..%d", wdf::kTpMaxWarmTiles);
    if (int rc = memset_async(state, 0, tp_state(nullptr, B, 0).bytes, (hipStream_t)stream)) return rc;
    if (min_warm_tiles > 0 &&
        hipMemsetD32Async((hipDeviceptr_t)((char*)state + offsetof(wdf::TpCtl, j_floor)), min_warm_tiles, 1, (hipStream_t)stream) != hipSuccess)
        return fail(WDF_ELAUNCH, "hipMemsetD32Async failed");
    return WDF_OK;
}

int wdf_clipper_fwd_tp_warm(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down, float* y,
                            float* zstash, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks, int warmup,
                            float tol, void* ws, void* status, void* state, int max_warm_tiles, int flags, void* stream)
{
    if (!state) return fail(WDF_EINVAL, "null state");
    const ChunkGeom g = chunk_geom(T, n_chunks, wdf::kTile);
    if ((int64_t)max_warm_tiles * wdf::kWarmStep > g.L)
        return fail(WDF_EINVAL, "max_warm_tiles * 16 must not exceed the chunk length (%lld)", (long long)g.L);
    return fwd_tp_common(x, r, theta, fs, n_up, n_down, y, zstash, z0, zT, B, T, n_chunks, warmup, tol, ws, status, state,
                         max_warm_tiles, flags, stream);
}

static int bwd_tp_common(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down,
                         const float* zstash, const float* gy, const float* target, const float* zT, float gscale,
                         void* ws, float* gtheta, float* sse, float* gz0, int accumulate, int64_t B, int64_t T,
                         int n_chunks, int flags, void* stream, const float* gcoef = nullptr, int64_t skip = 0,
                         wdf::AdamTail adam = wdf::AdamTail{});

size_t wdf_clipper_bwd_tp_ws_bytes(int64_t B, int n_chunks)
{
    return (B > 0 && n_chunks > 0) ? tp_bwd_ws(nullptr, B, n_chunks).bytes : 0;
}

int wdf_clipper_bwd_tp_ws_init(void* ws, int64_t B, int n_chunks, void* stream)
{
    if (!ws || B <= 0 || n_chunks <= 0) return fail(WDF_EINVAL, "null ws / bad B, n_chunks");
    return memset_async(tp_bwd_ws(ws, B, n_chunks).tickets, 0, bwd_ticket_bytes(B), (hipStream_t)stream);
}

int wdf_clipper_bwd_tp(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down,
                       const float* zstash, const float* gy, void* ws, float* gtheta, float* gz0, int accumulate,
                       int64_t B, int64_t T, int n_chunks, int flags, void* stream)
{
    if (!gy) return fail(WDF_EINVAL, "null gy");
    return bwd_tp_common(x, r, theta, fs, n_up, n_down, zstash, gy, nullptr, nullptr, 0.0f, ws, gtheta, nullptr, gz0,
                         accumulate, B, T, n_chunks, flags, stream);
}

int wdf_clipper_bwd_mse_tp(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down,
                           const float* zstash, const float* zT, const float* target, float gscale, void* ws,
                           float* gtheta, float* sse, float* gz0, int accumulate, int64_t B, int64_t T, int n_chunks,
                           int flags, void* stream)
{
    if (!zT || !target) return fail(WDF_EINVAL, "null zT/target");
    return bwd_tp_common(x, r, theta, fs, n_up, n_down, zstash, nullptr, target, zT, gscale, ws, gtheta, sse, gz0,
                         accumulate, B, T, n_chunks, flags, stream);
}

static int bwd_tp_common(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down,
                         const float* zstash, const float* gy, const float* target, const float* zT, float gscale,
                         void* ws, float* gtheta, float* sse, float* gz0, int accumulate, int64_t B, int64_t T,
                         int n_chunks, int flags, void* stream, const float* gcoef, int64_t skip, wdf::AdamTail adam)
{
    int rc = check_common(x, theta, n_up, n_down, B, T, flags);
    if (rc) return rc;
    if (!zstash || !ws || !gtheta) return fail(WDF_EINVAL, "null zstash/ws/gtheta");
    if (!(fs > 0.0f)) return fail(WDF_EINVAL, "fs must be positive");
    if (n_chunks < 1) return fail(WDF_EINVAL, "n_chunks >= 1");
    if (B >= ((int64_t)1 << 30)) return fail(WDF_EINVAL, "time-parallel kernels address a [B] row with 32-bit byte offsets: B < 2^30");
    if (flags & WDF_PREC_F64) return fail(WDF_EUNSUPPORTED, "WDF_PREC_F64 applies to wdf_clipper_fwd and wdf_omega_f64 only");
    const ChunkGeom g = chunk_geom(T, n_chunks, wdf::kTile);
    const TpBwdWs w = tp_bwd_ws(ws, B, n_chunks);                   // (laid out for n_chunks, as wdf_clipper_bwd_tp_ws_init cleared it)
    const bool tm = (flags & WDF_X_TIME_MAJOR) != 0;
    const bool v4 = !tm && (T % 4 == 0) && aligned16(x) && (!r || aligned16(r));
    const bool ok = dispatch4([&](auto DYN, auto SYM, auto TM, auto V4) {
        launch_bwd_tp<DYN(), SYM(), TM(), V4()>(x, r, theta, fs, n_up, n_down, zstash, gy, target, zT, gscale, w.part, w.sums, gz0, B, T, g, gcoef,
                                                skip, w.tickets, gtheta, accumulate, target ? sse : nullptr, adam,
                                                (flags & WDF_GENERAL_ROOT) ? 1 : 0, (hipStream_t)stream);
    }, Bools{r != nullptr}, n_up == n_down, tm, v4);
    return ok ? check_launch("wdf_clipper_bwd_tp") : no_kernel("wdf_clipper_bwd_tp");
}

int wdf_clipper_bwd_mse_tp_adam(const float* x, const float* r, float* theta, float fs, int n_up, int n_down,
                                const float* zstash, const float* zT, const float* target, float gscale, void* ws,
                                float* gtheta, float* sse, int64_t B, int64_t T, int n_chunks, int flags, float* m,
                                float* v, int32_t* step, const float* lr, float beta1, float beta2, float eps,
                                const float* lo, const float* hi, void* stream)
{
    if (!zT || !target) return fail(WDF_EINVAL, "null zT/target");
    if (!m || !v || !step || !lr) return fail(WDF_EINVAL, "null m/v/step/lr");
    return bwd_tp_common(x, r, theta, fs, n_up, n_down, zstash, nullptr, target, zT, gscale, ws, gtheta, sse, nullptr, 0, B,
                         T, n_chunks, flags, stream, nullptr, 0, adam_tail(theta, m, v, step, lr, beta1, beta2, eps, lo, hi));
}

int wdf_clipper_bwd_esr_tp(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down,
                           const float* zstash, const float* zT, const float* target, const float* gcoef, int64_t skip,
                           void* ws, float* gtheta, float* sse, float* gz0, int accumulate, int64_t B, int64_t T,
                           int n_chunks, int flags, void* stream)
{
    if (!zT || !target || !gcoef) return fail(WDF_EINVAL, "null zT/target/gcoef");
    if (skip < 0 || skip > T) return fail(WDF_EINVAL, "skip must be in 0..T");
    return bwd_tp_common(x, r, theta, fs, n_up, n_down, zstash, nullptr, target, zT, 0.0f, ws, gtheta, sse, gz0,
                         accumulate, B, T, n_chunks, flags, stream, gcoef, skip);
}

size_t wdf_clipper_step_mse_tp_ws_bytes(int64_t B, int n_chunks)
{
    return (B > 0 && n_chunks > 0) ? fused_ws(nullptr, B, n_chunks).bytes : 0;
}

int wdf_clipper_step_mse_tp_ws_init(void* ws, int64_t B, int n_chunks, void* stream)
{
    if (!ws || B <= 0 || n_chunks <= 0) return fail(WDF_EINVAL, "null ws / bad B, n_chunks");
    const FusedWs w = fused_ws(ws, B, n_chunks);
    return memset_async(w.tickets, 0, w.clear_bytes, (hipStream_t)stream);
}

static int step_tp_common(const float* x, const float* r, float* theta, float fs, int n_up, int n_down, const float* target,
                          float hgs, int64_t skip, float* y, const float* z0, float* zT, int64_t B, int64_t T, int n_chunks,
                          int warmup, float tol, void* ws, void* status, void* state, int max_warm_tiles, bool esr,
                          wdf::FusedOut out, int flags, void* stream, const char* what)
{
    int rc = check_common(x, theta, n_up, n_down, B, T, flags & ~(WDF_ONE_SEQUENCE_PER_LANE | WDF_R_PER_SEQUENCE | WDF_NO_Y_STORE));
    if (rc) return rc;
    // WDF_NO_Y_STORE: the training-only step; a y handed in with it would silently stay unwritten
    const bool store_y = !(flags & WDF_NO_Y_STORE);
    if (!store_y && y) return fail(WDF_EINVAL, "%s: y must be NULL with WDF_NO_Y_STORE (it would stay unwritten)", what);
    if (!target || (store_y && !y) || !ws || !status) return fail(WDF_EINVAL, "null target/y/ws/status");
    if (!(fs > 0.0f)) return fail(WDF_EINVAL, "fs must be positive");
    if (n_chunks < 1 || warmup < 0 || !(tol >= 0.0f)) return fail(WDF_EINVAL, "n_chunks >= 1, warmup >= 0, tol >= 0");
    if (skip < 0 || skip > T) return fail(WDF_EINVAL, "skip must be in 0..T");
    if (B >= ((int64_t)1 << 24)) return fail(WDF_EINVAL, "the one-pass step addresses a 32-row tile with 32-bit offsets: B < 2^24");
    if (flags & WDF_PREC_F64) return fail(WDF_EUNSUPPORTED, "WDF_PREC_F64 applies to wdf_clipper_fwd and wdf_omega_f64 only");
    const ChunkGeom g = chunk_geom(T, n_chunks, wdf::kTile);
    if ((rc = check_tiles(g, n_chunks, T, wdf::kTile, "wdf_clipper_tp_chunks"))) return rc;
    const int64_t W = round_up((int64_t)warmup, wdf::kTile);
    TpWarm warm{nullptr, nullptr, 1};
    if (state) {
        if (max_warm_tiles < 1 || max_warm_tiles > wdf::kTpMaxWarmTiles)
            return fail(WDF_EINVAL, "max_warm_tiles must be in 1..%d", wdf::kTpMaxWarmTiles);
        if ((int64_t)max_warm_tiles * wdf::kWarmStep > g.L)
            return fail(WDF_EINVAL, "max_warm_tiles * 16 must not exceed the chunk length (%lld)", (long long)g.L);
        if (g.K >= (1 << 20)) return fail(WDF_EINVAL, "too many chunks for a warm-start state");
        const TpState st = tp_state(state, B, 0);           // wdf_clipper_fwd_tp_warm's state; its ticket area is unused here
        warm = TpWarm{st.ctl, st.snap, max_warm_tiles + 1};
    }
    const bool tm = (flags & WDF_X_TIME_MAJOR) != 0;
    const bool v4 = !tm && (T % 4 == 0) && T < (1 << 23) && aligned16(x) && (!r || aligned16(r));
    // two adjacent sequences per lane (8-byte row accesses, packed arithmetic) whenever the rows allow it (a null y: aligned)
    const bool pairs = !(flags & WDF_ONE_SEQUENCE_PER_LANE) && (B % 2 == 0) && aligned8(x) && aligned8(target) && aligned8(y) &&
                       (!r || aligned8(r));
    // WDF_R_PER_SEQUENCE: one pot value per sequence (the caller vouches for it): calc_impedance once per chunk, the channel not streamed
    const int dyn = r == nullptr ? 0 : ((flags & WDF_R_PER_SEQUENCE) ? 2 : 1);
    const int64_t n_waves = (B + (pairs ? 127 : 63)) / (pairs ? 128 : 64) * (int64_t)g.K;
    // (a step without y is built for the default form only: the finish launch; one chunk: the chunk kernel alone)
    const int form = store_y ? fused_form(g.K, !tm && v4 && dyn != 1)    // (wdf::fused_x_window)
                             : (g.K < 2 ? wdf::kFusedInKernel : wdf::kFusedFinishLater);
    const int64_t skew = fused_skew(n_waves, g.K, g.L, T, state ? max_warm_tiles : 0, form == wdf::kFusedGroup);
    if (!store_y) {                                          // the instantiations without the y store: wdf_capi_clipper_noy.hip
        const FusedWs w = fused_ws(ws, B, g.K);
        const FusedNoYLaunch a{x, r, theta, fs, n_up, n_down, target, hgs, skip, z0, zT, w.zwarm, w.zend, w.rec, w.part, w.wpart, w.tickets,
                               w.gticket, w.grp, (wdf::TpStatus*)status, warm.ctl, warm.snap, warm.J, tol, B, T, g.K, g.L, W,
                               (flags & WDF_GENERAL_ROOT) ? 1 : 0, pairs, esr, out, skew, form, (hipStream_t)stream};
        if (!launch_fused_noy(dyn, n_up == n_down, tm, v4, a)) return no_kernel(what);
        return check_launch(what);
    }
    const bool ok = dispatch4([&](auto DYN, auto SYM, auto TM, auto V4) {
        launch_fused<DYN(), SYM(), TM(), V4()>(x, r, theta, fs, n_up, n_down, target, hgs, skip, y, z0, zT, fused_ws(ws, B, g.K),
                                               (wdf::TpStatus*)status, tol, B, T, g, W, warm, (flags & WDF_GENERAL_ROOT) ? 1 : 0, pairs, esr, out,
                                               skew, form, (hipStream_t)stream);
    }, Values<int, 0, 1, 2>{dyn}, n_up == n_down, tm, v4);
    if (!ok) return no_kernel(what);
    return check_launch(what);
}

int wdf_clipper_step_mse_tp(const float* x, const float* r, float* theta, float fs, int n_up, int n_down,
                            const float* target, float gscale, int64_t skip, float* y, const float* z0, float* zT,
                            int64_t B, int64_t T, int n_chunks, int warmup, float tol, void* ws, void* status, void* state,
                            int max_warm_tiles, float* gtheta, float* sse, int accumulate, float* m, float* v, int32_t* step,
                            const float* lr, float beta1, float beta2, float eps, const float* lo, const float* hi, int flags,
                            void* stream)
{
    if (!gtheta || !sse) return fail(WDF_EINVAL, "null gtheta/sse");
    if (int rc = adam_check(m, v, step, lr)) return rc;
    const wdf::FusedOut out{gtheta, accumulate, sse, adam_tail(theta, m, v, step, lr, beta1, beta2, eps, lo, hi), 0.0, 0.0, nullptr, nullptr, wdf::TpFinishCtx{nullptr, nullptr, 0, nullptr, 0.0f, 0, 0, 0, false}};
    return step_tp_common(x, r, theta, fs, n_up, n_down, target, 0.5f * gscale, skip, y, z0, zT, B, T, n_chunks, warmup, tol, ws,
                          status, state, max_warm_tiles, false, out, flags, stream, "wdf_clipper_step_mse_tp");
}

int wdf_clipper_step_esr_tp(const float* x, const float* r, float* theta, float fs, int n_up, int n_down,
                            const float* target, double n_global, double eps_energy, int64_t skip, float* y, const float* z0,
                            float* zT, int64_t B, int64_t T, int n_chunks, int warmup, float tol, void* ws, void* status,
                            void* state, int max_warm_tiles, float* sums10, float* gtheta, float* loss3, float* m, float* v,
                            int32_t* step, const float* lr, float beta1, float beta2, float eps, const float* lo,
                            const float* hi, int flags, void* stream)
{
    if (!sums10) return fail(WDF_EINVAL, "null sums10");
    if (!(n_global > 0.0)) return fail(WDF_EINVAL, "n_global must be positive");
    if (m && !gtheta) return fail(WDF_EINVAL, "Adam: the update reads the gradient from gtheta");
    if (int rc = adam_check(m, v, step, lr)) return rc;
    const wdf::FusedOut out{gtheta, 0, nullptr, adam_tail(theta, m, v, step, lr, beta1, beta2, eps, lo, hi), n_global, eps_energy, sums10, loss3, wdf::TpFinishCtx{nullptr, nullptr, 0, nullptr, 0.0f, 0, 0, 0, false}};
    return step_tp_common(x, r, theta, fs, n_up, n_down, target, 0.5f, skip, y, z0, zT, B, T, n_chunks, warmup, tol, ws, status,
                          state, max_warm_tiles, true, out, flags, stream, "wdf_clipper_step_esr_tp");
}

int wdf_esr_finish(const float* sums10, double n_global, double eps_energy, float* gtheta, float* loss3, void* stream)
{
    if (!sums10 || !gtheta || !(n_global > 0.0)) return fail(WDF_EINVAL, "wdf_esr_finish: null sums10/gtheta or n_global <= 0");
    // (the finish of the MSE + ESR step after the ranks' sums10 have been all-reduced: wdf_esr.h, four entries)
    hipLaunchKernelGGL(wdf::esr_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums10, 4, n_global, eps_energy, gtheta, loss3);
    return check_launch("wdf_esr_finish");
}

int wdf_omega_f64(const double* x, double* w, int32_t* iters, int64_t n, void* stream)
{
    if (!x || !w || n <= 0) return fail(WDF_EINVAL, "wdf_omega_f64: bad arguments");
    hipLaunchKernelGGL(wdf::omega64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, w, iters, n);
    return check_launch("wdf_omega_f64");
}

}  // extern "C"
