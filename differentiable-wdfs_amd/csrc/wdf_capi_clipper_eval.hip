// wdf_capi_clipper_eval.hip -- C ABI of the diode clipper's loss-only evaluation pass (csrc/wdf_clipper_eval.h): argument
// checking, workspace layout, template dispatch and launches of wdf_clipper_eval_tp.  A translation unit of its own: it compiles
// beside the training step's two.
#include "wdf_capi_clipper_step.h"
#include "wdf_clipper_eval.h"
using namespace wdfcapi;

namespace {

// [tiles][2] doubles (the tiles' partials), [64-sequence slots][K][2] doubles (the chunk waves' own sums, one pair per sequence
// slot of a lane), zwarm / zend [K][B], then -- on a 64-byte line of their own: wdf_clipper_eval_tp_ws_init clears it -- the
// verification's accumulators (wdf::TpAcc) and the count of finished tiles.
struct EvalWs { double* part; double* wpart; float* zwarm; float* zend; unsigned* tickets; unsigned* gticket; size_t bytes; };
constexpr size_t kEvalClearBytes = 64;

inline EvalWs eval_ws(void* ws, int64_t B, int K)
{
    const size_t tiles = waves64(B) + 1;                       // >= tiles x slots for either lane form
    Carver c(ws);
    EvalWs w;
    w.part = c.take<double>(tiles * wdf::kEvalNP);
    w.wpart = c.take<double>(tiles * (size_t)K * wdf::kEvalNP);
    w.zwarm = c.take<float>((size_t)K * (size_t)B);
    w.zend = c.take<float>((size_t)K * (size_t)B);
    c.align(64);
    w.tickets = c.take<unsigned>(kEvalClearBytes / sizeof(unsigned));
    w.gticket = w.tickets + 8;
    w.bytes = c.off;
    return w;
}

struct EvalLaunch {
    const float* x; const float* r; const float* theta; float fs; int n_up, n_down; const float* target; int64_t skip; float* y;
    const float* z0; float* zT; EvalWs w; wdf::TpStatus* status; TpWarm warm; float tol; int64_t B, T; ChunkGeom g; int64_t W;
    int general; bool pairs; wdf::EvalOut out; hipStream_t s;
};

template <int DYN_R, bool SYM, bool TM, bool V4>
void launch_eval(const EvalLaunch& a)
{
    // pairs: two adjacent sequences per lane, packed fp32 arithmetic; a tile is then 128 sequences
    const int per_tile = a.pairs ? 128 : 64;
    const dim3 grid((unsigned)((a.B + per_tile - 1) / per_tile), (unsigned)a.g.K);
    const int64_t skew = 0;                                    // equal chunk spans
    dispatch([&](auto PAIRS, auto STORE_Y) {
        using V = std::conditional_t<PAIRS(), wdf::v2f, float>;
        constexpr int N = PAIRS() ? 2 : 1;
        {
            EventBracket bracket(a.s);
            hipLaunchKernelGGL((wdf::clipper_eval_tp_kernel<DYN_R, SYM, TM, V4, V, STORE_Y()>), grid, dim3(64), 0, a.s, a.x, a.r, a.theta, a.fs,
                               a.n_up, a.n_down, a.target, a.skip, a.y, a.z0, a.zT, a.w.zwarm, a.w.zend, a.status, a.warm.ctl, a.warm.snap, a.warm.J,
                               a.w.tickets, a.w.gticket, a.tol, a.B, a.T, (int64_t)a.g.K, a.g.L, a.W, a.general, a.w.part, a.w.wpart, a.out, skew);
        }
        if (a.g.K > 1)                                         // one chunk: no boundary, no second launch
            hipLaunchKernelGGL((wdf::clipper_eval_finish_kernel<DYN_R, SYM, TM, N, STORE_Y()>), dim3(grid.x), dim3(64), 0, a.s, a.x, a.r, a.theta,
                               a.fs, a.n_up, a.n_down, a.target, a.skip, a.y, a.zT, a.w.zwarm, a.w.zend, a.B, a.T, (int64_t)a.g.K, a.g.L, a.tol,
                               a.status, a.warm.ctl, a.warm.snap, a.warm.J, a.w.tickets, a.w.gticket, a.general, a.w.part, a.w.wpart, a.out, skew,
                               a.W);
    }, Bools{a.pairs}, Bools{a.y != nullptr});
}

}  // namespace

extern "C" {

size_t wdf_clipper_eval_tp_ws_bytes(int64_t B, int n_chunks)
{
    return (B > 0 && n_chunks > 0) ? eval_ws(nullptr, B, n_chunks).bytes : 0;
}

int wdf_clipper_eval_tp_ws_init(void* ws, int64_t B, int n_chunks, void* stream)
{
    if (!ws || B <= 0 || n_chunks <= 0) return fail(WDF_EINVAL, "null ws / bad B, n_chunks");
    return memset_async(eval_ws(ws, B, n_chunks).tickets, 0, kEvalClearBytes, (hipStream_t)stream);
}

int wdf_clipper_eval_tp(const float* x, const float* r, const float* theta, float fs, int n_up, int n_down, const float* target,
                        double n_global, double eps_energy, int64_t skip, float* y, const float* z0, float* zT, int64_t B, int64_t T,
                        int n_chunks, int warmup, float tol, void* ws, void* status, void* state, int max_warm_tiles, double* sums,
                        float* loss3, int flags, void* stream)
{
    const char* what = "wdf_clipper_eval_tp";
    // every refusal before any HIP call (as step_tp_common's)
    if (!x || !theta) return fail(WDF_EINVAL, "%s: null x/theta", what);
    if (B <= 0 || T <= 0) return fail(WDF_EINVAL, "B and T must be positive (got B=%lld T=%lld)", (long long)B, (long long)T);
    if (n_up < 1 || n_down < 1 || n_up > 16 || n_down > 16) return fail(WDF_EINVAL, "n_up/n_down must be in [1,16]");
    if (flags & ~(WDF_X_TIME_MAJOR | WDF_GENERAL_ROOT | WDF_R_PER_SEQUENCE | WDF_ONE_SEQUENCE_PER_LANE))
        return fail(WDF_EINVAL, "%s: unknown flag bits 0x%x", what, flags);
    if (!target || !ws || !status || !sums) return fail(WDF_EINVAL, "%s: null target/ws/status/sums", what);
    if (!(fs > 0.0f)) return fail(WDF_EINVAL, "fs must be positive");
    if (n_chunks < 1 || warmup < 0 || !(tol >= 0.0f)) return fail(WDF_EINVAL, "n_chunks >= 1, warmup >= 0, tol >= 0");
    if (skip < 0 || skip >= T) return fail(WDF_EINVAL, "%s: skip must be in 0..T-1 (a loss over no sample)", what);
    if (!(n_global > 0.0)) return fail(WDF_EINVAL, "n_global must be positive");
    if (!(eps_energy >= 0.0)) return fail(WDF_EINVAL, "eps_energy must not be negative");
    if ((flags & WDF_R_PER_SEQUENCE) && !r) return fail(WDF_EINVAL, "%s: WDF_R_PER_SEQUENCE without a resistance channel r", what);
    if (B >= ((int64_t)1 << 24)) return fail(WDF_EINVAL, "the evaluation pass addresses a 32-row tile with 32-bit offsets: B < 2^24");
    const ChunkGeom g = chunk_geom(T, n_chunks, wdf::kTile);
    if (int rc = check_tiles(g, n_chunks, T, wdf::kTile, "wdf_clipper_tp_chunks")) return rc;
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
    const int dyn = r == nullptr ? 0 : ((flags & WDF_R_PER_SEQUENCE) ? 2 : 1);
    const EvalLaunch a{x, r, theta, fs, n_up, n_down, target, skip, y, z0, zT, eval_ws(ws, B, g.K), (wdf::TpStatus*)status, warm, tol, B, T, g, W,
                       (flags & WDF_GENERAL_ROOT) ? 1 : 0, pairs, wdf::EvalOut{sums, loss3, n_global, eps_energy}, (hipStream_t)stream};
    const bool ok = dispatch4([&](auto DYN, auto SYM, auto TM, auto V4) { launch_eval<DYN(), SYM(), TM(), V4()>(a); },
                              Values<int, 0, 1, 2>{dyn}, n_up == n_down, tm, v4);
    return ok ? check_launch(what) : no_kernel(what);
}

}  // extern "C"
