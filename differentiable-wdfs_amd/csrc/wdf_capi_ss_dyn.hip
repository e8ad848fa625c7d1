// wdf_capi_ss_dyn.hip -- C ABI of the state-space recursion with per-sample coefficient rows and the MLP root on
// any small tree (csrc/wdf_ss_dyn.h): argument checking, template dispatch, launches.
#include "wdf_capi_common.h"
#include "wdf_ss_dyn.h"
#include "wdf_ss_dyn_rows.h"
using namespace wdfcapi;

namespace {

bool dyn_ok(int ns, int ni) { return ns >= 0 && ns <= wdf::kDynMaxS && ni >= 1 && ni <= wdf::kDynMaxI; }

bool dyn_mlp_ok(int h, int nl) { return (nl == 3 && (h == 4 || h == 8 || h == 16)) || (nl == 5 && (h == 4 || h == 8)); }

int dyn_check(const char* who, const float* x, const float* crow, int ns, int ni, int root, const float* rootp, const float* w,
              int hidden, int n_tanh_layers, int n_up, int n_down, int64_t B, int64_t T, int per_sample)
{
    if (!x || !crow) return fail(WDF_EINVAL, "%s: null x / rows", who);
    if (B <= 0 || T <= 0) return fail(WDF_EINVAL, "%s: B and T must be positive", who);
    if (!dyn_ok(ns, ni)) return fail(WDF_EUNSUPPORTED, "%s: ns <= %d, 1 <= ni <= %d (got %d, %d)", who, wdf::kDynMaxS, wdf::kDynMaxI, ns, ni);
    if (per_sample < 0 || per_sample > 2) return fail(WDF_EINVAL, "%s: per_sample is 0 (one static row), 1 (a row per sample) or 2 (a row per sequence)", who);
    if (root == WDF_ROOT_DIODE_PAIR) {
        if (!rootp) return fail(WDF_EINVAL, "%s: diode root needs rootp = {Is, nVt}", who);
        if (n_up < 1 || n_down < 1) return fail(WDF_EINVAL, "%s: n_up, n_down >= 1", who);
    } else if (root == WDF_ROOT_MLP) {
        if (!w) return fail(WDF_EINVAL, "%s: MLP root needs the flat weights", who);
        if (!dyn_mlp_ok(hidden, n_tanh_layers))
            return fail(WDF_EUNSUPPORTED, "%s: MLP root on a generic tree: width 4 / 8 / 16 with 3 tanh layers, 4 / 8 with 5 (got %d, %d)",
                        who, hidden, n_tanh_layers);
    } else if (root == WDF_ROOT_ASYM_PAIR) {
        if (!rootp) return fail(WDF_EINVAL, "%s: the two-different-diode root needs rootp = {Is_up, nVt_up, Is_down, nVt_down}", who);
        if (ns > 4)
            return fail(WDF_EUNSUPPORTED, "%s: the two-different-diode root runs on trees of at most four capacitors (got %d): the "
                                          "eight-slot kernels' reverse sweep needs scratch under this root and is not built", who, ns);
    } else if (root != WDF_ROOT_NONE) {
        return fail(WDF_EINVAL, "%s: unknown root kind %d", who, root);
    }
    return WDF_OK;
}

}  // namespace

namespace {

constexpr int kUnit = 8;                     // chunk lengths: multiples of 8 steps

// The instantiation a call's root selects: only a diode pair can be asymmetric and only a network has a depth, so the other
// roots take SYM = true and NL = 3 and no kernel is built for the combinations dyn_built() leaves out.
struct DynKind { int root; bool sym; int nl; };
DynKind dyn_kind(int root, int n_up, int n_down, int n_tanh_layers)
{
    return {root, root != WDF_ROOT_DIODE_PAIR || n_up == n_down, root == WDF_ROOT_MLP && n_tanh_layers != 3 ? 5 : 3};
}
// (two different diodes: four state slots only -- with eight the sequential sweep spills to scratch)
constexpr bool dyn_built(int root, bool sym, int nl, int ms = 4)
{
    return (root == wdf::kDynRootDiode || sym) && (root == wdf::kDynRootMlp || nl == 3) && (root != wdf::kDynRootAsym || ms == 4);
}
using DynRoots = Values<int, wdf::kDynRootNone, wdf::kDynRootDiode, wdf::kDynRootMlp, wdf::kDynRootAsym>;
using DynDepths = Values<int, 3, 5>;
using DynSlots = Values<int, 4, 8>;          // state slots the kernel is compiled for (4: trees of up to four capacitors; 8: five to eight)

// grid.x: one lane per sequence, or -- the network root, evaluated in 16-lane rows (wdf_ss_dyn.h DynLanes) -- four sequences per wave
unsigned dyn_grid_x(bool rows, int64_t B) { return (unsigned)(rows ? (B + 3) / 4 : waves64(B)); }

template <class... A> bool launch_dyn_fwd(DynKind k, int ns, int64_t B, int gy, hipStream_t s, A... args)
{
    const dim3 grid(dyn_grid_x(k.root == WDF_ROOT_MLP, B), (unsigned)gy);
    return dispatch([&](auto ROOT, auto SYM, auto NL, auto MS) {
        if constexpr (!dyn_built(ROOT(), SYM(), NL(), MS())) return false;
        else {
            hipLaunchKernelGGL((wdf::ss_dyn_fwd_kernel<ROOT(), SYM(), 16, NL(), MS()>), grid, dim3(64), 0, s, args...);
            return true;
        }
    }, DynRoots{k.root}, Bools{k.sym}, DynDepths{k.nl}, DynSlots{ns > 4 ? 8 : 4});
}

// the reverse sweep's kernel in one of its modes (0: sequential, 1: chunk maps + root partials, 2: the emitting pass -- no root
// code in it, so one instantiation per root kind and a lane per sequence)
template <int MODE, class... A> bool launch_dyn_bwd(DynKind k, int ns, int64_t B, int gy, hipStream_t s, A... args)
{
    if (MODE == 2) k = DynKind{k.root, true, 3};
    const dim3 grid(dyn_grid_x(MODE != 2 && k.root == WDF_ROOT_MLP, B), (unsigned)gy);
    return dispatch([&](auto ROOT, auto SYM, auto NL, auto MS) {
        if constexpr (!dyn_built(ROOT(), SYM(), NL(), MS()) || (MODE == 2 && (!SYM() || NL() != 3))) return false;
        else {
            hipLaunchKernelGGL((wdf::ss_dyn_bwd_kernel<ROOT(), SYM(), 16, NL(), MODE, MS()>), grid, dim3(64), 0, s, args...);
            return true;
        }
    }, DynRoots{k.root}, Bools{k.sym}, DynDepths{k.nl}, DynSlots{ns > 4 ? 8 : 4});
}

// The reverse sweeps' workspaces by root kind: the per-(chunk, wave) root sums -- 2 doubles, 4 under two different diodes -- then
// (chunked) the chunk maps, the entering adjoints and the root's partials of every step (5 floats, 7 under two different
// diodes).  One walk for the *_ws_bytes functions (null base: counts only) and the entry points.
int dyn_root_sums(int root) { return root == WDF_ROOT_ASYM_PAIR ? 4 : 2; }
int dyn_root_rpart(int root) { return root == WDF_ROOT_ASYM_PAIR ? wdf::kDynRpartOf<wdf::kDynRootAsym> : wdf::kDynRpart; }
bool dyn_root_known(int root) { return root == WDF_ROOT_NONE || root == WDF_ROOT_DIODE_PAIR || root == WDF_ROOT_MLP || root == WDF_ROOT_ASYM_PAIR; }

struct DynBwdTpWs { double* part; float *rec, *lam_in, *rpart; size_t bytes; };
DynBwdTpWs dyn_bwd_tp_carve(void* ws, int root, int ns, int64_t B, int64_t T, int K)
{
    const size_t nsa = ns > 0 ? ns : 1, waves = waves64(B);
    Carver c(ws);
    DynBwdTpWs w;
    w.part = c.take<double>((size_t)K * waves * dyn_root_sums(root));
    w.rec = c.take<float>((size_t)K * (nsa + 1) * nsa * (size_t)B);
    w.lam_in = c.take<float>((size_t)K * nsa * (size_t)B);
    w.rpart = c.take<float>((size_t)T * dyn_root_rpart(root) * (size_t)B);
    w.bytes = c.off;
    return w;
}

}  // namespace

extern "C" {

int wdf_ss_dyn_row_len(int ns, int ni) { return dyn_ok(ns, ni) ? wdf::DynLayout(ns, ni).n : 0; }

int wdf_ss_dyn_fwd(const float* x, const float* rows, int per_sample, int ns, int ni, int root, const float* rootp, const float* w,
                   int hidden, int n_tanh_layers, int n_up, int n_down, float* y, float* zstash, const float* z0, float* zT,
                   int64_t B, int64_t T, void* stream)
{
    int rc = dyn_check("wdf_ss_dyn_fwd", x, rows, ns, ni, root, rootp, w, hidden, n_tanh_layers, n_up, n_down, B, T, per_sample);
    if (rc) return rc;
    if (!y) return fail(WDF_EINVAL, "wdf_ss_dyn_fwd: null y");
    const int64_t n = wdf::DynLayout(ns, ni).n;
    const int64_t cs = per_sample ? B : 1, ts = per_sample == 1 ? n * B : 0, bs = per_sample ? 1 : 0;   // (2: rows [n][B], the same row at every step)
    hipStream_t s = (hipStream_t)stream;
    EventBracket bracket(s);
    if (!launch_dyn_fwd(dyn_kind(root, n_up, n_down, n_tanh_layers), ns, B, 1, s, x, rows, cs, ts, bs, rootp, w, n_up, n_down, y, zstash, z0, zT,
                        ns, ni, B, T, T, (int64_t)0, (float*)nullptr, (float*)nullptr, (const unsigned*)nullptr, (const float*)nullptr, hidden))
        return no_kernel("wdf_ss_dyn_fwd");
    return check_launch("wdf_ss_dyn_fwd");
}

size_t wdf_ss_dyn_fwd_tp_ws_bytes(int ns, int64_t B, int n_chunks)
{
    if (ns < 0 || B <= 0 || n_chunks <= 0) return 0;
    return (size_t)2 * (size_t)n_chunks * (size_t)(ns > 0 ? ns : 1) * (size_t)B * sizeof(float) + waves64(B) * sizeof(unsigned);
}

int wdf_ss_dyn_fwd_tp(const float* x, const float* rows, int per_sample, int ns, int ni, int root, const float* rootp, const float* w,
                      int hidden, int n_tanh_layers, int n_up, int n_down, float* y, float* zstash, const float* z0, float* zT,
                      int64_t B, int64_t T, int n_chunks, int warmup, float tol, const float* zinit, void* ws, void* status, void* stream)
{
    int rc = dyn_check("wdf_ss_dyn_fwd_tp", x, rows, ns, ni, root, rootp, w, hidden, n_tanh_layers, n_up, n_down, B, T, per_sample);
    if (rc) return rc;
    if (!y || !ws || !status) return fail(WDF_EINVAL, "wdf_ss_dyn_fwd_tp: null y / ws / status");
    if (ns < 1) return fail(WDF_EINVAL, "wdf_ss_dyn_fwd_tp: a tree without states has no chunks to verify: use wdf_ss_dyn_fwd");
    if (warmup < 0 || !(tol >= 0.0f)) return fail(WDF_EINVAL, "wdf_ss_dyn_fwd_tp: warmup >= 0, tol >= 0");
    if (n_chunks < 1) return fail(WDF_EINVAL, "wdf_ss_dyn_fwd_tp: n_chunks >= 1");
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    if ((rc = check_tiles(g, n_chunks, T, kUnit, nullptr))) return rc;
    const int K = g.K;
    const int64_t Lc = g.L;
    const int64_t n = wdf::DynLayout(ns, ni).n;
    const int64_t cs = per_sample ? B : 1, ts = per_sample == 1 ? n * B : 0, bs = per_sample ? 1 : 0;   // (2: rows [n][B], the same row at every step)
    float* zwarm = (float*)ws;
    float* zend = zwarm + (size_t)K * (size_t)ns * (size_t)B;
    unsigned* gate = (unsigned*)(zend + (size_t)K * (size_t)ns * (size_t)B);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = memset_async(status, 0, sizeof(wdf::SsTpStatus), s))) return rc;
    const DynKind kind = dyn_kind(root, n_up, n_down, n_tanh_layers);
    bool ok;
    {
        EventBracket bracket(s);
        ok = launch_dyn_fwd(kind, ns, B, K, s, x, rows, cs, ts, bs, rootp, w, n_up, n_down, y, zstash, z0, zT, ns, ni, B, T, Lc,
                            (int64_t)warmup, zwarm, zend, (const unsigned*)nullptr, zinit, hidden);
    }
    if (ok && K > 1) {
        hipLaunchKernelGGL(wdf::ss_tp_verify_kernel, dim3(waves64(B)), dim3(64), 0, s, (const float*)zwarm, (const float*)zend, ns,
                           B, (int64_t)K, tol, gate, (wdf::SsTpStatus*)status);
        // the 64-sequence groups with a miss again, sequentially (the gate lets the others leave at once)
        ok = launch_dyn_fwd(kind, ns, B, 1, s, x, rows, cs, ts, bs, rootp, w, n_up, n_down, y, zstash, z0, zT, ns, ni, B, T, T, (int64_t)0,
                            (float*)nullptr, (float*)nullptr, (const unsigned*)gate, (const float*)nullptr, hidden);
    }
    return ok ? check_launch("wdf_ss_dyn_fwd_tp") : no_kernel("wdf_ss_dyn_fwd_tp");
}

size_t wdf_ss_dyn_bwd_ws_bytes(int64_t B) { return B > 0 ? waves64(B) * 2 * sizeof(double) : 0; }

size_t wdf_ss_dyn_bwd_root_ws_bytes(int root, int64_t B)
{
    return (B > 0 && dyn_root_known(root)) ? waves64(B) * dyn_root_sums(root) * sizeof(double) : 0;
}

int wdf_ss_dyn_bwd(const float* x, const float* rows, int per_sample, int ns, int ni, int root, const float* rootp, const float* w,
                   int hidden, int n_tanh_layers, int n_up, int n_down, const float* zstash, const float* gy, float* grows,
                   void* ws, float* gb, float* ain, float* lrin, float* gz0, int64_t B, int64_t T, void* stream)
{
    int rc = dyn_check("wdf_ss_dyn_bwd", x, rows, ns, ni, root, rootp, w, hidden, n_tanh_layers, n_up, n_down, B, T, per_sample);
    if (rc) return rc;
    if (!gy || !grows || !ws || (ns > 0 && !zstash)) return fail(WDF_EINVAL, "wdf_ss_dyn_bwd: null gy / grows / ws / zstash");
    if (root == WDF_ROOT_MLP && (!gb || !ain || !lrin)) return fail(WDF_EINVAL, "wdf_ss_dyn_bwd: the MLP root needs gb / ain / lrin [T][B]");
    const int64_t n = wdf::DynLayout(ns, ni).n;
    const int64_t cs = per_sample ? B : 1, ts = per_sample == 1 ? n * B : 0, bs = per_sample ? 1 : 0;   // (2: rows [n][B], the same row at every step)
    hipStream_t s = (hipStream_t)stream;
    const int acc = per_sample != 1;       // rows that do not change in time: dL/d(row) summed over the steps -> grows [1][n][B]
    EventBracket bracket(s);
    if (!launch_dyn_bwd<0>(dyn_kind(root, n_up, n_down, n_tanh_layers), ns, B, 1, s, x, rows, cs, ts, bs, rootp, w, n_up, n_down, zstash, gy, grows,
                           (double*)ws, gb, ain, lrin, gz0, ns, ni, B, T, T, (float*)nullptr, (float*)nullptr, (const float*)nullptr, hidden, acc))
        return no_kernel("wdf_ss_dyn_bwd");
    return check_launch("wdf_ss_dyn_bwd");
}

// ws: double [K waves][2] partial sums | rec float [K][(ns + 1) ns][B] | lam_in float [K][ns][B] | rpart float [T][5][B]
size_t wdf_ss_dyn_bwd_tp_ws_bytes(int ns, int64_t B, int64_t T, int n_chunks)
{
    if (ns < 0 || B <= 0 || T <= 0 || n_chunks <= 0) return 0;
    const size_t nsa = ns > 0 ? ns : 1, waves = waves64(B);
    return (size_t)n_chunks * waves * 2 * sizeof(double) +
           ((size_t)n_chunks * (nsa + 1) * nsa + (size_t)n_chunks * nsa + (size_t)T * wdf::kDynRpart) * (size_t)B * sizeof(float);
}

// the same by root kind (the old roots: the value above)
size_t wdf_ss_dyn_bwd_tp_root_ws_bytes(int root, int ns, int64_t B, int64_t T, int n_chunks)
{
    if (ns < 0 || B <= 0 || T <= 0 || n_chunks <= 0 || !dyn_root_known(root)) return 0;
    return dyn_bwd_tp_carve(nullptr, root, ns, B, T, n_chunks).bytes;
}

int wdf_ss_dyn_bwd_tp(const float* x, const float* rows, int per_sample, int ns, int ni, int root, const float* rootp, const float* w,
                      int hidden, int n_tanh_layers, int n_up, int n_down, const float* zstash, const float* gy, float* grows,
                      void* ws, float* gb, float* ain, float* lrin, float* gz0, int64_t B, int64_t T, int n_chunks, void* stream)
{
    int rc = dyn_check("wdf_ss_dyn_bwd_tp", x, rows, ns, ni, root, rootp, w, hidden, n_tanh_layers, n_up, n_down, B, T, per_sample);
    if (rc) return rc;
    if (!gy || !grows || !ws || !zstash) return fail(WDF_EINVAL, "wdf_ss_dyn_bwd_tp: null gy / grows / ws / zstash");
    if (ns < 1) return fail(WDF_EINVAL, "wdf_ss_dyn_bwd_tp: a tree without states has no adjoint to chunk: use wdf_ss_dyn_bwd");
    if (root == WDF_ROOT_MLP && (!gb || !ain || !lrin)) return fail(WDF_EINVAL, "wdf_ss_dyn_bwd_tp: the MLP root needs gb / ain / lrin [T][B]");
    if (n_chunks < 1) return fail(WDF_EINVAL, "wdf_ss_dyn_bwd_tp: n_chunks >= 1");
    const ChunkGeom g = chunk_geom(T, n_chunks, kUnit);
    if ((rc = check_tiles(g, n_chunks, T, kUnit, nullptr))) return rc;
    const int K = g.K;
    const int64_t Lc = g.L;
    const int64_t n = wdf::DynLayout(ns, ni).n;
    const int64_t cs = per_sample ? B : 1, ts = per_sample == 1 ? n * B : 0, bs = per_sample ? 1 : 0;   // (2: rows [n][B], the same row at every step)
    const size_t waves = waves64(B);
    const DynBwdTpWs wsl = dyn_bwd_tp_carve(ws, root, ns, B, T, K);
    double* part = wsl.part;
    float *rec = wsl.rec, *lam_in = wsl.lam_in, *rpart = wsl.rpart;
    hipStream_t s = (hipStream_t)stream;
    const int acc = per_sample != 1;       // (grows [K][n][B] then: one partial per chunk, added up by the caller)
    const DynKind kind = dyn_kind(root, n_up, n_down, n_tanh_layers);
    bool ok;
    {
        EventBracket bracket(s);
        ok = launch_dyn_bwd<1>(kind, ns, B, K, s, x, rows, cs, ts, bs, rootp, w, n_up, n_down, zstash, gy, grows, part, gb, ain, lrin, gz0, ns, ni,
                               B, T, Lc, rpart, rec, (const float*)nullptr, hidden, acc);
    }
    if (!ok) return no_kernel("wdf_ss_dyn_bwd_tp");
    hipLaunchKernelGGL(wdf::ss_dyn_bwd_combine_kernel, dim3((unsigned)waves), dim3(64), 0, s, (const float*)rec, lam_in, ns, B, (int64_t)K);
    if (!launch_dyn_bwd<2>(kind, ns, B, K, s, x, rows, cs, ts, bs, rootp, w, n_up, n_down, zstash, gy, grows, part, gb, ain, lrin, gz0, ns, ni, B, T,
                           Lc, rpart, rec, (const float*)lam_in, hidden, acc))
        return no_kernel("wdf_ss_dyn_bwd_tp");
    return check_launch("wdf_ss_dyn_bwd_tp");
}


/* ---- the coefficient rows from the probed step's tape (wdf_ss_dyn_rows.h) ---- */
namespace {
// checks the tape (host arrays) and packs it for the kernels' argument block
int rows_pack(const char* who, const int32_t* ops, int n_ops, const double* consts, int n_consts, const int32_t* outs, int n_out,
              int n_params, int chan, wdf::RowsTape& tp)
{
    if (!ops || !outs || (n_consts > 0 && !consts)) return fail(WDF_EINVAL, "%s: null tape", who);
    if (n_ops < 1 || n_ops > wdf::kRowsMaxOps || n_consts < 0 || n_consts > wdf::kRowsMaxConsts || n_out < 1 || n_out > wdf::kRowsMaxOut ||
        n_params < 0 || n_params > wdf::kRowsMaxParams)
        return fail(WDF_EUNSUPPORTED, "%s: the device evaluates tapes of <= %d operations, %d constants, %d row entries, %d component values "
                                      "(got %d, %d, %d, %d)", who, wdf::kRowsMaxOps, wdf::kRowsMaxConsts, wdf::kRowsMaxOut, wdf::kRowsMaxParams,
                    n_ops, n_consts, n_out, n_params);
    if (chan < -1 || chan >= n_params) return fail(WDF_EINVAL, "%s: chan = %d with %d component values", who, chan, n_params);
    for (int i = 0; i < n_ops; ++i) {
        const int op = ops[3 * i], a = ops[3 * i + 1], b = ops[3 * i + 2];
        bool ok;
        switch (op) {
        case wdf::kOpConst: ok = a >= 0 && a < n_consts; break;
        case wdf::kOpParam: ok = a >= 0 && a < n_params; break;
        case wdf::kOpAdd: case wdf::kOpSub: case wdf::kOpMul: case wdf::kOpDiv: ok = a >= 0 && a < i && b >= 0 && b < i; break;
        case wdf::kOpNeg: case wdf::kOpRecip: ok = a >= 0 && a < i; break;
        default: ok = false;
        }
        if (!ok) return fail(WDF_EINVAL, "%s: operation %d of the tape (%d, %d, %d) is not one the probe records", who, i, op, a, b);
        tp.code[i] = (uint32_t)op | ((uint32_t)a << 8) | ((uint32_t)(op >= wdf::kOpAdd && op <= wdf::kOpDiv ? b : 0) << 16);
    }
    for (int k = 0; k < n_out; ++k) {
        if (outs[k] < 0 || outs[k] >= n_ops) return fail(WDF_EINVAL, "%s: row entry %d names node %d of %d", who, k, outs[k], n_ops);
        tp.outs[k] = (uint8_t)outs[k];
    }
    for (int j = 0; j < n_consts; ++j) tp.consts[j] = consts[j];
    tp.n_ops = n_ops; tp.n_out = n_out; tp.n_params = n_params; tp.chan = chan;
    return WDF_OK;
}

int64_t rows_blocks_t(int64_t T) { return (T + wdf::kRowsSteps - 1) / wdf::kRowsSteps; }

// a launch with more than the default 64 KB of dynamic LDS asks for it first (per function and device: asked every such call)
int rows_lds_limit(const char* who, const void* kernel, size_t lds)
{
    if (lds <= 64 * 1024) return WDF_OK;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return fail(WDF_ELAUNCH, "%s: %zu bytes of LDS for this tape could not be asked for", who, lds);
    return WDF_OK;
}

int rows_args(const char* who, const double* params, int n_params, int chan, const float* r, int64_t B, int64_t T)
{
    if (B <= 0 || T <= 0) return fail(WDF_EINVAL, "%s: B and T must be positive", who);
    if (rows_blocks_t(T) > 65535) return fail(WDF_EUNSUPPORTED, "%s: T <= %d", who, 65535 * wdf::kRowsSteps);
    if (n_params > 0 && !params) return fail(WDF_EINVAL, "%s: null params", who);
    if ((chan >= 0) != (r != nullptr)) return fail(WDF_EINVAL, "%s: a channel parameter (chan >= 0) and its values r [T][B] come together", who);
    return WDF_OK;
}
}  // namespace

int wdf_ss_dyn_rows(const int32_t* tape_ops, int n_ops, const double* consts, int n_consts, const int32_t* outs, int n_out,
                    const double* params, int n_params, int chan, const float* r, float* rows, int64_t B, int64_t T, void* stream)
{
    wdf::RowsTape tp{};
    int rc = rows_pack("wdf_ss_dyn_rows", tape_ops, n_ops, consts, n_consts, outs, n_out, n_params, chan, tp);
    if (rc) return rc;
    if ((rc = rows_args("wdf_ss_dyn_rows", params, n_params, chan, r, B, T))) return rc;
    if (!rows) return fail(WDF_EINVAL, "wdf_ss_dyn_rows: null rows");
    const dim3 grid(waves64(B), (unsigned)rows_blocks_t(T));
    const size_t lds = (size_t)n_ops * 64 * sizeof(double);
    if ((rc = rows_lds_limit("wdf_ss_dyn_rows", (const void*)wdf::ss_dyn_rows_kernel, lds))) return rc;
    hipLaunchKernelGGL(wdf::ss_dyn_rows_kernel, grid, dim3(64), lds, (hipStream_t)stream, tp, params, r, rows, B, T);
    return check_launch("wdf_ss_dyn_rows");
}

size_t wdf_ss_dyn_rows_bwd_ws_bytes(int n_params, int64_t B, int64_t T)
{
    if (B <= 0 || T <= 0 || n_params < 1 || n_params > wdf::kRowsMaxParams) return 0;
    return waves64(B) * (size_t)rows_blocks_t(T) * (size_t)n_params * sizeof(double);
}

int wdf_ss_dyn_rows_bwd(const int32_t* tape_ops, int n_ops, const double* consts, int n_consts, const int32_t* outs, int n_out,
                        const double* params, int n_params, int chan, const float* r, const float* grows, void* ws, double* gparams,
                        int64_t B, int64_t T, void* stream)
{
    wdf::RowsTape tp{};
    int rc = rows_pack("wdf_ss_dyn_rows_bwd", tape_ops, n_ops, consts, n_consts, outs, n_out, n_params, chan, tp);
    if (rc) return rc;
    if ((rc = rows_args("wdf_ss_dyn_rows_bwd", params, n_params, chan, r, B, T))) return rc;
    if (n_params < 1) return fail(WDF_EINVAL, "wdf_ss_dyn_rows_bwd: no component values to differentiate");
    if (!grows || !ws || !gparams) return fail(WDF_EINVAL, "wdf_ss_dyn_rows_bwd: null grows / ws / gparams");
    const dim3 grid(waves64(B), (unsigned)rows_blocks_t(T));
    const size_t lds = (size_t)n_ops * 64 * (sizeof(double) + sizeof(float)) + (size_t)n_params * 64 * sizeof(double);
    if ((rc = rows_lds_limit("wdf_ss_dyn_rows_bwd", (const void*)wdf::ss_dyn_rows_bwd_kernel, lds))) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(wdf::ss_dyn_rows_bwd_kernel, grid, dim3(64), lds, s, tp, params, r, grows, (double*)ws, B, T);
    rc = check_launch("wdf_ss_dyn_rows_bwd");
    if (rc) return rc;
    hipLaunchKernelGGL(wdf::ss_dyn_rows_reduce_kernel, dim3((unsigned)n_params), dim3(256), 0, s, (const double*)ws,
                       (int64_t)grid.x * (int64_t)grid.y, n_params, gparams);
    return check_launch("wdf_ss_dyn_rows_reduce");
}

}  // extern "C"
