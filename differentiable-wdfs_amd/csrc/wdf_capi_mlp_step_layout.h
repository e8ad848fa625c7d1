// wdf_capi_mlp_step_layout.h -- what wdf_capi_mlp_step.hip and wdf_capi_mlp_eval.hip share: the layout of the resident MLP-root
// step's state block (ONE walk: the *_state_bytes export, the plan / read / set functions, the training step and the evaluation
// pass all carve the same block), the shape check, and the state block's part of the kernels' argument structure.
#pragma once
#include "wdf_capi_common.h"
#include "wdf_mlp_step.h"

namespace wdfcapi {

struct StepLayout {
    size_t ctl, items, cols, wcol, cool, wpeak, ticket, ticket2, nflag, colseq, flag, hwid, colmiss, zwarm, zend, zpre, lossblk, colsum,
        maps, snap, wsw, total;
    int n_cols, kw;
    int64_t lw;
};

inline bool step_arch_ok(int hidden, int n_layers, int activation)
{
    return (hidden == 4 || hidden == 8 || hidden == 16) && n_layers >= 3 && n_layers <= 5 && (activation == 0 || activation == 1);
}

inline int step_weight_count(int H, int NL) { return 3 * H + (NL - 1) * (H * H + H) + H + 1; }

inline StepLayout step_layout(int hidden, int n_layers, int64_t B, int64_t T, int n_items, int wgrad_chunks)
{
    StepLayout L{};
    L.n_cols = (int)((B + 15) / 16);
    const ChunkGeom gw = chunk_geom(T, wgrad_chunks, 16);
    L.lw = gw.L;
    L.kw = gw.K;
    const size_t nc = (size_t)L.n_cols, ni = (size_t)n_items, nb = (size_t)(T / 16);
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o = round_up(o + bytes, 256); return at; };
    L.ctl = take(sizeof(wdf::MlpStepCtl));
    L.items = take(ni * sizeof(wdf::MlpStepItem));
    L.cols = take(nc * sizeof(wdf::MlpStepCol));
    L.wcol = take(nc * 4); L.cool = take(nc * 4); L.wpeak = take(nc * 4); L.ticket = take(nc * 4); L.ticket2 = take(nc * 4);
    L.nflag = take(nc * 4); L.colseq = take(nc * 4); L.flag = take(ni * 4); L.hwid = take(ni * 8); L.colmiss = take(nc * 16);
    L.zwarm = take(ni * 16 * 4); L.zend = take(ni * 16 * 4);
    L.zpre = take(ni * wdf::kStepPre * 16 * 4);
    L.lossblk = take(nb * nc * 2 * 4); L.colsum = take(nc * 2 * 8);
    L.maps = take(nb * 3 * (size_t)B * 4);
    L.snap = take(2 * nb * (size_t)B * 4);
    L.wsw = take(nc * (size_t)L.kw * (size_t)step_weight_count(hidden, n_layers) * 4);
    L.total = o;
    return L;
}

inline int step_check_shape(int hidden, int n_layers, int activation, int64_t B, int64_t T, int n_items, int wgrad_chunks)
{
    if (!step_arch_ok(hidden, n_layers, activation))
        return fail(WDF_EUNSUPPORTED, "MLP-root training step: width in {4,8,16}, 3..5 hidden layers, activation 0 (tanh) or 1 (relu); "
                                      "got width %d, %d layers, activation %d", hidden, n_layers, activation);
    if (B <= 0 || T <= 0 || (T & 15)) return fail(WDF_EUNSUPPORTED, "MLP-root training step: T must be a positive multiple of 16 (got %lld)", (long long)T);
    if (n_items < (B + 15) / 16 || wgrad_chunks < 1) return fail(WDF_EINVAL, "n_items >= ceil(B/16), wgrad_chunks >= 1");
    return WDF_OK;
}

// the state block's arrays, and the shape, of the kernels' arguments (the caller adds its data pointers)
inline wdf::MlpStepArgs step_state_args(void* state, const StepLayout& L, int hidden, int64_t B, int64_t T, int64_t skip, int n_items,
                                        float fs)
{
    char* base = (char*)state;
    wdf::MlpStepArgs A{};
    A.maps = (float*)(base + L.maps); A.snap = (float*)(base + L.snap);
    A.zwarm = (float*)(base + L.zwarm); A.zend = (float*)(base + L.zend);
    A.zpre = (float*)(base + L.zpre);
    A.lossblk = (float*)(base + L.lossblk); A.colsum = (double*)(base + L.colsum);
    A.items = (const wdf::MlpStepItem*)(base + L.items); A.cols = (const wdf::MlpStepCol*)(base + L.cols);
    A.wcol = (int*)(base + L.wcol); A.cool = (int*)(base + L.cool); A.wpeak = (int*)(base + L.wpeak);
    A.ticket = (unsigned*)(base + L.ticket); A.ticket2 = (unsigned*)(base + L.ticket2);
    A.hwid = (unsigned*)(base + L.hwid); A.colmiss = (float*)(base + L.colmiss);
    A.flag = (unsigned*)(base + L.flag); A.nflag = (unsigned*)(base + L.nflag); A.colseq = (unsigned*)(base + L.colseq);
    A.ctl = (wdf::MlpStepCtl*)(base + L.ctl);
    A.B = B; A.T = T; A.skip = skip; A.H = hidden; A.n_items = n_items; A.n_cols = L.n_cols; A.fs = fs;
    return A;
}

}  // namespace wdfcapi
