// wdf_capi_common.h -- shared by the translation units of libwdf_hip.so: error string, launch
// check, the one-shot event bracket, and the host-side scaffolding every entry-point family uses: chunk
// geometry, the runtime-value -> template-argument dispatcher, the workspace carver.  No algorithm lives here.
#pragma once
#include <atomic>
#include <type_traits>

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/wdf_hip.h"

namespace wdfcapi {

extern thread_local char g_err[512];

inline int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

inline int check_launch(const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WDF_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return WDF_OK;
}

// wdf_event_bracket_next(): events to record immediately before / after the next RECURRENCE
// kernel the library launches (the forward or reverse sweep itself, not the verify / combine /
// reduce helpers that share its C call), so a harness can time exactly the kernel rocprofv3
// reports.  One-shot, process-wide: the call that consumes it may come from another thread
// than the one that armed it (torch's autograd engine runs a backward on its own thread).
struct EventPair { hipEvent_t e0, e1; };
extern std::atomic<EventPair*> g_bracket;          // armed pair or null: ONE word, so a start never goes without its stop

struct EventBracket {
    hipStream_t s;
    EventPair* p;
    explicit EventBracket(hipStream_t stream) : s(stream), p(g_bracket.exchange(nullptr))
    {
        if (p && p->e0) (void)hipEventRecord(p->e0, s);
    }
    ~EventBracket()
    {
        if (p) {
            if (p->e1) (void)hipEventRecord(p->e1, s);
            delete p;
        }
    }
};

inline int memset_async(void* p, int value, size_t bytes, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(p, value, bytes, s);
    return e == hipSuccess ? WDF_OK : fail(WDF_ELAUNCH, "hipMemsetAsync: %s", hipGetErrorString(e));
}

// the optional in-kernel Adam update is asked for by passing m: its other three buffers then have to be there
inline int adam_check(const void* m, const void* v, const void* step, const void* lr)
{
    return (m && (!v || !step || !lr)) ? fail(WDF_EINVAL, "Adam: m, v, step and lr go together") : WDF_OK;
}

// ---- chunk geometry: T steps in at most n_chunks chunks of L steps, L a multiple of `unit` ------------------------
template <class T> constexpr T round_up(T v, int64_t a) { return (v + (T)a - 1) / (T)a * (T)a; }
inline size_t waves64(int64_t B) { return (size_t)((B + 63) / 64); }          // 64-lane waves, one sequence per lane

struct ChunkGeom { int64_t L; int K; };

inline ChunkGeom chunk_geom(int64_t T, int n_chunks, int unit)
{
    if (n_chunks < 1) n_chunks = 1;
    const int64_t L = round_up((T + n_chunks - 1) / n_chunks, unit);
    return {L, (int)((T + L - 1) / L)};
}

// entry points that size buffers by n_chunks want exactly that many: hint (or null) names the export that returns a count that fits
inline int check_tiles(ChunkGeom g, int n_chunks, int64_t T, int unit, const char* hint)
{
    if (g.K == n_chunks) return WDF_OK;
    if (hint) return fail(WDF_EINVAL, "n_chunks = %d does not tile T = %lld in %d-step units: use %s (%d)", n_chunks, (long long)T, unit, hint, g.K);
    return fail(WDF_EINVAL, "n_chunks = %d does not tile T = %lld in %d-step units (%d does)", n_chunks, (long long)T, unit, g.K);
}

// ---- runtime values -> template arguments -------------------------------------------------------------------------
// dispatch(f, Bools{dyn}, Values<int, 3, 4, 5>{nl}) calls f(std::bool_constant<dyn>{}, std::integral_constant<int, nl>{}) for the
// listed combination the runtime values name, and returns false when they name none: the entry point then fails with
// no_kernel() instead of launching nothing.  f may itself return false (an `if constexpr` that leaves a combination out, so
// that no kernel is instantiated for it); a void f counts as true.
template <class T, T... Vs> struct Values { T v; };
using Bools = Values<bool, false, true>;

template <class F> bool dispatch(F&& f)
{
    if constexpr (std::is_void_v<decltype(f())>) { f(); return true; }
    else return f();
}

template <class F, class T, T... Vs, class... Rest> bool dispatch(F&& f, Values<T, Vs...> head, Rest... rest)
{
    return ((head.v == Vs && dispatch([&](auto... c) { return f(std::integral_constant<T, Vs>{}, c...); }, rest...)) || ...);
}

inline int no_kernel(const char* what) { return fail(WDF_EUNSUPPORTED, "%s: no kernel is built for this combination of arguments", what); }

// ---- workspace layouts --------------------------------------------------------------------------------------------
// Walks a layout once, handing out naturally aligned arrays from `base`.  With a null base it only counts, so a *_ws_bytes
// function and the entry point that carves the buffer share ONE walk.
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* b) : base((char*)b) {}
    void align(size_t a) { off = round_up(off, (int64_t)a); }
    template <class T> T* take(size_t count)
    {
        align(alignof(T));
        T* p = base ? (T*)(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace wdfcapi
