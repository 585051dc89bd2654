// What the host side of libtcrisk_hip.so is written with: the error path, the owners of device and pinned memory, the per-call
// bag of temporaries, the dispatch over the kernels' evaluation variants and the prologue of an entry point.  Every host file
// behind the C ABI (tcr_stage.hip ... tcr_rowpack.hip; the list is tcr_abi.hip's) uses these and nothing else of its neighbours.
//
// Invariants kept HERE, not by convention:
//   epoch    every allocation of context memory goes through DevArray::grow, which bumps HostCtx::epoch.  A captured round
//            (tcr_round_dev) holds the workspaces' addresses and the parameters by value; its graph is keyed by the epoch, so a
//            graph of an older epoch is dropped and the round captured again.  Whatever else a graph holds by value (parameters,
//            launch shape, a freed static plane) bumps the epoch where it changes.
//   capture  no allocation while HostCtx::capturing: grow refuses ("internal: allocation while a round is being captured")
//            before it touches the old block.  tcr_round_dev runs every new descriptor directly before it captures it, and that
//            run sizes every workspace.
//   copies   never touch the legacy default stream: copy_sync goes through a stream of the context.
//   owners   device memory of a context lives in DevArray, pinned host memory in PinnedArray, a call's temporaries in DevBuf;
//            events and graphs are destroyed by the structs that hold them (tcr_ctx.h).  Destroying a context is `delete ctx`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "tcr_device.h"

// What every helper here needs of a context; tcr_ctx (tcr_ctx.h) derives from it, so its members — the owners of everything
// that lives on the device — are destroyed first and the stream last.
struct HostCtx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    uint64_t epoch = 0;                         // bumped by every allocation / parameter change (see above)
    bool capturing = false;                     // tcr_round_dev is capturing a round on this context
    ~HostCtx() { if (stream) (void)hipStreamDestroy(stream); }
};

namespace {

thread_local std::string g_create_error;

int fail(HostCtx *ctx, const char *fmt, const char *a = "", const char *b = "")
{
    char buf[512];
    snprintf(buf, sizeof buf, fmt, a, b);
    if (ctx) ctx->err = buf; else g_create_error = buf;
    return -1;
}

#define HIPCHK(ctx, call)                                                              \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) return fail(ctx, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// Synchronous copies go through the context's own stream, never the legacy default stream: a legacy-stream operation
// fails ("would make the legacy stream depend on a capturing blocking stream") whenever ANY thread of the process is
// capturing a round (tcr_round_dev use_graph), and invalidates that capture.
inline hipError_t copy_sync(hipStream_t st, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    if (!bytes) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// A block of device memory a context owns: grow-only, cap in elements.
template <typename T>
struct DevArray {
    T *p = nullptr;
    size_t cap = 0;
    DevArray() = default;
    DevArray(DevArray &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }      // (a vector of owners may move them; no copies)
    ~DevArray() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // Room for `need` elements: -1 on failure, 1 when the block is a new one of need + slack elements (uninitialised; the old
    // block's contents are gone), 0 when the old one does.  The old block goes before the new one comes: the two never add up.
    int grow(HostCtx *ctx, size_t need, size_t slack = 0)
    {
        if (need <= cap) return 0;
        if (ctx->capturing) return fail(ctx, "internal: allocation while a round is being captured");
        reset();
        HIPCHK(ctx, hipMalloc(reinterpret_cast<void **>(&p), (need + slack) * sizeof(T) + 256));
        cap = need + slack;
        ++ctx->epoch;               // captured rounds hold addresses: they are re-captured (GraphCache::drop)
        return 1;
    }
    // room for n (+ slack) elements, then the n of `host` copied there synchronously on the context's stream
    int upload(HostCtx *ctx, const T *host, size_t n, size_t slack = 0)
    {
        if (grow(ctx, n, slack) < 0) return -1;
        HIPCHK(ctx, copy_sync(ctx->stream, p, host, n * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
    // exactly `bytes` (tcr_ctx_create's fixed blocks, before there is anything to re-capture)
    hipError_t alloc_bytes(size_t bytes)
    {
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), bytes);
        if (e == hipSuccess) cap = bytes / sizeof(T);
        return e;
    }
};

// The same for pinned host memory (no epoch: nothing on the device holds its address beyond the call that uses it).
template <typename T>
struct PinnedArray {
    T *p = nullptr;
    size_t cap = 0;
    PinnedArray() = default;
    PinnedArray(const PinnedArray &) = delete;
    ~PinnedArray() { reset(); }
    void reset() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    hipError_t alloc(size_t count)
    {
        reset();
        const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), count * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) cap = count;
        return e;
    }
};

inline void destroy_events(hipEvent_t *ev, size_t n)
{
    for (size_t i = 0; i < n; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);
}

// The temporaries of one _host entry point: freed when the call returns.
struct DevBuf {
    std::vector<void *> ptrs;
    ~DevBuf() { for (void *p : ptrs) (void)hipFree(p); }
    template <typename T>
    T *get(size_t count)
    {
        void *p = nullptr;
        if (hipMalloc(&p, count * sizeof(T) + 256) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return static_cast<T *>(p);
    }
    template <typename T>
    T *put(const T *host, size_t count)
    {
        T *d = get<T>(count);
        if (d && hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    }
};

// Device -> host copy of an output the caller may leave out (dst == NULL).
template <typename T>
int d2h(HostCtx *ctx, T *dst, const T *src, size_t count)
{
    if (dst) HIPCHK(ctx, copy_sync(ctx->stream, dst, src, count * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
}

// The prologue of an entry point: the context's device made current; the stream the call works on, NULL on failure.
inline hipStream_t enter(HostCtx *ctx, void *stream_ = nullptr)
{
    if (!ctx) return nullptr;
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) { fail(ctx, "%s failed: %s", "hipSetDevice(ctx->device)", hipGetErrorString(e)); return nullptr; }
    return stream_ ? (hipStream_t)stream_ : ctx->stream;
}

// k_integrate<R, AFFINE, PROBE, SM>, k_probe_rhs<R, AFFINE, SM>, k_init_m<AFFINE, SM>: pick the instantiation.  The narrow
// static modes exist for affine grids only (a context whose grids are not all affine has had its static planes widened to fp64
// by settle_static).  f(std::bool_constant<AFFINE>, std::integral_constant<int, SM>) is called for the one combination that holds.
template <class F>
void with_eval_variant(bool affine, int static_mode, F &&f)
{
    using tcr::kStatF64; using tcr::kStatF64Split; using tcr::kStatPack16; using tcr::kStatU8F32; using tcr::kStatPack64;
    if (affine) {
        switch (static_mode) {
        case kStatF64Split: f(std::true_type{}, std::integral_constant<int, kStatF64Split>{}); break;
        case kStatPack16: f(std::true_type{}, std::integral_constant<int, kStatPack16>{}); break;
        case kStatU8F32: f(std::true_type{}, std::integral_constant<int, kStatU8F32>{}); break;
        case kStatPack64: f(std::true_type{}, std::integral_constant<int, kStatPack64>{}); break;
        default: f(std::true_type{}, std::integral_constant<int, kStatF64>{}); break;
        }
    } else if (static_mode == kStatF64Split) f(std::false_type{}, std::integral_constant<int, kStatF64Split>{});
    else f(std::false_type{}, std::integral_constant<int, kStatF64>{});
}

// two flags -> two std::bool_constant arguments (k_emit<R, AFFINE, OVERFLOW>)
template <class F>
void with_flags(bool a, bool b, F &&f)
{
    if (a) { if (b) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
    else if (b) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}

}  // namespace
