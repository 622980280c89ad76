// zk_transcript.hip -- the Fiat-Shamir transcript of include/zkhip.h on the device: a SHA-256 hash chain whose 32-byte state lives
// in device memory, so that kernels can draw challenges without a host round trip (the transcript-driven sumchecks of zk_fs.hip).
//   K15  init / absorb / challenges: one lane each (sha256.cuh); the work of a call is a handful of compressions.
// Every call is enqueued on the ctx stream; only zk_transcript_challenges and zk_transcript_state wait for it.
#include "sha256.cuh"
#include "zk_ctx.hpp"

#include <cstring>

namespace zk {

static constexpr size_t kInlineBytes = 2048;  // host bytes up to this length travel as a kernel argument
// One lane hashes an absorb byte by byte (~16 compressions per KiB): a transcript takes statements, commitments and values, not
// tables.  Longer strings are refused; a caller that wants a table in the transcript commits to it and absorbs the commitment.
static constexpr size_t kAbsorbMax = (size_t)1 << 20;
struct InlineBytes {
    unsigned char b[kInlineBytes];
};

__global__ void k_transcript_init(u32* __restrict__ state, InlineBytes label, unsigned len) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const char tag[] = "zkhip-fs-v1";
    Sha256Bytes s;
    s.init();
    for (int i = 0; i < 11; i++) s.put((u32)tag[i]);
    for (unsigned i = 0; i < len; i++) s.put(label.b[i]);
    s.finish();
    fs_state_store(state, s.h);
}

__device__ __forceinline__ void absorb_bytes(u32* __restrict__ state, const unsigned char* __restrict__ data, size_t len) {
    u32 st[8];
    fs_state_load(st, state);
    Sha256Bytes s;
    s.init();
    for (int i = 0; i < 8; i++)
        for (int k = 24; k >= 0; k -= 8) s.put(st[i] >> k);
    s.put(0x00);
    for (size_t i = 0; i < len; i++) s.put(data[i]);
    s.finish();
    fs_state_store(state, s.h);
}
__global__ void k_transcript_absorb_inline(u32* __restrict__ state, InlineBytes data, unsigned len) {
    if (threadIdx.x == 0 && blockIdx.x == 0) absorb_bytes(state, data.b, len);
}
__global__ void k_transcript_absorb(u32* __restrict__ state, const unsigned char* __restrict__ data, size_t len) {
    if (threadIdx.x == 0 && blockIdx.x == 0) absorb_bytes(state, data, len);
}

__global__ void k_transcript_challenges(u32* __restrict__ state, unsigned count, void* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    u32 st[8];
    fs_state_load(st, state);
    for (unsigned i = 0; i < count; i++) fr_store(out, i, fs_challenge(st));
    fs_state_store(state, st);
}

static int transcript_check(zk_ctx* ctx, const zk_transcript* t, const char* who) {
    if (!t) return fail(ctx, ZK_ERR_INVALID, "%s: null transcript", who);
    if (t->ctx != ctx) return fail(ctx, ZK_ERR_INVALID, "%s: the transcript belongs to another ctx", who);
    return ZK_OK;
}

int transcript_create(zk_ctx* ctx, const void* h_label, size_t label_len, zk_transcript** out) {
    *out = nullptr;
    if (label_len > kInlineBytes) return fail(ctx, ZK_ERR_INVALID, "zk_transcript_create: label of %zu bytes (at most %zu)", label_len, kInlineBytes);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    zk_transcript* t = new zk_transcript();
    t->ctx = ctx;
    hipError_t e = device_alloc(ctx, (void**)&t->d_state, 256);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->staged, hipEventDisableTiming);
    if (e != hipSuccess) {
        transcript_free(t);
        return hip_fail(ctx, e, "zk_transcript_create");
    }
    InlineBytes lb;
    std::memset(&lb, 0, sizeof(lb));
    if (label_len) std::memcpy(lb.b, h_label, label_len);
    hipLaunchKernelGGL(k_transcript_init, dim3(1), dim3(64), 0, ctx->stream, t->d_state, lb, (unsigned)label_len);
    e = hipGetLastError();
    if (e != hipSuccess) {
        transcript_free(t);
        return hip_fail(ctx, e, "k_transcript_init");
    }
    *out = t;
    return ZK_OK;
}

void transcript_free(zk_transcript* t) {
    if (!t) return;
    hipSetDevice(t->ctx->device);
    hipStreamSynchronize(t->ctx->stream);
    if (t->d_state) hipFree(t->d_state);
    if (t->d_stage) hipFree(t->d_stage);
    if (t->h_stage) hipHostFree(t->h_stage);
    if (t->staged) hipEventDestroy(t->staged);
    delete t;
}

int transcript_absorb(zk_ctx* ctx, zk_transcript* t, const void* h_bytes, size_t len) {
    const int rc = transcript_check(ctx, t, "zk_transcript_absorb");
    if (rc) return rc;
    if (len > kAbsorbMax) return fail(ctx, ZK_ERR_INVALID, "zk_transcript_absorb: %zu bytes (at most %zu per absorb)", len, kAbsorbMax);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    if (len <= kInlineBytes) {
        InlineBytes d;
        std::memset(&d, 0, sizeof(d));
        if (len) std::memcpy(d.b, h_bytes, len);
        hipLaunchKernelGGL(k_transcript_absorb_inline, dim3(1), dim3(64), 0, ctx->stream, t->d_state, d, (unsigned)len);
        ZK_HIP(ctx, hipGetLastError());
        return ZK_OK;
    }
    // a long string goes through the transcript's own pinned staging block; an earlier long absorb may still be reading it
    if (t->stage_busy) ZK_HIP(ctx, hipEventSynchronize(t->staged));
    if (len > t->stage_cap) {
        if (t->d_stage) hipFree(t->d_stage);
        if (t->h_stage) hipHostFree(t->h_stage);
        t->d_stage = nullptr, t->h_stage = nullptr, t->stage_cap = 0;
        ZK_HIP(ctx, hipHostMalloc((void**)&t->h_stage, len, hipHostMallocDefault));
        ZK_HIP(ctx, device_alloc(ctx, (void**)&t->d_stage, len));
        t->stage_cap = len;
    }
    std::memcpy(t->h_stage, h_bytes, len);
    ZK_HIP(ctx, hipMemcpyAsync(t->d_stage, t->h_stage, len, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_transcript_absorb, dim3(1), dim3(64), 0, ctx->stream, t->d_state, (const unsigned char*)t->d_stage, len);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipEventRecord(t->staged, ctx->stream));
    t->stage_busy = true;
    return ZK_OK;
}

int transcript_absorb_device(zk_ctx* ctx, zk_transcript* t, const void* d_ptr, size_t len) {
    const int rc = transcript_check(ctx, t, "zk_transcript_absorb_device");
    if (rc) return rc;
    if (len > kAbsorbMax) return fail(ctx, ZK_ERR_INVALID, "zk_transcript_absorb_device: %zu bytes (at most %zu per absorb)", len, kAbsorbMax);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_transcript_absorb, dim3(1), dim3(64), 0, ctx->stream, t->d_state, (const unsigned char*)d_ptr, len);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

int transcript_challenges(zk_ctx* ctx, zk_transcript* t, size_t count, uint64_t* h_out) {
    const int rc = transcript_check(ctx, t, "zk_transcript_challenges");
    if (rc) return rc;
    if (count == 0) return ZK_OK;
    if (count > ((size_t)1 << 20)) return fail(ctx, ZK_ERR_INVALID, "zk_transcript_challenges: %zu challenges in one call", count);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    void* res = pinned(ctx, count * 32);  // the kernel writes the results straight into pinned host memory
    if (!res) return ZK_ERR_OOM;
    hipLaunchKernelGGL(k_transcript_challenges, dim3(1), dim3(64), 0, ctx->stream, t->d_state, (unsigned)count, res);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(h_out, res, count * 32);
    return ZK_OK;
}

int transcript_state(zk_ctx* ctx, zk_transcript* t, uint8_t* h_state32) {
    const int rc = transcript_check(ctx, t, "zk_transcript_state");
    if (rc) return rc;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    ZK_HIP(ctx, hipMemcpyAsync(h_state32, t->d_state, 32, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
}

}  // namespace zk
