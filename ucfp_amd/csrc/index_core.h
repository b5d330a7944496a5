// index_core.h -- the object lifecycle and the call protocol (IndexCore) of every index that keeps per-tenant state and
// one shared workspace: the posting indexes (postings.h) and the exact-scan indexes (scan_index.h).  Host code in
// namespace ucfp; the few aliases and constants their kernels share sit in the unnamed namespace.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>

#include "common.h"

namespace {

using ucfp::capi_fail;
using ucfp::DevArr;

constexpr int kThreads = 256;
constexpr uint64_t kEmpty64 = ~0ull;
constexpr uint32_t kEmpty32 = 0xffffffffu;

}  // namespace

namespace ucfp {

// What an index holds besides its tenants and workspaces.  The workspace is shared by every call, so a call that
// uses it holds `mu`, waits for `done` (begin) and records `done` behind the work it enqueued (end / end_sync).
struct IndexCore {
    ucfp_ctx* ctx = nullptr;
    int device = 0;
    std::mutex mu;
    hipStream_t own = nullptr;   // the host-pointer calls run here
    hipEvent_t done = nullptr;   // the previous call's last work: the workspace is free after it

    ~IndexCore() {
        if (done) (void)hipEventDestroy(done);
        if (own) (void)hipStreamDestroy(own);
    }
    int begin() {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipEventSynchronize(done));
        return UCFP_OK;
    }
    // returns rc, unless the record fails
    int end(hipStream_t st, int rc = UCFP_OK) {
        HIP_TRY(hipEventRecord(done, st));
        return rc;
    }
    // the end of a call on `own` that copies results to the host: they have landed once the stream is drained.  A
    // failed call still drains what it enqueued and records `done`.
    int end_sync(int rc) {
        if (rc) {
            (void)hipStreamSynchronize(own);
            (void)hipEventRecord(done, own);
            return rc;
        }
        HIP_TRY(hipStreamSynchronize(own));
        return end(own);
    }
    // before the buffers of a destroyed index are freed
    void quiesce() {
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
    }
};

// A new index with its stream and `done` (recorded once, so the first call does not wait).  On failure nothing is left
// allocated.
template <class Ix>
int create_index(ucfp_ctx* ctx, const char* what, Ix** out) {
    Ix* ix = new (std::nothrow) Ix();
    if (!ix) return capi_fail(UCFP_E_INDEX, "out of host memory");
    ix->ctx = ctx;
    ix->device = ctx_device(ctx);
    hipError_t e = hipSetDevice(ix->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ix->own, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ix->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ix->done, ix->own);
    if (e != hipSuccess) {
        delete ix;   // ~IndexCore destroys what was created
        return capi_fail(UCFP_E_INDEX, "%s setup failed: %s", what, hipGetErrorString(e));
    }
    *out = ix;
    return UCFP_OK;
}

// the flush call: every dirty tenant is rebuilt on the index's own stream
template <class Ix, class Rebuild>
int flush_dirty(Ix* ix, Rebuild rebuild) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    int rc = ix->begin();
    for (auto it = ix->tenants.begin(); !rc && it != ix->tenants.end(); ++it)
        if (it->second.dirty) rc = rebuild(ix, it->second, ix->own);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ix->own));
    return ix->end(ix->own);
}

}  // namespace ucfp
