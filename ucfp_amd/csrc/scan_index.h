// scan_index.h -- the exact-scan core shared by tlsh_index.hip, image_match.hip (A16) and
// minhash_index.hip (A17).
//
// All three keep a tenant's rows on the host, in an id-ordered map, and rebuild its device rows lazily after a change;
// a query writes one u32 key per (query, row) in passes whose key matrix stays below `key_bytes`, and topk.hip's
// select_topk_u32 + merge tree pick the k smallest by (key, id) -- rows are in ascending id order, so ties by row are
// ties by id.  This file owns the tenant table and its mutations, the head of the rebuild, the query driver with the
// pass loop, and the two call shapes (device pointers on the caller's stream, host pointers staged on the index's own).
// An index derives from ScanIndex<Row> and supplies
//   size_t rec_bytes() const                       bytes of a record as callers pass it (a row or a query)
//   Row to_row(const uint8_t* rec) const           what the table keeps of a record
//   size_t row_len() const, kPad                   elements of Row::value_type per flattened row, and their fill
//   int upload(rows, h_rows, n, stride, st)        flattened rows -> the tenant's device rows
// and, per query, its key kernel and what it needs before it.  Kernels are in the unnamed namespace (one copy per
// translation unit, as in postings.h); the rest is host code in namespace ucfp.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "index_core.h"

namespace {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// empty answers for every query (unknown tenant / no rows); out_u32 is optional
__global__ void scan_empty(size_t nq, uint32_t k, uint64_t* __restrict__ out_ids, uint32_t* __restrict__ out_u32,
                           float* __restrict__ out_scores, uint32_t* __restrict__ out_n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq * k) {
        out_ids[i] = kEmpty64;
        if (out_u32) out_u32[i] = kEmpty32;
        out_scores[i] = -1.0f;
    }
    if (i < nq) out_n[i] = 0;
}

}  // namespace

namespace ucfp {

constexpr size_t kScanKeyBytes = (size_t)1 << 30;   // key matrix of one pass (scan_key_bytes_env overrides it)
constexpr size_t kScanMaxRows = (size_t)1 << 31;

template <class Row>
struct ScanTenant {
    std::map<uint64_t, Row> recs;   // id -> row; ascending id = row order, so ties by row are ties by id
    bool dirty = true;
    size_t n = 0, stride = 0;       // valid when !dirty; stride = n rounded up to 64, for the indexes that store planes
    DevArr rows, ids;
};

template <class R>
struct ScanIndex : IndexCore {
    using Row = R;
    using Tenant = ScanTenant<R>;
    std::unordered_map<uint32_t, Tenant> tenants;
    size_t key_bytes = kScanKeyBytes;
    DevArr b_packed;                // rebuild staging
    DevArr q_in, q_ws, q_out;       // host-pointer queries, the pass workspace, host-pointer answers
};

// the device answers of a query: [nq][k] each, n [nq]; u32 is NULL for an index without such an array
struct ScanOut {
    uint64_t* ids;
    uint32_t* u32;
    float* scores;
    uint32_t* n;
};

// at creation: a smaller key matrix means more passes over the rows -- for tuning, and for tests of the pass loop at
// small sizes
template <class Ix>
void scan_key_bytes_env(Ix* ix, const char* var) {
    if (const char* e = getenv(var)) ix->key_bytes = std::max<size_t>(4096, strtoull(e, nullptr, 10));
}

template <class Ix>
void scan_destroy(Ix* ix) {
    if (!ix) return;
    ix->quiesce();
    for (auto& kv : ix->tenants)
        for (DevArr* a : {&kv.second.rows, &kv.second.ids}) a->release();
    for (DevArr* a : {&ix->b_packed, &ix->q_in, &ix->q_ws, &ix->q_out}) a->release();
    delete ix;
}

// ---------------------------------------------------------------- mutations: bookkeeping on the host table

// n > 0 host records into the table; the caller holds ix->mu
template <class Ix>
void scan_insert(Ix* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* recs, size_t n) {
    auto& T = ix->tenants[tenant];
    const size_t rb = ix->rec_bytes();
    for (size_t i = 0; i < n; i++)
        T.recs.insert_or_assign(T.recs.end(), ids[i], ix->to_row(recs + i * rb));   // the hint: ascending ids append in constant time
    T.dirty = true;
}

// `what` names the record argument in the message
template <class Ix>
int scan_upsert(Ix* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* recs, size_t n, const char* what) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (!n) return UCFP_OK;
    if (!ids || !recs) return capi_fail(UCFP_E_INVALID, "ids/%s is NULL", what);
    std::lock_guard<std::mutex> lk(ix->mu);
    scan_insert(ix, tenant, ids, recs, n);
    return UCFP_OK;
}

template <class Ix>
int scan_upsert_dev(Ix* ix, uint32_t tenant, const uint64_t* d_ids, const uint8_t* d_recs, size_t n, const char* what,
                    void* stream) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (!n) return UCFP_OK;
    if (!d_ids || !d_recs) return capi_fail(UCFP_E_INVALID, "ids/%s is NULL", what);
    std::lock_guard<std::mutex> lk(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    // the row table lives on the host (mutations are bookkeeping; the device rows are rebuilt at the next query)
    std::vector<uint64_t> ids(n);
    std::vector<uint8_t> recs(n * ix->rec_bytes());
    HIP_TRY(hipMemcpyAsync(ids.data(), d_ids, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(recs.data(), d_recs, recs.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    scan_insert(ix, tenant, ids.data(), recs.data(), n);
    return UCFP_OK;
}

template <class Ix>
int scan_delete(Ix* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (n && !ids) return capi_fail(UCFP_E_INVALID, "ids is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    size_t removed = 0;
    auto it = ix->tenants.find(tenant);
    if (it != ix->tenants.end()) {
        for (size_t i = 0; i < n; i++) removed += it->second.recs.erase(ids[i]);
        if (removed) it->second.dirty = true;
    }
    if (n_removed) *n_removed = removed;
    return UCFP_OK;
}

template <class Ix>
int scan_size(Ix* ix, uint32_t tenant, size_t* rows) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    auto it = ix->tenants.find(tenant);
    if (rows) *rows = it == ix->tenants.end() ? 0 : it->second.recs.size();
    return UCFP_OK;
}

// ---------------------------------------------------------------- rebuild

// The tenant's rows flattened in id order (row_len() elements each, kPad where a row is shorter), the ids uploaded,
// the rows handed to the index's upload.  One synchronisation: the host vectors go out of scope.
template <class Ix>
int scan_rebuild(Ix* ix, typename Ix::Tenant& T, hipStream_t st) {
    using Elem = typename Ix::Row::value_type;
    const size_t n = T.recs.size();
    if (n >= kScanMaxRows) return capi_fail(UCFP_E_INVALID, "too many rows in one tenant (%zu)", n);
    const size_t stride = (n + 63) & ~(size_t)63, len = ix->row_len();
    std::vector<Elem> h_rows(n * len, Ix::kPad);
    std::vector<uint64_t> h_ids(n);
    size_t i = 0;
    for (auto& kv : T.recs) {
        h_ids[i] = kv.first;
        memcpy(h_rows.data() + i * len, kv.second.data(), kv.second.size() * sizeof(Elem));
        i++;
    }
    int rc;
    if ((rc = T.ids.ensure(n * 8))) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(T.ids.p, h_ids.data(), n * 8, hipMemcpyHostToDevice, st));
    if ((rc = ix->upload(T.rows, h_rows.data(), n, stride, st))) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    T.n = n;
    T.stride = stride;
    T.dirty = false;
    return UCFP_OK;
}

template <class Ix>
int scan_flush(Ix* ix) { return flush_dirty(ix, scan_rebuild<Ix>); }

// ---------------------------------------------------------------- query

// The selection of nq queries against a tenant, on `st`, for a caller that holds ix->mu and has passed begin().
//   prep(uint8_t* q_area)                    once: q_bytes of workspace (256-byte aligned) for the queries in kernel form
//   keys(T, q0, cnt, uint32_t* keymat)       per pass: keymat[q - q0][row] for the queries [q0, q0 + cnt)
//   fit(n, chunk) -> rc                      optional: a refusal by tenant size and pass size, before the workspace grows
// prep and keys launch; the driver looks at hipGetLastError behind them.  *sel is left NULL when the answers are
// already final (k = 0, unknown tenant, no rows); otherwise o.ids and o.n are written and *sel -- o.u32, or workspace
// when that is NULL -- holds the selected keys [nq][k], 0xffffffff past a query's count, for the index's score kernel.
template <class Ix, class Prep, class Keys, class Fit = std::nullptr_t>
int scan_query(Ix* ix, uint32_t tenant, size_t nq, uint32_t k, size_t q_bytes, const ScanOut& o, hipStream_t st, uint32_t** sel,
               Prep prep, Keys keys, Fit fit = nullptr) {
    int rc;
    *sel = nullptr;
    if (k == 0) {
        HIP_TRY(hipMemsetAsync(o.n, 0, nq * 4, st));
        return UCFP_OK;
    }
    auto it = ix->tenants.find(tenant);
    if (it != ix->tenants.end() && it->second.dirty && (rc = scan_rebuild(ix, it->second, st))) return rc;
    if (it == ix->tenants.end() || it->second.n == 0) {
        hipLaunchKernelGGL(scan_empty, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, st, nq, k, o.ids, o.u32, o.scores, o.n);
        HIP_TRY(hipGetLastError());
        return UCFP_OK;
    }
    const typename Ix::Tenant& T = it->second;
    const size_t n = T.n;
    // queries per pass: the key matrix stays below key_bytes; queries ride on gridDim.y of the select kernel
    size_t chunk = std::max<size_t>(1, ix->key_bytes / (4 * n));
    chunk = std::min<size_t>(std::min<size_t>(chunk, 32768), nq);
    if constexpr (!std::is_same<Fit, std::nullptr_t>::value)
        if ((rc = fit(n, chunk))) return rc;
    const SelectPlan sp = select_plan(n, (uint32_t)chunk);
    const size_t tmp_e = 2 * topk_merge_tmp_entries(sp.slices, (uint32_t)chunk, k);   // both tree levels
    size_t off = align256(q_bytes);
    const size_t o_keys = off;
    off = align256(off + chunk * n * 4 + 64);
    const size_t o_pid = off;
    off = align256(off + (size_t)sp.slices * chunk * k * 8);
    const size_t o_pk = off;
    off = align256(off + (size_t)sp.slices * chunk * k * 4);
    const size_t o_pc = off;
    off = align256(off + (size_t)sp.slices * chunk * 4);
    const size_t o_tid = off;
    off = align256(off + tmp_e * 8);
    const size_t o_tk = off;
    off = align256(off + tmp_e * 4);
    const size_t o_sel = off;   // the selected keys of every query, when the caller has no array for them
    if (!o.u32) off = align256(off + nq * k * 4);
    if ((rc = ix->q_ws.ensure(off))) return rc;
    uint8_t* w = ix->q_ws.template as<uint8_t>();
    uint32_t* keymat = reinterpret_cast<uint32_t*>(w + o_keys);
    uint64_t* pid = reinterpret_cast<uint64_t*>(w + o_pid);
    uint32_t* pk = reinterpret_cast<uint32_t*>(w + o_pk);
    uint32_t* okeys = o.u32 ? o.u32 : reinterpret_cast<uint32_t*>(w + o_sel);
    prep(w);
    HIP_TRY(hipGetLastError());
    for (size_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t cnt = (uint32_t)std::min(chunk, nq - q0);
        keys(T, q0, cnt, keymat);
        HIP_TRY(hipGetLastError());
        SelectPlan pl = select_plan(n, cnt);
        if (pl.slices > sp.slices) {   // the partial lists were sized for the full pass
            pl.per_slice = (((n + sp.slices - 1) / sp.slices) + 63) & ~(size_t)63;
            pl.slices = (uint32_t)((n + pl.per_slice - 1) / pl.per_slice);
        }
        launch_select_topk_u32(keymat, T.ids.template as<uint64_t>(), n, pl, cnt, k, pid, pk, reinterpret_cast<uint32_t*>(w + o_pc), st);
        launch_topk_merge_tree_u32(pid, pk, pl.slices, cnt, k, reinterpret_cast<uint64_t*>(w + o_tid),
                                   reinterpret_cast<uint32_t*>(w + o_tk), o.ids + q0 * k, okeys + q0 * k, o.n + q0, st);
        HIP_TRY(hipGetLastError());
    }
    *sel = okeys;
    return UCFP_OK;
}

// A query with device pointers: run(st) enqueues it on the caller's stream.
template <class Ix, class Run>
int scan_query_dev(Ix* ix, void* stream, Run run) {
    std::lock_guard<std::mutex> lk(ix->mu);
    int rc;
    if ((rc = ix->begin())) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = run(st);
    return ix->end(st, rc);
}

// A query with host pointers (nq > 0), on the index's own stream: the queries are staged in q_in, run(d_q, o, st)
// answers into q_out -- ids, the u32 array if the index has one (out_u32 != NULL), scores, counts, each at a 256-byte
// boundary -- and the answers are copied back.
template <class Ix, class Run>
int scan_query_host(Ix* ix, const uint8_t* q, size_t nq, uint32_t k, uint64_t* out_ids, uint32_t* out_u32, float* out_scores,
                    uint32_t* out_n, Run run) {
    std::lock_guard<std::mutex> lk(ix->mu);
    int rc;
    if ((rc = ix->begin())) return rc;
    hipStream_t st = ix->own;
    const size_t nk = nq * k, q_bytes = nq * ix->rec_bytes();
    const size_t o_u32 = align256(nk * 8), o_sc = out_u32 ? align256(o_u32 + nk * 4) : o_u32, o_n = align256(o_sc + nk * 4);
    if ((rc = ix->q_in.ensure(q_bytes)) || (rc = ix->q_out.ensure(o_n + nq * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(ix->q_in.p, q, q_bytes, hipMemcpyHostToDevice, st));
    uint8_t* ob = ix->q_out.template as<uint8_t>();
    rc = run(ix->q_in.template as<uint8_t>(),
             ScanOut{(uint64_t*)ob, out_u32 ? (uint32_t*)(ob + o_u32) : nullptr, (float*)(ob + o_sc), (uint32_t*)(ob + o_n)}, st);
    if (rc) return ix->end_sync(rc);
    if (nk) {
        HIP_TRY(hipMemcpyAsync(out_ids, ob, nk * 8, hipMemcpyDeviceToHost, st));
        if (out_u32) HIP_TRY(hipMemcpyAsync(out_u32, ob + o_u32, nk * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_scores, ob + o_sc, nk * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(out_n, ob + o_n, nq * 4, hipMemcpyDeviceToHost, st));
    return ix->end_sync(UCFP_OK);
}

}  // namespace ucfp
