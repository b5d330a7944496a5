// tlsh_index.hip -- GPU index over TLSH digests: "the k stored digests nearest to this one", exact.
//
// Spec (the distance of the published TLSH comparison, as the reference's SDK applies it to `tlsh-128-1` records): a row
// and a query are 35 bytes, swap(checksum) swap(L) (Q1 << 4 | Q2) body[32]; un-swapped,
//   dist = f(md(L, L', 256)) + g(md(Q1, Q1', 16)) + g(md(Q2, Q2', 16)) + (checksum != checksum') + sum over the 128 bit pairs
//          of |a - b| with 3 counted as 6;   md(x, y, R) = min(|x - y|, R - |x - y|), f(l) = l <= 1 ? l : 12 l,
//          g(q) = q <= 1 ? q : 12 (q - 1)
// hits: dist <= max_distance, ordered (dist asc, id asc), first k; score = (float)(2473 - dist) / 2473.0f.
//
// Layout of a tenant after a (lazy) rebuild: rows in ascending id order, stored as 13 dword planes of `stride` rows each
// (structure of arrays, so lane = row loads coalesce): the body as three thermometer bit planes (a >= 1, a >= 2, a >= 3;
// 4 dwords each), then a header word checksum | L << 8 | Q1 << 16 | Q2 << 20.  Over the XORed planes the body distance is
// popc(d1) + popc(d2) + popc(d3) + 3 popc(d1 & d2 & d3): |a - b| planes differ, and all three differ exactly when |a - b| = 3.
//
// Query: tl_pack brings the queries into the same form (16 dwords per query); then, in passes whose key matrix stays
// below 1 GiB,
//   tl_keys   lane = row, its 13 dwords in registers across the queries of the pass (their words are wave-uniform:
//             scalar loads), one u32 key per (query, row): the distance, or 0xffffffff above max_distance
//   topk.hip  select_topk_u32 + the merge tree, the selector of the cosine search: exact by (key, id)
// and tl_scores turns the selected distances into scores.  ALU-bound once a pass carries more than a few queries: about
// 60 integer instructions per (query, row) against 52 bytes per row.
// Not here: sharding over GPUs, a search micro-batcher, save / load (ucfp_hip.h says so).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <map>
#include <unordered_map>
#include <vector>

#include "postings.h"

namespace {

constexpr uint32_t kRowBytes = UCFP_TLSH_BYTES;
constexpr uint32_t kPlanes = 13;                 // dwords per stored row
constexpr uint32_t kQueryWords = 16;             // dwords per packed query
constexpr size_t kKeyBytes = (size_t)1 << 30;    // key matrix of one pass (UCFP_TLSH_KEY_BYTES at creation overrides it)
constexpr size_t kMaxRows = (size_t)1 << 31;

// packed 35-byte digests -> planes; word w of item i goes to out[w * stride_w + i * stride_i]
__global__ void tl_pack(const uint8_t* __restrict__ in, size_t n, uint32_t* __restrict__ out, size_t stride_w, size_t stride_i) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* d = in + i * kRowBytes;
    const uint32_t b0 = d[0], b1 = d[1], b2 = d[2];
    const uint32_t ck = ((b0 & 15u) << 4) | (b0 >> 4), L = ((b1 & 15u) << 4) | (b1 >> 4);
    uint32_t* o = out + i * stride_i;
    for (uint32_t w = 0; w < 4; w++) {
        uint32_t p1 = 0, p2 = 0, p3 = 0;
        for (uint32_t j = 0; j < 8; j++) {
            const uint32_t c = d[3 + 8 * w + j];
            for (uint32_t t = 0; t < 4; t++) {
                const uint32_t a = (c >> (2 * t)) & 3u, bit = 4 * j + t;
                p1 |= (a >= 1 ? 1u : 0u) << bit;
                p2 |= (a >= 2 ? 1u : 0u) << bit;
                p3 |= (a >= 3 ? 1u : 0u) << bit;
            }
        }
        o[(size_t)w * stride_w] = p1;
        o[(size_t)(4 + w) * stride_w] = p2;
        o[(size_t)(8 + w) * stride_w] = p3;
    }
    o[(size_t)12 * stride_w] = ck | (L << 8) | ((b2 >> 4) << 16) | ((b2 & 15u) << 20);
}

__device__ __forceinline__ uint32_t ring(uint32_t x, uint32_t y, uint32_t r) {
    const uint32_t d = x > y ? x - y : y - x;
    return d < r - d ? d : r - d;
}

// keys[q][row] for the nq queries of a pass
__global__ __launch_bounds__(kThreads) void tl_keys(const uint32_t* __restrict__ rows, size_t n, size_t stride,
                                                     const uint32_t* __restrict__ qw, uint32_t nq, uint32_t max_distance,
                                                     uint32_t* __restrict__ keys) {
    const size_t row = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (row >= n) return;
    uint32_t r[kPlanes];
#pragma unroll
    for (uint32_t w = 0; w < kPlanes; w++) r[w] = rows[(size_t)w * stride + row];
    const uint32_t r_ck = r[12] & 255u, r_l = (r[12] >> 8) & 255u, r_q1 = (r[12] >> 16) & 15u, r_q2 = (r[12] >> 20) & 15u;
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t* __restrict__ qq = qw + (size_t)q * kQueryWords;   // wave-uniform
        uint32_t d = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
            const uint32_t d1 = r[w] ^ qq[w], d2 = r[4 + w] ^ qq[4 + w], d3 = r[8 + w] ^ qq[8 + w];
            d += (uint32_t)__popc(d1) + (uint32_t)__popc(d2) + (uint32_t)__popc(d3) + 3u * (uint32_t)__popc(d1 & d2 & d3);
        }
        const uint32_t h = qq[12];
        const uint32_t l = ring(r_l, (h >> 8) & 255u, 256u);
        const uint32_t a = ring(r_q1, (h >> 16) & 15u, 16u), b = ring(r_q2, (h >> 20) & 15u, 16u);
        d += l <= 1 ? l : 12u * l;
        d += a <= 1 ? a : 12u * (a - 1);
        d += b <= 1 ? b : 12u * (b - 1);
        d += r_ck != (h & 255u) ? 1u : 0u;
        keys[(size_t)q * n + row] = d <= max_distance ? d : kEmpty32;
    }
}

__global__ void tl_scores(const uint32_t* __restrict__ dist, size_t total, float* __restrict__ scores) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint32_t d = dist[i];
    scores[i] = d == kEmpty32 ? -1.0f : (float)(UCFP_TLSH_MAX_DISTANCE - d) / (float)UCFP_TLSH_MAX_DISTANCE;
}

// empty answers for every query (unknown tenant / no rows)
__global__ void tl_empty(size_t nq, uint32_t k, uint64_t* __restrict__ out_ids, uint32_t* __restrict__ out_dist,
                         float* __restrict__ out_scores, uint32_t* __restrict__ out_n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq * k) {
        out_ids[i] = kEmpty64;
        out_dist[i] = kEmpty32;
        out_scores[i] = -1.0f;
    }
    if (i < nq) out_n[i] = 0;
}

using Row = std::array<uint8_t, kRowBytes>;

struct Tenant {
    std::map<uint64_t, Row> recs;   // id -> digest; ascending id = row order, so ties by row are ties by id
    bool dirty = true;
    size_t n = 0, stride = 0;       // valid when !dirty
    DevArr rows, ids;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

struct ucfp_tlsh_index : ucfp::IndexCore {
    std::unordered_map<uint32_t, Tenant> tenants;
    size_t key_bytes = kKeyBytes;
    DevArr b_packed;                // rebuild staging
    DevArr q_in, q_ws, q_out;       // host-pointer queries, the pass workspace, host-pointer answers
};

namespace {

int rebuild(ucfp_tlsh_index* ix, Tenant& T, hipStream_t st) {
    const size_t n = T.recs.size();
    if (n >= kMaxRows) return capi_fail(UCFP_E_INVALID, "too many rows in one tenant (%zu)", n);
    const size_t stride = (n + 63) & ~(size_t)63;
    std::vector<uint8_t> h_rows(n * kRowBytes);
    std::vector<uint64_t> h_ids(n);
    size_t i = 0;
    for (auto& kv : T.recs) {
        h_ids[i] = kv.first;
        memcpy(h_rows.data() + i * kRowBytes, kv.second.data(), kRowBytes);
        i++;
    }
    int rc;
    if ((rc = T.ids.ensure(n * 8)) || (rc = T.rows.ensure(stride * kPlanes * 4)) || (rc = ix->b_packed.ensure(n * kRowBytes)))
        return rc;
    if (n) {
        HIP_TRY(hipMemcpyAsync(T.ids.p, h_ids.data(), n * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ix->b_packed.p, h_rows.data(), n * kRowBytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(T.rows.p, 0, stride * kPlanes * 4, st));
        hipLaunchKernelGGL(tl_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ix->b_packed.as<uint8_t>(), n,
                           T.rows.as<uint32_t>(), stride, (size_t)1);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));   // the host vectors above go out of scope
    T.n = n;
    T.stride = stride;
    T.dirty = false;
    return UCFP_OK;
}

int do_upsert(ucfp_tlsh_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* digests, size_t n) {
    if (!n) return UCFP_OK;
    if (!ids || !digests) return capi_fail(UCFP_E_INVALID, "ids/digests is NULL");
    Tenant& T = ix->tenants[tenant];
    for (size_t i = 0; i < n; i++) {
        Row r;
        memcpy(r.data(), digests + i * kRowBytes, kRowBytes);
        T.recs.insert_or_assign(T.recs.end(), ids[i], r);   // the hint: ascending ids append in constant time
    }
    T.dirty = true;
    return UCFP_OK;
}

int query_impl(ucfp_tlsh_index* ix, uint32_t tenant, const uint8_t* d_q, size_t nq, uint32_t k, uint32_t max_distance,
               uint64_t* d_ids, uint32_t* d_dist, float* d_scores, uint32_t* d_n, hipStream_t st) {
    int rc;
    if (k == 0) {
        HIP_TRY(hipMemsetAsync(d_n, 0, nq * 4, st));
        return UCFP_OK;
    }
    auto it = ix->tenants.find(tenant);
    if (it != ix->tenants.end() && it->second.dirty && (rc = rebuild(ix, it->second, st))) return rc;
    if (it == ix->tenants.end() || it->second.n == 0) {
        hipLaunchKernelGGL(tl_empty, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, st, nq, k, d_ids, d_dist, d_scores, d_n);
        HIP_TRY(hipGetLastError());
        return UCFP_OK;
    }
    Tenant& T = it->second;
    const size_t n = T.n;
    // queries per pass: the key matrix stays below key_bytes; queries ride on gridDim.y of the select kernel
    size_t chunk = std::max<size_t>(1, ix->key_bytes / (4 * n));
    chunk = std::min<size_t>(std::min<size_t>(chunk, 32768), nq);
    const ucfp::SelectPlan sp = ucfp::select_plan(n, (uint32_t)chunk);
    const size_t tmp_e = 2 * ucfp::topk_merge_tmp_entries(sp.slices, (uint32_t)chunk, k);   // both tree levels
    size_t off = 0;
    const size_t o_qw = off;
    off = align256(off + nq * kQueryWords * 4);
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
    if ((rc = ix->q_ws.ensure(off))) return rc;
    uint8_t* w = ix->q_ws.as<uint8_t>();
    uint32_t* qw = reinterpret_cast<uint32_t*>(w + o_qw);
    uint32_t* keymat = reinterpret_cast<uint32_t*>(w + o_keys);
    hipLaunchKernelGGL(tl_pack, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_q, nq, qw, (size_t)1, (size_t)kQueryWords);
    HIP_TRY(hipGetLastError());
    for (size_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t cnt = (uint32_t)std::min(chunk, nq - q0);
        hipLaunchKernelGGL(tl_keys, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, T.rows.as<uint32_t>(), n,
                           T.stride, qw + q0 * kQueryWords, cnt, max_distance, keymat);
        HIP_TRY(hipGetLastError());
        ucfp::SelectPlan pl = ucfp::select_plan(n, cnt);
        if (pl.slices > sp.slices) {   // the partial lists were sized for the full pass
            pl.per_slice = (((n + sp.slices - 1) / sp.slices) + 63) & ~(size_t)63;
            pl.slices = (uint32_t)((n + pl.per_slice - 1) / pl.per_slice);
        }
        ucfp::launch_select_topk_u32(keymat, T.ids.as<uint64_t>(), n, pl, cnt, k, reinterpret_cast<uint64_t*>(w + o_pid),
                                     reinterpret_cast<uint32_t*>(w + o_pk), reinterpret_cast<uint32_t*>(w + o_pc), st);
        ucfp::launch_topk_merge_tree_u32(reinterpret_cast<uint64_t*>(w + o_pid), reinterpret_cast<uint32_t*>(w + o_pk), pl.slices,
                                         cnt, k, reinterpret_cast<uint64_t*>(w + o_tid), reinterpret_cast<uint32_t*>(w + o_tk),
                                         d_ids + q0 * k, d_dist + q0 * k, d_n + q0, st);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(tl_scores, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, st, d_dist, nq * k, d_scores);
    HIP_TRY(hipGetLastError());
    return UCFP_OK;
}

int query_args(ucfp_tlsh_index* ix, const void* digests, size_t nq, uint32_t k, const void* out_ids, const void* out_dist,
               const void* out_scores, const void* out_n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (k > UCFP_INDEX_MAX_K) return capi_fail(UCFP_E_INVALID, "k = %u exceeds UCFP_INDEX_MAX_K = %u", k, UCFP_INDEX_MAX_K);
    if (nq > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "too many queries");
    if (nq && (!digests || !out_n)) return capi_fail(UCFP_E_INVALID, "digests/out_n is NULL");
    if (nq && k && (!out_ids || !out_dist || !out_scores)) return capi_fail(UCFP_E_INVALID, "an output buffer is NULL");
    return UCFP_OK;
}

}  // namespace

extern "C" {

int ucfp_tlsh_index_create(ucfp_ctx* ctx, uint32_t flags, ucfp_tlsh_index** out) {
    if (!ctx || !out) return capi_fail(UCFP_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (flags != 0) return capi_fail(UCFP_E_INVALID, "no TLSH index flags are defined (got %u)", flags);
    const int rc = ucfp::create_index(ctx, "TLSH index", out);
    // a smaller key matrix means more passes over the rows: for tuning, and for tests of the pass loop at small sizes
    if (const char* e = rc ? nullptr : getenv("UCFP_TLSH_KEY_BYTES")) (*out)->key_bytes = std::max<size_t>(4096, strtoull(e, nullptr, 10));
    return rc;
}

void ucfp_tlsh_index_destroy(ucfp_tlsh_index* ix) {
    if (!ix) return;
    ix->quiesce();
    for (auto& kv : ix->tenants)
        for (DevArr* a : {&kv.second.rows, &kv.second.ids}) a->release();
    for (DevArr* a : {&ix->b_packed, &ix->q_in, &ix->q_ws, &ix->q_out}) a->release();
    delete ix;
}

int ucfp_tlsh_index_upsert(ucfp_tlsh_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* digests, size_t n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    return do_upsert(ix, tenant, ids, digests, n);
}

int ucfp_tlsh_index_upsert_dev(ucfp_tlsh_index* ix, uint32_t tenant, const uint64_t* d_ids, const uint8_t* d_digests, size_t n,
                               void* stream) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (!n) return UCFP_OK;
    if (!d_ids || !d_digests) return capi_fail(UCFP_E_INVALID, "ids/digests is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    // the row table lives on the host (mutations are bookkeeping; the planes are rebuilt at the next query)
    std::vector<uint64_t> ids(n);
    std::vector<uint8_t> rows(n * kRowBytes);
    HIP_TRY(hipMemcpyAsync(ids.data(), d_ids, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(rows.data(), d_digests, n * kRowBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return do_upsert(ix, tenant, ids.data(), rows.data(), n);
}

int ucfp_tlsh_index_delete(ucfp_tlsh_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed) {
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

int ucfp_tlsh_index_size(ucfp_tlsh_index* ix, uint32_t tenant, size_t* rows) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    auto it = ix->tenants.find(tenant);
    if (rows) *rows = it == ix->tenants.end() ? 0 : it->second.recs.size();
    return UCFP_OK;
}

int ucfp_tlsh_index_flush(ucfp_tlsh_index* ix) { return ucfp::flush_dirty(ix, rebuild); }

int ucfp_tlsh_index_query_dev(ucfp_tlsh_index* ix, uint32_t tenant, const uint8_t* d_digests, size_t nq, uint32_t k,
                              uint32_t max_distance, uint64_t* d_out_ids, uint32_t* d_out_dist, float* d_out_scores,
                              uint32_t* d_out_n, void* stream) {
    int rc = query_args(ix, d_digests, nq, k, d_out_ids, d_out_dist, d_out_scores, d_out_n);
    if (rc || nq == 0) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    if ((rc = ix->begin())) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = query_impl(ix, tenant, d_digests, nq, k, max_distance, d_out_ids, d_out_dist, d_out_scores, d_out_n, st);
    return ix->end(st, rc);
}

int ucfp_tlsh_index_query(ucfp_tlsh_index* ix, uint32_t tenant, const uint8_t* digests, size_t nq, uint32_t k,
                          uint32_t max_distance, uint64_t* out_ids, uint32_t* out_dist, float* out_scores, uint32_t* out_n) {
    int rc = query_args(ix, digests, nq, k, out_ids, out_dist, out_scores, out_n);
    if (rc || nq == 0) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    if ((rc = ix->begin())) return rc;
    hipStream_t st = ix->own;
    const size_t nk = nq * k;
    const size_t o_dist = align256(nk * 8), o_sc = align256(o_dist + nk * 4), o_n = align256(o_sc + nk * 4);
    if ((rc = ix->q_in.ensure(nq * kRowBytes)) || (rc = ix->q_out.ensure(o_n + nq * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(ix->q_in.p, digests, nq * kRowBytes, hipMemcpyHostToDevice, st));
    uint8_t* ob = ix->q_out.as<uint8_t>();
    rc = query_impl(ix, tenant, ix->q_in.as<uint8_t>(), nq, k, max_distance, (uint64_t*)ob, (uint32_t*)(ob + o_dist),
                    (float*)(ob + o_sc), (uint32_t*)(ob + o_n), st);
    if (rc) return ix->end_sync(rc);
    if (nk) {
        HIP_TRY(hipMemcpyAsync(out_ids, ob, nk * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_dist, ob + o_dist, nk * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_scores, ob + o_sc, nk * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(out_n, ob + o_n, nq * 4, hipMemcpyDeviceToHost, st));
    return ix->end_sync(UCFP_OK);
}

}  // extern "C"
