// minhash_index.hip -- GPU index over MinHash-128 records: "the k stored records that agree with this one
// in the most slots", exact.
//
// Spec (ours; the quantity is the score numerator of ucfp_lsh_query_dev and the `agree` of ucfp_lsh_dedup_dev, lsh.hip):
// a row and a query are UCFP_MINHASH_BYTES = 1032 bytes, 8 header bytes (neither compared nor validated, as lsh.hip:44)
// and 128 u64 LE slots;
//   agree(q, r) = #{ i < 128 : slot_i(q) == slot_i(r) }      all 64 bits, the same index only
// hits: agree >= min_agree (0 .. 128), ordered (agree desc, id asc), first k; score = (float)agree / 128.0f, exact.
//
// Layout of a tenant after a (lazy) rebuild: rows in ascending id order, each row its 1024 slot bytes as they are (the
// header is dropped on the host, so a row starts on a 16-byte boundary); no repack into planes.
//
// Query, in passes whose key matrix stays below 1 GiB:
//   mh_keys   lanes = slots: a wave reads a row as one 16-byte load per lane (slots 2 lane, 2 lane + 1) and keeps the same
//             two slots of QT queries in registers.  Per (query, row): two 64-bit equality compares into scalar masks,
//             two scalar population counts, one scalar add, and one v_writelane that files the count under lane
//             (row mod 64) of the query's key register; after 64 rows that register is stored as 256 contiguous bytes.
//             key = 128 - agree, or 0xffffffff below min_agree: ascending keys with ties by row are the required order.
//             A block is four waves.  Up to 16 queries: the four waves split the block's rows (QT = 1, 4 or 16 by the
//             size of the pass).  Up to 32: two waves read the same rows against 16 queries each, two ways over the rows.
//             More: the four waves read the same rows against 16 queries each, so a row comes from memory once per 64
//             queries and the other reads hit the cache.
//   topk.hip  select_topk_u32 + the merge tree, the selector of the cosine search: exact by (key, id)
// and mh_scores turns the selected keys into agree and score.  One query is bound by the 1024 bytes per row; a large
// batch by instructions: 3 VALU + 3 SALU per (query, row) against 16 bytes per (query, row) at 64 queries.
// Not here: a compact filter plane (the low 16 bits of every slot bound agree from above and would prune exactly at a
// quarter of the bytes), device-resident appends, sharding over GPUs, a search micro-batcher, save / load.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <map>
#include <unordered_map>
#include <vector>

#include "postings.h"

namespace {

constexpr uint32_t kRecBytes = UCFP_MINHASH_BYTES;
constexpr uint32_t kHeaderBytes = 8;
constexpr uint32_t kSlots = 128;
constexpr uint32_t kRowBytes = kSlots * 8;        // a stored row: the slots alone
constexpr uint32_t kRowVec = kRowBytes / 16;      // uint4 per row = lanes per wave
constexpr uint32_t kTile = 16;                    // queries a wave keeps in registers (the largest QT)
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kGroupRows = 64;               // rows whose counts one key register collects, one per lane
constexpr uint32_t kGroups = 8;                   // groups of a block
constexpr uint32_t kBlockRows = kGroupRows * kGroups;
constexpr uint32_t kUnroll = 4;                   // rows in flight per wave
constexpr size_t kKeyBytes = (size_t)1 << 30;     // key matrix of one pass (UCFP_MINHASH_KEY_BYTES at creation overrides it)
constexpr size_t kMaxRows = (size_t)1 << 31;

// records: 1032 bytes each, only 4-byte alignment guaranteed (lsh.hip:42)
__device__ __forceinline__ uint64_t load_slot(const uint8_t* rec, uint32_t i) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(rec + kHeaderBytes + 8 * (size_t)i);
    return (uint64_t)p[0] | ((uint64_t)p[1] << 32);
}

// v_writelane_b32: clang has no builtin for it, so the LLVM intrinsic is bound by name (as hip's own headers bind theirs)
extern "C" __device__ int mh_writelane(int src, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

// keys[q][row] for the nq queries of a pass.  QT queries per wave; WQ of the block's four waves take different queries
// (the other 4 / WQ ways split the block's row groups).  Block b: query group b % nqg, rows [b / nqg * kBlockRows, ...).
template <int QT, int WQ>
__global__ __launch_bounds__(kThreads) void mh_keys(const uint4* __restrict__ rows, size_t n, const uint8_t* __restrict__ q,
                                                     uint32_t nq, uint32_t nqg, uint32_t min_agree,
                                                     uint32_t* __restrict__ keys) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t qg = blockIdx.x % nqg;
    const size_t row_base = (size_t)(blockIdx.x / nqg) * kBlockRows;
    const uint32_t q0 = (qg * WQ + wave % WQ) * QT;
    if (q0 >= nq) return;   // wave-uniform
    uint64_t qa[QT], qb[QT];
#pragma unroll
    for (int t = 0; t < QT; t++) {
        const uint32_t qi = q0 + t < nq ? q0 + t : nq - 1;   // a short tile repeats the last query; it is not stored
        const uint8_t* rec = q + (size_t)qi * kRecBytes;
        qa[t] = load_slot(rec, 2 * lane);
        qb[t] = load_slot(rec, 2 * lane + 1);
    }
    for (uint32_t g = wave / WQ; g < kGroups; g += kWaves / WQ) {
        const size_t r0 = row_base + (size_t)g * kGroupRows;
        if (r0 >= n) break;
        uint32_t acc[QT];
#pragma unroll
        for (int t = 0; t < QT; t++) acc[t] = 0;
#pragma unroll 1
        for (uint32_t j = 0; j < kGroupRows; j += kUnroll) {
            if (r0 + j >= n) break;
            uint4 v[kUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; u++) {
                const size_t r = r0 + j + u < n ? r0 + j + u : n - 1;   // past the end: a row that exists; its lane is not stored
                v[u] = rows[r * kRowVec + lane];
            }
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; u++) {
                const uint64_t ra = (uint64_t)v[u].x | ((uint64_t)v[u].y << 32), rb = (uint64_t)v[u].z | ((uint64_t)v[u].w << 32);
#pragma unroll
                for (int t = 0; t < QT; t++) {
                    const uint32_t cnt = (uint32_t)__popcll(__ballot(ra == qa[t])) + (uint32_t)__popcll(__ballot(rb == qb[t]));
                    acc[t] = (uint32_t)mh_writelane((int)cnt, (int)(j + u), (int)acc[t]);
                }
            }
        }
        const size_t row = r0 + lane;
        if (row < n) {
#pragma unroll
            for (int t = 0; t < QT; t++)
                if (q0 + t < nq) keys[(size_t)(q0 + t) * n + row] = acc[t] >= min_agree ? kSlots - acc[t] : kEmpty32;
        }
    }
}

// the selected keys -> agree (in place) and score
__global__ void mh_scores(uint32_t* __restrict__ agree, size_t total, float* __restrict__ scores) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint32_t key = agree[i];
    if (key == kEmpty32) {
        scores[i] = -1.0f;
    } else {
        agree[i] = kSlots - key;
        scores[i] = (float)(kSlots - key) / 128.0f;
    }
}

// empty answers for every query (unknown tenant / no rows)
__global__ void mh_empty(size_t nq, uint32_t k, uint64_t* __restrict__ out_ids, uint32_t* __restrict__ out_agree,
                         float* __restrict__ out_scores, uint32_t* __restrict__ out_n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq * k) {
        out_ids[i] = kEmpty64;
        out_agree[i] = kEmpty32;
        out_scores[i] = -1.0f;
    }
    if (i < nq) out_n[i] = 0;
}

using Row = std::array<uint8_t, kRowBytes>;

struct Tenant {
    std::map<uint64_t, Row> recs;   // id -> slots; ascending id = row order, so ties by row are ties by id
    bool dirty = true;
    size_t n = 0;                   // valid when !dirty
    DevArr rows, ids;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

struct ucfp_minhash_index : ucfp::IndexCore {
    std::unordered_map<uint32_t, Tenant> tenants;
    size_t key_bytes = kKeyBytes;
    DevArr q_in, q_ws, q_out;       // host-pointer queries, the pass workspace, host-pointer answers
};

namespace {

int rebuild(ucfp_minhash_index*, Tenant& T, hipStream_t st) {
    const size_t n = T.recs.size();
    if (n >= kMaxRows) return capi_fail(UCFP_E_INVALID, "too many rows in one tenant (%zu)", n);
    std::vector<uint8_t> h_rows(n * kRowBytes);
    std::vector<uint64_t> h_ids(n);
    size_t i = 0;
    for (auto& kv : T.recs) {
        h_ids[i] = kv.first;
        memcpy(h_rows.data() + i * kRowBytes, kv.second.data(), kRowBytes);
        i++;
    }
    int rc;
    if ((rc = T.ids.ensure(n * 8)) || (rc = T.rows.ensure(n * kRowBytes))) return rc;
    if (n) {
        HIP_TRY(hipMemcpyAsync(T.ids.p, h_ids.data(), n * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(T.rows.p, h_rows.data(), n * kRowBytes, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));   // the host vectors above go out of scope
    T.n = n;
    T.dirty = false;
    return UCFP_OK;
}

int do_upsert(ucfp_minhash_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* records, size_t n) {
    if (!n) return UCFP_OK;
    if (!ids || !records) return capi_fail(UCFP_E_INVALID, "ids/records is NULL");
    Tenant& T = ix->tenants[tenant];
    for (size_t i = 0; i < n; i++) {
        Row r;
        memcpy(r.data(), records + i * kRecBytes + kHeaderBytes, kRowBytes);
        T.recs.insert_or_assign(T.recs.end(), ids[i], r);   // the hint: ascending ids append in constant time
    }
    T.dirty = true;
    return UCFP_OK;
}

template <int QT, int WQ>
void launch_keys(const Tenant& T, const uint8_t* d_q, uint32_t cnt, uint32_t min_agree, uint32_t* keymat, hipStream_t st) {
    const uint32_t per = QT * WQ;   // queries of a block
    const uint32_t nqg = (cnt + per - 1) / per;
    const size_t blocks = (size_t)nqg * ((T.n + kBlockRows - 1) / kBlockRows);
    hipLaunchKernelGGL((mh_keys<QT, WQ>), dim3((unsigned)blocks), dim3(kThreads), 0, st, T.rows.as<uint4>(), T.n, d_q, cnt, nqg,
                       min_agree, keymat);
}

int query_impl(ucfp_minhash_index* ix, uint32_t tenant, const uint8_t* d_q, size_t nq, uint32_t k, uint32_t min_agree,
               uint64_t* d_ids, uint32_t* d_agree, float* d_scores, uint32_t* d_n, hipStream_t st) {
    int rc;
    if (k == 0) {
        HIP_TRY(hipMemsetAsync(d_n, 0, nq * 4, st));
        return UCFP_OK;
    }
    auto it = ix->tenants.find(tenant);
    if (it != ix->tenants.end() && it->second.dirty && (rc = rebuild(ix, it->second, st))) return rc;
    if (it == ix->tenants.end() || it->second.n == 0) {
        hipLaunchKernelGGL(mh_empty, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, st, nq, k, d_ids, d_agree, d_scores, d_n);
        HIP_TRY(hipGetLastError());
        return UCFP_OK;
    }
    Tenant& T = it->second;
    const size_t n = T.n;
    // queries per pass: the key matrix stays below key_bytes; queries ride on gridDim.y of the select kernel
    size_t chunk = std::max<size_t>(1, ix->key_bytes / (4 * n));
    chunk = std::min<size_t>(std::min<size_t>(chunk, 32768), nq);
    // mh_keys numbers its blocks (query group, row block) in one dimension
    if (((chunk + kTile - 1) / kTile) * ((n + kBlockRows - 1) / kBlockRows) > 0x7fffffffu)
        return capi_fail(UCFP_E_INVALID, "too many rows for one launch (%zu)", n);
    const ucfp::SelectPlan sp = ucfp::select_plan(n, (uint32_t)chunk);
    const size_t tmp_e = 2 * ucfp::topk_merge_tmp_entries(sp.slices, (uint32_t)chunk, k);   // both tree levels
    size_t off = 0;
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
    uint32_t* keymat = reinterpret_cast<uint32_t*>(w + o_keys);
    for (size_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t cnt = (uint32_t)std::min(chunk, nq - q0);
        const uint8_t* qp = d_q + q0 * kRecBytes;
        if (cnt == 1) launch_keys<1, 1>(T, qp, cnt, min_agree, keymat, st);
        else if (cnt <= 4) launch_keys<4, 1>(T, qp, cnt, min_agree, keymat, st);
        else if (cnt <= kTile) launch_keys<kTile, 1>(T, qp, cnt, min_agree, keymat, st);
        else if (cnt <= 2 * kTile) launch_keys<kTile, 2>(T, qp, cnt, min_agree, keymat, st);   // 26 queries fit a pass over 10 M rows
        else launch_keys<kTile, kWaves>(T, qp, cnt, min_agree, keymat, st);
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
                                         d_ids + q0 * k, d_agree + q0 * k, d_n + q0, st);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(mh_scores, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, st, d_agree, nq * k, d_scores);
    HIP_TRY(hipGetLastError());
    return UCFP_OK;
}

int query_args(ucfp_minhash_index* ix, const void* records, size_t nq, uint32_t k, uint32_t min_agree, const void* out_ids,
               const void* out_agree, const void* out_scores, const void* out_n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (k > UCFP_INDEX_MAX_K) return capi_fail(UCFP_E_INVALID, "k = %u exceeds UCFP_INDEX_MAX_K = %u", k, UCFP_INDEX_MAX_K);
    if (min_agree > kSlots) return capi_fail(UCFP_E_INVALID, "min_agree = %u exceeds the %u slots of a record", min_agree, kSlots);
    if (nq > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "too many queries");
    if (nq && (!records || !out_n)) return capi_fail(UCFP_E_INVALID, "records/out_n is NULL");
    if (nq && k && (!out_ids || !out_agree || !out_scores)) return capi_fail(UCFP_E_INVALID, "an output buffer is NULL");
    return UCFP_OK;
}

}  // namespace

extern "C" {

uint32_t ucfp_minhash_agree(const uint8_t* a, const uint8_t* b) {
    if (!a || !b) return 0;
    uint32_t agree = 0;
    for (uint32_t i = 0; i < kSlots; i++) agree += memcmp(a + kHeaderBytes + 8 * i, b + kHeaderBytes + 8 * i, 8) == 0 ? 1u : 0u;
    return agree;
}

int ucfp_minhash_index_create(ucfp_ctx* ctx, uint32_t flags, ucfp_minhash_index** out) {
    if (!ctx || !out) return capi_fail(UCFP_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (flags != 0) return capi_fail(UCFP_E_INVALID, "no MinHash index flags are defined (got %u)", flags);
    const int rc = ucfp::create_index(ctx, "MinHash index", out);
    // a smaller key matrix means more passes over the rows: for tuning, and for tests of the pass loop at small sizes
    if (const char* e = rc ? nullptr : getenv("UCFP_MINHASH_KEY_BYTES")) (*out)->key_bytes = std::max<size_t>(4096, strtoull(e, nullptr, 10));
    return rc;
}

void ucfp_minhash_index_destroy(ucfp_minhash_index* ix) {
    if (!ix) return;
    ix->quiesce();
    for (auto& kv : ix->tenants)
        for (DevArr* a : {&kv.second.rows, &kv.second.ids}) a->release();
    for (DevArr* a : {&ix->q_in, &ix->q_ws, &ix->q_out}) a->release();
    delete ix;
}

int ucfp_minhash_index_upsert(ucfp_minhash_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* records, size_t n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    return do_upsert(ix, tenant, ids, records, n);
}

int ucfp_minhash_index_upsert_dev(ucfp_minhash_index* ix, uint32_t tenant, const uint64_t* d_ids, const uint8_t* d_records,
                                  size_t n, void* stream) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (!n) return UCFP_OK;
    if (!d_ids || !d_records) return capi_fail(UCFP_E_INVALID, "ids/records is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    // the row table lives on the host (mutations are bookkeeping; the device rows are rebuilt at the next query)
    std::vector<uint64_t> ids(n);
    std::vector<uint8_t> rows(n * kRecBytes);
    HIP_TRY(hipMemcpyAsync(ids.data(), d_ids, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(rows.data(), d_records, n * kRecBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return do_upsert(ix, tenant, ids.data(), rows.data(), n);
}

int ucfp_minhash_index_delete(ucfp_minhash_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed) {
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

int ucfp_minhash_index_size(ucfp_minhash_index* ix, uint32_t tenant, size_t* rows) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    auto it = ix->tenants.find(tenant);
    if (rows) *rows = it == ix->tenants.end() ? 0 : it->second.recs.size();
    return UCFP_OK;
}

int ucfp_minhash_index_flush(ucfp_minhash_index* ix) { return ucfp::flush_dirty(ix, rebuild); }

int ucfp_minhash_index_query_dev(ucfp_minhash_index* ix, uint32_t tenant, const uint8_t* d_records, size_t nq, uint32_t k,
                                 uint32_t min_agree, uint64_t* d_out_ids, uint32_t* d_out_agree, float* d_out_scores,
                                 uint32_t* d_out_n, void* stream) {
    int rc = query_args(ix, d_records, nq, k, min_agree, d_out_ids, d_out_agree, d_out_scores, d_out_n);
    if (rc || nq == 0) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    if ((rc = ix->begin())) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = query_impl(ix, tenant, d_records, nq, k, min_agree, d_out_ids, d_out_agree, d_out_scores, d_out_n, st);
    return ix->end(st, rc);
}

int ucfp_minhash_index_query(ucfp_minhash_index* ix, uint32_t tenant, const uint8_t* records, size_t nq, uint32_t k,
                             uint32_t min_agree, uint64_t* out_ids, uint32_t* out_agree, float* out_scores, uint32_t* out_n) {
    int rc = query_args(ix, records, nq, k, min_agree, out_ids, out_agree, out_scores, out_n);
    if (rc || nq == 0) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    if ((rc = ix->begin())) return rc;
    hipStream_t st = ix->own;
    const size_t nk = nq * k;
    const size_t o_agree = align256(nk * 8), o_sc = align256(o_agree + nk * 4), o_n = align256(o_sc + nk * 4);
    if ((rc = ix->q_in.ensure(nq * kRecBytes)) || (rc = ix->q_out.ensure(o_n + nq * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(ix->q_in.p, records, nq * kRecBytes, hipMemcpyHostToDevice, st));
    uint8_t* ob = ix->q_out.as<uint8_t>();
    rc = query_impl(ix, tenant, ix->q_in.as<uint8_t>(), nq, k, min_agree, (uint64_t*)ob, (uint32_t*)(ob + o_agree),
                    (float*)(ob + o_sc), (uint32_t*)(ob + o_n), st);
    if (rc) return ix->end_sync(rc);
    if (nk) {
        HIP_TRY(hipMemcpyAsync(out_ids, ob, nk * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_agree, ob + o_agree, nk * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_scores, ob + o_sc, nk * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(out_n, ob + o_n, nq * 4, hipMemcpyDeviceToHost, st));
    return ix->end_sync(UCFP_OK);
}

}  // extern "C"
