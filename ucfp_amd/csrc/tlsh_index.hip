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
// The tenant table, its mutations, the head of the rebuild, the pass loop and the call protocol are scan_index.h's
// (UCFP_TLSH_KEY_BYTES at creation overrides the size of a pass's key matrix).

#include <hip/hip_runtime.h>

#include <array>

#include "scan_index.h"

namespace {

constexpr uint32_t kRowBytes = UCFP_TLSH_BYTES;
constexpr uint32_t kPlanes = 13;                 // dwords per stored row
constexpr uint32_t kQueryWords = 16;             // dwords per packed query

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

using Row = std::array<uint8_t, kRowBytes>;   // the digest: no allocation per row

}  // namespace

struct ucfp_tlsh_index : ucfp::ScanIndex<Row> {
    static constexpr uint8_t kPad = 0;
    size_t rec_bytes() const { return kRowBytes; }
    size_t row_len() const { return kRowBytes; }
    Row to_row(const uint8_t* rec) const {
        Row r;
        memcpy(r.data(), rec, kRowBytes);
        return r;
    }
    // n digests -> 13 planes of `stride` rows
    int upload(DevArr& rows, const uint8_t* h_rows, size_t n, size_t stride, hipStream_t st) {
        int rc;
        if ((rc = rows.ensure(stride * kPlanes * 4)) || (rc = b_packed.ensure(n * kRowBytes))) return rc;
        if (!n) return UCFP_OK;
        HIP_TRY(hipMemcpyAsync(b_packed.p, h_rows, n * kRowBytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(rows.p, 0, stride * kPlanes * 4, st));
        hipLaunchKernelGGL(tl_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, b_packed.as<uint8_t>(), n,
                           rows.as<uint32_t>(), stride, (size_t)1);
        HIP_TRY(hipGetLastError());
        return UCFP_OK;
    }
};

namespace {

int query_impl(ucfp_tlsh_index* ix, uint32_t tenant, const uint8_t* d_q, size_t nq, uint32_t k, uint32_t max_distance,
               const ucfp::ScanOut& o, hipStream_t st) {
    uint32_t* qw = nullptr;   // the packed queries, in the workspace
    uint32_t* dist = nullptr;
    const int rc = ucfp::scan_query(
        ix, tenant, nq, k, nq * kQueryWords * 4, o, st, &dist,
        [&](uint8_t* q_area) {
            qw = reinterpret_cast<uint32_t*>(q_area);
            hipLaunchKernelGGL(tl_pack, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, d_q, nq, qw, (size_t)1, (size_t)kQueryWords);
        },
        [&](const ucfp_tlsh_index::Tenant& T, size_t q0, uint32_t cnt, uint32_t* keymat) {
            hipLaunchKernelGGL(tl_keys, dim3((unsigned)((T.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, T.rows.as<uint32_t>(),
                               T.n, T.stride, qw + q0 * kQueryWords, cnt, max_distance, keymat);
        });
    if (rc || !dist) return rc;
    hipLaunchKernelGGL(tl_scores, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, st, dist, nq * k, o.scores);
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
    if (!rc) ucfp::scan_key_bytes_env(*out, "UCFP_TLSH_KEY_BYTES");
    return rc;
}

void ucfp_tlsh_index_destroy(ucfp_tlsh_index* ix) { ucfp::scan_destroy(ix); }

int ucfp_tlsh_index_upsert(ucfp_tlsh_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* digests, size_t n) {
    return ucfp::scan_upsert(ix, tenant, ids, digests, n, "digests");
}

int ucfp_tlsh_index_upsert_dev(ucfp_tlsh_index* ix, uint32_t tenant, const uint64_t* d_ids, const uint8_t* d_digests, size_t n,
                               void* stream) {
    return ucfp::scan_upsert_dev(ix, tenant, d_ids, d_digests, n, "digests", stream);
}

int ucfp_tlsh_index_delete(ucfp_tlsh_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed) {
    return ucfp::scan_delete(ix, tenant, ids, n, n_removed);
}

int ucfp_tlsh_index_size(ucfp_tlsh_index* ix, uint32_t tenant, size_t* rows) { return ucfp::scan_size(ix, tenant, rows); }

int ucfp_tlsh_index_flush(ucfp_tlsh_index* ix) { return ucfp::scan_flush(ix); }

int ucfp_tlsh_index_query_dev(ucfp_tlsh_index* ix, uint32_t tenant, const uint8_t* d_digests, size_t nq, uint32_t k,
                              uint32_t max_distance, uint64_t* d_out_ids, uint32_t* d_out_dist, float* d_out_scores,
                              uint32_t* d_out_n, void* stream) {
    const int rc = query_args(ix, d_digests, nq, k, d_out_ids, d_out_dist, d_out_scores, d_out_n);
    if (rc || nq == 0) return rc;
    return ucfp::scan_query_dev(ix, stream, [&](hipStream_t st) {
        return query_impl(ix, tenant, d_digests, nq, k, max_distance, {d_out_ids, d_out_dist, d_out_scores, d_out_n}, st);
    });
}

int ucfp_tlsh_index_query(ucfp_tlsh_index* ix, uint32_t tenant, const uint8_t* digests, size_t nq, uint32_t k,
                          uint32_t max_distance, uint64_t* out_ids, uint32_t* out_dist, float* out_scores, uint32_t* out_n) {
    const int rc = query_args(ix, digests, nq, k, out_ids, out_dist, out_scores, out_n);
    if (rc || nq == 0) return rc;
    return ucfp::scan_query_host(ix, digests, nq, k, out_ids, out_dist, out_scores, out_n,
                                 [&](const uint8_t* d_q, const ucfp::ScanOut& o, hipStream_t st) {
                                     return query_impl(ix, tenant, d_q, nq, k, max_distance, o, st);
                                 });
}

}  // extern "C"
