// image_match.hip -- GPU index over whole imgfprint records: "the k stored images most similar to this
// one", scoring the global hash AND the 16 block hashes of every algorithm, exact.
//
// Spec (ours; the arithmetic of imgfprint's own compare is not in the tree): a 168-byte record gives 17
// u64 LE codes (global at byte 32, blocks at 40 .. 160), a 536-byte bundle 3 x 17 in the order ahash, phash, dhash (records
// at bytes 32, 200, 368).  Per algorithm, query q against row r:
//   g = popc(Gq ^ Gr), d_b = popc(Bq[b] ^ Br[b]), S = sum over b of (d_b <= T ? 64 - d_b : 0)
//   sg = (float)(64 - g) * 2^-6, sb = (float)S * 2^-10, s_a = (wg * sg) + (wb * sb)          one f32 operation at a time
// score = s_a (168 bytes) or ((wa * s_ahash) + (wp * s_phash)) + (wd * s_dhash) (bundle); the build passes
// -ffp-contract=off, so host and device round alike.  hits: score >= min_score, ordered (score desc, id asc), first k.
//
// Layout of a tenant after a (lazy) rebuild: rows in ascending id order, stored as 17 or 51 u64 planes of `stride` rows
// each (structure of arrays, stride a multiple of 64, so lane = row loads coalesce).
//
// Query: im_pack brings the queries into code order (17 or 51 u64 per query); then, in passes whose key matrix stays
// below 1 GiB,
//   im_keys   lane = row, its codes in registers across the queries of the pass (their words are wave-uniform: scalar
//             loads), one u32 key per (query, row): 0x7f800000 - bits(score), which orders like (score desc) because a
//             score is finite and >= +0; 0xffffffff below min_score
//   topk.hip  select_topk_u32 + the merge tree, the selector of the cosine search: exact by (key, id)
// and im_scores turns the selected keys back into the scores' bit patterns.  ALU-bound once a pass carries more than a
// few queries: about 400 vector instructions per (query, row) on a bundle against 408 bytes per row.
// Not here: sharding over GPUs, a search micro-batcher, save / load (ucfp_hip.h says so).
// The tenant table, its mutations, the head of the rebuild, the pass loop and the call protocol are scan_index.h's
// (UCFP_IMAGE_MATCH_KEY_BYTES at creation overrides the size of a pass's key matrix).

#include <hip/hip_runtime.h>

#include <cmath>

#include "scan_index.h"

namespace {

constexpr uint32_t kCodes = 17;                  // u64 codes of one algorithm: global, 16 blocks
constexpr uint32_t kRecBytes = 168;              // one algorithm's record: exact[32] | global | 16 blocks
constexpr uint32_t kBundleBytes = 536;           // 32-byte header, then the ahash, phash and dhash records
constexpr uint32_t kKeyZero = 0x7f800000u;       // the key of score +0; a larger score has a smaller key

// What one pair costs, on the host and on the device alike.  c points to the 17 or 51 codes of each side.
struct Weights {
    float wa, wp, wd, wg, wb;
    uint32_t T;
};

template <int A, class R, class Q>
__host__ __device__ __forceinline__ float pair_score(const R& r, const Q& q, const Weights& w) {
    float s[A];
#pragma unroll
    for (int a = 0; a < A; a++) {
        const uint32_t g = (uint32_t)__builtin_popcountll(r[a * kCodes] ^ q[a * kCodes]);
        uint32_t S = 0;
#pragma unroll
        for (uint32_t b = 1; b < kCodes; b++) {
            const uint32_t d = (uint32_t)__builtin_popcountll(r[a * kCodes + b] ^ q[a * kCodes + b]);
            S += d <= w.T ? 64u - d : 0u;
        }
        const float sg = (float)(64u - g) * 0.015625f;
        const float sb = (float)S * 0.0009765625f;
        const float tg = w.wg * sg;
        const float tb = w.wb * sb;
        s[a] = tg + tb;
    }
    if constexpr (A == 1) {
        return s[0];
    } else {
        const float ta = w.wa * s[0];
        const float tp = w.wp * s[1];
        const float td = w.wd * s[2];
        const float tap = ta + tp;
        return tap + td;
    }
}

// n items of item_bytes each -> u64 words; word w of item i is read LE at byte base + (w / 17) * algo_stride + (w % 17) * 8
// of the item and goes to out[w * stride_w + i * stride_i].  Records: base 32 (64 in a bundle), algo_stride 168; the
// host's row table, already in code order: base 0, algo_stride 136.
__global__ void im_pack(const uint8_t* __restrict__ in, size_t n, uint32_t words, uint32_t item_bytes, uint32_t base,
                        uint32_t algo_stride, uint64_t* __restrict__ out, size_t stride_w, size_t stride_i) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * words) return;
    const size_t i = t / words;
    const uint32_t w = (uint32_t)(t % words);
    const uint8_t* p = in + i * item_bytes + base + (w / kCodes) * algo_stride + (w % kCodes) * 8u;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) v |= (uint64_t)p[j] << (8 * j);
    out[(size_t)w * stride_w + i * stride_i] = v;
}

// keys[q][row] for the nq queries of a pass; A = algorithms per record (1 or 3)
template <int A>
__global__ __launch_bounds__(kThreads) void im_keys(const uint64_t* __restrict__ rows, size_t n, size_t stride,
                                                     const uint64_t* __restrict__ qw, uint32_t nq, Weights w, float min_score,
                                                     uint32_t* __restrict__ keys) {
    const size_t row = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (row >= n) return;
    uint64_t r[A * kCodes];
#pragma unroll
    for (uint32_t c = 0; c < A * kCodes; c++) r[c] = rows[(size_t)c * stride + row];
    for (uint32_t q = 0; q < nq; q++) {
        const uint64_t* __restrict__ qq = qw + (size_t)q * (A * kCodes);   // wave-uniform
        const float s = pair_score<A>(r, qq, w);
        keys[(size_t)q * n + row] = s >= min_score ? kKeyZero - __float_as_uint(s) : kEmpty32;
    }
}

__global__ void im_scores(const uint32_t* __restrict__ key, size_t total, float* __restrict__ scores) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint32_t k = key[i];
    scores[i] = k == kEmpty32 ? -1.0f : __uint_as_float(kKeyZero - k);
}

inline bool unit(float x) { return std::isfinite(x) && x >= 0.0f && x <= 1.0f; }

// M4; `bundle`: the three algorithm weights count.  -0.0f is taken as +0.0f, so no product is ever negative zero.
int check_config(const ucfp_image_match_config* in, bool bundle, Weights* w, float* min_score) {
    ucfp_image_match_config c;
    if (in)
        c = *in;
    else
        ucfp_image_match_config_default(&c);
    if (!unit(c.ahash_weight) || !unit(c.phash_weight) || !unit(c.dhash_weight) || !unit(c.global_weight) ||
        !unit(c.block_weight))
        return capi_fail(UCFP_E_INVALID, "image match: every weight must be finite and within [0, 1]");
    if (bundle && c.ahash_weight == 0.0f && c.phash_weight == 0.0f && c.dhash_weight == 0.0f)
        return capi_fail(UCFP_E_INVALID, "image match: ahash_weight, phash_weight and dhash_weight are all zero");
    if (c.global_weight == 0.0f && c.block_weight == 0.0f)
        return capi_fail(UCFP_E_INVALID, "image match: global_weight and block_weight are both zero");
    if (c.block_distance_threshold > 64)
        return capi_fail(UCFP_E_INVALID, "image match: block_distance_threshold = %u exceeds 64", c.block_distance_threshold);
    if (!std::isfinite(c.min_score) || c.min_score < 0.0f)
        return capi_fail(UCFP_E_INVALID, "image match: min_score must be finite and not negative");
    *w = Weights{c.ahash_weight + 0.0f, c.phash_weight + 0.0f, c.dhash_weight + 0.0f, c.global_weight + 0.0f,
                 c.block_weight + 0.0f,  c.block_distance_threshold};
    *min_score = c.min_score + 0.0f;
    return UCFP_OK;
}

inline bool algo_ok(uint32_t algo) {
    return algo == UCFP_IMG_AHASH || algo == UCFP_IMG_PHASH || algo == UCFP_IMG_DHASH || algo == UCFP_IMG_MULTI;
}

// the codes of one host record, in code order
inline void record_codes(const uint8_t* rec, bool bundle, uint64_t* out) {
    const uint32_t algos = bundle ? 3 : 1, base = bundle ? 64 : 32;
    for (uint32_t a = 0; a < algos; a++)
        for (uint32_t c = 0; c < kCodes; c++) {
            const uint8_t* p = rec + base + a * kRecBytes + c * 8;
            uint64_t v = 0;
            for (uint32_t j = 0; j < 8; j++) v |= (uint64_t)p[j] << (8 * j);
            out[a * kCodes + c] = v;
        }
}

}  // namespace

struct ucfp_image_match_index : ucfp::ScanIndex<std::vector<uint64_t>> {
    static constexpr uint64_t kPad = 0;
    bool bundle = false;            // 536-byte bundles (51 codes) or 168-byte records (17)

    uint32_t words() const { return bundle ? 3 * kCodes : kCodes; }
    size_t rec_bytes() const { return bundle ? kBundleBytes : kRecBytes; }
    size_t row_len() const { return words(); }
    Row to_row(const uint8_t* rec) const {
        Row c(words());
        record_codes(rec, bundle, c.data());
        return c;
    }
    // n rows of W codes -> W planes of `stride` rows
    int upload(DevArr& rows, const uint64_t* h_rows, size_t n, size_t stride, hipStream_t st) {
        const uint32_t W = words();
        int rc;
        if ((rc = rows.ensure(stride * W * 8)) || (rc = b_packed.ensure(n * W * 8))) return rc;
        if (!n) return UCFP_OK;
        HIP_TRY(hipMemcpyAsync(b_packed.p, h_rows, n * W * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(rows.p, 0, stride * W * 8, st));
        hipLaunchKernelGGL(im_pack, dim3((unsigned)((n * W + 255) / 256)), dim3(256), 0, st, b_packed.as<uint8_t>(), n, W, W * 8u, 0u,
                           kCodes * 8u, rows.as<uint64_t>(), stride, (size_t)1);
        HIP_TRY(hipGetLastError());
        return UCFP_OK;
    }
};

namespace {

int query_impl(ucfp_image_match_index* ix, uint32_t tenant, const uint8_t* d_q, size_t nq, uint32_t k, const Weights& wt,
               float min_score, const ucfp::ScanOut& o, hipStream_t st) {
    const uint32_t W = ix->words();
    uint64_t* qw = nullptr;   // the queries in code order, in the workspace
    uint32_t* okeys = nullptr;
    const int rc = ucfp::scan_query(
        ix, tenant, nq, k, nq * W * 8, o, st, &okeys,
        [&](uint8_t* q_area) {
            qw = reinterpret_cast<uint64_t*>(q_area);
            hipLaunchKernelGGL(im_pack, dim3((unsigned)((nq * W + 255) / 256)), dim3(256), 0, st, d_q, nq, W, (uint32_t)ix->rec_bytes(),
                               ix->bundle ? 64u : 32u, kRecBytes, qw, (size_t)1, (size_t)W);
        },
        [&](const ucfp_image_match_index::Tenant& T, size_t q0, uint32_t cnt, uint32_t* keymat) {
            const dim3 grid((unsigned)((T.n + kThreads - 1) / kThreads));
            if (ix->bundle)
                hipLaunchKernelGGL(im_keys<3>, grid, dim3(kThreads), 0, st, T.rows.as<uint64_t>(), T.n, T.stride, qw + q0 * W, cnt, wt,
                                   min_score, keymat);
            else
                hipLaunchKernelGGL(im_keys<1>, grid, dim3(kThreads), 0, st, T.rows.as<uint64_t>(), T.n, T.stride, qw + q0 * W, cnt, wt,
                                   min_score, keymat);
        });
    if (rc || !okeys) return rc;
    hipLaunchKernelGGL(im_scores, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, st, okeys, nq * k, o.scores);
    HIP_TRY(hipGetLastError());
    return UCFP_OK;
}

int query_args(ucfp_image_match_index* ix, const void* records, size_t nq, uint32_t k, const void* out_ids,
               const void* out_scores, const void* out_n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (k > UCFP_INDEX_MAX_K) return capi_fail(UCFP_E_INVALID, "k = %u exceeds UCFP_INDEX_MAX_K = %u", k, UCFP_INDEX_MAX_K);
    if (nq > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "too many queries");
    if (nq && (!records || !out_n)) return capi_fail(UCFP_E_INVALID, "records/out_n is NULL");
    if (nq && k && (!out_ids || !out_scores)) return capi_fail(UCFP_E_INVALID, "an output buffer is NULL");
    return UCFP_OK;
}

}  // namespace

extern "C" {

void ucfp_image_match_config_default(ucfp_image_match_config* cfg) {
    if (!cfg) return;
    cfg->ahash_weight = 0.1f;
    cfg->phash_weight = 0.6f;
    cfg->dhash_weight = 0.3f;
    cfg->global_weight = 0.4f;
    cfg->block_weight = 0.6f;
    cfg->block_distance_threshold = 32;
    cfg->min_score = 0.0f;
}

int ucfp_image_match_score(const uint8_t* a, const uint8_t* b, uint32_t algo, const ucfp_image_match_config* cfg, float* out) {
    if (!a || !b || !out) return capi_fail(UCFP_E_INVALID, "a/b/out is NULL");
    if (!algo_ok(algo)) return capi_fail(UCFP_E_INVALID, "image match: algo = %u is not one of UCFP_IMG_*", algo);
    const bool bundle = algo == UCFP_IMG_MULTI;
    Weights w;
    float min_score;
    const int rc = check_config(cfg, bundle, &w, &min_score);
    if (rc) return rc;
    uint64_t ca[3 * kCodes], cb[3 * kCodes];
    record_codes(a, bundle, ca);
    record_codes(b, bundle, cb);
    *out = bundle ? pair_score<3>(ca, cb, w) : pair_score<1>(ca, cb, w);
    return UCFP_OK;
}

int ucfp_image_match_index_create(ucfp_ctx* ctx, uint32_t algo, uint32_t flags, ucfp_image_match_index** out) {
    if (!ctx || !out) return capi_fail(UCFP_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (!algo_ok(algo)) return capi_fail(UCFP_E_INVALID, "image match: algo = %u is not one of UCFP_IMG_*", algo);
    if (flags != 0) return capi_fail(UCFP_E_INVALID, "no image match index flags are defined (got %u)", flags);
    const int rc = ucfp::create_index(ctx, "image match index", out);
    if (rc) return rc;
    (*out)->bundle = algo == UCFP_IMG_MULTI;
    ucfp::scan_key_bytes_env(*out, "UCFP_IMAGE_MATCH_KEY_BYTES");
    return UCFP_OK;
}

void ucfp_image_match_index_destroy(ucfp_image_match_index* ix) { ucfp::scan_destroy(ix); }

int ucfp_image_match_index_upsert(ucfp_image_match_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* records,
                                  size_t n) {
    return ucfp::scan_upsert(ix, tenant, ids, records, n, "records");
}

int ucfp_image_match_index_upsert_dev(ucfp_image_match_index* ix, uint32_t tenant, const uint64_t* d_ids,
                                      const uint8_t* d_records, size_t n, void* stream) {
    return ucfp::scan_upsert_dev(ix, tenant, d_ids, d_records, n, "records", stream);
}

int ucfp_image_match_index_delete(ucfp_image_match_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed) {
    return ucfp::scan_delete(ix, tenant, ids, n, n_removed);
}

int ucfp_image_match_index_size(ucfp_image_match_index* ix, uint32_t tenant, size_t* rows) {
    return ucfp::scan_size(ix, tenant, rows);
}

int ucfp_image_match_index_flush(ucfp_image_match_index* ix) { return ucfp::scan_flush(ix); }

int ucfp_image_match_index_query_dev(ucfp_image_match_index* ix, uint32_t tenant, const uint8_t* d_records, size_t nq, uint32_t k,
                                     const ucfp_image_match_config* cfg, uint64_t* d_out_ids, float* d_out_scores,
                                     uint32_t* d_out_n, void* stream) {
    int rc = query_args(ix, d_records, nq, k, d_out_ids, d_out_scores, d_out_n);
    if (rc) return rc;
    Weights wt;
    float min_score;
    if ((rc = check_config(cfg, ix->bundle, &wt, &min_score)) || nq == 0) return rc;
    return ucfp::scan_query_dev(ix, stream, [&](hipStream_t st) {
        return query_impl(ix, tenant, d_records, nq, k, wt, min_score, {d_out_ids, nullptr, d_out_scores, d_out_n}, st);
    });
}

int ucfp_image_match_index_query(ucfp_image_match_index* ix, uint32_t tenant, const uint8_t* records, size_t nq, uint32_t k,
                                 const ucfp_image_match_config* cfg, uint64_t* out_ids, float* out_scores, uint32_t* out_n) {
    int rc = query_args(ix, records, nq, k, out_ids, out_scores, out_n);
    if (rc) return rc;
    Weights wt;
    float min_score;
    if ((rc = check_config(cfg, ix->bundle, &wt, &min_score)) || nq == 0) return rc;
    return ucfp::scan_query_host(ix, records, nq, k, out_ids, nullptr, out_scores, out_n,
                                 [&](const uint8_t* d_q, const ucfp::ScanOut& o, hipStream_t st) {
                                     return query_impl(ix, tenant, d_q, nq, k, wt, min_score, o, st);
                                 });
}

}  // extern "C"
