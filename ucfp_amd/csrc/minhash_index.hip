// minhash_index.hip -- GPU index over MinHash records of H slots: "the k stored records that agree
// with this one in the most slots", exact.  H is fixed when the index is created (128 by ucfp_minhash_index_create).
//
// Spec (ours; the quantity is the score numerator of ucfp_lsh_query_dev and the `agree` of ucfp_lsh_dedup_dev, lsh.hip):
// a row and a query are 8 + 8 H bytes (UCFP_MINHASH_BYTES = 1032 at H = 128), 8 header bytes (neither compared nor
// validated, as lsh.hip:44) and H u64 LE slots;
//   agree(q, r) = #{ i < H : slot_i(q) == slot_i(r) }      all 64 bits, the same index only
// hits: agree >= min_agree (0 .. H), ordered (agree desc, id asc), first k; score = (float)agree / (float)H, one division.
//
// Layout of a tenant after a (lazy) rebuild: rows in ascending id order, each row its 8 H slot bytes as they are (the
// header is dropped on the host, so a row starts on a 16-byte boundary), padded with ~0 slots to C = ceil(H / 128) chunks
// of 128 slots; no repack into planes.  A query's registers hold 0 at the pad positions, so a pad never agrees.
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
//             H slots: the kernel is templated on C as well; a lane loads one 16-byte vector per chunk and the C pairs of
//             ballots of a (query, row) are summed before the one v_writelane.  The query tile shrinks so that QT C stays
//             at or under the 16 query-slot pairs a lane holds at C = 1, and fewer rows are in flight (kUnroll rows of C
//             vectors).  Dispatched (C, QT, WQ), with T = 16, 8, 4, 4, 2, 2, 2, 2 for C = 1 .. 8:
//               1 query (C, 1, 1); up to min(4, T) (C, min(4, T), 1); up to T (C, T, 1); up to 2 T (C, T, 2); more (C, T, 4).
//             C = 1 is the dispatch H = 128 has always had; its key is H - agree.
//   topk.hip  select_topk_u32 + the merge tree, the selector of the cosine search: exact by (key, id)
// and mh_scores turns the selected keys into agree and score.  One query is bound by the 1024 bytes per row; a large
// batch by instructions: 3 VALU + 3 SALU per (query, row) against 16 bytes per (query, row) at 64 queries.
// Not here: packing two H = 64 rows into one wave load (an H = 64 row is half pad); a compact filter plane (the low 16 bits of every slot bound agree from above and would prune exactly at a
// quarter of the bytes), device-resident appends, sharding over GPUs, a search micro-batcher, save / load.

// The tenant table, its mutations, the head of the rebuild, the pass loop and the call protocol are scan_index.h's
// (UCFP_MINHASH_KEY_BYTES at creation overrides the size of a pass's key matrix).

#include <hip/hip_runtime.h>

#include "scan_index.h"

namespace {

constexpr uint32_t kHeaderBytes = 8;
constexpr uint32_t kChunkSlots = 128;             // slots a wave compares per load: two per lane
constexpr uint32_t kChunkBytes = kChunkSlots * 8;
constexpr uint32_t kChunkVec = kChunkBytes / 16;  // uint4 per chunk = lanes per wave
constexpr uint32_t kTile = 16;                    // query-slot pairs a lane keeps in registers: QT C at the most
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kGroupRows = 64;               // rows whose counts one key register collects, one per lane
constexpr uint32_t kGroups = 8;                   // groups of a block
constexpr uint32_t kBlockRows = kGroupRows * kGroups;
constexpr uint32_t kUnroll = 4;                   // 16-byte vectors in flight per lane: 4 / C rows, one at the least

// records: 8 + 8 h bytes each, only 4-byte alignment guaranteed (lsh.hip:42); a slot at or past h reads as 0
__device__ __forceinline__ uint64_t load_slot(const uint8_t* rec, uint32_t i, uint32_t h) {
    if (i >= h) return 0;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(rec + kHeaderBytes + 8 * (size_t)i);
    return (uint64_t)p[0] | ((uint64_t)p[1] << 32);
}

// v_writelane_b32: clang has no builtin for it, so the LLVM intrinsic is bound by name (as hip's own headers bind theirs)
extern "C" __device__ int mh_writelane(int src, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

// keys[q][row] for the nq queries of a pass.  Rows of C chunks (h slots, the rest pad); QT queries per wave; WQ of the
// block's four waves take different queries (the other 4 / WQ ways split the block's row groups).  Block b: query group
// b % nqg, rows [b / nqg * kBlockRows, ...).
template <int C, int QT, int WQ>
__global__ __launch_bounds__(kThreads) void mh_keys(const uint4* __restrict__ rows, size_t n, const uint8_t* __restrict__ q,
                                                     uint32_t nq, uint32_t nqg, uint32_t min_agree, uint32_t h,
                                                     uint32_t* __restrict__ keys) {
    constexpr uint32_t U = kUnroll / C ? kUnroll / C : 1;   // rows in flight
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t qg = blockIdx.x % nqg;
    const size_t row_base = (size_t)(blockIdx.x / nqg) * kBlockRows;
    const uint32_t q0 = (qg * WQ + wave % WQ) * QT;
    if (q0 >= nq) return;   // wave-uniform
    const size_t rec_bytes = kHeaderBytes + 8 * (size_t)h;
    uint64_t qa[QT][C], qb[QT][C];
#pragma unroll
    for (int t = 0; t < QT; t++) {
        const uint32_t qi = q0 + t < nq ? q0 + t : nq - 1;   // a short tile repeats the last query; it is not stored
        const uint8_t* rec = q + (size_t)qi * rec_bytes;
#pragma unroll
        for (int c = 0; c < C; c++) {
            qa[t][c] = load_slot(rec, kChunkSlots * c + 2 * lane, h);
            qb[t][c] = load_slot(rec, kChunkSlots * c + 2 * lane + 1, h);
        }
    }
    for (uint32_t g = wave / WQ; g < kGroups; g += kWaves / WQ) {
        const size_t r0 = row_base + (size_t)g * kGroupRows;
        if (r0 >= n) break;
        uint32_t acc[QT];
#pragma unroll
        for (int t = 0; t < QT; t++) acc[t] = 0;
#pragma unroll 1
        for (uint32_t j = 0; j < kGroupRows; j += U) {
            if (r0 + j >= n) break;
            uint4 v[U][C];
#pragma unroll
            for (uint32_t u = 0; u < U; u++) {
                const size_t r = r0 + j + u < n ? r0 + j + u : n - 1;   // past the end: a row that exists; its lane is not stored
#pragma unroll
                for (int c = 0; c < C; c++) v[u][c] = rows[(r * C + c) * kChunkVec + lane];
            }
#pragma unroll
            for (uint32_t u = 0; u < U; u++) {
#pragma unroll
                for (int t = 0; t < QT; t++) {
                    uint32_t cnt = 0;
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        const uint64_t ra = (uint64_t)v[u][c].x | ((uint64_t)v[u][c].y << 32);
                        const uint64_t rb = (uint64_t)v[u][c].z | ((uint64_t)v[u][c].w << 32);
                        cnt += (uint32_t)__popcll(__ballot(ra == qa[t][c])) + (uint32_t)__popcll(__ballot(rb == qb[t][c]));
                    }
                    acc[t] = (uint32_t)mh_writelane((int)cnt, (int)(j + u), (int)acc[t]);
                }
            }
        }
        const size_t row = r0 + lane;
        if (row < n) {
#pragma unroll
            for (int t = 0; t < QT; t++)
                if (q0 + t < nq) keys[(size_t)(q0 + t) * n + row] = acc[t] >= min_agree ? h - acc[t] : kEmpty32;
        }
    }
}

// the selected keys -> agree (in place) and score
__global__ void mh_scores(uint32_t* __restrict__ agree, size_t total, uint32_t h, float* __restrict__ scores) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint32_t key = agree[i];
    if (key == kEmpty32) {
        scores[i] = -1.0f;
    } else {
        agree[i] = h - key;
        scores[i] = (float)(h - key) / (float)h;
    }
}

}  // namespace

struct ucfp_minhash_index : ucfp::ScanIndex<std::vector<uint8_t>> {   // a row: the 8 h slot bytes of a record
    static constexpr uint8_t kPad = 0xff;   // pad slots are ~0
    uint32_t h = 128;               // slots of a record
    uint32_t chunks = 1;            // C = ceil(h / 128): a device row is chunks * 1024 bytes

    size_t rec_bytes() const { return kHeaderBytes + 8 * (size_t)h; }
    size_t row_len() const { return (size_t)chunks * kChunkBytes; }
    Row to_row(const uint8_t* rec) const { return Row(rec + kHeaderBytes, rec + kHeaderBytes + 8 * (size_t)h); }
    // the padded rows as they are
    int upload(DevArr& rows, const uint8_t* h_rows, size_t n, size_t, hipStream_t st) {
        if (int rc = rows.ensure(n * row_len())) return rc;
        if (n) HIP_TRY(hipMemcpyAsync(rows.p, h_rows, n * row_len(), hipMemcpyHostToDevice, st));
        return UCFP_OK;
    }
};

namespace {

using Tenant = ucfp_minhash_index::Tenant;

template <int C, int QT, int WQ>
void launch_keys(const Tenant& T, const uint8_t* d_q, uint32_t cnt, uint32_t min_agree, uint32_t h, uint32_t* keymat,
                 hipStream_t st) {
    const uint32_t per = QT * WQ;   // queries of a block
    const uint32_t nqg = (cnt + per - 1) / per;
    const size_t blocks = (size_t)nqg * ((T.n + kBlockRows - 1) / kBlockRows);
    hipLaunchKernelGGL((mh_keys<C, QT, WQ>), dim3((unsigned)blocks), dim3(kThreads), 0, st, T.rows.as<uint4>(), T.n, d_q, cnt, nqg,
                       min_agree, h, keymat);
}

// the query tile of C chunks: QT C <= kTile (C = 3 and 5 .. 7 round down to a power of two)
constexpr uint32_t tile_of(uint32_t c) { return c == 1 ? kTile : c == 2 ? kTile / 2 : c <= 4 ? kTile / 4 : kTile / 8; }

// the arm of a pass of cnt queries (file header)
template <int C>
void dispatch_keys(const Tenant& T, const uint8_t* qp, uint32_t cnt, uint32_t min_agree, uint32_t h, uint32_t* keymat,
                   hipStream_t st) {
    constexpr int QT = (int)tile_of(C), QS = QT < 4 ? QT : 4;
    if (cnt == 1) launch_keys<C, 1, 1>(T, qp, cnt, min_agree, h, keymat, st);
    else if (cnt <= (uint32_t)QS) launch_keys<C, QS, 1>(T, qp, cnt, min_agree, h, keymat, st);
    else if (cnt <= (uint32_t)QT) launch_keys<C, QT, 1>(T, qp, cnt, min_agree, h, keymat, st);
    else if (cnt <= 2u * QT) launch_keys<C, QT, 2>(T, qp, cnt, min_agree, h, keymat, st);   // 26 queries fit a pass over 10 M rows
    else launch_keys<C, QT, kWaves>(T, qp, cnt, min_agree, h, keymat, st);
}

int query_impl(ucfp_minhash_index* ix, uint32_t tenant, const uint8_t* d_q, size_t nq, uint32_t k, uint32_t min_agree,
               const ucfp::ScanOut& o, hipStream_t st) {
    const uint32_t h = ix->h, tile = tile_of(ix->chunks);
    uint32_t* agree = nullptr;
    const int rc = ucfp::scan_query(
        ix, tenant, nq, k, 0, o, st, &agree, [](uint8_t*) {},   // the kernel reads the records as they are
        [&](const Tenant& T, size_t q0, uint32_t cnt, uint32_t* keymat) {
            const uint8_t* qp = d_q + q0 * ix->rec_bytes();
            switch (ix->chunks) {
                case 1: dispatch_keys<1>(T, qp, cnt, min_agree, h, keymat, st); break;
                case 2: dispatch_keys<2>(T, qp, cnt, min_agree, h, keymat, st); break;
                case 3: dispatch_keys<3>(T, qp, cnt, min_agree, h, keymat, st); break;
                case 4: dispatch_keys<4>(T, qp, cnt, min_agree, h, keymat, st); break;
                case 5: dispatch_keys<5>(T, qp, cnt, min_agree, h, keymat, st); break;
                case 6: dispatch_keys<6>(T, qp, cnt, min_agree, h, keymat, st); break;
                case 7: dispatch_keys<7>(T, qp, cnt, min_agree, h, keymat, st); break;
                default: dispatch_keys<8>(T, qp, cnt, min_agree, h, keymat, st); break;
            }
        },
        [&](size_t n, size_t chunk) {   // mh_keys numbers its blocks (query group, row block) in one dimension
            if (((chunk + tile - 1) / tile) * ((n + kBlockRows - 1) / kBlockRows) > 0x7fffffffu)
                return capi_fail(UCFP_E_INVALID, "too many rows for one launch (%zu)", n);
            return (int)UCFP_OK;
        });
    if (rc || !agree) return rc;
    hipLaunchKernelGGL(mh_scores, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, st, agree, nq * k, h, o.scores);
    HIP_TRY(hipGetLastError());
    return UCFP_OK;
}

int query_args(ucfp_minhash_index* ix, const void* records, size_t nq, uint32_t k, uint32_t min_agree, const void* out_ids,
               const void* out_agree, const void* out_scores, const void* out_n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (k > UCFP_INDEX_MAX_K) return capi_fail(UCFP_E_INVALID, "k = %u exceeds UCFP_INDEX_MAX_K = %u", k, UCFP_INDEX_MAX_K);
    if (min_agree > ix->h) return capi_fail(UCFP_E_INVALID, "min_agree = %u exceeds the %u slots of a record", min_agree, ix->h);
    if (nq > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "too many queries");
    if (nq && (!records || !out_n)) return capi_fail(UCFP_E_INVALID, "records/out_n is NULL");
    if (nq && k && (!out_ids || !out_agree || !out_scores)) return capi_fail(UCFP_E_INVALID, "an output buffer is NULL");
    return UCFP_OK;
}

}  // namespace

extern "C" {

uint32_t ucfp_minhash_agree_h(const uint8_t* a, const uint8_t* b, uint32_t h) {
    if (!a || !b || h < UCFP_MINHASH_H_MIN || h > UCFP_MINHASH_H_MAX || h % UCFP_MINHASH_H_STEP != 0) return 0;
    uint32_t agree = 0;
    for (uint32_t i = 0; i < h; i++) agree += memcmp(a + kHeaderBytes + 8 * i, b + kHeaderBytes + 8 * i, 8) == 0 ? 1u : 0u;
    return agree;
}

uint32_t ucfp_minhash_agree(const uint8_t* a, const uint8_t* b) { return ucfp_minhash_agree_h(a, b, 128); }

int ucfp_minhash_index_create_h(ucfp_ctx* ctx, uint32_t flags, uint32_t h, ucfp_minhash_index** out) {
    if (!ctx || !out) return capi_fail(UCFP_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (flags != 0) return capi_fail(UCFP_E_INVALID, "no MinHash index flags are defined (got %u)", flags);
    if (int rc = ucfp::minhash_h_check(h)) return rc;
    const int rc = ucfp::create_index(ctx, "MinHash index", out);
    if (rc) return rc;
    (*out)->h = h;
    (*out)->chunks = (h + kChunkSlots - 1) / kChunkSlots;
    ucfp::scan_key_bytes_env(*out, "UCFP_MINHASH_KEY_BYTES");
    return rc;
}

int ucfp_minhash_index_create(ucfp_ctx* ctx, uint32_t flags, ucfp_minhash_index** out) {
    return ucfp_minhash_index_create_h(ctx, flags, 128, out);
}

uint32_t ucfp_minhash_index_slots(ucfp_minhash_index* ix) { return ix ? ix->h : 0; }

void ucfp_minhash_index_destroy(ucfp_minhash_index* ix) { ucfp::scan_destroy(ix); }

int ucfp_minhash_index_upsert(ucfp_minhash_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* records, size_t n) {
    return ucfp::scan_upsert(ix, tenant, ids, records, n, "records");
}

int ucfp_minhash_index_upsert_dev(ucfp_minhash_index* ix, uint32_t tenant, const uint64_t* d_ids, const uint8_t* d_records,
                                  size_t n, void* stream) {
    return ucfp::scan_upsert_dev(ix, tenant, d_ids, d_records, n, "records", stream);
}

int ucfp_minhash_index_delete(ucfp_minhash_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed) {
    return ucfp::scan_delete(ix, tenant, ids, n, n_removed);
}

int ucfp_minhash_index_size(ucfp_minhash_index* ix, uint32_t tenant, size_t* rows) { return ucfp::scan_size(ix, tenant, rows); }

int ucfp_minhash_index_flush(ucfp_minhash_index* ix) { return ucfp::scan_flush(ix); }

int ucfp_minhash_index_query_dev(ucfp_minhash_index* ix, uint32_t tenant, const uint8_t* d_records, size_t nq, uint32_t k,
                                 uint32_t min_agree, uint64_t* d_out_ids, uint32_t* d_out_agree, float* d_out_scores,
                                 uint32_t* d_out_n, void* stream) {
    const int rc = query_args(ix, d_records, nq, k, min_agree, d_out_ids, d_out_agree, d_out_scores, d_out_n);
    if (rc || nq == 0) return rc;
    return ucfp::scan_query_dev(ix, stream, [&](hipStream_t st) {
        return query_impl(ix, tenant, d_records, nq, k, min_agree, {d_out_ids, d_out_agree, d_out_scores, d_out_n}, st);
    });
}

int ucfp_minhash_index_query(ucfp_minhash_index* ix, uint32_t tenant, const uint8_t* records, size_t nq, uint32_t k,
                             uint32_t min_agree, uint64_t* out_ids, uint32_t* out_agree, float* out_scores, uint32_t* out_n) {
    const int rc = query_args(ix, records, nq, k, min_agree, out_ids, out_agree, out_scores, out_n);
    if (rc || nq == 0) return rc;
    return ucfp::scan_query_host(ix, records, nq, k, out_ids, out_agree, out_scores, out_n,
                                 [&](const uint8_t* d_q, const ucfp::ScanOut& o, hipStream_t st) {
                                     return query_impl(ix, tenant, d_q, nq, k, min_agree, o, st);
                                 });
}

}  // extern "C"
