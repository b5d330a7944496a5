// bm25.hip -- BM25 keyword search over a per-tenant inverted index on the device.
//
// Spec (the reference's src/index/embedded/bm25.rs:79-628, restated in DESIGN A11; K1 = 1.2f, B = 0.75f, f32, one IEEE
// operation at a time):
//   document   (key, tf) pairs with distinct keys and tf > 0; dl = sum tf; N live documents, T = sum dl
//   P_j        the live documents holding query key t_j; df = |P_j|; idf_j = logf((nf - df + 0.5f) / (df + 0.5f) + 1)
//              computed on the HOST with the C library's logf (what Rust's f32::ln calls), from the device's df
//   norm(d)    K1 * ((1 - B) + (B * dl) / fmaxf(avgdl, 1)),   avgdl = (float)T / (float)N
//   c(j, d)    (idf_j * (tf * (K1 + 1))) / fmaxf(tf + norm(d), 1e-6f);  score(d) = 0 + c(1, d) + c(2, d) + ... (ascending j)
//   hits       every d in some P_j, whatever its score; (score desc, id asc); first k
//
// Layout of a tenant after a (lazy) rebuild: postings u64 [P] (ordinal | tf << 32) sorted by (key, ordinal) -- one run
// P_j per distinct key -- with the distinct keys u64 [U], their run starts u32 [U + 1], a directory dir[b] = first
// distinct key with key >> shift >= b (shift puts the largest key in 18 bits), the id of each ordinal and norm per
// ordinal.  Ordinals follow ascending record id, so (score desc, ordinal asc) is the spec's (score desc, id asc).  The
// rebuild is postings.h's: rocPRIM's stable radix sort of (key, ordinal | tf << 32), the compaction post_count /
// post_scan_tiles / post_compact with BmHead (a key's first posting) and BmEmit (ukeys, ustart), post_directory on
// key >> shift; bm_norm computes norm.
//
// Query (one launch sequence for a ragged batch of key lists):
//   bm_lookup    one thread per query key: its run (start, df)
//   host         reads df back once, computes idf and V = sum df per query, picks a path per query
//   bm_small     V <= kLdsPostings: one block per query, an LDS open-addressing table ordinal -> score; the terms are
//                added in order with a barrier between them (within one term an ordinal occurs once: no atomic add);
//                then a bitonic sort of the packed candidates (~bits(score) << 32 | ordinal) in LDS
//   bm_range     larger V: block (r, q) owns ordinals [r R, (r + 1) R) of query q and keeps their scores dense in LDS,
//                walking the terms in order with a binary search into each P_j; a running top-k of the range
//                (topk_offer) goes to a parts buffer (k u64 candidate keys per range)
//   bm_merge     one block per large query: running top-k over its parts
//   bm_explain   optional: tf and the contribution of every (hit, position), by binary search in P_j
// Scores are >= 0, so ~bits(score) is monotone decreasing in the score and a zero score still sorts before the empty
// key ~0 (ordinals < 2^32 - 1).  No float atomics anywhere: every score is the same sum in the same order on both paths.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <unordered_map>
#include <vector>

#include "postings.h"

namespace {

constexpr float K1 = 1.2f;
constexpr float B = 0.75f;
constexpr uint32_t kDirBits = 18;
constexpr uint32_t kSlots = 8192;                   // bm_small LDS table: 64 KiB of (ordinal, score)
constexpr uint32_t kSlotsPerThread = kSlots / kThreads;
constexpr uint64_t kLdsPostings = UCFP_BM25_LDS_POSTINGS;   // at most 75 % load; a query with more takes bm_range
constexpr uint32_t kRange = 8192;                   // bm_range: ordinals per block (32 KiB of scores)
constexpr uint32_t kSmall = 0xffffffffu;            // path[q] of a query on bm_small
constexpr size_t kPartsBudget = (size_t)32 << 20;   // bm_range candidates per launch (256 MiB of u64)

static_assert(kLdsPostings * 4 <= (uint64_t)kSlots * 3, "bm_small needs a free slot for every posting");

__device__ __forceinline__ uint64_t cand_key(float score, uint32_t ord) {
    return ((uint64_t)(~__float_as_uint(score)) << 32) | ord;
}

// the spec's contribution, one IEEE operation at a time (the build passes -ffp-contract=off; '/' is correctly rounded)
__host__ __device__ __forceinline__ float contribution(float idf, uint32_t tf, float norm) {
    const float ftf = (float)tf;
    const float den = ftf + norm;
    const float num = idf * (ftf * (K1 + 1.0f));
    return num / fmaxf(den, 1e-6f);
}

// s_key[0, n) sorted ascending (entries past n are not read); one block writes query q's first k
__device__ void write_hits(const uint64_t* s_key, uint32_t n, uint32_t q, uint32_t k, const uint64_t* __restrict__ ids,
                           uint64_t* __restrict__ out_ids, float* __restrict__ out_scores, uint32_t* __restrict__ out_n,
                           uint32_t* __restrict__ hord) {
    const uint32_t j = threadIdx.x;
    const uint64_t sk = j < k && j < n ? s_key[j] : kEmpty64;
    const bool valid = sk != kEmpty64;
    if (j < k) {
        const size_t o = (size_t)q * k + j;
        out_ids[o] = valid ? ids[(uint32_t)sk] : kEmpty64;
        out_scores[o] = valid ? __uint_as_float(~(uint32_t)(sk >> 32)) : -1.0f;
        hord[o] = valid ? (uint32_t)sk : kEmpty32;
    }
    const int cnt = __syncthreads_count(valid);
    if (threadIdx.x == 0) out_n[q] = (uint32_t)cnt;
}

// first index in [lo, hi) of postings whose ordinal is >= ord
__device__ __forceinline__ uint32_t lower_ord(const uint64_t* __restrict__ post, uint32_t lo, uint32_t hi, uint32_t ord) {
    while (lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        if ((uint32_t)post[m] < ord) lo = m + 1;
        else hi = m;
    }
    return lo;
}

// ---------------------------------------------------------------- rebuild

// postings sorted by (key, ordinal): a head is the start of a key's run
struct BmHead {
    const uint64_t* keys;
    __device__ bool operator()(size_t i) const { return i == 0 || keys[i] != keys[i - 1]; }
};

// the distinct keys and where their runs start
struct BmEmit {
    const uint64_t* keys;
    uint64_t* ukeys;
    uint32_t* ustart;
    __device__ void operator()(size_t i, uint64_t o) const {
        ukeys[o] = keys[i];
        ustart[o] = (uint32_t)i;
    }
};

__global__ void bm_norm(const uint32_t* __restrict__ dl, size_t n, float avgdl, float* __restrict__ norm) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float bdl = B * (float)dl[i];
    const float r = bdl / fmaxf(avgdl, 1.0f);
    norm[i] = K1 * ((1.0f - B) + r);
}

// ---------------------------------------------------------------- query

// one thread per query key: its run [lo, lo + df) in the postings (df = 0 when the key is absent)
__global__ void bm_lookup(const uint64_t* __restrict__ qkeys, size_t total, const uint64_t* __restrict__ ukeys,
                          const uint32_t* __restrict__ ustart, const uint32_t* __restrict__ dir, uint32_t shift,
                          uint32_t nb, uint32_t* __restrict__ run_lo, uint32_t* __restrict__ run_df) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint64_t key = qkeys[i];
    const uint64_t b = key >> shift;
    uint32_t lo = 0, df = 0;
    if (b < nb) {
        uint32_t l = dir[b], r = dir[b + 1];
        while (l < r) {
            const uint32_t m = (l + r) >> 1;
            if (ukeys[m] < key) l = m + 1;
            else r = m;
        }
        if (l < dir[b + 1] && ukeys[l] == key) {
            lo = ustart[l];
            df = ustart[l + 1] - lo;
        }
    }
    run_lo[i] = lo;
    run_df[i] = df;
}

__device__ __forceinline__ uint32_t slot32(uint32_t ord) { return (ord * 0x9E3779B1u) >> 19; }   // 13 bits

// one block per query; queries with path[q] != kSmall are left to bm_range / bm_merge
__global__ __launch_bounds__(kThreads) void bm_small(const uint64_t* __restrict__ qoff, const uint32_t* __restrict__ path,
                                                      const uint32_t* __restrict__ run_lo,
                                                      const uint32_t* __restrict__ run_df, const float* __restrict__ idf,
                                                      const uint64_t* __restrict__ post, const float* __restrict__ norm,
                                                      const uint64_t* __restrict__ ids, uint32_t k,
                                                      uint64_t* __restrict__ out_ids, float* __restrict__ out_scores,
                                                      uint32_t* __restrict__ out_n, uint32_t* __restrict__ hord) {
    __shared__ uint64_t s_tab[kSlots];   // 64 KiB: (ordinal u32 [kSlots], score f32 [kSlots]), then the sort keys
    __shared__ uint32_t s_cnt;
    const uint32_t q = blockIdx.x;
    if (path[q] != kSmall) return;
    const uint64_t a = qoff[q], e = qoff[q + 1];
    uint32_t* t_ord = reinterpret_cast<uint32_t*>(s_tab);
    float* t_sc = reinterpret_cast<float*>(s_tab) + kSlots;
    for (uint32_t s = threadIdx.x; s < kSlots; s += kThreads) {
        t_ord[s] = kEmpty32;
        t_sc[s] = 0.0f;
    }
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    for (uint64_t j = a; j < e; j++) {   // ascending j; a barrier between terms
        const uint32_t df = run_df[j];
        if (df == 0) continue;           // uniform: the whole block skips
        const uint32_t lo = run_lo[j];
        const float w = idf[j];
        for (uint32_t p = threadIdx.x; p < df; p += kThreads) {
            const uint64_t ent = post[lo + p];
            const uint32_t ord = (uint32_t)ent, tf = (uint32_t)(ent >> 32);
            const float c = contribution(w, tf, norm[ord]);
            uint32_t s = slot32(ord);
            for (;;) {   // at most kLdsPostings distinct ordinals: a free slot always exists
                const uint32_t prev = atomicCAS(&t_ord[s], kEmpty32, ord);
                if (prev == kEmpty32 || prev == ord) break;
                s = (s + 1) & (kSlots - 1);
            }
            t_sc[s] = t_sc[s] + c;   // this term holds ord once: no other lane touches slot s before the barrier
        }
        __syncthreads();
    }
    uint32_t ro[kSlotsPerThread];
    float rs[kSlotsPerThread];
#pragma unroll
    for (uint32_t i = 0; i < kSlotsPerThread; i++) {
        ro[i] = t_ord[threadIdx.x + i * kThreads];
        rs[i] = t_sc[threadIdx.x + i * kThreads];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t i = 0; i < kSlotsPerThread; i++)
        if (ro[i] != kEmpty32) s_tab[atomicAdd(&s_cnt, 1u)] = cand_key(rs[i], ro[i]);
    __syncthreads();
    const uint32_t nc = s_cnt;
    uint32_t n = 1;
    while (n < nc) n <<= 1;
    for (uint32_t i = nc + threadIdx.x; i < n; i += kThreads) s_tab[i] = kEmpty64;
    __syncthreads();
    bitonic_sort(s_tab, n);
    write_hits(s_tab, nc, q, k, ids, out_ids, out_scores, out_n, hord);
}

// block (r, l): ordinals [r kRange, (r + 1) kRange) of large query lq[l]; its best k candidate keys to parts
__global__ __launch_bounds__(kThreads) void bm_range(const uint64_t* __restrict__ qoff, const uint32_t* __restrict__ lq,
                                                      const uint32_t* __restrict__ run_lo,
                                                      const uint32_t* __restrict__ run_df, const float* __restrict__ idf,
                                                      const uint64_t* __restrict__ post, const float* __restrict__ norm,
                                                      uint32_t n_ord, uint32_t k, uint64_t* __restrict__ parts) {
    __shared__ float s_sc[kRange];
    __shared__ uint32_t s_hit[kRange / 32];
    __shared__ uint64_t s_top[2 * kThreads];
    const uint32_t r = blockIdx.x, q = lq[blockIdx.y];
    const uint32_t r0 = r * kRange, r1 = min(r0 + kRange, n_ord);
    for (uint32_t i = threadIdx.x; i < kRange; i += kThreads) s_sc[i] = 0.0f;
    for (uint32_t i = threadIdx.x; i < kRange / 32; i += kThreads) s_hit[i] = 0;
    for (uint32_t i = threadIdx.x; i < 2 * kThreads; i += kThreads) s_top[i] = kEmpty64;
    __syncthreads();
    const uint64_t a = qoff[q], e = qoff[q + 1];
    for (uint64_t j = a; j < e; j++) {
        const uint32_t df = run_df[j];
        if (df == 0) continue;
        const uint32_t lo = run_lo[j];
        // every lane finds the same sub-run of P_j (ordinals ascending within a run)
        const uint32_t pa = lower_ord(post, lo, lo + df, r0);
        const uint32_t pb = lower_ord(post, pa, lo + df, r1);
        const float w = idf[j];
        for (uint32_t p = pa + threadIdx.x; p < pb; p += kThreads) {
            const uint64_t ent = post[p];
            const uint32_t ord = (uint32_t)ent, tf = (uint32_t)(ent >> 32);
            const uint32_t l = ord - r0;
            s_sc[l] = s_sc[l] + contribution(w, tf, norm[ord]);
            atomicOr(&s_hit[l >> 5], 1u << (l & 31));
        }
        __syncthreads();
    }
    for (uint32_t c = 0; c < kRange; c += kThreads) {
        const uint32_t l = c + threadIdx.x;
        const bool hit = (s_hit[l >> 5] >> (l & 31)) & 1u;
        topk_offer(s_top, k, hit ? cand_key(s_sc[l], r0 + l) : kEmpty64);
    }
    uint64_t* out = parts + ((size_t)blockIdx.y * gridDim.x + r) * k;
    for (uint32_t j = threadIdx.x; j < k; j += kThreads) out[j] = s_top[j];
}

// one block per large query: the best k of its n_parts * k candidates
__global__ __launch_bounds__(kThreads) void bm_merge(const uint64_t* __restrict__ parts, const uint32_t* __restrict__ lq,
                                                      uint32_t n_parts, const uint64_t* __restrict__ ids, uint32_t k,
                                                      uint64_t* __restrict__ out_ids, float* __restrict__ out_scores,
                                                      uint32_t* __restrict__ out_n, uint32_t* __restrict__ hord) {
    __shared__ uint64_t s_top[2 * kThreads];
    for (uint32_t i = threadIdx.x; i < 2 * kThreads; i += kThreads) s_top[i] = kEmpty64;
    __syncthreads();
    const uint64_t* row = parts + (size_t)blockIdx.x * n_parts * k;
    const size_t m = (size_t)n_parts * k;
    for (size_t c = 0; c < m; c += kThreads) {
        const size_t i = c + threadIdx.x;
        topk_offer(s_top, k, i < m ? row[i] : kEmpty64);
    }
    write_hits(s_top, k, lq[blockIdx.x], k, ids, out_ids, out_scores, out_n, hord);
}

// one block per query: tf and contribution of (hit h, position j) at k * qoff[q] + h * m + j (0 when d is not in P_j)
__global__ __launch_bounds__(kThreads) void bm_explain(const uint64_t* __restrict__ qoff, const uint32_t* __restrict__ run_lo,
                                                        const uint32_t* __restrict__ run_df, const float* __restrict__ idf,
                                                        const uint64_t* __restrict__ post, const float* __restrict__ norm,
                                                        const uint32_t* __restrict__ hord, uint32_t k,
                                                        uint32_t* __restrict__ out_tf, float* __restrict__ out_c) {
    const uint32_t q = blockIdx.x;
    const uint64_t a = qoff[q], m = qoff[q + 1] - a;
    for (uint64_t i = threadIdx.x; i < (uint64_t)k * m; i += kThreads) {
        const uint32_t h = (uint32_t)(i / m);
        const uint64_t j = a + i % m;
        const uint32_t ord = hord[(size_t)q * k + h];
        uint32_t tf = 0;
        float c = 0.0f;
        if (ord != kEmpty32 && run_df[j]) {
            const uint32_t lo = run_lo[j], hi = lo + run_df[j];
            const uint32_t p = lower_ord(post, lo, hi, ord);
            if (p < hi && (uint32_t)post[p] == ord) {
                tf = (uint32_t)(post[p] >> 32);
                c = contribution(idf[j], tf, norm[ord]);
            }
        }
        const size_t o = (size_t)k * a + i;
        if (out_tf) out_tf[o] = tf;
        if (out_c) out_c[o] = c;
    }
}

// empty answers for every query (unknown or empty tenant)
__global__ void bm_empty(size_t nq, uint32_t k, uint64_t* __restrict__ out_ids, float* __restrict__ out_scores,
                         uint32_t* __restrict__ out_n, uint32_t* __restrict__ hord) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq * k) {
        out_ids[i] = kEmpty64;
        out_scores[i] = -1.0f;
        hord[i] = kEmpty32;
    }
    if (i < nq) out_n[i] = 0;
}

struct Doc {
    std::vector<uint64_t> keys;
    std::vector<uint32_t> tfs;
    uint32_t dl = 0;
};

struct Tenant {
    std::map<uint64_t, Doc> docs;   // ascending id = ordinal order
    uint64_t total_len = 0;         // T
    size_t n_post = 0;              // (key, document) pairs
    bool dirty = true;
    size_t n_keys = 0;              // distinct keys, valid when !dirty
    uint32_t shift = 0, nb = 0;     // directory, valid when !dirty
    DevArr post, ukeys, ustart, dir, ids, norm;
};

}  // namespace

struct ucfp_bm25_index : ucfp::IndexCore {
    std::unordered_map<uint32_t, Tenant> tenants;
    // rebuild workspace
    DevArr b_keys_a, b_keys_b, b_vals_a, b_dl, b_cnt, b_off, b_tmp;
    // query workspace
    DevArr q_keys, q_off, q_lo, q_df, q_idf, q_path, q_lq, q_parts, q_hord, q_out;
    std::vector<uint64_t> h_off;
    std::vector<uint32_t> h_df, h_path, h_lq;
    std::vector<float> h_idf;
};

namespace {

int check_docs(const uint64_t* ids, const uint64_t* keys, const uint32_t* tfs, const uint64_t* offsets, size_t n) {
    if (n && (!offsets || !ids)) return capi_fail(UCFP_E_INVALID, "ids/offsets is NULL");
    if (!n) return UCFP_OK;
    if (offsets[0] != 0) return capi_fail(UCFP_E_INVALID, "offsets[0] must be 0");
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return capi_fail(UCFP_E_INVALID, "offsets decrease at %zu", i);
    if (offsets[n] && (!keys || !tfs)) return capi_fail(UCFP_E_INVALID, "keys/tfs is NULL");
    std::vector<uint64_t> s;
    for (size_t i = 0; i < n; i++) {
        uint64_t dl = 0;
        for (uint64_t j = offsets[i]; j < offsets[i + 1]; j++) {
            if (tfs[j] == 0) return capi_fail(UCFP_E_INVALID, "document %zu has tf = 0 at pair %llu", i, (unsigned long long)j);
            dl += tfs[j];
        }
        if (dl > 0xffffffffull) return capi_fail(UCFP_E_INVALID, "document %zu has %llu tokens (>= 2^32)", i,
                                                 (unsigned long long)dl);
        s.assign(keys + offsets[i], keys + offsets[i + 1]);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end())
            return capi_fail(UCFP_E_INVALID, "document %zu holds a key twice", i);
    }
    return UCFP_OK;
}

int do_upsert(ucfp_bm25_index* ix, uint32_t tenant, const uint64_t* ids, const uint64_t* keys, const uint32_t* tfs,
              const uint64_t* offsets, size_t n) {
    int rc = check_docs(ids, keys, tfs, offsets, n);
    if (rc || !n) return rc;
    Tenant& T = ix->tenants[tenant];
    for (size_t i = 0; i < n; i++) {
        Doc& d = T.docs[ids[i]];
        T.total_len -= d.dl;
        T.n_post -= d.keys.size();
        d.keys.assign(keys + offsets[i], keys + offsets[i + 1]);
        d.tfs.assign(tfs + offsets[i], tfs + offsets[i + 1]);
        uint64_t dl = 0;
        for (uint32_t t : d.tfs) dl += t;
        d.dl = (uint32_t)dl;
        T.total_len += d.dl;
        T.n_post += d.keys.size();
    }
    T.dirty = true;
    return UCFP_OK;
}

int rebuild(ucfp_bm25_index* ix, Tenant& T, hipStream_t st) {
    const size_t n = T.n_post, nd = T.docs.size();
    if (nd >= 0xffffffffull) return capi_fail(UCFP_E_INVALID, "too many documents in one tenant");
    if (n >= 0xffffffffull) return capi_fail(UCFP_E_INVALID, "too many postings in one tenant (%zu)", n);
    std::vector<uint64_t> h_keys(n), h_vals(n), h_ids(nd);
    std::vector<uint32_t> h_dl(nd);
    uint64_t maxkey = 0;
    size_t o = 0;
    uint32_t ord = 0;
    for (auto& kv : T.docs) {
        h_ids[ord] = kv.first;
        h_dl[ord] = kv.second.dl;
        const Doc& d = kv.second;
        for (size_t j = 0; j < d.keys.size(); j++) {
            h_keys[o + j] = d.keys[j];
            h_vals[o + j] = (uint64_t)ord | ((uint64_t)d.tfs[j] << 32);
            maxkey = std::max(maxkey, d.keys[j]);
        }
        o += d.keys.size();
        ord++;
    }
    uint32_t bits = 0;
    while (bits < 64 && (maxkey >> bits)) bits++;
    T.shift = bits > kDirBits ? bits - kDirBits : 0;
    T.nb = (uint32_t)(maxkey >> T.shift) + 1;
    int rc;
    if ((rc = T.ids.ensure(nd * 8)) || (rc = T.norm.ensure(nd * 4)) || (rc = T.dir.ensure(((size_t)T.nb + 1) * 4)) ||
        (rc = ix->b_dl.ensure(nd * 4)) || (rc = T.post.ensure(n * 8)))
        return rc;
    if (nd) {
        HIP_TRY(hipMemcpyAsync(T.ids.p, h_ids.data(), nd * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ix->b_dl.p, h_dl.data(), nd * 4, hipMemcpyHostToDevice, st));
        // avgdl on the host, norm on the device with the spec's f32 operations
        const float avgdl = (float)T.total_len / (float)nd;
        hipLaunchKernelGGL(bm_norm, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, ix->b_dl.as<uint32_t>(), nd, avgdl,
                           T.norm.as<float>());
        HIP_TRY(hipGetLastError());
    }
    size_t u = 0;
    if (n) {
        if ((rc = ix->b_keys_a.ensure(n * 8)) || (rc = ix->b_keys_b.ensure(n * 8)) || (rc = ix->b_vals_a.ensure(n * 8)))
            return rc;
        HIP_TRY(hipMemcpyAsync(ix->b_keys_a.p, h_keys.data(), n * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ix->b_vals_a.p, h_vals.data(), n * 8, hipMemcpyHostToDevice, st));
        // stable: the documents of one key keep ascending ordinals
        uint64_t* keys = ix->b_keys_b.as<uint64_t>();
        if ((rc = sort_pairs(ix->b_tmp, ix->b_keys_a.as<uint64_t>(), keys, ix->b_vals_a.as<uint64_t>(), T.post.as<uint64_t>(),
                             n, bits ? (int)bits : 1, st)) ||
            (rc = count_heads(BmHead{keys}, n, ix->b_cnt, ix->b_off, st, &u)) || (rc = T.ukeys.ensure(u * 8)) ||
            (rc = T.ustart.ensure((u + 1) * 4)) ||
            (rc = compact_heads(BmHead{keys}, BmEmit{keys, T.ukeys.as<uint64_t>(), T.ustart.as<uint32_t>()}, n, ix->b_off, st)))
            return rc;
    } else if ((rc = T.ukeys.ensure(0)) || (rc = T.ustart.ensure(4))) {
        return rc;
    }
    HIP_TRY(hipMemsetD32Async(T.ustart.as<uint32_t>() + u, (int)n, 1, st));   // ustart[U] = n
    if ((rc = build_directory(T.ukeys.as<uint64_t>(), u, T.shift, T.nb, T.dir.as<uint32_t>(), st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));   // the host vectors above go out of scope
    T.n_keys = u;
    T.dirty = false;
    return UCFP_OK;
}

// the host copy of the offsets is in ix->h_off; d_keys / d_off are device pointers
int query_impl(ucfp_bm25_index* ix, uint32_t tenant, const uint64_t* d_keys, const uint64_t* d_off, size_t nq, uint32_t k,
               uint64_t* d_ids, float* d_scores, uint32_t* d_n, float* out_idf, uint32_t* out_tf, float* out_c,
               hipStream_t st) {
    int rc;
    const std::vector<uint64_t>& off = ix->h_off;
    const size_t total = (size_t)off[nq];
    if (total && !d_keys) return capi_fail(UCFP_E_INVALID, "keys is NULL");
    if (total >= 0xffffffffull) return capi_fail(UCFP_E_INVALID, "too many query keys");
    if (k == 0) {
        HIP_TRY(hipMemsetAsync(d_n, 0, nq * 4, st));
        if (total && out_idf) HIP_TRY(hipMemsetAsync(out_idf, 0, total * 4, st));
        return UCFP_OK;
    }
    if ((rc = ix->q_hord.ensure(nq * k * 4))) return rc;
    auto it = ix->tenants.find(tenant);
    Tenant* T = it == ix->tenants.end() ? nullptr : &it->second;
    if (T && T->dirty && (rc = rebuild(ix, *T, st))) return rc;
    if (!T || T->docs.empty() || total == 0) {
        hipLaunchKernelGGL(bm_empty, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, st, nq, k, d_ids, d_scores, d_n,
                           ix->q_hord.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        if (total && out_idf) HIP_TRY(hipMemsetAsync(out_idf, 0, total * 4, st));
        if (total && out_tf) HIP_TRY(hipMemsetAsync(out_tf, 0, total * k * 4, st));
        if (total && out_c) HIP_TRY(hipMemsetAsync(out_c, 0, total * k * 4, st));
        return UCFP_OK;
    }
    // 1. runs and df of every query key; df back to the host
    if ((rc = ix->q_lo.ensure(total * 4)) || (rc = ix->q_df.ensure(total * 4)) || (rc = ix->q_idf.ensure(total * 4)) ||
        (rc = ix->q_path.ensure(nq * 4)))
        return rc;
    hipLaunchKernelGGL(bm_lookup, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_keys, total,
                       T->ukeys.as<uint64_t>(), T->ustart.as<uint32_t>(), T->dir.as<uint32_t>(), T->shift, T->nb,
                       ix->q_lo.as<uint32_t>(), ix->q_df.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    ix->h_df.resize(total);
    HIP_TRY(hipMemcpyAsync(ix->h_df.data(), ix->q_df.p, total * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // 2. idf with the host's logf; the path of each query
    const float nf = (float)T->docs.size();
    ix->h_idf.resize(total);
    for (size_t i = 0; i < total; i++) {
        float w = 0.0f;
        if (ix->h_df[i]) {
            const float df = (float)ix->h_df[i];
            const float x = (nf - df + 0.5f) / (df + 0.5f);
            w = logf(x + 1.0f);
        }
        ix->h_idf[i] = w;
    }
    ix->h_path.assign(nq, kSmall);
    ix->h_lq.clear();
    for (size_t q = 0; q < nq; q++) {
        uint64_t v = 0;
        for (uint64_t j = off[q]; j < off[q + 1]; j++) v += ix->h_df[j];
        if (v > kLdsPostings) {
            ix->h_path[q] = (uint32_t)ix->h_lq.size();
            ix->h_lq.push_back((uint32_t)q);
        }
    }
    const size_t n_large = ix->h_lq.size();
    if ((rc = ix->q_lq.ensure(n_large * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(ix->q_idf.p, ix->h_idf.data(), total * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ix->q_path.p, ix->h_path.data(), nq * 4, hipMemcpyHostToDevice, st));
    if (n_large) HIP_TRY(hipMemcpyAsync(ix->q_lq.p, ix->h_lq.data(), n_large * 4, hipMemcpyHostToDevice, st));
    if (out_idf) HIP_TRY(hipMemcpyAsync(out_idf, ix->q_idf.p, total * 4, hipMemcpyDefault, st));
    // 3. scoring and top-k
    const uint64_t* post = T->post.as<uint64_t>();
    const float* norm = T->norm.as<float>();
    const uint64_t* ids = T->ids.as<uint64_t>();
    hipLaunchKernelGGL(bm_small, dim3((unsigned)nq), dim3(kThreads), 0, st, d_off, ix->q_path.as<uint32_t>(),
                       ix->q_lo.as<uint32_t>(), ix->q_df.as<uint32_t>(), ix->q_idf.as<float>(), post, norm, ids, k, d_ids,
                       d_scores, d_n, ix->q_hord.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    if (n_large) {
        const uint32_t n_ord = (uint32_t)T->docs.size();
        const uint32_t n_parts = (n_ord + kRange - 1) / kRange;
        const size_t per_q = (size_t)n_parts * k;
        const size_t chunk = std::max<size_t>(1, std::min<size_t>({n_large, kPartsBudget / per_q, 65535}));   // grid.y
        if ((rc = ix->q_parts.ensure(chunk * per_q * 8))) return rc;
        for (size_t c0 = 0; c0 < n_large; c0 += chunk) {   // stream order makes the parts buffer reusable
            const size_t c = std::min(chunk, n_large - c0);
            const uint32_t* lq = ix->q_lq.as<uint32_t>() + c0;
            hipLaunchKernelGGL(bm_range, dim3(n_parts, (unsigned)c), dim3(kThreads), 0, st, d_off, lq,
                               ix->q_lo.as<uint32_t>(), ix->q_df.as<uint32_t>(), ix->q_idf.as<float>(), post, norm, n_ord,
                               k, ix->q_parts.as<uint64_t>());
            hipLaunchKernelGGL(bm_merge, dim3((unsigned)c), dim3(kThreads), 0, st, ix->q_parts.as<uint64_t>(), lq, n_parts,
                               ids, k, d_ids, d_scores, d_n, ix->q_hord.as<uint32_t>());
            HIP_TRY(hipGetLastError());
        }
    }
    // 4. explain
    if (out_tf || out_c) {
        hipLaunchKernelGGL(bm_explain, dim3((unsigned)nq), dim3(kThreads), 0, st, d_off, ix->q_lo.as<uint32_t>(),
                           ix->q_df.as<uint32_t>(), ix->q_idf.as<float>(), post, norm, ix->q_hord.as<uint32_t>(), k,
                           out_tf, out_c);
        HIP_TRY(hipGetLastError());
    }
    return UCFP_OK;
}

int query_args(ucfp_bm25_index* ix, const uint64_t* offsets, size_t nq, uint32_t k, const void* out_ids,
               const void* out_scores, const void* out_n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (k > UCFP_INDEX_MAX_K) return capi_fail(UCFP_E_INVALID, "k = %u exceeds UCFP_INDEX_MAX_K = %u", k, UCFP_INDEX_MAX_K);
    if (nq > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "too many queries");
    if (nq && (!offsets || !out_n)) return capi_fail(UCFP_E_INVALID, "offsets/out_n is NULL");
    if (nq && k && (!out_ids || !out_scores)) return capi_fail(UCFP_E_INVALID, "an output buffer is NULL");
    return UCFP_OK;
}

int check_offsets(const std::vector<uint64_t>& off, size_t nq) {
    if (off[0] != 0) return capi_fail(UCFP_E_INVALID, "offsets[0] must be 0");
    for (size_t i = 0; i < nq; i++)
        if (off[i + 1] < off[i]) return capi_fail(UCFP_E_INVALID, "offsets decrease at %zu", i);
    return UCFP_OK;
}

}  // namespace

extern "C" {

int ucfp_bm25_index_create(ucfp_ctx* ctx, uint32_t flags, ucfp_bm25_index** out) {
    if (!ctx || !out) return capi_fail(UCFP_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (flags != 0) return capi_fail(UCFP_E_INVALID, "no BM25 index flags are defined (got %u)", flags);
    return ucfp::create_index(ctx, "BM25 index", out);
}

void ucfp_bm25_index_destroy(ucfp_bm25_index* ix) {
    if (!ix) return;
    ix->quiesce();
    for (auto& kv : ix->tenants)
        for (DevArr* a : {&kv.second.post, &kv.second.ukeys, &kv.second.ustart, &kv.second.dir, &kv.second.ids,
                          &kv.second.norm})
            a->release();
    for (DevArr* a : {&ix->b_keys_a, &ix->b_keys_b, &ix->b_vals_a, &ix->b_dl, &ix->b_cnt, &ix->b_off,
                      &ix->b_tmp, &ix->q_keys, &ix->q_off, &ix->q_lo, &ix->q_df, &ix->q_idf, &ix->q_path, &ix->q_lq,
                      &ix->q_parts, &ix->q_hord, &ix->q_out})
        a->release();
    delete ix;
}

int ucfp_bm25_index_upsert(ucfp_bm25_index* ix, uint32_t tenant, const uint64_t* ids, const uint64_t* keys,
                           const uint32_t* tfs, const uint64_t* offsets, size_t n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    return do_upsert(ix, tenant, ids, keys, tfs, offsets, n);
}

int ucfp_bm25_index_upsert_dev(ucfp_bm25_index* ix, uint32_t tenant, const uint64_t* d_ids, const uint64_t* d_keys,
                               const uint32_t* d_tfs, const uint64_t* d_offsets, size_t n, void* stream) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (!n) return UCFP_OK;
    if (!d_ids || !d_offsets) return capi_fail(UCFP_E_INVALID, "ids/offsets is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    // the document table lives on the host (mutations are bookkeeping; the postings are rebuilt at the next query)
    std::vector<uint64_t> ids(n), offs(n + 1);
    HIP_TRY(hipMemcpyAsync(ids.data(), d_ids, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(offs.data(), d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int rc = check_offsets(offs, n);
    if (rc) return rc;
    const size_t m = offs[n];
    std::vector<uint64_t> keys(m);
    std::vector<uint32_t> tfs(m);
    if (m) {
        if (!d_keys || !d_tfs) return capi_fail(UCFP_E_INVALID, "keys/tfs is NULL");
        HIP_TRY(hipMemcpyAsync(keys.data(), d_keys, m * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(tfs.data(), d_tfs, m * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return do_upsert(ix, tenant, ids.data(), keys.data(), tfs.data(), offs.data(), n);
}

int ucfp_bm25_index_delete(ucfp_bm25_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (n && !ids) return capi_fail(UCFP_E_INVALID, "ids is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    size_t removed = 0;
    auto it = ix->tenants.find(tenant);
    if (it != ix->tenants.end()) {
        Tenant& T = it->second;
        for (size_t i = 0; i < n; i++) {
            auto d = T.docs.find(ids[i]);
            if (d == T.docs.end()) continue;
            T.total_len -= d->second.dl;
            T.n_post -= d->second.keys.size();
            T.docs.erase(d);
            removed++;
        }
        if (removed) T.dirty = true;
    }
    if (n_removed) *n_removed = removed;
    return UCFP_OK;
}

int ucfp_bm25_index_size(ucfp_bm25_index* ix, uint32_t tenant, size_t* docs, size_t* postings) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    auto it = ix->tenants.find(tenant);
    if (docs) *docs = it == ix->tenants.end() ? 0 : it->second.docs.size();
    if (postings) *postings = it == ix->tenants.end() ? 0 : it->second.n_post;
    return UCFP_OK;
}

int ucfp_bm25_index_flush(ucfp_bm25_index* ix) { return ucfp::flush_dirty(ix, rebuild); }

int ucfp_bm25_index_query_dev(ucfp_bm25_index* ix, uint32_t tenant, const uint64_t* d_keys, const uint64_t* d_offsets,
                              size_t nq, uint32_t k, uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_n,
                              float* d_out_idf, uint32_t* d_out_tf, float* d_out_contrib, void* stream) {
    int rc = query_args(ix, d_offsets, nq, k, d_out_ids, d_out_scores, d_out_n);
    if (rc || nq == 0) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    if ((rc = ix->begin())) return rc;
    hipStream_t st = (hipStream_t)stream;
    ix->h_off.resize(nq + 1);
    HIP_TRY(hipMemcpyAsync(ix->h_off.data(), d_offsets, (nq + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = check_offsets(ix->h_off, nq))) return rc;
    rc = query_impl(ix, tenant, d_keys, d_offsets, nq, k, d_out_ids, d_out_scores, d_out_n, d_out_idf, d_out_tf,
                    d_out_contrib, st);
    return ix->end(st, rc);
}

int ucfp_bm25_index_query(ucfp_bm25_index* ix, uint32_t tenant, const uint64_t* keys, const uint64_t* offsets, size_t nq,
                          uint32_t k, uint64_t* out_ids, float* out_scores, uint32_t* out_n, float* out_idf,
                          uint32_t* out_tf, float* out_contrib) {
    int rc = query_args(ix, offsets, nq, k, out_ids, out_scores, out_n);
    if (rc || nq == 0) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    ix->h_off.assign(offsets, offsets + nq + 1);
    if ((rc = check_offsets(ix->h_off, nq))) return rc;
    const size_t total = offsets[nq], nk = nq * k;
    if (total && !keys) return capi_fail(UCFP_E_INVALID, "keys is NULL");
    if ((rc = ix->begin())) return rc;
    hipStream_t st = ix->own;
    // outputs: ids [nk] u64, scores [nk], n [nq], idf [total], tf [total k], contributions [total k]
    const size_t o_sc = nk * 8, o_n = o_sc + nk * 4, o_idf = o_n + nq * 4, o_tf = o_idf + total * 4,
                 o_c = o_tf + total * k * 4, o_end = o_c + total * k * 4;
    if ((rc = ix->q_keys.ensure(total * 8)) || (rc = ix->q_off.ensure((nq + 1) * 8)) || (rc = ix->q_out.ensure(o_end)))
        return rc;
    if (total) HIP_TRY(hipMemcpyAsync(ix->q_keys.p, keys, total * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ix->q_off.p, offsets, (nq + 1) * 8, hipMemcpyHostToDevice, st));
    uint8_t* ob = ix->q_out.as<uint8_t>();
    rc = query_impl(ix, tenant, ix->q_keys.as<uint64_t>(), ix->q_off.as<uint64_t>(), nq, k, (uint64_t*)ob,
                    (float*)(ob + o_sc), (uint32_t*)(ob + o_n), out_idf ? (float*)(ob + o_idf) : nullptr,
                    out_tf ? (uint32_t*)(ob + o_tf) : nullptr, out_contrib ? (float*)(ob + o_c) : nullptr, st);
    if (rc) return ix->end_sync(rc);
    if (nk) {
        HIP_TRY(hipMemcpyAsync(out_ids, ob, nk * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_scores, ob + o_sc, nk * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(out_n, ob + o_n, nq * 4, hipMemcpyDeviceToHost, st));
    if (total && out_idf) HIP_TRY(hipMemcpyAsync(out_idf, ob + o_idf, total * 4, hipMemcpyDeviceToHost, st));
    if (total && nk && out_tf) HIP_TRY(hipMemcpyAsync(out_tf, ob + o_tf, total * k * 4, hipMemcpyDeviceToHost, st));
    if (total && nk && out_contrib) HIP_TRY(hipMemcpyAsync(out_contrib, ob + o_c, total * k * 4, hipMemcpyDeviceToHost, st));
    return ix->end_sync(UCFP_OK);
}

}  // extern "C"
