// landmark.hip -- GPU landmark index over Wang hashes: "which recording is this, and where in it?"
//
// Spec (ours; the reference has no audio matcher):
//   landmark  8 bytes: u32 LE hash, u32 LE t (the Wang record layout); t < 2^31
//   R_r, Q    the distinct (hash, t) pairs of a record / a query
//   P(h)      postings (record, t) with hash h over the live records of the tenant; h is stopped if max_postings > 0
//             and P(h) > max_postings
//   count(r, d) = |{(h, t) in Q : h not stopped, (h, t + d) in R_r}|;  votes(r) = max_d count,  offset(r) = smallest
//             d attaining it;  hits: votes >= max(min_votes, 1), (votes desc, id asc), first k;
//             score = (float)votes / (float)|Q|
//
// Layout of a tenant after a (lazy) rebuild: postings sorted by (hash, t, ordinal), deduplicated, as two arrays --
// hashes u32 [P] and entries u64 [P] (ordinal | t << 32) -- plus a directory dir[b] = first posting whose hash >> 14
// is >= b (b < 2^18 + 1: the f_a|f_b bits) and the id of each ordinal.  Ordinals follow ascending record id, so the
// (votes desc, ordinal asc) order is the (votes desc, id asc) order of the spec.  The rebuild is postings.h's: rocPRIM's
// stable radix sort of (hash << 32 | t, ordinal), the compaction post_count / post_scan_tiles / post_compact with
// LmHead (a new (key, ordinal) pair) and LmEmit (hashes, entries), and post_directory on hash >> 14.
//
// Query (one launch sequence for a ragged batch):
//   lm_qprep / lm_qkeys   check the offsets and t < 2^31, pack keys = hash << 32 | t
//   rocPRIM               segmented radix sort of the keys per query (a library primitive, as in lsh.hip)
//   lm_qruns              one block per query: drop duplicates, look each hash up, apply the stop cap; |Q| and the
//                         number of votes V of the query
//   lm_vote               one block per query: the votes (ordinal, t_r - t_q) are expanded chunk by chunk (a block scan
//                         of the run lengths, then every lane takes the next vote) and counted in an LDS hash table of
//                         kSlots keys; then the per-ordinal best (count, smallest offset) in a second LDS table, and a
//                         bitonic sort of the candidates picks the top k.  Distinct keys <= V, so a query with
//                         V <= kLdsVotes (75 % of the slots) always fits; a larger one writes its votes to a global
//                         spill buffer instead.
//   spill path            rocPRIM segmented sort of the spilled votes; lm_spill_best: every run end of equal
//                         (ordinal, offset) keys takes its count from a binary search for the run start and folds
//                         (count, -offset) into a dense per-(query, ordinal) best with atomicMax; lm_spill_topk scans
//                         that row 256 ordinals at a time and merges candidates into an LDS top-k (topk_offer).
// The host reads two small arrays per query batch (the checked sizes, then V per query) to size the sort and the
// spill buffers; everything else is asynchronous.

#include <hip/hip_runtime.h>

#include <map>
#include <unordered_map>
#include <vector>

#include "postings.h"

namespace {

constexpr uint32_t kDirBits = 14;                  // hash >> 14 = f_a | f_b
constexpr uint32_t kDirSize = 1u << 18;
constexpr uint32_t kSlots = 4096;                  // LDS vote table (48 KiB with the counts)
constexpr uint32_t kSlotsPerThread = kSlots / kThreads;
constexpr uint64_t kLdsVotes = 3072;               // at most 75 % load: a query with more votes spills
constexpr uint32_t kBias = 0x80000000u;            // offset d stored as d + 2^31 (monotone in d)
constexpr uint64_t kNoSpill = ~0ull;

// candidate sort key: (votes desc, ordinal asc); kEmpty64 sorts last
__device__ __forceinline__ uint64_t cand_key(uint32_t votes, uint32_t ord) {
    return ((uint64_t)(0xffffffffu - votes) << 32) | ord;
}

// best-of-ordinal value: (count desc, offset asc) under atomicMax
__device__ __forceinline__ uint64_t best_val(uint32_t cnt, uint32_t dbias) {
    return ((uint64_t)cnt << 32) | (0xffffffffu - dbias);
}

// s_key/s_dbias sorted ascending, n entries; one block writes query q's k results
__device__ void write_hits(const uint64_t* s_key, const uint32_t* s_dbias, uint32_t n, uint32_t q, uint32_t k, uint32_t qn,
                           const uint64_t* __restrict__ ids, uint64_t* __restrict__ out_ids,
                           uint32_t* __restrict__ out_votes, int32_t* __restrict__ out_offsets,
                           float* __restrict__ out_scores, uint32_t* __restrict__ out_n) {
    const uint32_t j = threadIdx.x;   // k <= UCFP_INDEX_MAX_K < kThreads
    const uint64_t sk = j < k && j < n ? s_key[j] : kEmpty64;
    const bool valid = sk != kEmpty64;
    if (j < k) {
        const size_t o = (size_t)q * k + j;
        const uint32_t votes = valid ? 0xffffffffu - (uint32_t)(sk >> 32) : 0u;
        out_ids[o] = valid ? ids[(uint32_t)sk] : kEmpty64;
        out_votes[o] = votes;
        out_offsets[o] = valid ? (int32_t)(s_dbias[j] - kBias) : 0;
        out_scores[o] = valid ? (float)votes / (float)qn : -1.0f;
    }
    const int cnt = __syncthreads_count(valid);
    if (threadIdx.x == 0) out_n[q] = (uint32_t)cnt;
}

__device__ __forceinline__ void find_run(const uint32_t* __restrict__ hashes, const uint32_t* __restrict__ dir, uint32_t h,
                                         uint32_t& lo, uint32_t& len) {
    const uint32_t b = h >> kDirBits;
    uint32_t a = dir[b], e = dir[b + 1];
    uint32_t l = a, r = e;
    while (l < r) {   // first >= h
        const uint32_t m = (l + r) >> 1;
        if (hashes[m] < h) l = m + 1;
        else r = m;
    }
    uint32_t u = l, r2 = e;
    while (u < r2) {  // first > h
        const uint32_t m = (u + r2) >> 1;
        if (hashes[m] <= h) u = m + 1;
        else r2 = m;
    }
    lo = l;
    len = u - l;
}

// ---------------------------------------------------------------- rebuild

// postings sorted by (hash, t, ordinal): a head is a new (key, ordinal) -- duplicates of one record are dropped
struct LmHead {
    const uint64_t* keys;
    const uint32_t* ords;
    __device__ bool operator()(size_t i) const { return i == 0 || keys[i] != keys[i - 1] || ords[i] != ords[i - 1]; }
};

struct LmEmit {
    const uint64_t* keys;
    const uint32_t* ords;
    uint32_t* hashes;
    uint64_t* entries;
    __device__ void operator()(size_t i, uint64_t o) const {
        const uint64_t key = keys[i];
        hashes[o] = (uint32_t)(key >> 32);
        entries[o] = (uint64_t)ords[i] | ((key & 0xffffffffull) << 32);
    }
};

// ---------------------------------------------------------------- query

// one block: offsets (bytes) -> landmark offsets; info[0] = landmarks in the batch; err |= 1 on a bad offset
__global__ void lm_qprep(const uint64_t* __restrict__ off, size_t nq, uint64_t* __restrict__ loff,
                         uint64_t* __restrict__ info, uint32_t* __restrict__ err) {
    bool bad = false;
    for (size_t i = threadIdx.x; i <= nq; i += kThreads) {
        const uint64_t o = off[i];
        loff[i] = o >> 3;
        bad |= (o & 7) != 0;
        if (i == 0) bad |= o != 0;
        else bad |= o < off[i - 1];
    }
    if (bad) atomicOr(err, 1u);
    if (threadIdx.x == 0) info[0] = off[nq] >> 3;
}

__global__ void lm_qkeys(const uint32_t* __restrict__ lm, size_t n, uint64_t* __restrict__ keys, uint32_t* __restrict__ err) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = lm[2 * i], t = lm[2 * i + 1];
    if (t >= kBias) atomicOr(err, 2u);
    keys[i] = ((uint64_t)h << 32) | t;
}

// one block per query: duplicates and stopped hashes get an empty run; qn[q] = |Q|, votes[q] = V
__global__ __launch_bounds__(kThreads) void lm_qruns(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ loff,
                                                      const uint32_t* __restrict__ hashes, const uint32_t* __restrict__ dir,
                                                      uint32_t max_postings, uint32_t* __restrict__ run_lo,
                                                      uint32_t* __restrict__ run_len, uint32_t* __restrict__ qn,
                                                      uint64_t* __restrict__ votes) {
    __shared__ uint64_t s_w[4];
    const uint32_t q = blockIdx.x;
    const uint64_t a = loff[q], e = loff[q + 1];
    uint64_t nq_local = 0, v_local = 0;
    for (uint64_t i = a + threadIdx.x; i < e; i += kThreads) {
        const uint64_t key = keys[i];
        const bool dup = i > a && keys[i - 1] == key;
        uint32_t lo = 0, len = 0;
        if (!dup) {
            nq_local++;
            find_run(hashes, dir, (uint32_t)(key >> 32), lo, len);
            if (max_postings && len > max_postings) len = 0;
        }
        run_lo[i] = lo;
        run_len[i] = len;
        v_local += len;
    }
    const uint64_t tq = block_scan_incl(nq_local, s_w);
    const uint64_t tv = block_scan_incl(v_local, s_w);
    if (threadIdx.x == kThreads - 1) {
        qn[q] = (uint32_t)tq;
        votes[q] = tv;
    }
}

__device__ __forceinline__ uint32_t slot64(uint64_t key) {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 52);   // 12 bits: kSlots = 4096
}
__device__ __forceinline__ uint32_t slot32(uint32_t ord) { return (ord * 0x9E3779B1u) >> 20; }

// one block per query
__global__ __launch_bounds__(kThreads) void lm_vote(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ loff,
                                                     const uint32_t* __restrict__ run_lo,
                                                     const uint32_t* __restrict__ run_len, const uint32_t* __restrict__ qn,
                                                     const uint64_t* __restrict__ votes,
                                                     const uint64_t* __restrict__ spill_base,
                                                     const uint64_t* __restrict__ entries, const uint64_t* __restrict__ ids,
                                                     uint32_t k, uint32_t min_votes, uint64_t* __restrict__ spill,
                                                     uint64_t* __restrict__ out_ids, uint32_t* __restrict__ out_votes,
                                                     int32_t* __restrict__ out_offsets, float* __restrict__ out_scores,
                                                     uint32_t* __restrict__ out_n) {
    __shared__ uint64_t s_tab[kSlots + kSlots / 2];   // 48 KiB, three views below
    __shared__ uint64_t s_inc[kThreads];
    __shared__ uint32_t s_lo[kThreads], s_tq[kThreads];
    __shared__ uint64_t s_w[4];
    __shared__ uint32_t s_cnt;
    const uint32_t q = blockIdx.x;
    const uint64_t base = spill_base[q];
    const bool spilling = base != kNoSpill;
    if (!spilling && votes[q] == 0) {
        write_hits(nullptr, nullptr, 0, q, k, 1, ids, out_ids, out_votes, out_offsets, out_scores, out_n);
        return;
    }
    uint64_t* t1_key = s_tab;                                  // phase 1: (ordinal, offset) -> count
    uint32_t* t1_cnt = reinterpret_cast<uint32_t*>(s_tab + kSlots);
    if (!spilling) {
        for (uint32_t s = threadIdx.x; s < kSlots; s += kThreads) {
            t1_key[s] = kEmpty64;
            t1_cnt[s] = 0;
        }
    }
    __syncthreads();
    const uint64_t a = loff[q], e = loff[q + 1];
    uint64_t done = 0;
    for (uint64_t c = a; c < e; c += kThreads) {
        const uint64_t l = c + threadIdx.x;
        const uint32_t len = l < e ? run_len[l] : 0u;
        const uint64_t inc = block_scan_incl(len, s_w);
        s_inc[threadIdx.x] = inc;
        s_lo[threadIdx.x] = l < e ? run_lo[l] : 0u;
        s_tq[threadIdx.x] = l < e ? (uint32_t)keys[l] : 0u;
        __syncthreads();
        const uint64_t total = s_inc[kThreads - 1];
        for (uint64_t j = threadIdx.x; j < total; j += kThreads) {
            uint32_t lo = 0, hi = kThreads - 1;   // first m with s_inc[m] > j
            while (lo < hi) {
                const uint32_t m = (lo + hi) >> 1;
                if (s_inc[m] > j) hi = m;
                else lo = m + 1;
            }
            const uint64_t excl = lo ? s_inc[lo - 1] : 0;
            const uint64_t ent = entries[s_lo[lo] + (j - excl)];
            const uint32_t ord = (uint32_t)ent, tr = (uint32_t)(ent >> 32);
            const uint64_t key = ((uint64_t)ord << 32) | (uint32_t)(tr - s_tq[lo] + kBias);
            if (spilling) {
                spill[base + done + j] = key;
            } else {
                uint32_t s = slot64(key);
                for (;;) {   // at most kLdsVotes distinct keys: a free slot always exists
                    const uint64_t prev = atomicCAS((unsigned long long*)&t1_key[s], (unsigned long long)kEmpty64,
                                                    (unsigned long long)key);
                    if (prev == kEmpty64 || prev == key) {
                        atomicAdd(&t1_cnt[s], 1u);
                        break;
                    }
                    s = (s + 1) & (kSlots - 1);
                }
            }
        }
        done += total;
        __syncthreads();
    }
    if (spilling) return;
    // phase 2: per ordinal the best (count, smallest offset)
    uint64_t rk[kSlotsPerThread];
    uint32_t rc[kSlotsPerThread];
#pragma unroll
    for (uint32_t j = 0; j < kSlotsPerThread; j++) {
        rk[j] = t1_key[threadIdx.x + j * kThreads];
        rc[j] = t1_cnt[threadIdx.x + j * kThreads];
    }
    __syncthreads();
    uint32_t* t2_ord = reinterpret_cast<uint32_t*>(s_tab);     // bytes [0, 16 KiB)
    uint64_t* t2_val = s_tab + kSlots / 2;                     // bytes [16, 48 KiB)
    for (uint32_t s = threadIdx.x; s < kSlots; s += kThreads) {
        t2_ord[s] = kEmpty32;
        t2_val[s] = 0;
    }
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kSlotsPerThread; j++) {
        if (rk[j] == kEmpty64) continue;
        const uint32_t ord = (uint32_t)(rk[j] >> 32);
        uint32_t s = slot32(ord);
        for (;;) {
            const uint32_t prev = atomicCAS(&t2_ord[s], kEmpty32, ord);
            if (prev == kEmpty32 || prev == ord) {
                atomicMax((unsigned long long*)&t2_val[s], (unsigned long long)best_val(rc[j], (uint32_t)rk[j]));
                break;
            }
            s = (s + 1) & (kSlots - 1);
        }
    }
    __syncthreads();
    // phase 3: the qualifying ordinals, packed to the front, then sorted
    const uint32_t minv = min_votes > 1 ? min_votes : 1u;
#pragma unroll
    for (uint32_t j = 0; j < kSlotsPerThread; j++) {
        const uint32_t s = threadIdx.x + j * kThreads;
        rc[j] = t2_ord[s];
        rk[j] = t2_val[s];
    }
    __syncthreads();
    uint64_t* s_key = s_tab;                                   // bytes [0, 32 KiB)
    uint32_t* s_db = reinterpret_cast<uint32_t*>(s_tab + kSlots);
#pragma unroll
    for (uint32_t j = 0; j < kSlotsPerThread; j++) {
        const uint32_t cnt = (uint32_t)(rk[j] >> 32);
        if (rc[j] != kEmpty32 && cnt >= minv) {
            const uint32_t p = atomicAdd(&s_cnt, 1u);
            s_key[p] = cand_key(cnt, rc[j]);
            s_db[p] = 0xffffffffu - (uint32_t)rk[j];
        }
    }
    __syncthreads();
    const uint32_t nc = s_cnt;
    uint32_t n = 1;
    while (n < nc) n <<= 1;
    for (uint32_t i = nc + threadIdx.x; i < n; i += kThreads) s_key[i] = kEmpty64;
    __syncthreads();
    bitonic_sort(s_key, n, s_db);
    write_hits(s_key, s_db, n, q, k, qn[q], ids, out_ids, out_votes, out_offsets, out_scores, out_n);
}

// one block per spilled query s: sorted votes spill[soff[s] .. soff[s+1])
__global__ __launch_bounds__(kThreads) void lm_spill_best(const uint64_t* __restrict__ spill, const uint64_t* __restrict__ soff,
                                                           uint32_t n_ord, uint64_t* __restrict__ best) {
    const uint32_t s = blockIdx.x;
    const uint64_t a = soff[s], e = soff[s + 1];
    uint64_t* row = best + (size_t)s * n_ord;
    for (uint64_t i = a + threadIdx.x; i < e; i += kThreads) {
        const uint64_t key = spill[i];
        if (i + 1 < e && spill[i + 1] == key) continue;   // not the end of its run
        uint64_t l = a, r = i;                            // run start: first index with spill[] == key
        while (l < r) {
            const uint64_t m = (l + r) >> 1;
            if (spill[m] < key) l = m + 1;
            else r = m;
        }
        atomicMax((unsigned long long*)&row[(uint32_t)(key >> 32)],
                  (unsigned long long)best_val((uint32_t)(i - l + 1), (uint32_t)key));
    }
}

__global__ __launch_bounds__(kThreads) void lm_spill_topk(const uint64_t* __restrict__ best, const uint32_t* __restrict__ spill_q,
                                                           uint32_t n_ord, const uint32_t* __restrict__ qn,
                                                           const uint64_t* __restrict__ ids, uint32_t k, uint32_t min_votes,
                                                           uint64_t* __restrict__ out_ids, uint32_t* __restrict__ out_votes,
                                                           int32_t* __restrict__ out_offsets, float* __restrict__ out_scores,
                                                           uint32_t* __restrict__ out_n) {
    __shared__ uint64_t s_key[2 * kThreads];
    __shared__ uint32_t s_db[2 * kThreads];
    const uint32_t s = blockIdx.x;
    const uint64_t* row = best + (size_t)s * n_ord;
    const uint32_t minv = min_votes > 1 ? min_votes : 1u;
    for (uint32_t i = threadIdx.x; i < 2 * kThreads; i += kThreads) {
        s_key[i] = kEmpty64;
        s_db[i] = 0;
    }
    __syncthreads();
    for (uint32_t b = 0; b < n_ord; b += kThreads) {
        const uint32_t o = b + threadIdx.x;
        const uint64_t v = o < n_ord ? row[o] : 0;
        const uint32_t cnt = (uint32_t)(v >> 32);
        topk_offer(s_key, k, cnt >= minv ? cand_key(cnt, o) : kEmpty64, s_db, 0xffffffffu - (uint32_t)v);
    }
    const uint32_t q = spill_q[s];
    write_hits(s_key, s_db, k, q, k, qn[q], ids, out_ids, out_votes, out_offsets, out_scores, out_n);
}

// empty answers for every query (unknown tenant / empty index)
__global__ void lm_empty(size_t nq, uint32_t k, uint64_t* __restrict__ out_ids, uint32_t* __restrict__ out_votes,
                         int32_t* __restrict__ out_offsets, float* __restrict__ out_scores, uint32_t* __restrict__ out_n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq * k) {
        out_ids[i] = kEmpty64;
        out_votes[i] = 0;
        out_offsets[i] = 0;
        out_scores[i] = -1.0f;
    }
    if (i < nq) out_n[i] = 0;
}

struct Tenant {
    std::map<uint64_t, std::vector<uint64_t>> recs;   // id -> landmarks as hash << 32 | t (ascending id = ordinal order)
    bool dirty = true;
    size_t postings = 0;                              // deduplicated, valid when !dirty
    DevArr hashes, entries, dir, ids;
};

}  // namespace

struct ucfp_landmark_index : ucfp::IndexCore {
    uint32_t max_postings = 0;
    std::unordered_map<uint32_t, Tenant> tenants;
    // rebuild workspace
    DevArr b_keys_a, b_keys_b, b_ords_a, b_ords_b, b_cnt, b_off, b_tmp;
    // query workspace
    DevArr q_lm, q_off, q_loff, q_info, q_keys_a, q_keys_b, q_tmp, q_lo, q_len, q_qn, q_votes, q_sbase, q_soff, q_sq,
        q_spill_a, q_spill_b, q_best, q_out;
    std::vector<uint64_t> h_votes, h_sbase, h_soff;
    std::vector<uint32_t> h_sq;
};

namespace {

int check_batch_host(const uint8_t* landmarks, const uint64_t* offsets, size_t n) {
    if (n && !offsets) return capi_fail(UCFP_E_INVALID, "offsets is NULL");
    if (!n) return UCFP_OK;
    if (offsets[0] != 0) return capi_fail(UCFP_E_INVALID, "offsets[0] must be 0");
    for (size_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i]) return capi_fail(UCFP_E_INVALID, "offsets decrease at %zu", i);
        if (offsets[i + 1] & 7) return capi_fail(UCFP_E_INVALID, "landmark bytes of item %zu are not a multiple of 8", i);
    }
    if (offsets[n] && !landmarks) return capi_fail(UCFP_E_INVALID, "landmarks is NULL");
    const size_t m = offsets[n] / 8;
    for (size_t i = 0; i < m; i++) {
        uint32_t t;
        memcpy(&t, landmarks + 8 * i + 4, 4);
        if (t >= kBias) return capi_fail(UCFP_E_INVALID, "landmark %zu has t = %u >= 2^31", i, t);
    }
    return UCFP_OK;
}

int rebuild(ucfp_landmark_index* ix, Tenant& T, hipStream_t st) {
    size_t n = 0;
    for (auto& kv : T.recs) n += kv.second.size();
    if (T.recs.size() >= 0xffffffffull) return capi_fail(UCFP_E_INVALID, "too many records in one tenant");
    if (n >= 0xffffffffull) return capi_fail(UCFP_E_INVALID, "too many landmarks in one tenant (%zu)", n);
    std::vector<uint64_t> h_keys(n), h_ids(T.recs.size());
    std::vector<uint32_t> h_ords(n);
    size_t o = 0;
    uint32_t ord = 0;
    for (auto& kv : T.recs) {
        h_ids[ord] = kv.first;
        memcpy(h_keys.data() + o, kv.second.data(), kv.second.size() * 8);
        std::fill(h_ords.begin() + o, h_ords.begin() + o + kv.second.size(), ord);
        o += kv.second.size();
        ord++;
    }
    int rc;
    if ((rc = T.ids.ensure(h_ids.size() * 8)) || (rc = T.dir.ensure((kDirSize + 1) * 4))) return rc;
    if (!h_ids.empty()) HIP_TRY(hipMemcpyAsync(T.ids.p, h_ids.data(), h_ids.size() * 8, hipMemcpyHostToDevice, st));
    size_t p = 0;
    if (n) {
        if ((rc = ix->b_keys_a.ensure(n * 8)) || (rc = ix->b_keys_b.ensure(n * 8)) || (rc = ix->b_ords_a.ensure(n * 4)) ||
            (rc = ix->b_ords_b.ensure(n * 4)))
            return rc;
        HIP_TRY(hipMemcpyAsync(ix->b_keys_a.p, h_keys.data(), n * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ix->b_ords_a.p, h_ords.data(), n * 4, hipMemcpyHostToDevice, st));
        // stable: equal (hash, t) keep ascending ordinals, so duplicates of one record are adjacent
        uint64_t* keys = ix->b_keys_b.as<uint64_t>();
        uint32_t* ords = ix->b_ords_b.as<uint32_t>();
        const LmHead head{keys, ords};
        if ((rc = sort_pairs(ix->b_tmp, ix->b_keys_a.as<uint64_t>(), keys, ix->b_ords_a.as<uint32_t>(), ords, n, 64, st)) ||
            (rc = count_heads(head, n, ix->b_cnt, ix->b_off, st, &p)) || (rc = T.hashes.ensure(p * 4)) ||
            (rc = T.entries.ensure(p * 8)) ||
            (rc = compact_heads(head, LmEmit{keys, ords, T.hashes.as<uint32_t>(), T.entries.as<uint64_t>()}, n, ix->b_off,
                                st)))
            return rc;
    } else if ((rc = T.hashes.ensure(0)) || (rc = T.entries.ensure(0))) {
        return rc;
    }
    if ((rc = build_directory(T.hashes.as<uint32_t>(), p, kDirBits, kDirSize, T.dir.as<uint32_t>(), st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));   // the host vectors above go out of scope
    T.postings = p;
    T.dirty = false;
    return UCFP_OK;
}

int do_upsert(ucfp_landmark_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* landmarks,
              const uint64_t* offsets, size_t n) {
    int rc = check_batch_host(landmarks, offsets, n);
    if (rc) return rc;
    if (n && !ids) return capi_fail(UCFP_E_INVALID, "ids is NULL");
    if (!n) return UCFP_OK;
    Tenant& T = ix->tenants[tenant];
    for (size_t i = 0; i < n; i++) {
        const size_t a = offsets[i] / 8, m = (offsets[i + 1] - offsets[i]) / 8;
        std::vector<uint64_t>& v = T.recs[ids[i]];
        v.resize(m);
        for (size_t j = 0; j < m; j++) {
            uint32_t ht[2];
            memcpy(ht, landmarks + 8 * (a + j), 8);
            v[j] = ((uint64_t)ht[0] << 32) | ht[1];
        }
    }
    T.dirty = true;
    return UCFP_OK;
}

int query_impl(ucfp_landmark_index* ix, uint32_t tenant, const uint8_t* d_lm, const uint64_t* d_off, size_t nq, uint32_t k,
               uint32_t min_votes, uint64_t* d_ids, uint32_t* d_votes, int32_t* d_offs, float* d_scores, uint32_t* d_n,
               hipStream_t st) {
    int rc;
    // 1. offsets and t < 2^31 (checked before anything else, whatever the tenant or k)
    if ((rc = ix->q_loff.ensure((nq + 1) * 8)) || (rc = ix->q_info.ensure(16))) return rc;
    HIP_TRY(hipMemsetAsync(ix->q_info.p, 0, 16, st));
    uint32_t* d_err = reinterpret_cast<uint32_t*>(ix->q_info.as<uint64_t>() + 1);
    hipLaunchKernelGGL(lm_qprep, dim3(1), dim3(kThreads), 0, st, d_off, nq, ix->q_loff.as<uint64_t>(),
                       ix->q_info.as<uint64_t>(), d_err);
    HIP_TRY(hipGetLastError());
    uint64_t info[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(info, ix->q_info.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (info[1]) return capi_fail(UCFP_E_INVALID, "query offsets must start at 0, not decrease and be multiples of 8");
    const size_t total = (size_t)info[0];
    if (total && !d_lm) return capi_fail(UCFP_E_INVALID, "landmarks is NULL");
    if (total >= 0xffffffffull) return capi_fail(UCFP_E_INVALID, "too many query landmarks");
    if ((rc = ix->q_keys_a.ensure(total * 8)) || (rc = ix->q_keys_b.ensure(total * 8))) return rc;
    if (total) {
        hipLaunchKernelGGL(lm_qkeys, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const uint32_t*)d_lm, total,
                           ix->q_keys_a.as<uint64_t>(), d_err);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(info + 1, d_err, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (info[1]) return capi_fail(UCFP_E_INVALID, "a query landmark has t >= 2^31");
    }
    if (k == 0) {
        HIP_TRY(hipMemsetAsync(d_n, 0, nq * 4, st));
        return UCFP_OK;
    }
    auto it = ix->tenants.find(tenant);
    if (it == ix->tenants.end() || total == 0) {
        hipLaunchKernelGGL(lm_empty, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, st, nq, k, d_ids, d_votes, d_offs,
                           d_scores, d_n);
        HIP_TRY(hipGetLastError());
        return UCFP_OK;
    }
    Tenant& T = it->second;
    if (T.dirty && (rc = rebuild(ix, T, st))) return rc;
    // 2. sort each query, runs, |Q| and V
    const uint64_t* lo = ix->q_loff.as<uint64_t>();
    if ((rc = sort_segments(ix->q_tmp, ix->q_keys_a.as<uint64_t>(), ix->q_keys_b.as<uint64_t>(), total, nq, lo, st)))
        return rc;
    if ((rc = ix->q_lo.ensure(total * 4)) || (rc = ix->q_len.ensure(total * 4)) || (rc = ix->q_qn.ensure(nq * 4)) ||
        (rc = ix->q_votes.ensure(nq * 8)) || (rc = ix->q_sbase.ensure(nq * 8)))
        return rc;
    hipLaunchKernelGGL(lm_qruns, dim3((unsigned)nq), dim3(kThreads), 0, st, ix->q_keys_b.as<uint64_t>(), lo,
                       T.hashes.as<uint32_t>(), T.dir.as<uint32_t>(), ix->max_postings, ix->q_lo.as<uint32_t>(),
                       ix->q_len.as<uint32_t>(), ix->q_qn.as<uint32_t>(), ix->q_votes.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    ix->h_votes.resize(nq);
    HIP_TRY(hipMemcpyAsync(ix->h_votes.data(), ix->q_votes.p, nq * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // 3. which queries spill
    ix->h_sbase.assign(nq, kNoSpill);
    ix->h_soff.assign(1, 0);
    ix->h_sq.clear();
    for (size_t q = 0; q < nq; q++)
        if (ix->h_votes[q] > kLdsVotes) {
            ix->h_sbase[q] = ix->h_soff.back();
            ix->h_soff.push_back(ix->h_soff.back() + ix->h_votes[q]);
            ix->h_sq.push_back((uint32_t)q);
        }
    const size_t n_spill = ix->h_sq.size(), n_votes = ix->h_soff.back();
    const uint32_t n_ord = (uint32_t)T.recs.size();
    if (n_spill && n_votes >= 0xffffffffull) return capi_fail(UCFP_E_INVALID, "a query batch spills %zu votes", n_votes);
    HIP_TRY(hipMemcpyAsync(ix->q_sbase.p, ix->h_sbase.data(), nq * 8, hipMemcpyHostToDevice, st));
    if (n_spill) {
        if ((rc = ix->q_spill_a.ensure(n_votes * 8)) || (rc = ix->q_spill_b.ensure(n_votes * 8)) ||
            (rc = ix->q_soff.ensure((n_spill + 1) * 8)) || (rc = ix->q_sq.ensure(n_spill * 4)) ||
            (rc = ix->q_best.ensure(n_spill * n_ord * 8)))
            return rc;
        HIP_TRY(hipMemcpyAsync(ix->q_soff.p, ix->h_soff.data(), (n_spill + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ix->q_sq.p, ix->h_sq.data(), n_spill * 4, hipMemcpyHostToDevice, st));
    }
    // 4. votes: LDS tables, or the spill buffer
    hipLaunchKernelGGL(lm_vote, dim3((unsigned)nq), dim3(kThreads), 0, st, ix->q_keys_b.as<uint64_t>(), lo,
                       ix->q_lo.as<uint32_t>(), ix->q_len.as<uint32_t>(), ix->q_qn.as<uint32_t>(),
                       ix->q_votes.as<uint64_t>(), ix->q_sbase.as<uint64_t>(), T.entries.as<uint64_t>(),
                       T.ids.as<uint64_t>(), k, min_votes, n_spill ? ix->q_spill_a.as<uint64_t>() : nullptr, d_ids, d_votes,
                       d_offs, d_scores, d_n);
    HIP_TRY(hipGetLastError());
    if (n_spill) {
        const uint64_t* so = ix->q_soff.as<uint64_t>();
        if ((rc = sort_segments(ix->q_tmp, ix->q_spill_a.as<uint64_t>(), ix->q_spill_b.as<uint64_t>(), n_votes, n_spill, so,
                                st)))
            return rc;
        HIP_TRY(hipMemsetAsync(ix->q_best.p, 0, n_spill * n_ord * 8, st));
        hipLaunchKernelGGL(lm_spill_best, dim3((unsigned)n_spill), dim3(kThreads), 0, st, ix->q_spill_b.as<uint64_t>(), so,
                           n_ord, ix->q_best.as<uint64_t>());
        hipLaunchKernelGGL(lm_spill_topk, dim3((unsigned)n_spill), dim3(kThreads), 0, st, ix->q_best.as<uint64_t>(),
                           ix->q_sq.as<uint32_t>(), n_ord, ix->q_qn.as<uint32_t>(), T.ids.as<uint64_t>(), k, min_votes,
                           d_ids, d_votes, d_offs, d_scores, d_n);
        HIP_TRY(hipGetLastError());
    }
    return UCFP_OK;
}

int query_args(ucfp_landmark_index* ix, const uint64_t* offsets, size_t nq, uint32_t k, const void* out_ids,
               const void* out_votes, const void* out_offsets, const void* out_scores, const void* out_n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (k > UCFP_INDEX_MAX_K) return capi_fail(UCFP_E_INVALID, "k = %u exceeds UCFP_INDEX_MAX_K = %u", k, UCFP_INDEX_MAX_K);
    if (nq > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "too many queries");
    if (nq && (!offsets || !out_n)) return capi_fail(UCFP_E_INVALID, "offsets/out_n is NULL");
    if (nq && k && (!out_ids || !out_votes || !out_offsets || !out_scores))
        return capi_fail(UCFP_E_INVALID, "an output buffer is NULL");
    return UCFP_OK;
}

}  // namespace

extern "C" {

int ucfp_landmark_index_create(ucfp_ctx* ctx, uint32_t max_postings, uint32_t flags, ucfp_landmark_index** out) {
    if (!ctx || !out) return capi_fail(UCFP_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (flags != 0) return capi_fail(UCFP_E_INVALID, "no landmark index flags are defined (got %u)", flags);
    const int rc = ucfp::create_index(ctx, "landmark index", out);
    if (!rc) (*out)->max_postings = max_postings;
    return rc;
}

void ucfp_landmark_index_destroy(ucfp_landmark_index* ix) {
    if (!ix) return;
    ix->quiesce();
    for (auto& kv : ix->tenants)
        for (DevArr* a : {&kv.second.hashes, &kv.second.entries, &kv.second.dir, &kv.second.ids}) a->release();
    for (DevArr* a : {&ix->b_keys_a, &ix->b_keys_b, &ix->b_ords_a, &ix->b_ords_b, &ix->b_cnt, &ix->b_off, &ix->b_tmp,
                      &ix->q_lm, &ix->q_off, &ix->q_loff, &ix->q_info, &ix->q_keys_a, &ix->q_keys_b, &ix->q_tmp, &ix->q_lo,
                      &ix->q_len, &ix->q_qn, &ix->q_votes, &ix->q_sbase, &ix->q_soff, &ix->q_sq, &ix->q_spill_a,
                      &ix->q_spill_b, &ix->q_best, &ix->q_out})
        a->release();
    delete ix;
}

int ucfp_landmark_index_upsert(ucfp_landmark_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* landmarks,
                               const uint64_t* offsets, size_t n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    return do_upsert(ix, tenant, ids, landmarks, offsets, n);
}

int ucfp_landmark_index_upsert_dev(ucfp_landmark_index* ix, uint32_t tenant, const uint64_t* d_ids,
                                   const uint8_t* d_landmarks, const uint64_t* d_offsets, size_t n, void* stream) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (!n) return UCFP_OK;
    if (!d_ids || !d_offsets) return capi_fail(UCFP_E_INVALID, "ids/offsets is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    // the record table lives on the host (mutations are bookkeeping; the postings are rebuilt at the next query)
    std::vector<uint64_t> ids(n), offs(n + 1);
    HIP_TRY(hipMemcpyAsync(ids.data(), d_ids, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(offs.data(), d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (offs[0] != 0 || offs[n] < offs[0]) return capi_fail(UCFP_E_INVALID, "offsets must start at 0 and not decrease");
    std::vector<uint8_t> lm(offs[n]);
    if (offs[n]) {
        if (!d_landmarks) return capi_fail(UCFP_E_INVALID, "landmarks is NULL");
        HIP_TRY(hipMemcpyAsync(lm.data(), d_landmarks, offs[n], hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return do_upsert(ix, tenant, ids.data(), lm.data(), offs.data(), n);
}

int ucfp_landmark_index_delete(ucfp_landmark_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed) {
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

int ucfp_landmark_index_size(ucfp_landmark_index* ix, uint32_t tenant, size_t* records, size_t* postings) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    size_t r = 0, p = 0;
    auto it = ix->tenants.find(tenant);
    if (it != ix->tenants.end()) {
        Tenant& T = it->second;
        if (T.dirty) {
            int rc = ix->begin();
            if (rc || (rc = rebuild(ix, T, ix->own)) || (rc = ix->end(ix->own))) return rc;
        }
        r = T.recs.size();
        p = T.postings;
    }
    if (records) *records = r;
    if (postings) *postings = p;
    return UCFP_OK;
}

int ucfp_landmark_index_flush(ucfp_landmark_index* ix) { return ucfp::flush_dirty(ix, rebuild); }

int ucfp_landmark_index_query_dev(ucfp_landmark_index* ix, uint32_t tenant, const uint8_t* d_landmarks,
                                  const uint64_t* d_offsets, size_t nq, uint32_t k, uint32_t min_votes, uint64_t* d_out_ids,
                                  uint32_t* d_out_votes, int32_t* d_out_offsets, float* d_out_scores, uint32_t* d_out_n,
                                  void* stream) {
    int rc = query_args(ix, d_offsets, nq, k, d_out_ids, d_out_votes, d_out_offsets, d_out_scores, d_out_n);
    if (rc || nq == 0) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    if ((rc = ix->begin())) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = query_impl(ix, tenant, d_landmarks, d_offsets, nq, k, min_votes, d_out_ids, d_out_votes, d_out_offsets,
                    d_out_scores, d_out_n, st);
    return ix->end(st, rc);
}

int ucfp_landmark_index_query(ucfp_landmark_index* ix, uint32_t tenant, const uint8_t* landmarks, const uint64_t* offsets,
                              size_t nq, uint32_t k, uint32_t min_votes, uint64_t* out_ids, uint32_t* out_votes,
                              int32_t* out_offsets, float* out_scores, uint32_t* out_n) {
    int rc = query_args(ix, offsets, nq, k, out_ids, out_votes, out_offsets, out_scores, out_n);
    if (rc || nq == 0) return rc;
    if ((rc = check_batch_host(landmarks, offsets, nq))) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    if ((rc = ix->begin())) return rc;
    hipStream_t st = ix->own;
    const size_t bytes = offsets[nq], nk = nq * k;
    const size_t o_votes = nk * 8, o_offs = o_votes + nk * 4, o_sc = o_offs + nk * 4, o_n = o_sc + nk * 4;
    if ((rc = ix->q_lm.ensure(bytes)) || (rc = ix->q_off.ensure((nq + 1) * 8)) || (rc = ix->q_out.ensure(o_n + nq * 4)))
        return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(ix->q_lm.p, landmarks, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ix->q_off.p, offsets, (nq + 1) * 8, hipMemcpyHostToDevice, st));
    uint8_t* ob = ix->q_out.as<uint8_t>();
    rc = query_impl(ix, tenant, ix->q_lm.as<uint8_t>(), ix->q_off.as<uint64_t>(), nq, k, min_votes, (uint64_t*)ob,
                    (uint32_t*)(ob + o_votes), (int32_t*)(ob + o_offs), (float*)(ob + o_sc), (uint32_t*)(ob + o_n), st);
    if (rc) return ix->end_sync(rc);
    if (nk) {
        HIP_TRY(hipMemcpyAsync(out_ids, ob, nk * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_votes, ob + o_votes, nk * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_offsets, ob + o_offs, nk * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_scores, ob + o_sc, nk * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(out_n, ob + o_n, nq * 4, hipMemcpyDeviceToHost, st));
    return ix->end_sync(UCFP_OK);
}

}  // extern "C"
