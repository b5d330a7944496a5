// haitsma_index.hip -- GPU index over Haitsma-Kalker sub-fingerprints: "which recording is this clip,
// and where in it?", by bit-error rate over the whole query block.
//
// Spec (ours; the reference has no audio matcher):
//   F_r[0 .. n_r)   the u32 sub-fingerprints of record r (the bytes of an audiofp-haitsma-v1 record), Q[0 .. m) a query
//   P(v)            positions (r, t) with F_r[t] == v over the live records of the tenant; v is stopped if
//                   max_postings > 0 and P(v) > max_postings
//   (r, d) is admissible iff 0 <= d and d + m <= n_r; a candidate iff additionally some j < m has
//                   popcount(F_r[d + j] ^ Q[j]) <= flip_bits with F_r[d + j] not stopped
//   dist(r, d) = sum_j popcount(F_r[d + j] ^ Q[j]); dist(r) = min over the candidates of r, offset(r) = the smallest d
//                   attaining it; hits: dist(r) * 10^6 <= max_ber_ppm * 32 * m, (dist asc, id asc), first k;
//                   score = 1.0f - (float)dist / (float)(32 * m)
//
// Layout of a tenant after a (lazy) rebuild: the frames of all live records flat in ordinal order (frames u32 [N]),
// start u64 [R + 1], ids u64 [R] with ordinals following ascending record id, and the postings as two arrays sorted by
// (value, position) -- vals u32 [N], pos u32 [N] -- by postings.h's sort_pairs (stable, positions fed ascending), plus
// build_directory on value >> 12.  Positions are distinct, so nothing is compacted and P(v) is a run length.
//
// Query (one launch sequence for a ragged batch):
//   hx_qprep    check the offsets and m <= UCFP_HAITSMA_MAX_QUERY_FRAMES; total and largest m (one read-back)
// then, in passes of at most kPassQueries queries:
//   hx_count    every (query frame, probe mask): the value's run through the directory, the stop cap; seeds per query
//               (positions found; admissibility is decided later), the first kLdsSeeds of them written down as
//               (position, j).  Read back once per pass.
// A query with at most kLdsSeeds seeds is answered by one block:
//   hx_small    the query block in LDS; each written seed's record by binary search in `start`, the admissible ones
//               (ordinal << 32 | d) into an LDS hash set (a clean clip seeds its true alignment up to m times: the set
//               holds it once); the set is packed and sorted (bitonic_sort), verified as below with the sums folded into
//               an LDS array, and the ordinals' best go through topk_offer.
// The others go through global memory, in slices of queries whose seeds fit the workspace:
//   hx_emit     the same probes; each wave walks its non-empty runs together (64 positions at a time), finds the
//               record of each position in `start`, and appends (ordinal << 32 | d) for admissible alignments
//   rocPRIM     segmented radix sort of the seeds per query: equal alignments become adjacent, ordinals ascend
//   hx_verify   the query block in LDS, blocks striding over the query's sorted seeds
//   hx_topk     one block per query: the ordinals' best (dist, d) under the threshold go through topk_offer by
//               (dist, ordinal); ids / dist / offsets / scores / counts
// Verification (verify_group) is the hot loop of both: one wave per candidate (the first of each run of equal keys;
// the others leave at once), four candidates in flight per wave: m consecutive u32 of `frames` per candidate, XOR with
// the query block, popcount, wave reduction; the sum is folded with an atomic minimum into the place of the first seed
// of the candidate's ordinal (found by binary search: the keys are sorted).  Both paths take the minimum over the same
// set of candidates and order by the same keys, so they give the same answer.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <unordered_map>
#include <vector>

#include "postings.h"

namespace {

constexpr uint32_t kDirShift = 12;                 // directory on value >> 12
constexpr uint32_t kDirSize = 1u << 20;
constexpr uint32_t kMaxM = UCFP_HAITSMA_MAX_QUERY_FRAMES;
constexpr uint64_t kSliceSeeds = 1ull << 25;       // seeds per slice of queries (three u64 arrays: 768 MiB)
constexpr uint32_t kInFlight = 4;                  // candidates per wave at a time
constexpr uint32_t kSlots = 4096;                  // LDS seed set of hx_small (32 KiB)
constexpr uint32_t kSlotsPerThread = kSlots / kThreads;
constexpr uint32_t kLdsSeeds = 3072;               // at most 75 % load: a query with more seeds takes the global path
constexpr size_t kPassQueries = 1024;              // queries per pass (their written seeds: 24 MiB)
constexpr uint32_t kVerifyStep = (kThreads / 64) * kInFlight;   // seeds per block and iteration

inline uint32_t probe_count(uint32_t flip_bits) { return flip_bits == 0 ? 1u : flip_bits == 1 ? 33u : flip_bits == 2 ? 529u : 0u; }

// probe p of 529: 0 -> no flip, 1 .. 32 -> one bit, 33 .. 528 -> the pairs (a < b) in order of a, then b
__device__ __forceinline__ uint32_t probe_mask(uint32_t p) {
    if (p == 0) return 0u;
    if (p <= 32) return 1u << (p - 1);
    uint32_t x = p - 33, a = 0;
    while (x >= 31 - a) {
        x -= 31 - a;
        a++;
    }
    return (1u << a) | (1u << (a + 1 + x));
}

// the run of value v in the sorted postings; empty when stopped
__device__ __forceinline__ void find_run(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ dir, uint32_t v,
                                         uint32_t max_postings, uint32_t& lo, uint32_t& len) {
    const uint32_t b = v >> kDirShift;
    const uint32_t e = dir[b + 1];
    uint32_t l = dir[b], r = e;
    while (l < r) {   // first >= v
        const uint32_t m = (l + r) >> 1;
        if (vals[m] < v) l = m + 1;
        else r = m;
    }
    lo = l;
    len = 0;
    if (l == e || vals[l] != v) return;   // most probes end here
    uint64_t step = 1;                     // runs are short as a rule: gallop to the first > v, then bisect
    while (l + step < e && vals[l + step] == v) step <<= 1;
    uint32_t u = l + (uint32_t)(step >> 1) + 1, r2 = l + step < e ? (uint32_t)(l + step) : e;
    while (u < r2) {
        const uint32_t m = (u + r2) >> 1;
        if (vals[m] <= v) u = m + 1;
        else r2 = m;
    }
    len = u - l;
    if (max_postings && len > max_postings) len = 0;
}

// ---------------------------------------------------------------- rebuild

__global__ void hx_iota(uint32_t* __restrict__ p, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (uint32_t)i;
}

// ---------------------------------------------------------------- query

// one block: info[0] = frames in the batch, info[1] = largest m; err |= 1 on a bad offset, |= 2 on m > kMaxM
__global__ void hx_qprep(const uint64_t* __restrict__ off, size_t nq, unsigned long long* __restrict__ info,
                         uint32_t* __restrict__ err) {
    uint32_t bad = 0;
    unsigned long long mx = 0;
    for (size_t i = threadIdx.x; i <= nq; i += kThreads) {
        const uint64_t o = off[i];
        if (i == 0) {
            if (o != 0) bad |= 1u;
        } else {
            const uint64_t prev = off[i - 1];
            if (o < prev) bad |= 1u;
            else {
                if (o - prev > kMaxM) bad |= 2u;
                if (o - prev > mx) mx = o - prev;
            }
        }
    }
    if (bad) atomicOr(err, bad);
    if (mx) atomicMax(&info[1], mx);
    if (threadIdx.x == 0) info[0] = off[nq];
}

// gx blocks per query of the pass [q0, q0 + np): seeds[q] += the run lengths of the query's probes.  While a query's
// seeds fit the LDS path they are written down as position << 32 | j in small[(q - q0) * kLdsSeeds ..], so that hx_small
// does not probe again; a query that outgrows kLdsSeeds leaves its part of `small` unused.
__global__ __launch_bounds__(kThreads) void hx_count(const uint32_t* __restrict__ qf, const uint64_t* __restrict__ qoff,
                                                      uint32_t q0, uint32_t gx, const uint32_t* __restrict__ vals,
                                                      const uint32_t* __restrict__ pos, const uint32_t* __restrict__ dir,
                                                      uint32_t n_probes, uint32_t max_postings,
                                                      unsigned long long* __restrict__ seeds, uint64_t* __restrict__ small) {
    const uint32_t ql = blockIdx.x / gx, c = blockIdx.x % gx, q = q0 + ql;
    const uint64_t a = qoff[q];
    const uint32_t items = (uint32_t)(qoff[q + 1] - a) * n_probes;   // <= 4096 * 529
    uint64_t* mine = small + (size_t)ql * kLdsSeeds;
    for (uint32_t t = c * kThreads + threadIdx.x; t < items; t += gx * kThreads) {
        const uint32_t j = t / n_probes, p = t - j * n_probes;
        uint32_t lo, len;
        find_run(vals, dir, qf[a + j] ^ probe_mask(p), max_postings, lo, len);
        if (!len) continue;
        const unsigned long long at = atomicAdd(&seeds[q], (unsigned long long)len);
        if (at + len <= kLdsSeeds)
            for (uint32_t x = 0; x < len; x++) mine[at + x] = ((uint64_t)pos[lo + x] << 32) | j;
    }
}

// the record of flat position p: the last ordinal with start[ord] <= p (records without frames are stepped over)
__device__ __forceinline__ uint32_t ordinal_of(const uint64_t* __restrict__ start, uint32_t n_ord, uint32_t p) {
    uint32_t l = 0, r = n_ord;   // first index with start[] > p; start[n_ord] = N > p
    while (l < r) {
        const uint32_t m = (l + r) >> 1;
        if (start[m] > p) r = m;
        else l = m + 1;
    }
    return l - 1;
}

// the seed of flat position p matched at query frame j: admissible -> key = ordinal << 32 | d
__device__ __forceinline__ bool seed_key(const uint64_t* __restrict__ start, uint32_t n_ord, uint32_t p, uint32_t j, uint32_t m,
                                         uint64_t& key) {
    const uint32_t ord = ordinal_of(start, n_ord, p);
    const uint64_t s = start[ord], n_r = start[ord + 1] - s, t_r = p - s;
    if (t_r < j || t_r - j + m > n_r) return false;
    key = ((uint64_t)ord << 32) | (uint32_t)(t_r - j);
    return true;
}

// gx blocks per query of the slice qlist[0 .. ns): keys[soff[ql] + ...] = ordinal << 32 | d of the admissible seeds,
// cursor[ql] of them (<= the count of hx_count, which sized the segment)
__global__ __launch_bounds__(kThreads) void hx_emit(const uint32_t* __restrict__ qf, const uint64_t* __restrict__ qoff,
                                                     const uint32_t* __restrict__ qlist, uint32_t gx, const uint32_t* __restrict__ vals,
                                                     const uint32_t* __restrict__ pos, const uint32_t* __restrict__ dir,
                                                     const uint64_t* __restrict__ start, uint32_t n_ord, uint32_t n_probes,
                                                     uint32_t max_postings, const uint64_t* __restrict__ soff,
                                                     uint32_t* __restrict__ cursor, uint64_t* __restrict__ keys) {
    const uint32_t ql = blockIdx.x / gx, c = blockIdx.x % gx;
    const uint32_t q = qlist[ql];
    const uint64_t a = qoff[q];
    const uint32_t m = (uint32_t)(qoff[q + 1] - a);
    const uint32_t items = m * n_probes;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1;
    uint64_t* out = keys + soff[ql];
    // t0 is the wave's first item, so a wave stays together in the loop
    for (uint32_t t0 = c * kThreads + (threadIdx.x - lane); t0 < items; t0 += gx * kThreads) {
        const uint32_t t = t0 + lane;
        uint32_t lo = 0, len = 0, j = 0;
        if (t < items) {
            j = t / n_probes;
            find_run(vals, dir, qf[a + j] ^ probe_mask(t - j * n_probes), max_postings, lo, len);
        }
        uint64_t live = __ballot(len > 0);
        while (live) {
            const int src = __ffsll((unsigned long long)live) - 1;
            live &= live - 1;
            const uint32_t rlo = __shfl(lo, src, 64), rlen = __shfl(len, src, 64), rj = __shfl(j, src, 64);
            for (uint32_t x0 = 0; x0 < rlen; x0 += 64) {
                const uint32_t x = x0 + lane;
                bool ok = false;
                uint64_t key = 0;
                if (x < rlen) ok = seed_key(start, n_ord, pos[rlo + x], rj, m, key);
                const uint64_t b = __ballot(ok);
                if (b) {
                    const int first = __ffsll((unsigned long long)b) - 1;
                    uint32_t base = 0;
                    if ((int)lane == first) base = atomicAdd(&cursor[ql], (uint32_t)__popcll(b));
                    base = __shfl(base, first, 64);
                    if (ok) out[base + __popcll(b & below)] = key;
                }
            }
        }
    }
}

// The hot loop.  keys[a .. e) is sorted; the wave takes keys[i .. i + kInFlight): for each one that is the first of its
// run of equal keys, dist = sum_j popcount(frames[start[ord] + d + j] ^ s_q[j]), then lane 0 calls fold(first, idx, dist)
// with `first` the place of the first key of the same ordinal.
template <class Fold>
__device__ __forceinline__ void verify_group(const uint64_t* keys, uint64_t a, uint64_t e, uint64_t i, const uint32_t* s_q,
                                             uint32_t m, const uint32_t* __restrict__ frames,
                                             const uint64_t* __restrict__ start, uint32_t lane, Fold fold) {
    uint64_t key[kInFlight];
    const uint32_t* row[kInFlight];
    bool head[kInFlight];
    uint32_t acc[kInFlight];
#pragma unroll
    for (uint32_t u = 0; u < kInFlight; u++) {
        const uint64_t idx = i + u;
        key[u] = idx < e ? keys[idx] : kEmpty64;
        head[u] = idx < e && (idx == a || keys[idx - 1] != key[u]);
        row[u] = head[u] ? frames + start[key[u] >> 32] + (uint32_t)key[u] : frames;
        acc[u] = 0;
    }
    for (uint32_t j = lane; j < m; j += 64) {
        const uint32_t qv = s_q[j];
        uint32_t f[kInFlight];
#pragma unroll
        for (uint32_t u = 0; u < kInFlight; u++) f[u] = head[u] ? row[u][j] : qv;   // the loads first, then the sums
#pragma unroll
        for (uint32_t u = 0; u < kInFlight; u++) acc[u] += (uint32_t)__popc(f[u] ^ qv);
    }
#pragma unroll
    for (uint32_t u = 0; u < kInFlight; u++) {
        if (!head[u]) continue;   // uniform over the wave
        uint32_t v = acc[u];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) {
            const uint64_t ord = key[u] >> 32;
            uint64_t l = a, r = i + u;   // first key of this ordinal
            while (l < r) {
                const uint64_t mid = (l + r) >> 1;
                if ((keys[mid] >> 32) < ord) l = mid + 1;
                else r = mid;
            }
            fold(l, i + u, v);
        }
    }
}

// gx blocks per query of the slice; keys sorted per query, [soff[ql], soff[ql] + cursor[ql]) in use.  best[i] for the
// first seed i of an ordinal = min (dist << 32 | d) over the ordinal's candidates.
__global__ __launch_bounds__(kThreads) void hx_verify(const uint32_t* __restrict__ qf, const uint64_t* __restrict__ qoff,
                                                       const uint32_t* __restrict__ qlist, uint32_t gx,
                                                       const uint64_t* __restrict__ keys, const uint64_t* __restrict__ soff,
                                                       const uint32_t* __restrict__ cursor,
                                                       const uint32_t* __restrict__ frames, const uint64_t* __restrict__ start,
                                                       unsigned long long* __restrict__ best) {
    __shared__ uint32_t s_q[kMaxM];
    const uint32_t ql = blockIdx.x / gx, c = blockIdx.x % gx;
    const uint64_t a = soff[ql], e = a + cursor[ql];
    if (a + (uint64_t)c * kVerifyStep >= e) return;
    const uint32_t q = qlist[ql];
    const uint64_t qa = qoff[q];
    const uint32_t m = (uint32_t)(qoff[q + 1] - qa);
    for (uint32_t j = threadIdx.x; j < m; j += kThreads) s_q[j] = qf[qa + j];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t i = a + (uint64_t)c * kVerifyStep + wave * kInFlight; i < e; i += (uint64_t)gx * kVerifyStep)
        verify_group(keys, a, e, i, s_q, m, frames, start, lane, [&](uint64_t first, uint64_t idx, uint32_t dist) {
            atomicMin(&best[first], ((unsigned long long)dist << 32) | (uint32_t)keys[idx]);
        });
}

// s_key / s_d = the block's top-k by (dist << 32 | ordinal) with d: one block writes query q's k results
__device__ void write_hits(const uint64_t* s_key, const uint32_t* s_d, uint32_t q, uint32_t k, uint64_t bits,
                           const uint64_t* __restrict__ ids, uint64_t* __restrict__ out_ids, uint32_t* __restrict__ out_dist,
                           int32_t* __restrict__ out_offsets, float* __restrict__ out_scores, uint32_t* __restrict__ out_n) {
    const uint32_t j = threadIdx.x;   // k <= UCFP_INDEX_MAX_K < kThreads
    const uint64_t sk = j < k ? s_key[j] : kEmpty64;
    const bool valid = sk != kEmpty64;
    if (j < k) {
        const size_t o = (size_t)q * k + j;
        const uint32_t dist = (uint32_t)(sk >> 32);
        out_ids[o] = valid ? ids[(uint32_t)sk] : kEmpty64;
        out_dist[o] = valid ? dist : kEmpty32;
        out_offsets[o] = valid ? (int32_t)s_d[j] : 0;
        out_scores[o] = valid ? 1.0f - (float)dist / (float)bits : -1.0f;
    }
    const int cnt = __syncthreads_count(valid);
    if (threadIdx.x == 0) out_n[q] = (uint32_t)cnt;
}

__device__ __forceinline__ uint32_t slot64(uint64_t key) {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 52);   // 12 bits: kSlots = 4096
}

// one block per query of qlist: at most kLdsSeeds seeds, so the set of distinct ones fits the LDS table
__global__ __launch_bounds__(kThreads) void hx_small(const uint32_t* __restrict__ qf, const uint64_t* __restrict__ qoff,
                                                      const uint32_t* __restrict__ qlist,
                                                      uint32_t q0, const unsigned long long* __restrict__ seeds,
                                                      const uint64_t* __restrict__ small,
                                                      const uint64_t* __restrict__ start, uint32_t n_ord,
                                                      const uint32_t* __restrict__ frames, const uint64_t* __restrict__ ids,
                                                      uint32_t k, uint32_t max_ber_ppm, uint64_t* __restrict__ out_ids,
                                                      uint32_t* __restrict__ out_dist, int32_t* __restrict__ out_offsets,
                                                      float* __restrict__ out_scores, uint32_t* __restrict__ out_n) {
    __shared__ __attribute__((aligned(8))) uint32_t s_q[kMaxM];   // 16 KiB; the top-k lists once the sums are done
    __shared__ uint64_t s_tab[kSlots];       // 32 KiB: the seed set, then the sorted candidates
    __shared__ uint32_t s_best[kLdsSeeds];   // 12 KiB: per first candidate of an ordinal, min (dist << 12 | place in the run)
    __shared__ uint64_t s_w[4];
    const uint32_t q = qlist[blockIdx.x];
    const uint64_t qa = qoff[q];
    const uint32_t m = (uint32_t)(qoff[q + 1] - qa);
    for (uint32_t j = threadIdx.x; j < m; j += kThreads) s_q[j] = qf[qa + j];
    for (uint32_t i = threadIdx.x; i < kSlots; i += kThreads) s_tab[i] = kEmpty64;
    for (uint32_t i = threadIdx.x; i < kLdsSeeds; i += kThreads) s_best[i] = kEmpty32;
    __syncthreads();
    // 1. the distinct admissible ones of the seeds hx_count wrote down
    const uint64_t* written = small + (size_t)(q - q0) * kLdsSeeds;
    const uint32_t n_seeds = (uint32_t)seeds[q];   // <= kLdsSeeds
    for (uint32_t t = threadIdx.x; t < n_seeds; t += kThreads) {
        const uint64_t rec = written[t];
        uint64_t key;
        if (!seed_key(start, n_ord, (uint32_t)(rec >> 32), (uint32_t)rec, m, key)) continue;
        uint32_t s = slot64(key);
        for (;;) {   // at most kLdsSeeds distinct keys: a free slot always exists
            const uint64_t prev = atomicCAS((unsigned long long*)&s_tab[s], (unsigned long long)kEmpty64,
                                            (unsigned long long)key);
            if (prev == kEmpty64 || prev == key) break;
            s = (s + 1) & (kSlots - 1);
        }
    }
    __syncthreads();
    // 2. packed to the front and sorted: the layout the global path gets from the segmented sort
    uint64_t rk[kSlotsPerThread];
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t u = 0; u < kSlotsPerThread; u++) {
        rk[u] = s_tab[threadIdx.x + u * kThreads];
        mine += rk[u] != kEmpty64 ? 1u : 0u;
    }
    const uint64_t incl = block_scan_incl(mine, s_w);   // its barriers separate the reads above from the writes below
    if (threadIdx.x == kThreads - 1) s_w[0] = incl;
    __syncthreads();
    const uint32_t nc = (uint32_t)s_w[0];
    uint32_t n = 1;
    while (n < nc) n <<= 1;
    uint32_t o = (uint32_t)incl - mine;
#pragma unroll
    for (uint32_t u = 0; u < kSlotsPerThread; u++)
        if (rk[u] != kEmpty64) s_tab[o++] = rk[u];
    __syncthreads();
    for (uint32_t i = nc + threadIdx.x; i < n; i += kThreads) s_tab[i] = kEmpty64;
    __syncthreads();
    bitonic_sort(s_tab, n);
    // 3. the sums
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t i = wave * kInFlight; i < nc; i += kVerifyStep)
        verify_group(s_tab, 0, nc, i, s_q, m, frames, start, lane, [&](uint64_t first, uint64_t idx, uint32_t dist) {
            atomicMin(&s_best[first], (dist << 12) | (uint32_t)(idx - first));   // dist < 2^18, a run < 2^12 candidates
        });
    __syncthreads();
    // 4. top k of the ordinals' best under the threshold (s_q is free now)
    uint64_t* s_key = reinterpret_cast<uint64_t*>(s_q);          // [2 * kThreads]
    uint32_t* s_d = s_q + 4 * kThreads;                          // [2 * kThreads]
    for (uint32_t i = threadIdx.x; i < 2 * kThreads; i += kThreads) {
        s_key[i] = kEmpty64;
        s_d[i] = 0;
    }
    __syncthreads();
    const uint64_t bits = 32ull * m;
    for (uint32_t b = 0; b < nc; b += kThreads) {
        const uint32_t i = b + threadIdx.x;
        uint64_t cand = kEmpty64;
        uint32_t d = 0;
        if (i < nc) {
            const uint64_t ord = s_tab[i] >> 32;
            if (i == 0 || (s_tab[i - 1] >> 32) != ord) {
                const uint32_t bv = s_best[i];
                const uint64_t dist = bv >> 12;
                if (dist * 1000000ull <= (uint64_t)max_ber_ppm * bits) {
                    cand = (dist << 32) | ord;
                    d = (uint32_t)s_tab[i + (bv & 4095u)];
                }
            }
        }
        topk_offer(s_key, k, cand, s_d, d);
    }
    write_hits(s_key, s_d, q, k, bits, ids, out_ids, out_dist, out_offsets, out_scores, out_n);
}

// one block per query of the slice
__global__ __launch_bounds__(kThreads) void hx_topk(const uint64_t* __restrict__ qoff, const uint32_t* __restrict__ qlist,
                                                     const uint64_t* __restrict__ keys, const uint64_t* __restrict__ soff,
                                                     const uint32_t* __restrict__ cursor,
                                                     const unsigned long long* __restrict__ best,
                                                     const uint64_t* __restrict__ ids, uint32_t k, uint32_t max_ber_ppm,
                                                     uint64_t* __restrict__ out_ids, uint32_t* __restrict__ out_dist,
                                                     int32_t* __restrict__ out_offsets, float* __restrict__ out_scores,
                                                     uint32_t* __restrict__ out_n) {
    __shared__ uint64_t s_key[2 * kThreads];
    __shared__ uint32_t s_d[2 * kThreads];
    const uint32_t ql = blockIdx.x, q = qlist[ql];
    const uint64_t a = soff[ql], e = a + cursor[ql];
    const uint64_t bits = 32ull * (qoff[q + 1] - qoff[q]);
    for (uint32_t i = threadIdx.x; i < 2 * kThreads; i += kThreads) {
        s_key[i] = kEmpty64;
        s_d[i] = 0;
    }
    __syncthreads();
    for (uint64_t b = a; b < e; b += kThreads) {
        const uint64_t i = b + threadIdx.x;
        uint64_t cand = kEmpty64;
        uint32_t d = 0;
        if (i < e) {
            const uint64_t ord = keys[i] >> 32;
            if (i == a || (keys[i - 1] >> 32) != ord) {
                const uint64_t bv = best[i], dist = bv >> 32;
                if (dist * 1000000ull <= (uint64_t)max_ber_ppm * bits) {
                    cand = (dist << 32) | ord;
                    d = (uint32_t)bv;
                }
            }
        }
        topk_offer(s_key, k, cand, s_d, d);
    }
    write_hits(s_key, s_d, q, k, bits, ids, out_ids, out_dist, out_offsets, out_scores, out_n);
}

// empty answers for every query (unknown tenant / no frames)
__global__ void hx_empty(size_t nq, uint32_t k, uint64_t* __restrict__ out_ids, uint32_t* __restrict__ out_dist,
                         int32_t* __restrict__ out_offsets, float* __restrict__ out_scores, uint32_t* __restrict__ out_n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq * k) {
        out_ids[i] = kEmpty64;
        out_dist[i] = kEmpty32;
        out_offsets[i] = 0;
        out_scores[i] = -1.0f;
    }
    if (i < nq) out_n[i] = 0;
}

struct Tenant {
    std::map<uint64_t, std::vector<uint32_t>> recs;   // id -> frames (ascending id = ordinal order)
    bool dirty = true;
    size_t n_frames = 0;                              // valid when !dirty
    DevArr frames, start, ids, vals, pos, dir;
};

struct Slice {
    size_t l0, l1, soff_at;   // queries qlist[l0 .. l1); their n + 1 segment offsets begin at h_soff[soff_at]
    uint64_t seeds, max_seeds;
};

}  // namespace

struct ucfp_haitsma_index : ucfp::IndexCore {
    uint32_t max_postings = 0;
    std::unordered_map<uint32_t, Tenant> tenants;
    // rebuild workspace
    DevArr b_iota, b_tmp;
    // query workspace
    DevArr q_frames, q_off, q_info, q_seeds, q_small, q_qlist, q_soff, q_cursor, q_keys_a, q_keys_b, q_best, q_tmp, q_out;
    std::vector<uint64_t> h_seeds, h_soff;
    std::vector<uint32_t> h_qlist;
};

namespace {

int check_batch_host(const uint32_t* frames, const uint64_t* offsets, size_t n, uint64_t max_item, const char* what) {
    if (n && !offsets) return capi_fail(UCFP_E_INVALID, "offsets is NULL");
    if (!n) return UCFP_OK;
    if (offsets[0] != 0) return capi_fail(UCFP_E_INVALID, "offsets[0] must be 0");
    for (size_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i]) return capi_fail(UCFP_E_INVALID, "offsets decrease at %zu", i);
        if (offsets[i + 1] - offsets[i] > max_item)
            return capi_fail(UCFP_E_INVALID, "%s %zu has %llu frames, more than %llu", what, i,
                             (unsigned long long)(offsets[i + 1] - offsets[i]), (unsigned long long)max_item);
    }
    if (offsets[n] && !frames) return capi_fail(UCFP_E_INVALID, "frames is NULL");
    return UCFP_OK;
}

int rebuild(ucfp_haitsma_index* ix, Tenant& T, hipStream_t st) {
    size_t n = 0;
    for (auto& kv : T.recs) n += kv.second.size();
    const size_t n_rec = T.recs.size();
    if (n_rec >= 0xffffffffull) return capi_fail(UCFP_E_INVALID, "too many records in one tenant");
    if (n >= 0xffffffffull) return capi_fail(UCFP_E_INVALID, "too many frames in one tenant (%zu)", n);
    std::vector<uint32_t> h_frames(n);
    std::vector<uint64_t> h_start(n_rec + 1), h_ids(n_rec);
    size_t o = 0, ord = 0;
    for (auto& kv : T.recs) {
        h_ids[ord] = kv.first;
        h_start[ord] = o;
        if (!kv.second.empty()) memcpy(h_frames.data() + o, kv.second.data(), kv.second.size() * 4);
        o += kv.second.size();
        ord++;
    }
    h_start[n_rec] = n;
    int rc;
    if ((rc = T.ids.ensure(n_rec * 8)) || (rc = T.start.ensure((n_rec + 1) * 8)) || (rc = T.dir.ensure((kDirSize + 1) * 4)) ||
        (rc = T.frames.ensure(n * 4)) || (rc = T.vals.ensure(n * 4)) || (rc = T.pos.ensure(n * 4)))
        return rc;
    if (n_rec) HIP_TRY(hipMemcpyAsync(T.ids.p, h_ids.data(), n_rec * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(T.start.p, h_start.data(), (n_rec + 1) * 8, hipMemcpyHostToDevice, st));
    if (n) {
        if ((rc = ix->b_iota.ensure(n * 4))) return rc;
        HIP_TRY(hipMemcpyAsync(T.frames.p, h_frames.data(), n * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(hx_iota, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ix->b_iota.as<uint32_t>(), n);
        HIP_TRY(hipGetLastError());
        // stable: equal values keep ascending positions
        if ((rc = sort_pairs(ix->b_tmp, T.frames.as<uint32_t>(), T.vals.as<uint32_t>(), ix->b_iota.as<uint32_t>(),
                             T.pos.as<uint32_t>(), n, 32, st)))
            return rc;
    }
    if ((rc = build_directory(T.vals.as<uint32_t>(), n, kDirShift, kDirSize, T.dir.as<uint32_t>(), st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));   // the host vectors above go out of scope
    T.n_frames = n;
    T.dirty = false;
    return UCFP_OK;
}

int do_upsert(ucfp_haitsma_index* ix, uint32_t tenant, const uint64_t* ids, const uint32_t* frames, const uint64_t* offsets,
              size_t n) {
    int rc = check_batch_host(frames, offsets, n, 0x7fffffffull, "record");
    if (rc) return rc;
    if (n && !ids) return capi_fail(UCFP_E_INVALID, "ids is NULL");
    if (!n) return UCFP_OK;
    Tenant& T = ix->tenants[tenant];
    for (size_t i = 0; i < n; i++) {
        std::vector<uint32_t>& v = T.recs[ids[i]];
        v.assign(frames + offsets[i], frames + offsets[i + 1]);
    }
    T.dirty = true;
    return UCFP_OK;
}

// blocks per query so that a thread takes a few items, with the grid below 2^31 blocks
uint32_t blocks_per_query(uint64_t items, uint32_t per_block, uint32_t cap, size_t nq) {
    uint64_t gx = (items + per_block - 1) / per_block;
    gx = std::max<uint64_t>(1, std::min<uint64_t>(gx, cap));
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(gx, 0x7fffffffull / nq));
}

// queries [p0, p0 + np) of a batch: seeds, then the LDS path or the global one
int query_pass(ucfp_haitsma_index* ix, Tenant& T, const uint32_t* d_qf, const uint64_t* d_off, size_t p0, size_t np,
               uint32_t max_m, uint32_t n_probes, uint32_t k, uint32_t max_ber_ppm, uint64_t* d_ids, uint32_t* d_dist,
               int32_t* d_offs, float* d_scores, uint32_t* d_n, hipStream_t st) {
    int rc;
    const uint32_t n_ord = (uint32_t)T.recs.size();
    // 2. seeds per query
    const uint32_t gp = blocks_per_query((uint64_t)max_m * n_probes, kThreads * 4, 256, np);
    hipLaunchKernelGGL(hx_count, dim3((unsigned)(np * gp)), dim3(kThreads), 0, st, d_qf, d_off, (uint32_t)p0, gp,
                       T.vals.as<uint32_t>(), T.pos.as<uint32_t>(), T.dir.as<uint32_t>(), n_probes, ix->max_postings,
                       ix->q_seeds.as<unsigned long long>(), ix->q_small.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    ix->h_seeds.resize(np);
    HIP_TRY(hipMemcpyAsync(ix->h_seeds.data(), ix->q_seeds.as<uint64_t>() + p0, np * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // the previous pass has also read h_qlist and h_soff by now
    // 3. the queries that go through global memory first in qlist, then the ones hx_small answers
    ix->h_qlist.clear();
    for (size_t i = 0; i < np; i++)
        if (ix->h_seeds[i] > kLdsSeeds) ix->h_qlist.push_back((uint32_t)(p0 + i));
    const size_t n_large = ix->h_qlist.size(), n_small = np - n_large;
    for (size_t i = 0; i < np; i++)
        if (ix->h_seeds[i] <= kLdsSeeds) ix->h_qlist.push_back((uint32_t)(p0 + i));
    HIP_TRY(hipMemcpyAsync(ix->q_qlist.p, ix->h_qlist.data(), np * 4, hipMemcpyHostToDevice, st));
    const uint32_t* d_qlist = ix->q_qlist.as<uint32_t>();
    if (n_small) {
        hipLaunchKernelGGL(hx_small, dim3((unsigned)n_small), dim3(kThreads), 0, st, d_qf, d_off, d_qlist + n_large, (uint32_t)p0,
                           ix->q_seeds.as<unsigned long long>(), ix->q_small.as<uint64_t>(), T.start.as<uint64_t>(), n_ord,
                           T.frames.as<uint32_t>(), T.ids.as<uint64_t>(), k, max_ber_ppm, d_ids, d_dist, d_offs, d_scores, d_n);
        HIP_TRY(hipGetLastError());
    }
    if (!n_large) return UCFP_OK;
    // 4. slices of them whose seeds fit the workspace (a query on its own may exceed it: the workspace grows)
    std::vector<Slice> slices;
    ix->h_soff.clear();
    uint64_t most = 0;
    size_t most_q = 0;
    for (size_t l = 0; l < n_large;) {
        Slice s{l, l, ix->h_soff.size(), 0, 0};
        ix->h_soff.push_back(0);
        while (s.l1 < n_large && (s.l1 == s.l0 || s.seeds + ix->h_seeds[ix->h_qlist[s.l1] - p0] <= kSliceSeeds)) {
            const uint64_t v = ix->h_seeds[ix->h_qlist[s.l1] - p0];
            if (v >= 0xffffffffull)
                return capi_fail(UCFP_E_INVALID, "query %u gathers %llu seeds", ix->h_qlist[s.l1], (unsigned long long)v);
            s.seeds += v;
            s.max_seeds = std::max(s.max_seeds, v);
            ix->h_soff.push_back(s.seeds);
            s.l1++;
        }
        most = std::max(most, s.seeds);
        most_q = std::max(most_q, s.l1 - s.l0);
        slices.push_back(s);
        l = s.l1;
    }
    if ((rc = ix->q_soff.ensure(ix->h_soff.size() * 8)) || (rc = ix->q_cursor.ensure(most_q * 4)) ||
        (rc = ix->q_keys_a.ensure(most * 8)) || (rc = ix->q_keys_b.ensure(most * 8)) || (rc = ix->q_best.ensure(most * 8)))
        return rc;
    HIP_TRY(hipMemcpyAsync(ix->q_soff.p, ix->h_soff.data(), ix->h_soff.size() * 8, hipMemcpyHostToDevice, st));
    // 5. per slice: seeds, sort, verify, top-k
    for (const Slice& s : slices) {
        const size_t ns = s.l1 - s.l0;
        const uint64_t* so = ix->q_soff.as<uint64_t>() + s.soff_at;
        const uint32_t* ql = d_qlist + s.l0;
        uint32_t* cursor = ix->q_cursor.as<uint32_t>();
        HIP_TRY(hipMemsetAsync(cursor, 0, ns * 4, st));
        // unused places of a segment (inadmissible seeds) stay kEmpty64 and sort last
        HIP_TRY(hipMemsetAsync(ix->q_keys_a.p, 0xff, s.seeds * 8, st));
        HIP_TRY(hipMemsetAsync(ix->q_best.p, 0xff, s.seeds * 8, st));
        const uint32_t ge = blocks_per_query((uint64_t)max_m * n_probes, kThreads * 4, 256, ns);
        hipLaunchKernelGGL(hx_emit, dim3((unsigned)(ns * ge)), dim3(kThreads), 0, st, d_qf, d_off, ql, ge, T.vals.as<uint32_t>(),
                           T.pos.as<uint32_t>(), T.dir.as<uint32_t>(), T.start.as<uint64_t>(), n_ord, n_probes,
                           ix->max_postings, so, cursor, ix->q_keys_a.as<uint64_t>());
        HIP_TRY(hipGetLastError());
        if ((rc = sort_segments(ix->q_tmp, ix->q_keys_a.as<uint64_t>(), ix->q_keys_b.as<uint64_t>(), (size_t)s.seeds, ns, so, st)))
            return rc;
        const uint32_t gv = blocks_per_query(s.max_seeds, kVerifyStep * 8, 4096, ns);
        hipLaunchKernelGGL(hx_verify, dim3((unsigned)(ns * gv)), dim3(kThreads), 0, st, d_qf, d_off, ql, gv,
                           ix->q_keys_b.as<uint64_t>(), so, cursor, T.frames.as<uint32_t>(), T.start.as<uint64_t>(),
                           ix->q_best.as<unsigned long long>());
        hipLaunchKernelGGL(hx_topk, dim3((unsigned)ns), dim3(kThreads), 0, st, d_off, ql, ix->q_keys_b.as<uint64_t>(), so, cursor,
                           ix->q_best.as<unsigned long long>(), T.ids.as<uint64_t>(), k, max_ber_ppm, d_ids, d_dist, d_offs,
                           d_scores, d_n);
        HIP_TRY(hipGetLastError());
    }
    return UCFP_OK;
}

int query_impl(ucfp_haitsma_index* ix, uint32_t tenant, const uint32_t* d_qf, const uint64_t* d_off, size_t nq, uint32_t k,
               uint32_t flip_bits, uint32_t max_ber_ppm, uint64_t* d_ids, uint32_t* d_dist, int32_t* d_offs, float* d_scores,
               uint32_t* d_n, hipStream_t st) {
    int rc;
    // 1. offsets and sizes (checked before anything else, whatever the tenant or k)
    if ((rc = ix->q_info.ensure(32))) return rc;
    HIP_TRY(hipMemsetAsync(ix->q_info.p, 0, 32, st));
    unsigned long long* d_info = ix->q_info.as<unsigned long long>();
    hipLaunchKernelGGL(hx_qprep, dim3(1), dim3(kThreads), 0, st, d_off, nq, d_info, reinterpret_cast<uint32_t*>(d_info + 2));
    HIP_TRY(hipGetLastError());
    uint64_t info[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(info, ix->q_info.p, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (info[2] & 1) return capi_fail(UCFP_E_INVALID, "query offsets must start at 0 and not decrease");
    if (info[2] & 2) return capi_fail(UCFP_E_INVALID, "a query has more than %u frames", kMaxM);
    const size_t total = (size_t)info[0];
    const uint32_t max_m = (uint32_t)info[1];
    if (total && !d_qf) return capi_fail(UCFP_E_INVALID, "frames is NULL");
    if (k == 0) {
        HIP_TRY(hipMemsetAsync(d_n, 0, nq * 4, st));
        return UCFP_OK;
    }
    auto it = ix->tenants.find(tenant);
    if (it != ix->tenants.end() && it->second.dirty && (rc = rebuild(ix, it->second, st))) return rc;
    if (it == ix->tenants.end() || total == 0 || it->second.n_frames == 0) {
        hipLaunchKernelGGL(hx_empty, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, st, nq, k, d_ids, d_dist, d_offs,
                           d_scores, d_n);
        HIP_TRY(hipGetLastError());
        return UCFP_OK;
    }
    Tenant& T = it->second;
    const uint32_t n_probes = probe_count(flip_bits);
    if ((rc = ix->q_seeds.ensure(nq * 8)) || (rc = ix->q_small.ensure(std::min(nq, kPassQueries) * kLdsSeeds * 8)) ||
        (rc = ix->q_qlist.ensure(std::min(nq, kPassQueries) * 4)))
        return rc;
    HIP_TRY(hipMemsetAsync(ix->q_seeds.p, 0, nq * 8, st));
    for (size_t p0 = 0; p0 < nq && !rc; p0 += kPassQueries)
        rc = query_pass(ix, T, d_qf, d_off, p0, std::min(kPassQueries, nq - p0), max_m, n_probes, k, max_ber_ppm, d_ids, d_dist,
                        d_offs, d_scores, d_n, st);
    return rc;
}

int query_args(ucfp_haitsma_index* ix, const uint64_t* offsets, size_t nq, uint32_t k, uint32_t flip_bits,
               uint32_t max_ber_ppm, const void* out_ids, const void* out_dist, const void* out_offsets,
               const void* out_scores, const void* out_n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (k > UCFP_INDEX_MAX_K) return capi_fail(UCFP_E_INVALID, "k = %u exceeds UCFP_INDEX_MAX_K = %u", k, UCFP_INDEX_MAX_K);
    if (flip_bits > 2) return capi_fail(UCFP_E_INVALID, "flip_bits = %u: 0, 1 or 2", flip_bits);
    if (max_ber_ppm > 1000000u) return capi_fail(UCFP_E_INVALID, "max_ber_ppm = %u exceeds 1000000", max_ber_ppm);
    if (nq > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "too many queries");
    if (nq && (!offsets || !out_n)) return capi_fail(UCFP_E_INVALID, "offsets/out_n is NULL");
    if (nq && k && (!out_ids || !out_dist || !out_offsets || !out_scores))
        return capi_fail(UCFP_E_INVALID, "an output buffer is NULL");
    return UCFP_OK;
}

}  // namespace

extern "C" {

size_t ucfp_haitsma_index_probes(uint32_t flip_bits) { return probe_count(flip_bits); }

int ucfp_haitsma_index_create(ucfp_ctx* ctx, uint32_t max_postings, uint32_t flags, ucfp_haitsma_index** out) {
    if (!ctx || !out) return capi_fail(UCFP_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (flags != 0) return capi_fail(UCFP_E_INVALID, "no Haitsma index flags are defined (got %u)", flags);
    const int rc = ucfp::create_index(ctx, "Haitsma index", out);
    if (!rc) (*out)->max_postings = max_postings;
    return rc;
}

void ucfp_haitsma_index_destroy(ucfp_haitsma_index* ix) {
    if (!ix) return;
    ix->quiesce();
    for (auto& kv : ix->tenants) {
        Tenant& T = kv.second;
        for (DevArr* a : {&T.frames, &T.start, &T.ids, &T.vals, &T.pos, &T.dir}) a->release();
    }
    for (DevArr* a : {&ix->b_iota, &ix->b_tmp, &ix->q_frames, &ix->q_off, &ix->q_info, &ix->q_seeds, &ix->q_small, &ix->q_qlist, &ix->q_soff, &ix->q_cursor,
                      &ix->q_keys_a, &ix->q_keys_b, &ix->q_best, &ix->q_tmp, &ix->q_out})
        a->release();
    delete ix;
}

int ucfp_haitsma_index_upsert(ucfp_haitsma_index* ix, uint32_t tenant, const uint64_t* ids, const uint32_t* frames,
                              const uint64_t* offsets, size_t n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    return do_upsert(ix, tenant, ids, frames, offsets, n);
}

int ucfp_haitsma_index_upsert_dev(ucfp_haitsma_index* ix, uint32_t tenant, const uint64_t* d_ids, const uint32_t* d_frames,
                                  const uint64_t* d_offsets, size_t n, void* stream) {
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
    if (offs[n] >= 0xffffffffull) return capi_fail(UCFP_E_INVALID, "too many frames in one batch");
    std::vector<uint32_t> fr(offs[n]);
    if (offs[n]) {
        if (!d_frames) return capi_fail(UCFP_E_INVALID, "frames is NULL");
        HIP_TRY(hipMemcpyAsync(fr.data(), d_frames, offs[n] * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return do_upsert(ix, tenant, ids.data(), fr.data(), offs.data(), n);
}

int ucfp_haitsma_index_delete(ucfp_haitsma_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed) {
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

int ucfp_haitsma_index_size(ucfp_haitsma_index* ix, uint32_t tenant, size_t* records, size_t* frames) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    size_t r = 0, f = 0;
    auto it = ix->tenants.find(tenant);
    if (it != ix->tenants.end()) {
        Tenant& T = it->second;
        if (T.dirty) {
            int rc = ix->begin();
            if (rc || (rc = rebuild(ix, T, ix->own)) || (rc = ix->end(ix->own))) return rc;
        }
        r = T.recs.size();
        f = T.n_frames;
    }
    if (records) *records = r;
    if (frames) *frames = f;
    return UCFP_OK;
}

int ucfp_haitsma_index_flush(ucfp_haitsma_index* ix) { return ucfp::flush_dirty(ix, rebuild); }

int ucfp_haitsma_index_query_dev(ucfp_haitsma_index* ix, uint32_t tenant, const uint32_t* d_frames, const uint64_t* d_offsets,
                                 size_t nq, uint32_t k, uint32_t flip_bits, uint32_t max_ber_ppm, uint64_t* d_out_ids,
                                 uint32_t* d_out_dist, int32_t* d_out_offsets, float* d_out_scores, uint32_t* d_out_n,
                                 void* stream) {
    int rc = query_args(ix, d_offsets, nq, k, flip_bits, max_ber_ppm, d_out_ids, d_out_dist, d_out_offsets, d_out_scores,
                        d_out_n);
    if (rc || nq == 0) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    if ((rc = ix->begin())) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = query_impl(ix, tenant, d_frames, d_offsets, nq, k, flip_bits, max_ber_ppm, d_out_ids, d_out_dist, d_out_offsets,
                    d_out_scores, d_out_n, st);
    return ix->end(st, rc);
}

int ucfp_haitsma_index_query(ucfp_haitsma_index* ix, uint32_t tenant, const uint32_t* frames, const uint64_t* offsets,
                             size_t nq, uint32_t k, uint32_t flip_bits, uint32_t max_ber_ppm, uint64_t* out_ids,
                             uint32_t* out_dist, int32_t* out_offsets, float* out_scores, uint32_t* out_n) {
    int rc = query_args(ix, offsets, nq, k, flip_bits, max_ber_ppm, out_ids, out_dist, out_offsets, out_scores, out_n);
    if (rc || nq == 0) return rc;
    if ((rc = check_batch_host(frames, offsets, nq, kMaxM, "query"))) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    if ((rc = ix->begin())) return rc;
    hipStream_t st = ix->own;
    const size_t bytes = offsets[nq] * 4, nk = nq * k;
    const size_t o_dist = nk * 8, o_offs = o_dist + nk * 4, o_sc = o_offs + nk * 4, o_n = o_sc + nk * 4;
    if ((rc = ix->q_frames.ensure(bytes)) || (rc = ix->q_off.ensure((nq + 1) * 8)) || (rc = ix->q_out.ensure(o_n + nq * 4)))
        return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(ix->q_frames.p, frames, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ix->q_off.p, offsets, (nq + 1) * 8, hipMemcpyHostToDevice, st));
    uint8_t* ob = ix->q_out.as<uint8_t>();
    rc = query_impl(ix, tenant, ix->q_frames.as<uint32_t>(), ix->q_off.as<uint64_t>(), nq, k, flip_bits, max_ber_ppm,
                    (uint64_t*)ob, (uint32_t*)(ob + o_dist), (int32_t*)(ob + o_offs), (float*)(ob + o_sc),
                    (uint32_t*)(ob + o_n), st);
    if (rc) return ix->end_sync(rc);
    if (nk) {
        HIP_TRY(hipMemcpyAsync(out_ids, ob, nk * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_dist, ob + o_dist, nk * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_offsets, ob + o_offs, nk * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_scores, ob + o_sc, nk * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(out_n, ob + o_n, nq * 4, hipMemcpyDeviceToHost, st));
    return ix->end_sync(UCFP_OK);
}

}  // extern "C"
