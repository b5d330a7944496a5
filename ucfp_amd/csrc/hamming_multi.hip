// hamming_multi.hip -- exact Hamming top-k for a batch in which every query names its own tenant (DESIGN M3).
//
// The per-tenant search (hamming.hip, hamming_direct.hip) is one chain of launches per tenant; ten thousand small tenants
// get ten thousand chains.  Here the launches of a batch do not depend on how many tenants it names: the host sorts the
// queries by tenant into segments and cuts every segment into work items (multi_plan.h), and five kernels walk the items or
// the queries of the whole batch.  A 64-bit Hamming distance has 65 values, so a histogram gives the k-th distance exactly:
//
//   hamming_multi_hist     one workgroup per item: lane = row (coalesced u64 loads), the item's queries wave-uniform; an LDS
//                          histogram [query][65] (ds_add without return), flushed to hist[position][65]
//   hamming_multi_tau      per query: tau = the smallest distance whose cumulative count reaches min(k, n), lt = rows below
//                          tau (< k), need = min(k, n) - lt, eq = hist[tau]; writes the count
//   hamming_multi_collect  the same items again: rows with d < tau go to the query's list (exactly lt entries: it cannot
//                          overflow), rows with d == tau to its tie list when eq <= kTieCap
//   hamming_multi_select   per query: the lt list in (d, id) order, then the `need` smallest ids of the ties, scores,
//                          distances and the padding
//   hamming_multi_ties     gated: a query with eq > kTieCap (thousands of identical codes) finds its need-th smallest tie
//                          id by a radix select over the tenant's rows -- eight passes of one byte each and a ninth that
//                          takes the ids -- whatever the row order.  Returns at once when no query is flagged.
//
// Everything is indexed by the POSITION p of a query in the tenant-sorted batch; perm[p] is the caller's query number, which
// only the loads of the query values and the stores of the outputs use.  Each tenant's rows are read twice (hist, collect).
// Row order carries no meaning for ids (a delete moves the last row into the hole), and an APPEND_ONLY shard may hold an
// id twice: ranks break ties of (d, id) by list position, so equal entries still take distinct places.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ucfp_hip.h"
#include "common.h"
#include "hamming64.h"
#include "multi_plan.h"

namespace ucfp {

namespace {

using multi::Item;
using multi::kBlock;
using multi::kQueryChunk;
using multi::kTieCap;
using multi::kTileRows;
using multi::Seg;

constexpr uint32_t kRowsPerLane = kTileRows / kBlock;
constexpr uint32_t kMaxK = UCFP_INDEX_MAX_K;   // sizes the LDS lists of the select and tie kernels
static_assert(kTileRows % kBlock == 0, "a tile is a whole number of rows per lane");
static_assert(kMaxK <= 256, "the LDS lists of hamming_multi_select / hamming_multi_ties were sized for k <= 256");

__global__ __launch_bounds__(256) void hamming_multi_hist(const Item* __restrict__ items, const Seg* __restrict__ segs,
                                                          const uint32_t* __restrict__ perm,
                                                          const uint64_t* __restrict__ queries, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kQueryChunk * 65];
    __shared__ uint64_t qs[kQueryChunk];
    const Item it = items[blockIdx.x];
    const Seg sg = segs[it.seg];
    const uint32_t tid = threadIdx.x, p0 = sg.first + it.q0;
    for (uint32_t e = tid; e < it.nq * 65; e += kBlock) h[e] = 0;
    if (tid < it.nq) qs[tid] = queries[perm[p0 + tid]];
    __syncthreads();
    const uint64_t r0 = (uint64_t)it.tile * kTileRows + tid;
    uint64_t x[kRowsPerLane];
    bool ok[kRowsPerLane];
#pragma unroll
    for (uint32_t u = 0; u < kRowsPerLane; u++) {
        const uint64_t r = r0 + (uint64_t)u * kBlock;
        ok[u] = r < sg.n;
        x[u] = ok[u] ? sg.rows[r] : 0ull;
    }
    for (uint32_t j = 0; j < it.nq; j++) {
        const uint64_t qv = qs[j];
#pragma unroll
        for (uint32_t u = 0; u < kRowsPerLane; u++)
            if (ok[u]) atomicAdd(&h[j * 65 + hamming64(qv, x[u])], 1u);
    }
    __syncthreads();
    for (uint32_t e = tid; e < it.nq * 65; e += kBlock) {
        const uint32_t c = h[e];
        if (c) atomicAdd(&hist[(size_t)p0 * 65 + e], c);
    }
}

// meta[p] = (tau, lt, need, eq); a query of a tenant without rows: (2^32 - 1, 0, 0, 0)
__global__ void hamming_multi_tau(const uint32_t* __restrict__ hist, const uint32_t* __restrict__ pos_seg,
                                  const Seg* __restrict__ segs, const uint32_t* __restrict__ perm, uint32_t cn, uint32_t k,
                                  uint4* __restrict__ meta, uint32_t* __restrict__ out_counts, uint32_t* __restrict__ flag) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= cn) return;
    const uint64_t n = segs[pos_seg[p]].n;
    const uint32_t cnt = n < (uint64_t)k ? (uint32_t)n : k;
    out_counts[perm[p]] = cnt;
    if (cnt == 0) {
        meta[p] = make_uint4(0xffffffffu, 0u, 0u, 0u);
        return;
    }
    uint32_t cum = 0, tau = 64, lt = 0, eq = 0;
    bool done = false;
    for (uint32_t b = 0; b < 65; b++) {
        const uint32_t c = hist[(size_t)p * 65 + b];
        if (!done && cum + c >= cnt) {
            tau = b;
            lt = cum;
            eq = c;
            done = true;
        }
        cum += c;
    }
    meta[p] = make_uint4(tau, lt, cnt - lt, eq);
    if (eq > kTieCap) *flag = 1u;
}

__global__ __launch_bounds__(256) void hamming_multi_collect(const Item* __restrict__ items, const Seg* __restrict__ segs,
                                                             const uint32_t* __restrict__ perm,
                                                             const uint64_t* __restrict__ queries,
                                                             const uint4* __restrict__ meta, uint32_t k,
                                                             uint32_t* __restrict__ lt_cnt, uint32_t* __restrict__ tie_cnt,
                                                             uint32_t* __restrict__ lt_d, uint64_t* __restrict__ lt_id,
                                                             uint64_t* __restrict__ tie_id) {
    __shared__ uint64_t qs[kQueryChunk];
    __shared__ uint32_t s_tau[kQueryChunk], s_eq[kQueryChunk];
    const Item it = items[blockIdx.x];
    const Seg sg = segs[it.seg];
    const uint32_t tid = threadIdx.x, p0 = sg.first + it.q0;
    if (tid < it.nq) {
        qs[tid] = queries[perm[p0 + tid]];
        const uint4 m = meta[p0 + tid];
        s_tau[tid] = m.x;
        s_eq[tid] = m.w;
    }
    __syncthreads();
    const uint64_t r0 = (uint64_t)it.tile * kTileRows + tid;
    uint64_t x[kRowsPerLane];
    bool ok[kRowsPerLane];
#pragma unroll
    for (uint32_t u = 0; u < kRowsPerLane; u++) {
        const uint64_t r = r0 + (uint64_t)u * kBlock;
        ok[u] = r < sg.n;
        x[u] = ok[u] ? sg.rows[r] : 0ull;
    }
    for (uint32_t j = 0; j < it.nq; j++) {
        const uint64_t qv = qs[j];
        const uint32_t tau = s_tau[j];
        const bool ties = s_eq[j] <= kTieCap;
        const size_t p = p0 + j;
#pragma unroll
        for (uint32_t u = 0; u < kRowsPerLane; u++) {
            if (!ok[u]) continue;
            const uint32_t d = hamming64(qv, x[u]);
            if (d < tau) {
                const uint32_t pos = atomicAdd(&lt_cnt[p], 1u);
                if (pos < k) {      // (always: lt < k rows lie below tau)
                    lt_d[p * k + pos] = d;
                    lt_id[p * k + pos] = sg.ids[r0 + (uint64_t)u * kBlock];
                }
            } else if (d == tau && ties) {
                const uint32_t pos = atomicAdd(&tie_cnt[p], 1u);
                if (pos < kTieCap) tie_id[p * kTieCap + pos] = sg.ids[r0 + (uint64_t)u * kBlock];   // (always: eq <= kTieCap)
            }
        }
    }
}

__device__ __forceinline__ void multi_store(uint64_t* __restrict__ out_ids, float* __restrict__ out_scores,
                                            uint32_t* __restrict__ out_dist, size_t at, uint64_t id, uint32_t d) {
    out_ids[at] = id;
    if (out_scores) out_scores[at] = d == 0xffffffffu ? -1.0f : 1.0f - (float)d * (1.0f / 64.0f);
    if (out_dist) out_dist[at] = d;
}

__global__ __launch_bounds__(256) void hamming_multi_select(const uint4* __restrict__ meta, const uint32_t* __restrict__ perm,
                                                            uint32_t k, const uint32_t* __restrict__ lt_d,
                                                            const uint64_t* __restrict__ lt_id,
                                                            const uint64_t* __restrict__ tie_id, uint64_t* __restrict__ out_ids,
                                                            float* __restrict__ out_scores, uint32_t* __restrict__ out_dist) {
    __shared__ uint64_t t_id[kTieCap];
    __shared__ uint64_t l_id[kMaxK];
    __shared__ uint32_t l_d[kMaxK];
    const size_t p = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint4 m = meta[p];
    const uint32_t tau = m.x, need = m.z, eq = m.w;
    const uint32_t lt = m.y < kMaxK ? m.y : kMaxK;
    const size_t row = (size_t)perm[p] * k;
    const bool ties = need > 0 && eq <= kTieCap;
    for (uint32_t e = tid; e < lt; e += kBlock) {
        l_d[e] = lt_d[p * k + e];
        l_id[e] = lt_id[p * k + e];
    }
    if (ties)
        for (uint32_t e = tid; e < eq; e += kBlock) t_id[e] = tie_id[p * kTieCap + e];
    __syncthreads();
    for (uint32_t e = tid; e < lt; e += kBlock) {
        const uint32_t d = l_d[e];
        const uint64_t id = l_id[e];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < lt; j++) {
            const uint32_t dj = l_d[j];
            const uint64_t ij = l_id[j];
            rank += (dj < d || (dj == d && (ij < id || (ij == id && j < e)))) ? 1u : 0u;
        }
        multi_store(out_ids, out_scores, out_dist, row + rank, id, d);
    }
    if (ties)
        for (uint32_t e = tid; e < eq; e += kBlock) {
            const uint64_t id = t_id[e];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < eq; j++) {
                const uint64_t ij = t_id[j];
                rank += (ij < id || (ij == id && j < e)) ? 1u : 0u;
            }
            if (rank < need) multi_store(out_ids, out_scores, out_dist, row + lt + rank, id, tau);
        }
    for (uint32_t r = lt + need + tid; r < k; r += kBlock) multi_store(out_ids, out_scores, out_dist, row + r, ~0ull, 0xffffffffu);
}

__global__ __launch_bounds__(256) void hamming_multi_ties(const uint32_t* __restrict__ flag, const uint4* __restrict__ meta,
                                                          const uint32_t* __restrict__ pos_seg, const Seg* __restrict__ segs,
                                                          const uint32_t* __restrict__ perm,
                                                          const uint64_t* __restrict__ queries, uint32_t k,
                                                          uint64_t* __restrict__ out_ids, float* __restrict__ out_scores,
                                                          uint32_t* __restrict__ out_dist) {
    if (*flag == 0u) return;
    const size_t p = blockIdx.x;
    const uint4 m = meta[p];
    const uint32_t tau = m.x, lt = m.y, eq = m.w;
    const uint32_t need = m.z < kMaxK ? m.z : kMaxK;
    if (eq <= kTieCap || need == 0) return;
    __shared__ uint32_t hb[256];
    __shared__ uint32_t s_bin, s_rem, s_taken, s_equal;
    __shared__ uint64_t list[kMaxK];
    const uint32_t tid = threadIdx.x;
    const Seg sg = segs[pos_seg[p]];
    const uint64_t qv = queries[perm[p]];
    // radix select of the need-th smallest id among the rows at distance tau, one byte per pass from the top
    uint64_t prefix = 0, mask = 0;
    uint32_t remaining = need;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hb[tid] = 0;
        __syncthreads();
        for (uint64_t r = tid; r < sg.n; r += kBlock) {
            if (hamming64(qv, sg.rows[r]) != tau) continue;
            const uint64_t id = sg.ids[r];
            if ((id & mask) == prefix) atomicAdd(&hb[(uint32_t)(id >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t cum = 0, b = 0;
            for (; b < 255; b++) {      // (the ids under the prefix number at least `remaining`: some bin reaches it)
                if (cum + hb[b] >= remaining) break;
                cum += hb[b];
            }
            s_bin = b;
            s_rem = remaining - cum;
        }
        __syncthreads();
        prefix |= (uint64_t)s_bin << shift;
        mask |= 0xffull << shift;
        remaining = s_rem;
        __syncthreads();
    }
    // every id below the threshold, and `remaining` of the rows that carry the threshold itself (one, unless an id repeats)
    if (tid == 0) {
        s_taken = 0;
        s_equal = 0;
    }
    __syncthreads();
    for (uint64_t r = tid; r < sg.n; r += kBlock) {
        if (hamming64(qv, sg.rows[r]) != tau) continue;
        const uint64_t id = sg.ids[r];
        bool take = id < prefix;
        if (id == prefix) take = atomicAdd(&s_equal, 1u) < remaining;
        if (take) {
            const uint32_t pos = atomicAdd(&s_taken, 1u);
            if (pos < kMaxK) list[pos] = id;
        }
    }
    __syncthreads();
    const uint32_t got = s_taken < need ? s_taken : need;
    const size_t row = (size_t)perm[p] * k;
    for (uint32_t e = tid; e < got; e += kBlock) {
        const uint64_t id = list[e];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < got; j++) {
            const uint64_t ij = list[j];
            rank += (ij < id || (ij == id && j < e)) ? 1u : 0u;
        }
        if (lt + rank < k) multi_store(out_ids, out_scores, out_dist, row + lt + rank, id, tau);
    }
}

size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

struct MultiLayout {
    size_t o_hist, o_ltc, o_tiec, o_flag, zero_bytes, o_meta, o_ltd, o_ltid, o_tie, total;
};

MultiLayout multi_layout(uint32_t cn, uint32_t k) {
    MultiLayout l;
    size_t off = 0;
    l.o_hist = off;
    off = a256(off + (size_t)cn * 65 * 4);
    l.o_ltc = off;
    off = a256(off + (size_t)cn * 4);
    l.o_tiec = off;
    off = a256(off + (size_t)cn * 4);
    l.o_flag = off;
    off = a256(off + 4);
    l.zero_bytes = off;        // histograms, list counters and the flag: one memset
    l.o_meta = off;
    off = a256(off + (size_t)cn * 16);
    l.o_ltd = off;
    off = a256(off + (size_t)cn * k * 4);
    l.o_ltid = off;
    off = a256(off + (size_t)cn * k * 8);
    l.o_tie = off;
    off = a256(off + (size_t)cn * kTieCap * 8);
    l.total = off;
    return l;
}

}  // namespace

size_t hamming_multi_ws_bytes(uint32_t cn, uint32_t k) { return multi_layout(cn, k).total; }

// One planned chunk of a multi-tenant batch: cn <= multi::kMaxBatch positions, 1 <= k <= UCFP_INDEX_MAX_K.  The tables are
// device copies of the plan; `queries` and the outputs are the chunk's own (query number 0 = the chunk's first).
// Seven enqueues whatever the tenants: a memset and the kernels above (the item kernels are skipped when no tenant has rows).
int launch_hamming_multi(uint8_t* ws, const uint32_t* perm, const uint32_t* pos_seg, const multi::Seg* segs,
                         const multi::Item* items, uint32_t n_items, const uint64_t* queries, uint32_t cn, uint32_t k,
                         uint64_t* out_ids, float* out_scores, uint32_t* out_dist, uint32_t* out_counts, hipStream_t stream) {
    const MultiLayout l = multi_layout(cn, k);
    uint32_t* hist = reinterpret_cast<uint32_t*>(ws + l.o_hist);
    uint32_t* lt_cnt = reinterpret_cast<uint32_t*>(ws + l.o_ltc);
    uint32_t* tie_cnt = reinterpret_cast<uint32_t*>(ws + l.o_tiec);
    uint32_t* flag = reinterpret_cast<uint32_t*>(ws + l.o_flag);
    uint4* meta = reinterpret_cast<uint4*>(ws + l.o_meta);
    uint32_t* lt_d = reinterpret_cast<uint32_t*>(ws + l.o_ltd);
    uint64_t* lt_id = reinterpret_cast<uint64_t*>(ws + l.o_ltid);
    uint64_t* tie_id = reinterpret_cast<uint64_t*>(ws + l.o_tie);
    if (hipMemsetAsync(ws, 0, l.zero_bytes, stream) != hipSuccess) return -1;
    if (n_items)
        hipLaunchKernelGGL(hamming_multi_hist, dim3(n_items), dim3(kBlock), 0, stream, items, segs, perm, queries, hist);
    hipLaunchKernelGGL(hamming_multi_tau, dim3((cn + 63) / 64), dim3(64), 0, stream, (const uint32_t*)hist, pos_seg, segs, perm, cn,
                       k, meta, out_counts, flag);
    if (n_items)
        hipLaunchKernelGGL(hamming_multi_collect, dim3(n_items), dim3(kBlock), 0, stream, items, segs, perm, queries,
                           (const uint4*)meta, k, lt_cnt, tie_cnt, lt_d, lt_id, tie_id);
    hipLaunchKernelGGL(hamming_multi_select, dim3(cn), dim3(kBlock), 0, stream, (const uint4*)meta, perm, k,
                       (const uint32_t*)lt_d, (const uint64_t*)lt_id, (const uint64_t*)tie_id, out_ids, out_scores, out_dist);
    hipLaunchKernelGGL(hamming_multi_ties, dim3(cn), dim3(kBlock), 0, stream, (const uint32_t*)flag, (const uint4*)meta, pos_seg,
                       segs, perm, queries, k, out_ids, out_scores, out_dist);
    return 0;
}

}  // namespace ucfp
