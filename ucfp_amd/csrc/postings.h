// postings.h -- the posting-index core shared by landmark.hip and bm25.hip (A11).
//
// Both keep per-tenant postings on the device, rebuilt lazily after a change: the host flattens the tenant, rocPRIM's
// stable radix sort orders it, and a compaction keeps the heads of the sorted runs (post_count, post_scan_tiles,
// post_compact: a head predicate and an emit functor say what a head is and what it writes), with a directory
// (post_directory) on the top bits of the key bounding every lookup.  Queries share the LDS block helpers below.
// The device code lives in an unnamed namespace, so each translation unit keeps its own kernels; the object lifecycle
// and the call protocol (IndexCore) are host code in namespace ucfp, in index_core.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>  // rocPRIM's texture iterator calls the host memset without including it

#include <rocprim/rocprim.hpp>

#include <cstddef>
#include <type_traits>

#include "index_core.h"

namespace {

constexpr uint32_t kCompactTile = 1024;   // rebuild compaction: elements per block

// ---------------------------------------------------------------- block helpers (256 threads)

__device__ __forceinline__ uint64_t block_scan_incl(uint64_t v, uint64_t* s_w) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    uint64_t add = 0;
    for (int i = 0; i < w; i++) add += s_w[i];
    __syncthreads();   // s_w may be reused by the next call
    return v + add;
}

// ascending bitonic sort of n (a power of two) keys, with a u32 payload s_val when one is passed; ends with a barrier
template <class Val = std::nullptr_t>
__device__ void bitonic_sort(uint64_t* s_key, uint32_t n, Val s_val = nullptr) {
    for (uint32_t k2 = 2; k2 <= n; k2 <<= 1)
        for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
                const uint32_t p = i ^ j;
                if (p > i) {
                    const uint64_t a = s_key[i], b = s_key[p];
                    if ((a > b) == ((i & k2) == 0)) {
                        s_key[i] = b;
                        s_key[p] = a;
                        if constexpr (!std::is_same<Val, std::nullptr_t>::value) {
                            const uint32_t t = s_val[i];
                            s_val[i] = s_val[p];
                            s_val[p] = t;
                        }
                    }
                }
            }
            __syncthreads();
        }
}

// Running top-k, one candidate key (and payload val) per thread: [0, k) of s_top holds the best k so far
// (k <= 128 < 256); a chunk of 256 candidates goes to [256, 512) and the 512 are sorted when one of them beats the
// current k-th.  s_top (and s_val) hold 2 * kThreads entries, kEmpty64 where empty.
template <class Val = std::nullptr_t>
__device__ __forceinline__ void topk_offer(uint64_t* s_top, uint32_t k, uint64_t key, Val s_val = nullptr,
                                           uint32_t val = 0) {
    const bool better = key < s_top[k - 1];
    if (__syncthreads_or(better)) {
        s_top[kThreads + threadIdx.x] = key;
        if constexpr (!std::is_same<Val, std::nullptr_t>::value) s_val[kThreads + threadIdx.x] = val;
        __syncthreads();
        bitonic_sort(s_top, 2 * kThreads, s_val);
    }
}

// ---------------------------------------------------------------- rebuild kernels

// heads per tile of kCompactTile sorted elements; head(i) is true when element i starts a new run
template <class Head>
__global__ void post_count(Head head, size_t n, uint32_t* __restrict__ block_counts) {
    const size_t base = (size_t)blockIdx.x * kCompactTile;
    uint32_t c = 0;
    for (uint32_t j = threadIdx.x; j < kCompactTile; j += kThreads) {
        const size_t i = base + j;
        if (i < n) c += head(i) ? 1u : 0u;
    }
    __shared__ uint64_t s_w[4];
    const uint64_t tot = block_scan_incl(c, s_w);
    if (threadIdx.x == kThreads - 1) block_counts[blockIdx.x] = (uint32_t)tot;
}

// exclusive scan of nb block counts (one block); out[nb] = total
__global__ void post_scan_tiles(const uint32_t* __restrict__ counts, size_t nb, uint64_t* __restrict__ out) {
    __shared__ uint64_t s_w[4];
    __shared__ uint64_t s_tot;
    uint64_t carry = 0;
    for (size_t base = 0; base < nb; base += kThreads) {
        const size_t i = base + threadIdx.x;
        const uint64_t v = i < nb ? counts[i] : 0;
        const uint64_t inc = block_scan_incl(v, s_w);
        if (i < nb) out[i] = carry + inc - v;
        if (threadIdx.x == kThreads - 1) s_tot = inc;
        __syncthreads();
        carry += s_tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[nb] = carry;
}

// emit(i, o) for every head i, o = its rank among the heads (block_off from post_scan_tiles)
template <class Head, class Emit>
__global__ void post_compact(Head head, Emit emit, size_t n, const uint64_t* __restrict__ block_off) {
    __shared__ uint64_t s_w[4];
    const size_t base = (size_t)blockIdx.x * kCompactTile;
    constexpr uint32_t kPer = kCompactTile / kThreads;
    // thread t owns elements [t * kPer, (t + 1) * kPer) of the tile, so the output keeps the input order
    bool keep[kPer];
    uint32_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        const size_t i = base + threadIdx.x * kPer + j;
        keep[j] = i < n && head(i);
        c += keep[j] ? 1u : 0u;
    }
    uint64_t o = block_off[blockIdx.x] + block_scan_incl(c, s_w) - c;
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++)
        if (keep[j]) emit(base + threadIdx.x * kPer + j, o++);
}

// dir[b] = first of the u sorted keys with key >> shift >= b, for b in [0, nb]
template <class K>
__global__ void post_directory(const K* __restrict__ keys, size_t u, uint32_t shift, uint32_t nb,
                               uint32_t* __restrict__ dir) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= u) return;
    const uint32_t b = (uint32_t)(keys[i] >> shift);
    const uint32_t from = i == 0 ? 0u : (uint32_t)(keys[i - 1] >> shift) + 1u;
    for (uint32_t x = from; x <= b; x++) dir[x] = (uint32_t)i;
    if (i + 1 == u)
        for (uint32_t x = b + 1; x <= nb; x++) dir[x] = (uint32_t)u;
}

// ---------------------------------------------------------------- rebuild drivers (host)

// rocPRIM's two-phase calls: ask for the temporary storage, grow tmp to it, sort
template <class K, class V>
int sort_pairs(DevArr& tmp, K* keys_in, K* keys_out, V* vals_in, V* vals_out, size_t n, int end_bit, hipStream_t st) {
    size_t bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out, n, 0, end_bit, st));
    const int rc = tmp.ensure(bytes);
    if (rc) return rc;
    HIP_TRY(rocprim::radix_sort_pairs(tmp.p, bytes, keys_in, keys_out, vals_in, vals_out, n, 0, end_bit, st));
    return UCFP_OK;
}

// n keys in nseg segments [off[s], off[s + 1]), each sorted on its own
template <class K>
int sort_segments(DevArr& tmp, K* keys_in, K* keys_out, size_t n, size_t nseg, const uint64_t* off, hipStream_t st) {
    size_t bytes = 0;
    HIP_TRY(rocprim::segmented_radix_sort_keys(nullptr, bytes, keys_in, keys_out, (unsigned)n, (unsigned)nseg, off,
                                               off + 1, 0, 64, st));
    const int rc = tmp.ensure(bytes);
    if (rc) return rc;
    HIP_TRY(rocprim::segmented_radix_sort_keys(tmp.p, bytes, keys_in, keys_out, (unsigned)n, (unsigned)nseg, off,
                                               off + 1, 0, 64, st));
    return UCFP_OK;
}

// Compaction of n > 0 sorted elements, first half: heads per tile, their scan into off, and the number of heads read
// back (one host synchronisation), so that the caller can size the outputs of compact_heads.
template <class Head>
int count_heads(Head head, size_t n, DevArr& cnt, DevArr& off, hipStream_t st, size_t* total) {
    const size_t nb = (n + kCompactTile - 1) / kCompactTile;
    int rc;
    if ((rc = cnt.ensure(nb * 4)) || (rc = off.ensure((nb + 1) * 8))) return rc;
    hipLaunchKernelGGL(post_count<Head>, dim3((unsigned)nb), dim3(kThreads), 0, st, head, n, cnt.as<uint32_t>());
    hipLaunchKernelGGL(post_scan_tiles, dim3(1), dim3(kThreads), 0, st, cnt.as<uint32_t>(), nb, off.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    uint64_t t = 0;
    HIP_TRY(hipMemcpyAsync(&t, off.as<uint64_t>() + nb, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *total = (size_t)t;
    return UCFP_OK;
}

// second half: emit(i, o) for every head
template <class Head, class Emit>
int compact_heads(Head head, Emit emit, size_t n, const DevArr& off, hipStream_t st) {
    const size_t nb = (n + kCompactTile - 1) / kCompactTile;
    hipLaunchKernelGGL((post_compact<Head, Emit>), dim3((unsigned)nb), dim3(kThreads), 0, st, head, emit, n,
                       off.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    return UCFP_OK;
}

// the directory of u sorted keys (all zero when u = 0)
template <class K>
int build_directory(const K* keys, size_t u, uint32_t shift, uint32_t nb, uint32_t* dir, hipStream_t st) {
    if (!u) {
        HIP_TRY(hipMemsetAsync(dir, 0, ((size_t)nb + 1) * 4, st));
        return UCFP_OK;
    }
    hipLaunchKernelGGL(post_directory<K>, dim3((unsigned)((u + 255) / 256)), dim3(256), 0, st, keys, u, shift, nb, dir);
    HIP_TRY(hipGetLastError());
    return UCFP_OK;
}

}  // namespace
