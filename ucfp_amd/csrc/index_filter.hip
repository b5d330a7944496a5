// index_filter.hip -- turning a query filter into a compact sub-shard (DESIGN F3 - F5).
//
// A filter is a Roaring set of record ids (roaring_parse.h flattens it into a sorted directory over a repacked payload
// image).  Three small kernels make the sub-shard that the Hamming and cosine searches then read exactly as they read a
// whole shard:
//   probe   lane = row: bisect the directory for id >> 16, probe the container for id & 0xffff; a ballot gives one 64-bit
//           mask word and one count per tile of 64 rows
//   scan    of the tile counts (launch_text_canon_scan: the tree's one-workgroup u64 scan)
//   gather  stable: row r of tile t goes to base[t] + popcount(mask[t] below r)

#include <hip/hip_runtime.h>

#include <new>

#include "../../include/ucfp_hip.h"
#include "common.h"
#include "roaring_parse.h"

namespace ucfp {

namespace {

constexpr unsigned kProbeWaves = 4;      // tiles per workgroup

// Is id in the set?  keys[nc] ascending; ents[nc]; image: see roaring_parse.h.
__device__ __forceinline__ bool filter_has(uint64_t id, const uint64_t* __restrict__ keys, const roaring::Entry* __restrict__ ents,
                                           uint32_t nc, const uint8_t* __restrict__ image) {
    const uint64_t key = id >> 16;
    const uint32_t low = (uint32_t)(id & 0xFFFFu);
    uint32_t lo = 0, hi = nc;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= nc || keys[lo] != key) return false;
    const roaring::Entry e = ents[lo];
    const uint8_t* c = image + e.off;
    if (e.type == roaring::kBitmap) {
        const uint64_t w = reinterpret_cast<const uint64_t*>(c)[low >> 6];      // 8-aligned in the image
        return (w >> (low & 63u)) & 1ull;
    }
    uint32_t a = 0, b = e.n;
    if (e.type == roaring::kArray) {
        const uint16_t* v = reinterpret_cast<const uint16_t*>(c);                // 2-aligned; <= 12 steps
        while (a < b) {
            const uint32_t mid = (a + b) >> 1;
            if (v[mid] < low) a = mid + 1;
            else b = mid;
        }
        return a < e.n && v[a] == low;
    }
    const uint32_t* pr = reinterpret_cast<const uint32_t*>(c);                   // 4-aligned: start | (length - 1) << 16
    while (a < b) {      // the last run that starts at or below `low`
        const uint32_t mid = (a + b) >> 1;
        if ((pr[mid] & 0xFFFFu) <= low) a = mid + 1;
        else b = mid;
    }
    if (a == 0) return false;
    const uint32_t p = pr[a - 1];
    return low - (p & 0xFFFFu) <= (p >> 16);
}

// one wave per tile of 64 rows: mask[t] = the allowed rows, cnt[1 + t] = how many (cnt is scanned in place afterwards)
__global__ __launch_bounds__(64 * kProbeWaves) void filter_probe_kernel(const uint64_t* __restrict__ ids, size_t n,
                                                                        const uint64_t* __restrict__ keys,
                                                                        const roaring::Entry* __restrict__ ents, uint32_t nc,
                                                                        const uint8_t* __restrict__ image,
                                                                        uint64_t* __restrict__ mask, uint64_t* __restrict__ cnt) {
    const size_t tile = (size_t)blockIdx.x * kProbeWaves + (threadIdx.x >> 6);
    const unsigned lane = threadIdx.x & 63u;
    const size_t row = tile * 64 + lane;
    bool ok = false;
    if (row < n) ok = filter_has(ids[row], keys, ents, nc, image);
    const uint64_t m = __ballot(ok);
    if (lane == 0 && tile * 64 < n) {
        mask[tile] = m;
        cnt[1 + tile] = (uint64_t)__popcll(m);
    }
}

// Hamming: lane = row, 8-byte id and 8-byte code
__global__ __launch_bounds__(256) void filter_gather_hamming_kernel(const uint64_t* __restrict__ ids,
                                                                    const uint64_t* __restrict__ rows, size_t n,
                                                                    const uint64_t* __restrict__ mask,
                                                                    const uint64_t* __restrict__ base, size_t n_out,
                                                                    uint64_t* __restrict__ out_ids, uint64_t* __restrict__ out_rows) {
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const size_t tile = row >> 6;
    const unsigned lane = (unsigned)(row & 63u);
    const uint64_t m = mask[tile];
    if (!((m >> lane) & 1ull)) return;
    const size_t dst = (size_t)base[tile] + (size_t)__popcll(m & ((1ull << lane) - 1ull));
    if (dst >= n_out) return;      // (cannot happen: the counts were scanned from these masks)
    out_ids[dst] = ids[row];
    out_rows[dst] = rows[row];
}

// Cosine: a workgroup of 4 waves per tile; wave w copies the allowed rows of rank w, w + 4, ... -- the row itself in
// 16-byte pieces where dim % 4 == 0 (rows of hipMalloc'ed buffers are then 16-byte aligned), its id and its norm.
__global__ __launch_bounds__(256) void filter_gather_cosine_kernel(const uint64_t* __restrict__ ids, const float* __restrict__ rows,
                                                                   const float* __restrict__ norms, size_t n, uint32_t dim,
                                                                   const uint64_t* __restrict__ mask,
                                                                   const uint64_t* __restrict__ base, size_t n_out,
                                                                   uint64_t* __restrict__ out_ids, float* __restrict__ out_rows,
                                                                   float* __restrict__ out_norms) {
    const size_t tile = blockIdx.x;
    if (tile * 64 >= n) return;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint64_t m = mask[tile];
    const size_t b0 = (size_t)base[tile];
    for (unsigned rank = 0; m; rank++, m &= m - 1ull) {
        if ((rank & 3u) != wave) continue;
        const size_t src = tile * 64 + (size_t)(__ffsll((unsigned long long)m) - 1);
        const size_t dst = b0 + rank;
        if (src >= n || dst >= n_out) return;      // (cannot happen)
        const float* s = rows + src * dim;
        float* d = out_rows + dst * dim;
        if ((dim & 3u) == 0) {
            const float4* s4 = reinterpret_cast<const float4*>(s);
            float4* d4 = reinterpret_cast<float4*>(d);
            for (uint32_t i = lane; i < dim / 4; i += 64) d4[i] = s4[i];
        } else {
            for (uint32_t i = lane; i < dim; i += 64) d[i] = s[i];
        }
        if (lane == 0) {
            out_ids[dst] = ids[src];
            out_norms[dst] = norms[src];
        }
    }
}

}  // namespace

void launch_filter_probe(const uint64_t* ids, size_t n, const uint64_t* keys, const void* ents, uint32_t nc, const uint8_t* image,
                         uint64_t* mask, uint64_t* cnt, hipStream_t stream) {
    if (n == 0) return;
    const size_t tiles = (n + 63) / 64;
    hipLaunchKernelGGL(filter_probe_kernel, dim3((unsigned)((tiles + kProbeWaves - 1) / kProbeWaves)), dim3(64 * kProbeWaves), 0,
                       stream, ids, n, keys, reinterpret_cast<const roaring::Entry*>(ents), nc, image, mask, cnt);
}

void launch_filter_gather_hamming(const uint64_t* ids, const uint64_t* rows, size_t n, const uint64_t* mask, const uint64_t* base,
                                  size_t n_out, uint64_t* out_ids, uint64_t* out_rows, hipStream_t stream) {
    if (n == 0 || n_out == 0) return;
    hipLaunchKernelGGL(filter_gather_hamming_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ids, rows, n, mask,
                       base, n_out, out_ids, out_rows);
}

void launch_filter_gather_cosine(const uint64_t* ids, const float* rows, const float* norms, size_t n, uint32_t dim,
                                 const uint64_t* mask, const uint64_t* base, size_t n_out, uint64_t* out_ids, float* out_rows,
                                 float* out_norms, hipStream_t stream) {
    if (n == 0 || n_out == 0) return;
    hipLaunchKernelGGL(filter_gather_cosine_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, stream, ids, rows, norms, n, dim,
                       mask, base, n_out, out_ids, out_rows, out_norms);
}

}  // namespace ucfp

extern "C" int ucfp_roaring_validate(const uint8_t* bytes, size_t len, uint64_t* cardinality) {
    char msg[160];
    msg[0] = 0;
    try {
        if (ucfp::roaring::parse(bytes, len, nullptr, cardinality, msg, sizeof msg) != 0) return ucfp::capi_fail(UCFP_E_INVALID, "%s", msg);
    } catch (const std::bad_alloc&) {
        return ucfp::capi_fail(UCFP_E_INDEX, "out of host memory while parsing a filter of %zu bytes", len);
    }
    return UCFP_OK;
}
