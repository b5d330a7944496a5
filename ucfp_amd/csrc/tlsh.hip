// tlsh.hip -- batched TLSH 128/1 digests for gfx950.
//
// Replaces the arithmetic behind the `tlsh` arm of the reference's text route (src/modality/text.rs:452-484, tag
// "tlsh-128-1"), i.e. txtfp's TlshFingerprinter over the bytes of the canonicalised text.  Spec (normative: DESIGN.md A15;
// CPU statement: tests/tlsh_ref.py): a sliding window of 5 bytes, six Pearson-hashed triplets per position into 128
// buckets, a Pearson checksum chained over the positions, the three quartiles of the counts, two bits per bucket.
//
// ONE WAVE PER DOCUMENT, no workgroup barrier.  The wave keeps the Pearson table (256 B), its 128 counters and a 256-byte
// stage of the text in LDS.
//   A  64 window positions per step, lane = position: five bytes from the stage, 18 table look-ups (the first level of
//      every triplet is folded into the salt: V[salt] ^ a0), one ds_add per bucket below 128.
//   B  the checksum is a dependent chain, one look-up per position: ck = V[t ^ ck] with t = V[V[1 ^ a0] ^ a1] computed
//      in A.  The chain stays in LDS: every lane reads the same byte (a broadcast), t of position j comes from lane j by
//      v_readlane.  One link costs a ds_read round trip (about 50 cycles issue to use on this part) plus the xor; it is
//      hidden by occupancy, not shortened: the kernel needs 1.2 KiB of LDS and few registers per wave, so 8 waves per SIMD
//      are resident and the other 7 issue while one waits.  Walking the chain through VGPR-held table registers with
//      v_readlane on scalar indices is the alternative (tlsh_kernel<true>, UCFP_TLSH_CHAIN=readlane): about 20 dependent
//      VALU / SALU issue slots per link that no other wave can hide.  Measured on 1 M documents of 4 KiB: 139 ms against
//      31.3 ms for the LDS chain, which is therefore the default; the other form stays for the comparison.
//   C  quartiles: lane = buckets lane and lane + 64; each counts how many of the 128 counters are below / not above its
//      own two (128 broadcast reads), the lane whose value has rank 31 / 63 / 95 inside that span hands it out.
// A document with at most 64 non-zero buckets is refused, so at least 65 of the 128 counts are non-zero and the sorted
// elements 63 .. 127 are: q2 and q3 cannot be 0 in a document that is not refused (the division below relies on it).
// Limits: one wave per document whatever its length (a 1 MiB document is a 1 Mi-link chain: tens of milliseconds);
// documents of 2^31 bytes or more are refused.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/ucfp_tlsh_ltab.h"
#include "ctx.h"

namespace {

using ucfp::capi_fail;

constexpr int kWavesPerBlock = 4;
constexpr uint32_t kMinLen = 50;
constexpr uint64_t kMaxLen = 1ull << 31;

#define UCFP_TLSH_PEARSON                                                                                                          \
    {1,   87,  49,  12,  176, 178, 102, 166, 121, 193, 6,   84,  249, 230, 44,  163, 14,  197, 213, 181, 161, 85,  218, 80,  64,  239, \
     24,  226, 236, 142, 38,  200, 110, 177, 104, 103, 141, 253, 255, 50,  77,  101, 81,  18,  45,  96,  31,  222, 25,  107, 190, 70,  \
     86,  237, 240, 34,  72,  242, 20,  214, 244, 227, 149, 235, 97,  234, 57,  22,  60,  250, 82,  175, 208, 5,   127, 199, 111, 62,  \
     135, 248, 174, 169, 211, 58,  66,  154, 106, 195, 245, 171, 17,  187, 182, 179, 0,   243, 132, 56,  148, 75,  128, 133, 158, 100, \
     130, 126, 91,  13,  153, 246, 216, 219, 119, 68,  223, 78,  83,  88,  201, 99,  122, 11,  92,  32,  136, 114, 52,  10,  138, 30,  \
     48,  183, 156, 35,  61,  26,  143, 74,  251, 94,  129, 162, 63,  152, 170, 7,   115, 167, 241, 206, 3,   150, 55,  59,  151, 220, \
     90,  53,  23,  131, 125, 173, 15,  238, 79,  95,  89,  16,  105, 137, 225, 224, 217, 160, 37,  123, 118, 73,  2,   157, 46,  116, \
     9,   145, 134, 228, 207, 212, 202, 215, 69,  229, 27,  188, 67,  124, 168, 252, 42,  4,   29,  108, 21,  247, 19,  205, 39,  203, \
     233, 40,  186, 147, 198, 192, 155, 33,  164, 191, 98,  204, 165, 180, 117, 76,  140, 36,  210, 172, 41,  54,  159, 8,   185, 232, \
     113, 196, 231, 47,  146, 120, 51,  65,  28,  144, 254, 221, 93,  189, 194, 139, 112, 43,  71,  109, 184, 209}

__device__ __attribute__((aligned(16))) const uint8_t d_pearson[256] = UCFP_TLSH_PEARSON;
__device__ const uint64_t d_ltab[UCFP_TLSH_LTAB_N] = UCFP_TLSH_LTAB_INIT;
const uint64_t h_ltab[UCFP_TLSH_LTAB_N] = UCFP_TLSH_LTAB_INIT;

// the pre-mapped salts V[2], V[3], V[5], V[7], V[11], V[13] (V[0] = 1 is the checksum's)
constexpr uint32_t kS2 = 49, kS3 = 12, kS5 = 178, kS7 = 166, kS11 = 84, kS13 = 230, kS0 = 1;

// the first class whose largest length is >= n
template <class T>
__host__ __device__ inline uint32_t length_class(const T* tab, uint64_t n) {
    uint32_t l = 0, r = UCFP_TLSH_LTAB_N - 1;   // tab[N - 1] = 2^64 - 1 >= n
    while (l < r) {
        const uint32_t m = (l + r) >> 1;
        if (tab[m] < n) l = m + 1;
        else r = m;
    }
    return l;
}

__host__ __device__ inline uint32_t swap_nibbles(uint32_t b) { return ((b & 15u) << 4) | ((b >> 4) & 15u); }

struct __attribute__((aligned(16))) WaveLds {
    uint8_t V[256];
    uint32_t hist[128];
    uint8_t stage[4 + 256 + 4];   // [0, 4): the four bytes before the chunk; [4, 260): the chunk
    uint8_t cls[128];
    uint8_t dig[40];
};

__device__ __forceinline__ void wave_sync() { ucfp::wave_lds_sync(); }

// REGWALK: the chain walks the table held in four registers (lane l of register k = V[64 k + l]) with v_readlane on
// scalar indices instead of reading it from LDS; everything else is the same code
template <bool REGWALK>
__global__ __launch_bounds__(64 * kWavesPerBlock) void tlsh_kernel(const uint8_t* __restrict__ bytes,
                                                                    const uint64_t* __restrict__ offsets, size_t n,
                                                                    uint8_t* __restrict__ out, int32_t* __restrict__ status) {
    __shared__ WaveLds lds[kWavesPerBlock];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t doc = (size_t)blockIdx.x * kWavesPerBlock + wave;
    if (doc >= n) return;   // whole wave
    WaveLds& W = lds[wave];
    const uint64_t o0 = offsets[doc], o1 = offsets[doc + 1];
    const uint64_t len = o1 > o0 ? o1 - o0 : 0;
    uint8_t* rec = out + doc * UCFP_TLSH_BYTES;
    if (len < kMinLen || len >= kMaxLen) {   // refused unread
        if (lane < (int)UCFP_TLSH_BYTES) rec[lane] = 0;
        if (status && lane == 0) status[doc] = UCFP_E_MODALITY;
        return;
    }
    const uint8_t* __restrict__ text = bytes + o0;
    const bool aligned4 = (reinterpret_cast<uintptr_t>(text) & 3u) == 0;
    reinterpret_cast<uint32_t*>(W.V)[lane] = reinterpret_cast<const uint32_t*>(d_pearson)[lane];
    W.hist[lane] = 0;
    W.hist[lane + 64] = 0;

    auto load_chunk = [&](uint64_t base) -> uint32_t {   // this lane's 4 bytes of [base, base + 256)
        const uint64_t o = base + 4 * (uint64_t)lane;
        if (o >= len) return 0u;
        if (aligned4 && o + 4 <= len) return *reinterpret_cast<const uint32_t*>(text + o);
        uint32_t v = 0;
        for (int j = 0; j < 4; j++)
            if (o + j < len) v |= (uint32_t)text[o + j] << (8 * j);
        return v;
    };
    auto bump = [&](uint32_t b) {
        if (b < 128u) atomicAdd(&W.hist[b], 1u);   // only buckets 0 .. 127 are kept
    };

    uint32_t ck = 0;   // the same value in every lane
    const int tv0 = d_pearson[lane], tv1 = d_pearson[64 + lane], tv2 = d_pearson[128 + lane], tv3 = d_pearson[192 + lane];
    auto link = [&](uint32_t c, uint32_t tj) -> uint32_t {   // c and tj are wave-uniform
        if (!REGWALK) return W.V[tj ^ c];
        const uint32_t idx = tj ^ c;
        const int l = (int)(idx & 63u);
        const uint32_t a = (uint32_t)__builtin_amdgcn_readlane(tv0, l), b = (uint32_t)__builtin_amdgcn_readlane(tv1, l);
        const uint32_t e = (uint32_t)__builtin_amdgcn_readlane(tv2, l), f = (uint32_t)__builtin_amdgcn_readlane(tv3, l);
        return idx < 128u ? (idx < 64u ? a : b) : (idx < 192u ? e : f);
    };
    uint32_t cur = load_chunk(0);
    for (uint64_t base = 0; base < len; base += 256) {
        const uint32_t nxt = load_chunk(base + 256);
        wave_sync();
        const uint32_t tail = *reinterpret_cast<const uint32_t*>(&W.stage[256]);   // bytes 252 .. 255 of the previous chunk
        wave_sync();
        if (lane == 0) *reinterpret_cast<uint32_t*>(&W.stage[0]) = tail;           // (unused for the first chunk)
        *reinterpret_cast<uint32_t*>(&W.stage[4 + 4 * lane]) = cur;
        wave_sync();
#pragma unroll 1
        for (int sub = 0; sub < 4; sub++) {
            const uint64_t s0 = base + 64 * (uint64_t)sub;
            if (s0 >= len) break;
            const uint64_t i = s0 + lane;
            const bool act = i >= 4 && i < len;
            const uint8_t* p = &W.stage[4 + 64 * sub + lane];
            uint32_t t = 0;
            if (act) {
                const uint32_t a0 = p[0], a1 = p[-1], a2 = p[-2], a3 = p[-3], a4 = p[-4];
                const uint8_t* V = W.V;
                t = V[V[kS0 ^ a0] ^ a1];
                const uint32_t v2 = V[V[kS2 ^ a0] ^ a1], v3 = V[V[kS3 ^ a0] ^ a1], v11 = V[V[kS11 ^ a0] ^ a1];
                const uint32_t v5 = V[V[kS5 ^ a0] ^ a2], v7 = V[V[kS7 ^ a0] ^ a2], v13 = V[V[kS13 ^ a0] ^ a3];
                bump(V[v2 ^ a2]);
                bump(V[v3 ^ a3]);
                bump(V[v5 ^ a3]);
                bump(V[v7 ^ a4]);
                bump(V[v11 ^ a4]);
                bump(V[v13 ^ a4]);
            }
            // the chain over this step's positions [lo, hi), in order
            const uint32_t lo = s0 == 0 ? 4u : 0u;
            const uint32_t hi = len - s0 < 64 ? (uint32_t)(len - s0) : 64u;
            if (lo == 0 && hi == 64) {
#pragma unroll
                for (int j = 0; j < 64; j++) ck = link(ck, (uint32_t)__builtin_amdgcn_readlane((int)t, j));
            } else {
                for (uint32_t j = lo; j < hi; j++) ck = link(ck, (uint32_t)__builtin_amdgcn_readlane((int)t, (int)j));
            }
        }
        cur = nxt;
    }
    wave_sync();

    // ---- quartiles of the 128 counts ----
    const uint32_t c0 = W.hist[lane], c1 = W.hist[lane + 64];
    const uint32_t nonzero = (uint32_t)__popcll(__ballot(c0 != 0)) + (uint32_t)__popcll(__ballot(c1 != 0));
    const bool ok = nonzero > 64;
    uint32_t less0 = 0, leq0 = 0, less1 = 0, leq1 = 0;
    for (int j = 0; j < 128; j++) {
        const uint32_t v = W.hist[j];
        less0 += v < c0 ? 1u : 0u;
        leq0 += v <= c0 ? 1u : 0u;
        less1 += v < c1 ? 1u : 0u;
        leq1 += v <= c1 ? 1u : 0u;
    }
    auto kth = [&](uint32_t r) -> uint32_t {   // element r of the sorted counts: some bucket's value spans rank r
        const uint64_t m0 = __ballot(less0 <= r && r < leq0);
        if (m0) return (uint32_t)__shfl((int)c0, __ffsll((unsigned long long)m0) - 1, 64);
        const uint64_t m1 = __ballot(less1 <= r && r < leq1);
        return (uint32_t)__shfl((int)c1, __ffsll((unsigned long long)m1) - 1, 64);
    };
    const uint32_t q1 = kth(31), q2 = kth(63), q3 = kth(95);
    W.cls[lane] = (uint8_t)((c0 > q1 ? 1u : 0u) + (c0 > q2 ? 1u : 0u) + (c0 > q3 ? 1u : 0u));
    W.cls[lane + 64] = (uint8_t)((c1 > q1 ? 1u : 0u) + (c1 > q2 ? 1u : 0u) + (c1 > q3 ? 1u : 0u));
    wave_sync();
    if (ok) {
        if (lane < 32) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(&W.cls[4 * lane]);
            W.dig[3 + 31 - lane] = (uint8_t)((w & 3u) | ((w >> 6) & 0xcu) | ((w >> 12) & 0x30u) | ((w >> 18) & 0xc0u));
        } else if (lane == 32) {
            const uint32_t L = length_class(d_ltab, len) & 255u;
            const uint32_t Q1 = (uint32_t)(((uint64_t)q1 * 100u / q3) & 15u), Q2 = (uint32_t)(((uint64_t)q2 * 100u / q3) & 15u);
            W.dig[0] = (uint8_t)swap_nibbles(ck & 255u);
            W.dig[1] = (uint8_t)swap_nibbles(L);
            W.dig[2] = (uint8_t)((Q1 << 4) | Q2);
        }
    }
    wave_sync();
    if (lane < (int)UCFP_TLSH_BYTES) rec[lane] = ok ? W.dig[lane] : (uint8_t)0;
    if (status && lane == 0) status[doc] = ok ? 0 : UCFP_E_MODALITY;
}

int tlsh_check(ucfp_ctx* ctx, const void* offsets, size_t n, const void* out) {
    if (!ctx) return capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (n && (!offsets || !out)) return capi_fail(UCFP_E_INVALID, "offsets/out is NULL");
    if (n > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "batch of %zu documents exceeds one launch", n);
    return UCFP_OK;
}

void launch_tlsh(const uint8_t* bytes, const uint64_t* offsets, size_t n, uint8_t* out, int32_t* status, hipStream_t st) {
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    const char* chain = getenv("UCFP_TLSH_CHAIN");   // "readlane": the register walk (DESIGN A15); anything else: LDS
    if (chain && !strcmp(chain, "readlane"))
        hipLaunchKernelGGL(tlsh_kernel<true>, dim3(grid), dim3(64 * kWavesPerBlock), 0, st, bytes, offsets, n, out, status);
    else
        hipLaunchKernelGGL(tlsh_kernel<false>, dim3(grid), dim3(64 * kWavesPerBlock), 0, st, bytes, offsets, n, out, status);
}

}  // namespace

extern "C" {

uint32_t ucfp_tlsh_lvalue(uint64_t n) { return length_class(h_ltab, n) & 255u; }

uint32_t ucfp_tlsh_distance(const uint8_t* a, const uint8_t* b) {
    if (!a || !b) return UCFP_TLSH_MAX_DISTANCE;
    auto md = [](uint32_t x, uint32_t y, uint32_t r) {
        const uint32_t d = x > y ? x - y : y - x;
        return d < r - d ? d : r - d;
    };
    uint32_t d = 0;
    const uint32_t l = md(swap_nibbles(a[1]), swap_nibbles(b[1]), 256);
    d += l <= 1 ? l : 12 * l;
    const uint32_t qa = md(a[2] >> 4, b[2] >> 4, 16), qb = md(a[2] & 15u, b[2] & 15u, 16);
    d += qa <= 1 ? qa : 12 * (qa - 1);
    d += qb <= 1 ? qb : 12 * (qb - 1);
    d += a[0] != b[0] ? 1u : 0u;
    for (int i = 3; i < (int)UCFP_TLSH_BYTES; i++)
        for (int j = 0; j < 8; j += 2) {
            const uint32_t x = (a[i] >> j) & 3u, y = (b[i] >> j) & 3u;
            const uint32_t e = x > y ? x - y : y - x;
            d += e == 3 ? 6u : e;
        }
    return d;
}

int ucfp_text_tlsh_batch_dev(ucfp_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, size_t n, uint8_t* d_out,
                             int32_t* d_status, void* stream) {
    int rc = tlsh_check(ctx, d_offsets, n, d_out);
    if (rc || n == 0) return rc;
    launch_tlsh(d_bytes, d_offsets, n, d_out, d_status, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UCFP_OK;
}

int ucfp_text_tlsh_batch(ucfp_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, size_t n, uint8_t* out, int32_t* status) {
    int rc = tlsh_check(ctx, offsets, n, out);
    if (rc || n == 0) return rc;
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return capi_fail(UCFP_E_INVALID, "offsets must be non-decreasing");
    const size_t base = offsets[0], total = offsets[n] - offsets[0];
    if (total && !bytes) return capi_fail(UCFP_E_INVALID, "bytes is NULL");
    const size_t o_off = (total + 16 + 255) & ~(size_t)255;
    const size_t in_bytes = o_off + (n + 1) * 8;
    const size_t o_st = (n * UCFP_TLSH_BYTES + 255) & ~(size_t)255;
    const size_t out_bytes = o_st + n * 4;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = ucfp::grow(&ctx->stage_in, &ctx->stage_in_cap, in_bytes))) return rc;
    if ((rc = ucfp::grow(&ctx->stage_out, &ctx->stage_out_cap, out_bytes))) return rc;
    hipStream_t st = ctx->host_stream;
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = offsets[i] - base;
    if (total) HIP_TRY(hipMemcpyAsync(ctx->stage_in, bytes + base, total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->stage_in + o_off, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    int32_t* d_st = reinterpret_cast<int32_t*>(ctx->stage_out + o_st);
    launch_tlsh(ctx->stage_in, reinterpret_cast<const uint64_t*>(ctx->stage_in + o_off), n, ctx->stage_out, d_st, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ctx->stage_out, n * UCFP_TLSH_BYTES, hipMemcpyDeviceToHost, st));
    if (status) HIP_TRY(hipMemcpyAsync(status, d_st, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return UCFP_OK;
}

}  // extern "C"
