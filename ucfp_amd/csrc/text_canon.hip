// text_canon.hip -- text mode UCFP_TEXT_RAW_UTF8: canonicalise and tokenise UTF-8 documents on the GPU (gfx950).
//
// Replaces, for documents over the covered set, what the host did for every non-ASCII document before
// hashing: the canonicaliser (NFKC + case fold + Cf stripping, src/modality/text.rs:112-114) and the UAX#29 word
// tokeniser behind text::fingerprint_minhash_with (text.rs:182-236).  The result is the byte string the host path
// submits PRETOKENIZED -- canonical tokens joined by single spaces -- so text_hash_kernel (text.hip) runs unchanged
// over it.  Spec: DESIGN.md U1..U6; plain-Python restatement: tests/text_canon_ref.py; table: include/ucfp_text_utab.h.
//
// ONE WAVE PER DOCUMENT, 64 source bytes per step, no workgroup barrier:
//   A  lane = byte.  A lead lane assembles its code point from the LDS byte stage (3 bytes of the previous step before,
//      3 of the next behind) and validates it strictly (U2); a continuation lane checks that a lead claims it.
//   B  the lead lane looks its code point up in the two-stage table (global memory, ~100 KiB, L2-resident) and a wave
//      scan of the output counts places M(c) -- 0 .. 6 canonical code points with class / alnum / vowel flags -- in
//      the LDS stage `x`, behind two words of context and the one code point the previous step could not decide.
//   C  lane = canonical code point: "boundary before x[i]" is a function of x[i-2 .. i+1] (U4).  The last code point
//      of a step waits for its right neighbour, so it is decided in the next step (or at the document's end).
//   D  ballots of (boundary, alnum) give every lane its segment's extent and whether the segment is a token (U5);
//      a scan of the kept bytes gives the output position.  Only the segment still OPEN at the end of a chunk is
//      undecided: it is written provisionally and, if it closes without an alphanumeric (however many steps later),
//      the write position goes back to where it began -- `_` x 200 + ` ` leaves nothing, `_` x 200 + `a` one token.
//
// SIZING: count -> scan -> emit (template <bool EMIT>, as panako_triplet_kernel).  A fixed 4x slot per document would
// save the second pass but leaves holes, and the hash kernel takes ONE offsets array: it would have to read the slots'
// padding or learn begin/end arrays.  The canon pass is a small part of the route's time (the hash pass is ALU-bound),
// so the compact blob wins.  The emit pass knows the final length and never writes past it: a provisional segment
// cannot touch the next document's bytes.
//
// Output writes are plain byte stores of vector lanes.  After a rewind other lanes store to the same bytes again: a
// wavefront-scope fence keeps the two generations of stores in program order (a device-scope fence there wrote back and
// invalidated caches on every fifth chunk and dominated the pass).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "../../include/ucfp_text_utab.h"
#include "common.h"
#include "ctx.h"

namespace ucfp {

namespace {

constexpr int kWavesPerBlock = 4;
constexpr uint32_t kCpMask = 0x1FFFFu, kAlnum = 1u << 28, kVowel = 1u << 27, kFlagMask = 0xFu << 23 | kAlnum | kVowel;
constexpr uint32_t kNone = kCpMask | 15u << 23;   // "no code point": class 15 is in no class set, the value no apostrophe
// Canonical code points a step can add: a code point whose lead byte lies in the step has at most 3x its own bytes of
// canonical UTF-8 (U1), and those code points span at most 64 + 3 bytes.
constexpr int kStepCps = 3 * 67;
constexpr int kXCap = 2 + 1 + kStepCps + 4;

__device__ const uint16_t d_stage1[UCFP_TEXT_UTAB_STAGE1_N] = UCFP_TEXT_UTAB_STAGE1_INIT;
__device__ const uint32_t d_stage2[UCFP_TEXT_UTAB_STAGE2_N] = UCFP_TEXT_UTAB_STAGE2_INIT;
__device__ const uint32_t d_pool[UCFP_TEXT_UTAB_POOL_N] = UCFP_TEXT_UTAB_POOL_INIT;
const uint16_t h_stage1[UCFP_TEXT_UTAB_STAGE1_N] = UCFP_TEXT_UTAB_STAGE1_INIT;
const uint32_t h_stage2[UCFP_TEXT_UTAB_STAGE2_N] = UCFP_TEXT_UTAB_STAGE2_INIT;
const uint32_t h_pool[UCFP_TEXT_UTAB_POOL_N] = UCFP_TEXT_UTAB_POOL_INIT;

struct CanonLds {
    uint8_t bytes[3 + 64 + 3 + 2];   // [0, 3): the previous step's last bytes; [3, 67): this step; [67, 70): the next step's first
    uint32_t x[kXCap];               // [0, 2): context; then the undecided code point of the last step, then this step's
};

__device__ __forceinline__ uint32_t in_set(uint32_t w, uint32_t set) { return (set >> ((w >> 23) & 15u)) & 1u; }

// U4: no boundary before b, given the canonical code points around it (kNone where there is none)
__device__ __forceinline__ bool no_boundary(uint32_t aa, uint32_t a, uint32_t b, uint32_t bb) {
    constexpr uint32_t HEB = 1u << 2, AHL = 1u << 1 | HEB, NUM = 1u << 3, KAT = 1u << 4, ENL = 1u << 5;
    constexpr uint32_t SQ = 1u << 9, DQ = 1u << 10, MIDL = 1u << 6 | 1u << 8 | SQ, MIDN = 1u << 7 | 1u << 8 | SQ;
    uint32_t j = in_set(a, AHL) & in_set(b, AHL);
    j |= in_set(a, AHL) & in_set(b, MIDL) & in_set(bb, AHL);
    j |= in_set(aa, AHL) & in_set(a, MIDL) & in_set(b, AHL);
    j |= in_set(a, HEB) & in_set(b, SQ);
    j |= in_set(a, HEB) & in_set(b, DQ) & in_set(bb, HEB);
    j |= in_set(aa, HEB) & in_set(a, DQ) & in_set(b, HEB);
    j |= in_set(a, NUM) & in_set(b, NUM | AHL);
    j |= in_set(a, AHL) & in_set(b, NUM);
    j |= in_set(aa, NUM) & in_set(a, MIDN) & in_set(b, NUM);
    j |= in_set(a, NUM) & in_set(b, MIDN) & in_set(bb, NUM);
    j |= in_set(a, KAT) & in_set(b, KAT);
    j |= in_set(a, AHL | NUM | KAT | ENL) & in_set(b, ENL);
    j |= in_set(a, ENL) & in_set(b, AHL | NUM | KAT);
    const uint32_t ca = a & kCpMask;
    j |= (uint32_t)((ca == 0x27u || ca == 0x2019u) && (b & kVowel));   // the `regex` module's apostrophe tailoring
    return j != 0;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

}  // namespace

// EMIT = false: tok_off[doc + 1] = the document's token bytes, status[doc] = 0 / UCFP_TEXT_NEEDS_HOST.
// EMIT = true (after the scan): the token bytes go to tokens + tok_off[doc].
template <bool EMIT>
__global__ __launch_bounds__(64 * kWavesPerBlock) void text_canon_kernel(
    const uint8_t* __restrict__ utf8, const uint64_t* __restrict__ offsets, size_t n, uint64_t* __restrict__ tok_off,
    uint8_t* __restrict__ tokens, int32_t* __restrict__ status) {
    __shared__ CanonLds lds[kWavesPerBlock];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t doc = (size_t)blockIdx.x * kWavesPerBlock + wave;
    if (doc >= n) return;  // whole wave
    CanonLds& L = lds[wave];
    const uint8_t* __restrict__ text = utf8 + offsets[doc];
    const size_t len = (size_t)(offsets[doc + 1] - offsets[doc]);
    uint8_t* out = nullptr;
    uint64_t final_len = 0;
    if (EMIT) {
        if (status[doc] != 0) return;
        out = tokens + tok_off[doc];
        final_len = tok_off[doc + 1] - tok_off[doc];
        if (final_len == 0) return;
    }

    // wave-uniform state.  Positions count the stream (' ' token)*: the output is that stream without its first byte.
    uint32_t pend = 0;            // 1: x[2] holds a code point whose boundary waits for its right neighbour
    uint64_t out_pos = 0;         // stream bytes so far, the open segment included
    uint64_t seg_start = 0;       // where the open segment began
    bool seg_alnum = false;       // the open segment has an alphanumeric: it is a token
    bool bad = false;
    if (lane < 3) {
        L.x[lane] = kNone;
        L.bytes[lane] = 0;        // an ASCII byte: a continuation byte at the document's start is claimed by nobody
    }

    for (size_t base = 0; base < len; base += 64) {
        const size_t pos = base + lane;
        const uint32_t c = pos < len ? text[pos] : 0u;
        wave_lds_sync();
        L.bytes[3 + lane] = (uint8_t)c;
        if (lane < 3) L.bytes[67 + lane] = base + 64 + lane < len ? text[base + 64 + lane] : (uint8_t)0;
        wave_lds_sync();

        // ---- A: decode (U2) ----
        bool lead = false, err = false;
        uint32_t cp = c;
        if (pos < len) {
            if (c < 0x80u) {
                lead = true;
            } else if (c < 0xC0u) {   // continuation: the nearest byte before it that is none must be a lead that reaches it
                const uint32_t b1 = L.bytes[2 + lane], b2 = L.bytes[1 + lane], b3 = L.bytes[lane];
                const uint32_t j = (b1 & 0xC0u) != 0x80u ? 1u : (b2 & 0xC0u) != 0x80u ? 2u : (b3 & 0xC0u) != 0x80u ? 3u : 0u;
                const uint32_t lb = j == 1 ? b1 : j == 2 ? b2 : b3;
                const uint32_t reach = lb >= 0xF0u ? 3u : lb >= 0xE0u ? 2u : lb >= 0xC0u ? 1u : 0u;
                err = j == 0 || reach < j;
            } else {
                lead = true;
                const uint32_t need = c >= 0xF0u ? 3u : c >= 0xE0u ? 2u : 1u;
                const uint32_t c1 = L.bytes[4 + lane], c2 = L.bytes[5 + lane], c3 = L.bytes[6 + lane];
                err = c < 0xC2u || c > 0xF4u || pos + need >= len || (c1 & 0xC0u) != 0x80u;
                if (need == 1) {
                    cp = (c & 0x1Fu) << 6 | (c1 & 0x3Fu);
                } else if (need == 2) {
                    cp = (c & 0x0Fu) << 12 | (c1 & 0x3Fu) << 6 | (c2 & 0x3Fu);
                    err |= (c2 & 0xC0u) != 0x80u || cp < 0x800u || cp - 0xD800u < 0x800u;
                } else {
                    cp = (c & 0x07u) << 18 | (c1 & 0x3Fu) << 12 | (c2 & 0x3Fu) << 6 | (c3 & 0x3Fu);
                    err |= (c2 & 0xC0u) != 0x80u || (c3 & 0xC0u) != 0x80u || cp < 0x10000u || cp > 0x10FFFFu;
                }
            }
        }
        // ---- B: M(c) through the table (U1, U3) ----
        uint32_t e = 0, nout = 0;
        if (lead && !err) {
            if (cp >= UCFP_TEXT_UTAB_LIMIT) {
                err = true;
            } else {
                e = d_stage2[((uint32_t)d_stage1[cp >> UCFP_TEXT_UTAB_SHIFT] << UCFP_TEXT_UTAB_SHIFT) |
                             (cp & ((1u << UCFP_TEXT_UTAB_SHIFT) - 1u))];
                if (!(e >> 31)) err = true;
                else nout = ((e >> 29) & 3u) == 2u ? (e >> 17) & 7u : 1u;
            }
        }
        if (__ballot(err)) {
            bad = true;
            break;
        }
        const uint32_t incl = wave_incl_scan(nout, lane);
        const uint32_t added = __shfl(incl, 63, 64);
        if (nout) {
            const uint32_t at = 2u + pend + incl - nout;   // < 2 + 1 + kStepCps
            const uint32_t kind = (e >> 29) & 3u;
            if (kind == 0) L.x[at] = cp | (e & kFlagMask);
            else if (kind == 1) L.x[at] = (e & kCpMask) | (e & kFlagMask);
            else
                for (uint32_t t = 0; t < nout; t++) L.x[at + t] = d_pool[(e & kCpMask) + t];
        }
        wave_lds_sync();

        // ---- C, D: boundaries, segments, tokens ----
        const bool final = base + 64 >= len;
        const uint32_t m = pend + added;
        const uint32_t ndec = final ? m : (m ? m - 1u : 0u);
        for (uint32_t j0 = 0; j0 < ndec; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool has = j < ndec;
            const uint32_t i = 2u + j;
            uint32_t w = kNone;
            bool bnd = false;
            if (has) {
                w = L.x[i];
                bnd = !no_boundary(L.x[i - 2], L.x[i - 1], w, j + 1 < m ? L.x[i + 1] : kNone);
            }
            const uint64_t bmask = __ballot(bnd), amask = __ballot(has && (w & kAlnum));
            // the carried segment runs up to the first boundary of the chunk; closed there without an alphanumeric, it goes
            const int fb = bmask ? __builtin_ctzll(bmask) : 64;
            const bool carried_has = seg_alnum || (amask & (fb == 64 ? ~0ull : (1ull << fb) - 1ull)) != 0;
            const bool drop0 = bmask != 0 && !carried_has;
            // this lane's segment: [its last boundary at or before the lane, the next boundary)
            const uint64_t le = bmask & (~0ull >> (63 - lane));
            const int sb = le ? 63 - __builtin_clzll(le) : -1;
            const uint64_t gt = lane == 63 ? 0ull : bmask & (~0ull << (lane + 1));
            const int eb = gt ? __builtin_ctzll(gt) : 64;
            const uint64_t range = (eb == 64 ? ~0ull : (1ull << eb) - 1ull) & (sb <= 0 ? ~0ull : ~((1ull << sb) - 1ull));
            const bool seg_has = (amask & range) != 0 || (sb < 0 && seg_alnum);
            const bool keep = has && (eb == 64 || seg_has);   // the open segment is kept provisionally
            const uint32_t cpw = w & kCpMask;
            const uint32_t nb = cpw < 0x80u ? 1u : cpw < 0x800u ? 2u : cpw < 0x10000u ? 3u : 4u;
            const uint32_t contrib = keep ? nb + (bnd ? 1u : 0u) : 0u;
            const uint32_t cincl = wave_incl_scan(contrib, lane);
            const uint32_t excl = cincl - contrib;
            const uint64_t base_pos = drop0 ? seg_start : out_pos;
            if (EMIT) {
                // A rewind: other lanes are about to store where the provisional bytes went.  One wave's stores are issued in
                // program order, so a fence at WAVEFRONT scope is all the ordering the two generations of stores need.
                if (drop0) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                if (keep) {
                    uint64_t p = base_pos + excl;   // stream position; the output byte is p - 1
                    uint32_t bytes, cnt = nb;
                    if (nb == 1) bytes = cpw;
                    else if (nb == 2) bytes = (0xC0u | cpw >> 6) | (0x80u | (cpw & 0x3Fu)) << 8;
                    else if (nb == 3) bytes = (0xE0u | cpw >> 12) | (0x80u | (cpw >> 6 & 0x3Fu)) << 8 | (0x80u | (cpw & 0x3Fu)) << 16;
                    else
                        bytes = (0xF0u | cpw >> 18) | (0x80u | (cpw >> 12 & 0x3Fu)) << 8 | (0x80u | (cpw >> 6 & 0x3Fu)) << 16 |
                                (0x80u | (cpw & 0x3Fu)) << 24;
                    if (bnd) {
                        if (p >= 1 && p - 1 < final_len) out[p - 1] = ' ';
                        p++;
                    }
                    for (uint32_t t = 0; t < cnt; t++, p++)
                        if (p >= 1 && p - 1 < final_len) out[p - 1] = (uint8_t)(bytes >> (8 * t));
                }
            }
            if (bmask) {
                const int hb = 63 - __builtin_clzll(bmask);
                seg_start = base_pos + __shfl(excl, hb, 64);
                seg_alnum = (amask >> hb) != 0;
            } else {
                seg_alnum = seg_alnum || amask != 0;
            }
            out_pos = base_pos + __shfl(cincl, 63, 64);
        }
        // context for the next step: the last two decided code points and the undecided one
        wave_lds_sync();
        const uint32_t keep3 = lane < 3 ? L.x[ndec + lane] : 0u;
        wave_lds_sync();
        if (lane < 3) L.x[lane] = keep3;
        if (lane >= 61) L.bytes[lane - 61] = (uint8_t)c;
        pend = m - ndec;
    }
    if (EMIT) return;
    if (!seg_alnum) out_pos = seg_start;   // the last segment closes at the document's end
    if (lane == 0) {
        tok_off[doc + 1] = bad || out_pos == 0 ? 0ull : out_pos - 1;
        status[doc] = bad ? UCFP_TEXT_NEEDS_HOST : 0;
    }
}

// off[1 .. n] hold the documents' token bytes: -> off[0] = 0, off[i + 1] = the bytes of documents 0 .. i (one workgroup)
__global__ __launch_bounds__(1024) void text_canon_scan_kernel(uint64_t* __restrict__ off, size_t n) {
    __shared__ uint64_t tot[1024];
    const size_t tid = threadIdx.x, per = (n + 1023) / 1024;
    const size_t i0 = tid * per < n ? tid * per : n, i1 = i0 + per < n ? i0 + per : n;
    uint64_t s = 0;
    for (size_t i = i0; i < i1; i++) s += off[1 + i];
    tot[tid] = s;
    __syncthreads();
    for (unsigned d = 1; d < 1024; d <<= 1) {
        const uint64_t v = tid >= d ? tot[tid - d] : 0ull;
        __syncthreads();
        tot[tid] += v;
        __syncthreads();
    }
    uint64_t run = tid ? tot[tid - 1] : 0ull;
    for (size_t i = i0; i < i1; i++) {
        run += off[1 + i];
        off[1 + i] = run;
    }
    if (tid == 0) off[0] = 0;
}

// the canon pass's NEEDS_HOST wins over the hash pass's status (the record of an empty token string is already zero)
__global__ void text_canon_merge_kernel(const int32_t* __restrict__ cstatus, size_t n, int32_t* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && cstatus[i] != 0) status[i] = cstatus[i];
}

int launch_text_canon(const uint8_t* utf8, const uint64_t* offsets, size_t n, uint8_t* tokens, uint64_t* tok_off,
                      int32_t* status, hipStream_t stream) {
    if (n == 0) return 0;
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(text_canon_kernel<false>, dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, utf8, offsets, n, tok_off,
                       tokens, status);
    hipLaunchKernelGGL(text_canon_scan_kernel, dim3(1), dim3(1024), 0, stream, tok_off, n);
    hipLaunchKernelGGL(text_canon_kernel<true>, dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, utf8, offsets, n, tok_off,
                       tokens, status);
    return 0;
}

// The device addresses of the code-point table, for the streaming canonicaliser (text_streams.hip): one copy of the
// table serves both, so what the offline path keeps L2-resident is what a stream push reads.  The tables have internal
// linkage (the runtime cannot look them up by name), so a one-thread kernel reports where they are.
__global__ void text_canon_tables_kernel(const void** out) {
    out[0] = d_stage1;
    out[1] = d_stage2;
    out[2] = d_pool;
}

int text_canon_tables(int device, const uint16_t** stage1, const uint32_t** stage2, const uint32_t** pool) {
    static std::mutex mu;
    static std::vector<const void*> known;   // three addresses per device, asked for once
    std::lock_guard<std::mutex> lk(mu);
    if (device < 0) return capi_fail(UCFP_E_INVALID, "device %d", device);
    if (known.size() < 3 * ((size_t)device + 1)) known.resize(3 * ((size_t)device + 1), nullptr);
    const void** h = &known[3 * (size_t)device];
    if (!h[0]) {
        const void** d = nullptr;
        const void* got[3] = {nullptr, nullptr, nullptr};
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMalloc((void**)&d, sizeof(got)));
        hipLaunchKernelGGL(text_canon_tables_kernel, dim3(1), dim3(1), 0, nullptr, d);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(got, d, sizeof(got), hipMemcpyDeviceToHost);   // waits for the kernel
        (void)hipFree(d);
        HIP_TRY(e);
        h[0] = got[0], h[1] = got[1], h[2] = got[2];
    }
    *stage1 = static_cast<const uint16_t*>(h[0]);
    *stage2 = static_cast<const uint32_t*>(h[1]);
    *pool = static_cast<const uint32_t*>(h[2]);
    return UCFP_OK;
}

// Mode UCFP_TEXT_RAW_UTF8 of the MinHash / SimHash calls: canon pass into the context's scratch, the hash pass over it
// PRETOKENIZED, statuses merged.  total_bytes = d_offsets[n] - d_offsets[0].  Everything is enqueued on `stream`; users
// of the scratch on other streams are ordered by canon_done, as the users of norm_ws are.
int text_utf8_hash(ucfp_ctx* ctx, bool sim, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, size_t total_bytes,
                   uint32_t k, uint8_t* d_out, int32_t* d_status, hipStream_t stream) {
    if (n == 0) return UCFP_OK;
    const size_t o_st = ((n + 1) * 8 + 255) & ~(size_t)255;
    const size_t o_tok = o_st + ((n * 4 + 255) & ~(size_t)255);
    const size_t need = o_tok + ucfp_text_canon_bound(total_bytes) + 64;   // the hash kernel reads whole dwords
    std::lock_guard<std::mutex> lk(ctx->canon_mu);
    HIP_TRY(hipStreamWaitEvent(stream, ctx->canon_done, 0));
    const int rc = grow(&ctx->canon_ws, &ctx->canon_ws_cap, need);   // (a hipFree waits for the device: no user is left)
    if (rc) return rc;
    uint64_t* tok_off = reinterpret_cast<uint64_t*>(ctx->canon_ws);
    int32_t* cstatus = reinterpret_cast<int32_t*>(ctx->canon_ws + o_st);
    uint8_t* tokens = ctx->canon_ws + o_tok;
    launch_text_canon(d_utf8, d_offsets, n, tokens, tok_off, cstatus, stream);
    if (sim) launch_text_simhash(tokens, tok_off, n, UCFP_TEXT_PRETOKENIZED, d_out, d_status, stream);
    else launch_text_minhash(tokens, tok_off, n, UCFP_TEXT_PRETOKENIZED, k, d_out, d_status, stream);
    if (d_status)
        hipLaunchKernelGGL(text_canon_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, cstatus, n, d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->canon_done, stream));
    return UCFP_OK;
}

}  // namespace ucfp

extern "C" {

const char* ucfp_text_utab_versions(void) { return "unicodedata " UCFP_TEXT_UTAB_UNIDATA " regex " UCFP_TEXT_UTAB_REGEX; }

int ucfp_text_utab_lookup(uint32_t cp, uint32_t out_cps[8], uint32_t* n, uint32_t* cls_flags) {
    using namespace ucfp;
    if (n) *n = 0;
    if (cls_flags) *cls_flags = 0;
    if (cp >= UCFP_TEXT_UTAB_LIMIT) return 0;
    const uint32_t e = h_stage2[((uint32_t)h_stage1[cp >> UCFP_TEXT_UTAB_SHIFT] << UCFP_TEXT_UTAB_SHIFT) |
                                (cp & ((1u << UCFP_TEXT_UTAB_SHIFT) - 1u))];
    if (!(e >> 31)) return 0;
    const uint32_t kind = (e >> 29) & 3u;
    if (kind == 2) {
        const uint32_t len = (e >> 17) & 7u;
        for (uint32_t t = 0; t < len && out_cps; t++) out_cps[t] = h_pool[(e & kCpMask) + t] & kCpMask;
        if (n) *n = len;
        return 1;
    }
    if (out_cps) out_cps[0] = kind == 0 ? cp : e & kCpMask;
    if (n) *n = 1;
    if (cls_flags) *cls_flags = ((e >> 23) & 15u) | (e & kAlnum ? 16u : 0u) | (e & kVowel ? 32u : 0u);
    return 1;
}

size_t ucfp_text_canon_bound(size_t n_bytes) { return n_bytes > SIZE_MAX / 4 ? SIZE_MAX : 4 * n_bytes; }

int ucfp_text_canon_batch_dev(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, uint8_t* d_tokens,
                              uint64_t* d_tok_offsets, int32_t* d_status, void* stream) {
    if (!ctx) return ucfp::capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (n > 0x7fffffffu) return ucfp::capi_fail(UCFP_E_INVALID, "batch of %zu documents exceeds one launch", n);
    if (n && (!d_offsets || !d_tokens || !d_tok_offsets || !d_status))
        return ucfp::capi_fail(UCFP_E_INVALID, "offsets/tokens/tok_offsets/status is NULL");
    (void)d_utf8;
    ucfp::launch_text_canon(d_utf8, d_offsets, n, d_tokens, d_tok_offsets, d_status, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UCFP_OK;
}

int ucfp_text_canon_batch(ucfp_ctx* ctx, const uint8_t* utf8, const uint64_t* offsets, size_t n, uint8_t* tokens,
                          size_t tokens_cap, uint64_t* tok_offsets, int32_t* status) {
    if (!ctx) return ucfp::capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (n > 0x7fffffffu) return ucfp::capi_fail(UCFP_E_INVALID, "batch of %zu documents exceeds one launch", n);
    if (n == 0) {
        if (tok_offsets) tok_offsets[0] = 0;
        return UCFP_OK;
    }
    if (!offsets || !tok_offsets || !status) return ucfp::capi_fail(UCFP_E_INVALID, "offsets/tok_offsets/status is NULL");
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return ucfp::capi_fail(UCFP_E_INVALID, "offsets must be non-decreasing");
    const size_t base = offsets[0], total = offsets[n] - offsets[0];
    if (total && !utf8) return ucfp::capi_fail(UCFP_E_INVALID, "utf8 is NULL");
    const size_t o_off = (total + 16 + 255) & ~(size_t)255;
    const size_t in_bytes = o_off + (n + 1) * 8;
    const size_t o_st = ((n + 1) * 8 + 255) & ~(size_t)255;
    const size_t o_tok = o_st + ((n * 4 + 255) & ~(size_t)255);
    const size_t out_bytes = o_tok + ucfp_text_canon_bound(total) + 64;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = ucfp::grow(&ctx->stage_in, &ctx->stage_in_cap, in_bytes);
    if (rc) return rc;
    rc = ucfp::grow(&ctx->stage_out, &ctx->stage_out_cap, out_bytes);
    if (rc) return rc;
    hipStream_t st = ctx->host_stream;
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = offsets[i] - base;
    if (total) HIP_TRY(hipMemcpyAsync(ctx->stage_in, utf8 + base, total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->stage_in + o_off, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    uint64_t* d_toff = reinterpret_cast<uint64_t*>(ctx->stage_out);
    ucfp::launch_text_canon(ctx->stage_in, reinterpret_cast<const uint64_t*>(ctx->stage_in + o_off), n, ctx->stage_out + o_tok,
                            d_toff, reinterpret_cast<int32_t*>(ctx->stage_out + o_st), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(tok_offsets, d_toff, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(status, ctx->stage_out + o_st, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const size_t made = (size_t)tok_offsets[n];
    if (made > tokens_cap || (made && !tokens))
        return ucfp::capi_fail(UCFP_E_INVALID, "the token blob has %zu bytes, the caller's buffer %zu (ucfp_text_canon_bound)", made,
                               tokens_cap);
    if (made) {
        HIP_TRY(hipMemcpyAsync(tokens, ctx->stage_out + o_tok, made, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return UCFP_OK;
}

}  // extern "C"
