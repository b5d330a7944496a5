// text_canon.hip -- text mode UCFP_TEXT_RAW_UTF8: canonicalise and tokenise UTF-8 documents on the GPU (gfx950).
//
// Replaces, for documents over the covered set, what the host did for every non-ASCII document before
// hashing: the canonicaliser (NFKC + case fold + Cf stripping, src/modality/text.rs:112-114) and the UAX#29 word
// tokeniser behind text::fingerprint_minhash_with (text.rs:182-236).  The result is the byte string the host path
// submits PRETOKENIZED -- canonical tokens joined by single spaces -- so text_hash_kernel (text.hip) runs unchanged
// over it.  Spec: DESIGN.md U1..U6; plain-Python restatement: tests/text_canon_ref.py; table: include/ucfp_text_utab.h.
//
// ONE WAVE PER DOCUMENT, 64 source bytes per step, no workgroup barrier.  The step body -- A + B canon_place, C + D
// canon_decide -- lives in text_canon_core.h, which the canon stage of text_stream_kernel (text_streams.hip) runs as well;
// the kernel below is the document's byte reader, the two passes' store (DocStore) and the state around them:
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

#include "ctx.h"
#include "text_canon_core.h"

namespace ucfp {

namespace {

__device__ const uint16_t d_stage1[UCFP_TEXT_UTAB_STAGE1_N] = UCFP_TEXT_UTAB_STAGE1_INIT;
__device__ const uint32_t d_stage2[UCFP_TEXT_UTAB_STAGE2_N] = UCFP_TEXT_UTAB_STAGE2_INIT;
__device__ const uint32_t d_pool[UCFP_TEXT_UTAB_POOL_N] = UCFP_TEXT_UTAB_POOL_INIT;
const uint16_t h_stage1[UCFP_TEXT_UTAB_STAGE1_N] = UCFP_TEXT_UTAB_STAGE1_INIT;
const uint32_t h_stage2[UCFP_TEXT_UTAB_STAGE2_N] = UCFP_TEXT_UTAB_STAGE2_INIT;
const uint32_t h_pool[UCFP_TEXT_UTAB_POOL_N] = UCFP_TEXT_UTAB_POOL_INIT;

// where a byte of the stream (' ' token)* goes: the output is that stream without its first byte, and the emit pass never
// writes past the length the count pass found.  EMIT = false: the count pass stores nothing.
template <bool EMIT>
struct DocStore {
    static constexpr bool kEmit = EMIT;
    uint8_t* out;
    uint64_t final_len;
    __device__ __forceinline__ void operator()(uint64_t p, uint8_t v) const {
        if (p >= 1 && p - 1 < final_len) out[p - 1] = v;
    }
};

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

    CanonSeg<uint64_t> S;
    const DocStore<EMIT> store{out, final_len};
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
        const CanonPlaced pl = canon_place(L, c, pos, len, lane, S.pend, d_stage1, d_stage2, d_pool);   // A, B
        if (pl.err) {
            bad = true;
            break;
        }
        canon_decide(L, S, c, pl.added, base + 64 >= len, lane, store);                                 // C, D
    }
    if (EMIT) return;
    const uint64_t out_pos = S.seg_alnum ? S.out_pos : S.seg_start;   // the last segment closes at the document's end
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

// the scan and the status merge on their own, for the grapheme tokeniser's canon pass (text_grapheme.hip)
void launch_text_canon_scan(uint64_t* tok_off, size_t n, hipStream_t stream) {
    hipLaunchKernelGGL(text_canon_scan_kernel, dim3(1), dim3(1024), 0, stream, tok_off, n);
}
void launch_text_canon_merge(const int32_t* cstatus, size_t n, int32_t* status, hipStream_t stream) {
    if (n) hipLaunchKernelGGL(text_canon_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, cstatus, n, status);
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
// PRETOKENIZED (MinHash: records of h slots), statuses merged.  total_bytes = d_offsets[n] - d_offsets[0].  Everything is enqueued on `stream`; users
// of the scratch on other streams are ordered by canon_done, as the users of norm_ws are.
int text_utf8_hash(ucfp_ctx* ctx, bool sim, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, size_t total_bytes,
                   uint32_t k, uint8_t* d_out, int32_t* d_status, hipStream_t stream, uint32_t h) {
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
    else launch_text_minhash(tokens, tok_off, n, UCFP_TEXT_PRETOKENIZED, k, d_out, d_status, stream, h);
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
