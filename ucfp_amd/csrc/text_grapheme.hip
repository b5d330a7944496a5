// text_grapheme.hip -- the grapheme tokeniser and caller-segmented tokens for MinHash-128 / SimHash-64 on gfx950.
//
// Replaces, for `tokenizer = grapheme` (src/server/dto.rs, handlers.rs:532-539), txtfp's GraphemeTokenizer behind
// ShingleTokenizer { k, inner } (src/modality/text.rs:66-83, 194-219) and the raw tokens SimHash is fed (text.rs:379-398);
// and gives any tokeniser the host runs itself (the reference's cjk-jp / cjk-ko) a way to hand its tokens to the GPU hash
// without a separator byte.  Spec: DESIGN.md T8 (G1..G8); plain-Python restatement: tests/text_grapheme_ref.py.
//
// ONE WAVE PER DOCUMENT, 64 bytes per step, the LDS batch, flush and record of text_core.h: the shape of text_hash_kernel
// (text.hip).  What differs is the step (text_step_marked): every byte is a token byte, tokens abut, and the token STARTS
// are a 64-bit mask the reader makes:
//   G_ASCII   a start at every byte but an LF whose previous byte is CR (one ballot; the previous byte of lane 0 is carried
//             from step to step, so a CR LF pair may straddle a step or a 256-byte chunk).  A-Z are lower-cased, a byte
//             >= 0x80 hands the document back.  One launch.
//   G_CANON   the same over canonical UTF-8, a start at every non-continuation byte.  Its input is the whole U3 stream,
//             written by text_gcanon_kernel below (count -> scan -> emit, as text_canon.hip sizes its blob): canon_place
//             of text_canon_core.h decodes, validates and maps, canon_whole re-encodes and decides the G3 hand-back.
//   G_TOKENS  starts come from the caller's token table.  The wave walks its slice of tok_offsets with a cursor, 64
//             entries at a time; an entry inside the step marks its byte in a 64-byte LDS row and one ballot reads the
//             row.  Two starts on one byte are one mark, which is the empty-token rule (G7).  The tables of a _dev call
//             are checked by the document's own wave before it reads a byte of the blob: a decreasing pair, or a range
//             outside the announced one, gives UCFP_E_INVALID and a zero record.
// The fold (text_flush, part D of text.hip's header) sees about six times the shingles per byte of the word route.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "ctx.h"
#include "text_canon_core.h"
#include "text_core.h"

namespace ucfp {

namespace {

enum { G_ASCII = 0, G_CANON = 1, G_TOKENS = 2 };

// the canon pass's store: stream position p of the document's canonical bytes, never past the length the count pass found
template <bool EMIT>
struct WholeStore {
    static constexpr bool kEmit = EMIT;
    uint8_t* out;
    uint64_t final_len;
    __device__ __forceinline__ void operator()(uint64_t p, uint8_t v) const {
        if (p < final_len) out[p] = v;
    }
};

}  // namespace

// EMIT = false: can_off[doc + 1] = the document's canonical bytes, status[doc] = 0 / UCFP_TEXT_NEEDS_HOST.
// EMIT = true (after the scan): the canonical bytes go to canon + can_off[doc].
template <bool EMIT>
__global__ __launch_bounds__(64 * kWavesPerBlock) void text_gcanon_kernel(
    const uint8_t* __restrict__ utf8, const uint64_t* __restrict__ offsets, size_t n, uint64_t* __restrict__ can_off,
    uint8_t* __restrict__ canon, int32_t* __restrict__ status, const uint16_t* __restrict__ stage1,
    const uint32_t* __restrict__ stage2, const uint32_t* __restrict__ pool) {
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
        out = canon + can_off[doc];
        final_len = can_off[doc + 1] - can_off[doc];
        if (final_len == 0) return;
    }
    const WholeStore<EMIT> store{out, final_len};
    uint64_t out_pos = 0;
    bool bad = false;
    if (lane < 3) L.bytes[lane] = 0;   // an ASCII byte: a continuation byte at the document's start is claimed by nobody

    for (size_t base = 0; base < len; base += 64) {
        const size_t pos = base + lane;
        const uint32_t c = pos < len ? text[pos] : 0u;
        wave_lds_sync();
        L.bytes[3 + lane] = (uint8_t)c;
        if (lane < 3) L.bytes[67 + lane] = base + 64 + lane < len ? text[base + 64 + lane] : (uint8_t)0;
        wave_lds_sync();
        const CanonPlaced pl = canon_place(L, c, pos, len, lane, 0u, stage1, stage2, pool);
        if (pl.err || !canon_whole(L, out_pos, c, pl.added, lane, store)) {
            bad = true;
            break;
        }
    }
    if (EMIT) return;
    if (lane == 0) {
        can_off[doc + 1] = bad ? 0ull : out_pos;
        status[doc] = bad ? UCFP_TEXT_NEEDS_HOST : 0;
    }
}

// MODE = T_MIN (false): MinHash (out 1032 B/doc); T_SIM (true): SimHash (out 8 B/doc); T_IDF / T_KEYS as text_hash_kernel.  G_ASCII / G_CANON: document i is
// bytes[offsets[i], offsets[i + 1]).  G_TOKENS: `offsets` is doc_tokens, token t is bytes[tok_off[t], tok_off[t + 1]).
// NR and h as in text_hash_kernel: NR = 0 the 128-slot record, NR >= 1 MinHash with h slots (out 8 + 8 h B/doc).
template <int MODE, int SRC, int NR = 0>
__global__ __launch_bounds__(64 * kWavesPerBlock) void text_marked_kernel(
    const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ tok_off, size_t n,
    uint32_t k, uint8_t* __restrict__ out, int32_t* __restrict__ status, TextIdfAux aux, uint32_t h) {
    constexpr int R = NR ? NR : 2;
    const uint32_t slots = NR ? h : 128u;
    __shared__ WaveLds lds[kWavesPerBlock];
    __shared__ uint8_t marks[SRC == G_TOKENS ? kWavesPerBlock : 1][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t doc = (size_t)blockIdx.x * kWavesPerBlock + wave;
    if (doc >= n) return;  // whole wave
    WaveLds& L = lds[wave];
    uint8_t* mark = marks[SRC == G_TOKENS ? wave : 0];

    uint64_t b0, b1, tcur = 0, t1 = 0;
    bool invalid = false;
    if (SRC == G_TOKENS) {
        // the announced ranges: tokens [T0, T1] of the table, bytes [lo, hi) of the blob
        const uint64_t T0 = offsets[0], T1 = offsets[n];
        const uint64_t t0 = offsets[doc];
        t1 = offsets[doc + 1];
        tcur = t0;
        b0 = b1 = 0;
        invalid = !(T0 <= t0 && t0 <= t1 && t1 <= T1);
        if (!invalid) {
            const uint64_t lo = tok_off[T0], hi = tok_off[T1];
            b0 = tok_off[t0];
            b1 = tok_off[t1];
            invalid = !(lo <= b0 && b0 <= b1 && b1 <= hi);
            bool dec = false;
            if (!invalid)
                for (uint64_t t = t0 + lane; t < t1; t += 64) dec |= tok_off[t] > tok_off[t + 1];
            invalid = invalid || __ballot(dec) != 0;
        }
        if (invalid) b0 = b1 = 0;
    } else {
        b0 = offsets[doc];
        b1 = offsets[doc + 1];
    }
    const uint8_t* __restrict__ text = bytes + b0;
    const size_t len = (size_t)(b1 - b0);
    const bool aligned4 = (reinterpret_cast<uintptr_t>(text) & 3u) == 0;

    TextWave W;
    uint64_t mx[text_mx_len(R)];
#pragma unroll
    for (int r = 0; r < text_mx_len(R); r++) mx[r] = ~0ull;
    bool nonascii = false, too_long = false;
    uint32_t prev_last = 0;   // the byte before the step's first (CR LF across a step)
    if (MODE == T_KEYS) {   // slots by bytes; by announced tokens for a token table (empty tokens merge: never more are cut)
        if (SRC == G_TOKENS) text_keys_doc(aux, tcur, invalid ? 0 : (size_t)(t1 - tcur), doc);
        else text_keys_doc(aux, b0, len, doc);
    }

    // ---- stream the document, 256 bytes per outer iteration, 64 per step (the reader of text_hash_kernel) ----
    auto load_chunk = [&](size_t base) -> uint32_t {  // this lane's 4 bytes of [base, base + 256)
        const size_t o = base + 4 * (size_t)lane;
        if (o >= len) return 0u;
        if (aligned4 && o + 4 <= len) return *reinterpret_cast<const uint32_t*>(text + o);
        uint32_t v = 0;
        for (int j = 0; j < 4; j++)
            if (o + j < len) v |= (uint32_t)text[o + j] << (8 * j);
        return v;
    };
    uint32_t cur = load_chunk(0);
    for (size_t base = 0; base < len && !too_long; base += 256) {
        const uint32_t nxt = load_chunk(base + 256);
        wave_sync();
        *reinterpret_cast<uint32_t*>(&L.stage[4 * lane]) = cur;
        wave_sync();
        if (SRC == G_ASCII) nonascii |= (cur & 0x80808080u) != 0;
#pragma unroll 1
        for (int sub = 0; sub < 4; sub++) {
            const size_t pos = base + 64 * sub + lane;
            if (base + 64 * sub >= len) break;
            if (text_batch_full_marked(W)) {   // make room
                text_flush<MODE, R>(L, W, k, lane, false, &aux, mx);
                if (text_batch_full_marked(W)) too_long = true;
                if (too_long) break;
            }
            const uint32_t c = L.stage[64 * sub + lane];
            uint32_t ch = c;
            uint64_t starts;
            if (SRC == G_TOKENS) {
                const uint64_t step0 = b0 + base + 64 * (size_t)sub;
                const uint64_t step1 = step0 + 64 < b1 ? step0 + 64 : b1;
                mark[lane] = 0;
                wave_sync();
                for (;;) {   // the table entries that fall into this step: a prefix of what the cursor sees (the table was checked)
                    const uint64_t t = tcur + lane;
                    const uint64_t o = t < t1 ? tok_off[t] : ~0ull;
                    const uint64_t in = __ballot(o < step1);
                    const uint32_t cnt = in == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~in);
                    if ((uint32_t)lane < cnt && o >= step0) mark[o - step0] = 1;
                    tcur += cnt;
                    if (cnt < 64u) break;
                }
                wave_sync();
                starts = __ballot(mark[lane] != 0);
            } else {
                uint32_t p = __shfl_up(c, 1, 64);
                if (lane == 0) p = prev_last;
                bool st = !(c == 0x0Au && p == 0x0Du);                        // CR LF is one cluster
                if (SRC == G_CANON) st = st && (c & 0xC0u) != 0x80u;           // a cluster = one canonical code point
                if (SRC == G_ASCII && ch - 'A' <= 25u) ch += 32;
                starts = __ballot(st);
                prev_last = __shfl(c, 63, 64);
            }
            text_step_marked(L, W, ch, starts, pos, len, lane);
        }
        cur = nxt;
    }
    // close the token that runs to the end of the document, then the final flush
    if (W.carry && W.ntok > 0 && lane == 0) L.cend[W.ntok - 1] = (uint16_t)(W.cbase + W.ntok - 1);
    if (!too_long) text_flush<MODE, R>(L, W, k, lane, true, &aux, mx);
    // ---- emit ----
    int32_t stv = text_emit<MODE, R>(out + doc * (MODE != T_MIN ? 8 : 8 + 8 * (size_t)slots), W, __ballot(nonascii) != 0,
                                     too_long || invalid, lane, slots, mx);
    if (invalid) stv = UCFP_E_INVALID;
    if (status && lane == 0) status[doc] = stv;
}

namespace {

template <int SRC, int NR>
void launch_marked_nr(const uint8_t* bytes, const uint64_t* offsets, const uint64_t* tok_off, size_t n, uint32_t k, uint32_t h,
                      uint8_t* out, int32_t* status, hipStream_t stream) {
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL((text_marked_kernel<T_MIN, SRC, NR>), dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, bytes, offsets,
                       tok_off, n, k, out, status, TextIdfAux{}, h);
}

// MinHash: h = 128 is the kernel of the 128-slot entries; any other h the instantiation of text_minhash_nr(h) minima per lane
template <int SRC>
void launch_marked(bool sim, const uint8_t* bytes, const uint64_t* offsets, const uint64_t* tok_off, size_t n, uint32_t k,
                   uint8_t* out, int32_t* status, hipStream_t stream, uint32_t h = 128) {
    if (n == 0) return;
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    if (sim) {
        hipLaunchKernelGGL((text_marked_kernel<T_SIM, SRC>), dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, bytes, offsets, tok_off,
                           n, 1u, out, status, TextIdfAux{}, 0u);
        return;
    }
    if (h == 128) {
        launch_marked_nr<SRC, 0>(bytes, offsets, tok_off, n, k, h, out, status, stream);
        return;
    }
    switch (text_minhash_nr(h)) {
        case 1: launch_marked_nr<SRC, 1>(bytes, offsets, tok_off, n, k, h, out, status, stream); break;
        case 2: launch_marked_nr<SRC, 2>(bytes, offsets, tok_off, n, k, h, out, status, stream); break;
        case 3: launch_marked_nr<SRC, 3>(bytes, offsets, tok_off, n, k, h, out, status, stream); break;
        case 4: launch_marked_nr<SRC, 4>(bytes, offsets, tok_off, n, k, h, out, status, stream); break;
        case 6: launch_marked_nr<SRC, 6>(bytes, offsets, tok_off, n, k, h, out, status, stream); break;
        case 8: launch_marked_nr<SRC, 8>(bytes, offsets, tok_off, n, k, h, out, status, stream); break;
        case 12: launch_marked_nr<SRC, 12>(bytes, offsets, tok_off, n, k, h, out, status, stream); break;
        default: launch_marked_nr<SRC, 16>(bytes, offsets, tok_off, n, k, h, out, status, stream); break;
    }
}

template <int SRC>
void launch_marked_idf(bool idf, const TextIdfAux& aux, const uint8_t* bytes, const uint64_t* offsets, const uint64_t* tok_off,
                       size_t n, uint8_t* out, int32_t* status, hipStream_t stream) {
    if (n == 0) return;
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    if (idf)
        hipLaunchKernelGGL((text_marked_kernel<T_IDF, SRC>), dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, bytes, offsets, tok_off,
                           n, 1u, out, status, aux, 0u);
    else
        hipLaunchKernelGGL((text_marked_kernel<T_KEYS, SRC>), dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, bytes, offsets, tok_off,
                           n, 1u, out, status, aux, 0u);
}

// Mode UCFP_TEXT_RAW_UTF8 of the grapheme calls: the canon pass into the context's scratch (shared with the word route,
// ordered by canon_done), the hash pass over the canonical bytes, statuses merged.
int grapheme_utf8_hash(ucfp_ctx* ctx, bool sim, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, size_t total_bytes,
                       uint32_t k, uint8_t* d_out, int32_t* d_status, hipStream_t stream, uint32_t h = 128) {
    if (n == 0) return UCFP_OK;
    const uint16_t* s1 = nullptr;
    const uint32_t *s2 = nullptr, *pool = nullptr;
    int rc = text_canon_tables(ctx->device, &s1, &s2, &pool);
    if (rc) return rc;
    const size_t o_st = ((n + 1) * 8 + 255) & ~(size_t)255;
    const size_t o_can = o_st + ((n * 4 + 255) & ~(size_t)255);
    const size_t need = o_can + ucfp_text_canon_bound(total_bytes) + 64;   // the hash kernel reads whole dwords
    std::lock_guard<std::mutex> lk(ctx->canon_mu);
    HIP_TRY(hipStreamWaitEvent(stream, ctx->canon_done, 0));
    rc = grow(&ctx->canon_ws, &ctx->canon_ws_cap, need);
    if (rc) return rc;
    uint64_t* can_off = reinterpret_cast<uint64_t*>(ctx->canon_ws);
    int32_t* cstatus = reinterpret_cast<int32_t*>(ctx->canon_ws + o_st);
    uint8_t* canon = ctx->canon_ws + o_can;
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(text_gcanon_kernel<false>, dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, d_utf8, d_offsets, n, can_off,
                       canon, cstatus, s1, s2, pool);
    launch_text_canon_scan(can_off, n, stream);
    hipLaunchKernelGGL(text_gcanon_kernel<true>, dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, d_utf8, d_offsets, n, can_off,
                       canon, cstatus, s1, s2, pool);
    launch_marked<G_CANON>(sim, canon, can_off, nullptr, n, k, d_out, d_status, stream, h);
    if (d_status) launch_text_canon_merge(cstatus, n, d_status, stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->canon_done, stream));
    return UCFP_OK;
}

int grapheme_check(ucfp_ctx* ctx, const void* offsets, size_t n, int mode, uint32_t k, const void* out) {
    if (!ctx) return capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (mode == UCFP_TEXT_PRETOKENIZED)
        return capi_fail(UCFP_E_INVALID, "the grapheme tokeniser takes raw text; tokens go to ucfp_text_*_tokens_batch");
    if (mode != UCFP_TEXT_RAW_ASCII && mode != UCFP_TEXT_RAW_UTF8) return capi_fail(UCFP_E_INVALID, "unknown text mode %d", mode);
    if (n && (!offsets || !out)) return capi_fail(UCFP_E_INVALID, "offsets/out is NULL");
    if (n > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "batch of %zu documents exceeds one launch", n);
    if (k == 0 || k > 64) return capi_fail(UCFP_E_MODALITY, "shingle k must be in [1, 64] (got %u)", k);
    return UCFP_OK;
}

int grapheme_dev(ucfp_ctx* ctx, bool sim, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, int mode, uint32_t k,
                 uint8_t* d_out, int32_t* d_status, hipStream_t stream, uint32_t h = 128) {
    int rc = grapheme_check(ctx, d_offsets, n, mode, k, d_out);
    if (rc || n == 0) return rc;
    if (mode == UCFP_TEXT_RAW_ASCII) {
        launch_marked<G_ASCII>(sim, d_utf8, d_offsets, nullptr, n, k, d_out, d_status, stream, h);
        HIP_TRY(hipGetLastError());
        return UCFP_OK;
    }
    // the scratch is sized by the batch's bytes, which only the device knows (as the word route's RAW_UTF8 _dev calls)
    uint64_t ends[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&ends[1], d_offsets + n, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (ends[1] < ends[0]) return capi_fail(UCFP_E_INVALID, "offsets must be non-decreasing");
    return grapheme_utf8_hash(ctx, sim, d_utf8, d_offsets, n, (size_t)(ends[1] - ends[0]), k, d_out, d_status, stream, h);
}

int grapheme_host(ucfp_ctx* ctx, bool sim, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode, uint32_t k,
                  uint8_t* out, int32_t* status, uint32_t h = 128) {
    int rc = grapheme_check(ctx, offsets, n, mode, k, out);
    if (rc || n == 0) return rc;
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return capi_fail(UCFP_E_INVALID, "offsets must be non-decreasing");
    const size_t base = offsets[0], total = offsets[n] - offsets[0];
    if (total && !utf8) return capi_fail(UCFP_E_INVALID, "utf8 is NULL");
    const size_t rec = sim ? UCFP_SIMHASH_BYTES : UCFP_MINHASH_RECORD_BYTES(h);
    const size_t o_off = (total + 16 + 255) & ~(size_t)255;
    const size_t in_bytes = o_off + (n + 1) * 8;
    const size_t o_st = (n * rec + 255) & ~(size_t)255;
    const size_t out_bytes = o_st + n * 4;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    rc = grow(&ctx->stage_in, &ctx->stage_in_cap, in_bytes);
    if (rc) return rc;
    rc = grow(&ctx->stage_out, &ctx->stage_out_cap, out_bytes);
    if (rc) return rc;
    hipStream_t st = ctx->host_stream;
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = offsets[i] - base;
    if (total) HIP_TRY(hipMemcpyAsync(ctx->stage_in, utf8 + base, total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->stage_in + o_off, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    const uint64_t* d_off = reinterpret_cast<const uint64_t*>(ctx->stage_in + o_off);
    int32_t* d_st = reinterpret_cast<int32_t*>(ctx->stage_out + o_st);
    if (mode == UCFP_TEXT_RAW_UTF8) {
        rc = grapheme_utf8_hash(ctx, sim, ctx->stage_in, d_off, n, total, k, ctx->stage_out, d_st, st, h);
        if (rc) return rc;
    } else {
        launch_marked<G_ASCII>(sim, ctx->stage_in, d_off, nullptr, n, k, ctx->stage_out, d_st, st, h);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ctx->stage_out, n * rec, hipMemcpyDeviceToHost, st));
    if (status) HIP_TRY(hipMemcpyAsync(status, d_st, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return UCFP_OK;
}

int tokens_check(ucfp_ctx* ctx, const void* tok_offsets, const void* doc_tokens, size_t n, uint32_t k, const void* out) {
    if (!ctx) return capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (n && (!tok_offsets || !doc_tokens || !out)) return capi_fail(UCFP_E_INVALID, "tok_offsets/doc_tokens/out is NULL");
    if (n > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "batch of %zu documents exceeds one launch", n);
    if (k == 0 || k > 64) return capi_fail(UCFP_E_MODALITY, "shingle k must be in [1, 64] (got %u)", k);
    return UCFP_OK;
}

int tokens_dev(ucfp_ctx* ctx, bool sim, const uint8_t* d_bytes, const uint64_t* d_tok_offsets, const uint64_t* d_doc_tokens,
               size_t n, uint32_t k, uint8_t* d_out, int32_t* d_status, hipStream_t stream, uint32_t h = 128) {
    int rc = tokens_check(ctx, d_tok_offsets, d_doc_tokens, n, k, d_out);
    if (rc || n == 0) return rc;
    launch_marked<G_TOKENS>(sim, d_bytes, d_doc_tokens, d_tok_offsets, n, k, d_out, d_status, stream, h);
    HIP_TRY(hipGetLastError());
    return UCFP_OK;
}

int tokens_host(ucfp_ctx* ctx, bool sim, const uint8_t* bytes, const uint64_t* tok_offsets, const uint64_t* doc_tokens, size_t n,
                uint32_t k, uint8_t* out, int32_t* status, uint32_t h = 128) {
    int rc = tokens_check(ctx, tok_offsets, doc_tokens, n, k, out);
    if (rc || n == 0) return rc;
    rc = ucfp_text_tokens_validate(tok_offsets, doc_tokens, n);
    if (rc) return rc;
    const uint64_t T0 = doc_tokens[0], nt = doc_tokens[n] - T0;
    const uint64_t base = tok_offsets[T0], total = tok_offsets[T0 + nt] - base;
    if (total && !bytes) return capi_fail(UCFP_E_INVALID, "bytes is NULL");
    const size_t rec = sim ? UCFP_SIMHASH_BYTES : UCFP_MINHASH_RECORD_BYTES(h);
    const size_t o_tok = ((size_t)total + 16 + 255) & ~(size_t)255;
    const size_t o_doc = o_tok + ((((size_t)nt + 1) * 8 + 255) & ~(size_t)255);
    const size_t in_bytes = o_doc + (n + 1) * 8;
    const size_t o_st = (n * rec + 255) & ~(size_t)255;
    const size_t out_bytes = o_st + n * 4;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    rc = grow(&ctx->stage_in, &ctx->stage_in_cap, in_bytes);
    if (rc) return rc;
    rc = grow(&ctx->stage_out, &ctx->stage_out_cap, out_bytes);
    if (rc) return rc;
    hipStream_t st = ctx->host_stream;
    std::vector<uint64_t> rel_tok((size_t)nt + 1), rel_doc(n + 1);
    for (size_t t = 0; t <= (size_t)nt; t++) rel_tok[t] = tok_offsets[T0 + t] - base;
    for (size_t i = 0; i <= n; i++) rel_doc[i] = doc_tokens[i] - T0;
    if (total) HIP_TRY(hipMemcpyAsync(ctx->stage_in, bytes + base, (size_t)total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->stage_in + o_tok, rel_tok.data(), ((size_t)nt + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->stage_in + o_doc, rel_doc.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    int32_t* d_st = reinterpret_cast<int32_t*>(ctx->stage_out + o_st);
    launch_marked<G_TOKENS>(sim, ctx->stage_in, reinterpret_cast<const uint64_t*>(ctx->stage_in + o_doc),
                            reinterpret_cast<const uint64_t*>(ctx->stage_in + o_tok), n, k, ctx->stage_out, d_st, st, h);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ctx->stage_out, n * rec, hipMemcpyDeviceToHost, st));
    if (status) HIP_TRY(hipMemcpyAsync(status, d_st, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // rel_tok / rel_doc stay alive until here
    return UCFP_OK;
}

int tokenizer_check(int tokenizer) {
    if (tokenizer != UCFP_TEXT_TOK_WORD && tokenizer != UCFP_TEXT_TOK_GRAPHEME)
        return capi_fail(UCFP_E_INVALID, "unknown tokenizer %d", tokenizer);
    return UCFP_OK;
}

}  // namespace

// the marked kernel in the two modes of DESIGN.md T9 (text_idf.hip): src 0 = ASCII graphemes, 1 = graphemes of a canonical
// stream, 2 = the caller's token table (`offsets` = doc_tokens); idf = true the weighted record, false the keys
int launch_text_idf_marked(int src, bool idf, const TextIdfAux& aux, const uint8_t* bytes, const uint64_t* offsets,
                           const uint64_t* tok_off, size_t n, uint8_t* out, int32_t* status, hipStream_t stream) {
    if (src == G_ASCII) launch_marked_idf<G_ASCII>(idf, aux, bytes, offsets, tok_off, n, out, status, stream);
    else if (src == G_CANON) launch_marked_idf<G_CANON>(idf, aux, bytes, offsets, tok_off, n, out, status, stream);
    else launch_marked_idf<G_TOKENS>(idf, aux, bytes, offsets, tok_off, n, out, status, stream);
    return 0;
}

// the grapheme tokeniser behind ucfp_text_minhash_h_batch[_dev] (capi.hip); h was validated there
int text_grapheme_minhash_h_dev(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, int mode, uint32_t k,
                                uint32_t h, uint8_t* d_out, int32_t* d_status, hipStream_t stream) {
    return grapheme_dev(ctx, false, d_utf8, d_offsets, n, mode, k, d_out, d_status, stream, h);
}
int text_grapheme_minhash_h(ucfp_ctx* ctx, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode, uint32_t k, uint32_t h,
                            uint8_t* out, int32_t* status) {
    return grapheme_host(ctx, false, utf8, offsets, n, mode, k, out, status, h);
}

// the grapheme canon pass on its own (count, scan, emit): the whole U3 stream of every document, can_off n + 1 words
int launch_text_gcanon(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, uint8_t* canon, uint64_t* can_off,
                       int32_t* cstatus, hipStream_t stream) {
    if (n == 0) return UCFP_OK;
    const uint16_t* s1 = nullptr;
    const uint32_t *s2 = nullptr, *pool = nullptr;
    const int rc = text_canon_tables(ctx->device, &s1, &s2, &pool);
    if (rc) return rc;
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(text_gcanon_kernel<false>, dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, d_utf8, d_offsets, n, can_off,
                       canon, cstatus, s1, s2, pool);
    launch_text_canon_scan(can_off, n, stream);
    hipLaunchKernelGGL(text_gcanon_kernel<true>, dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, d_utf8, d_offsets, n, can_off,
                       canon, cstatus, s1, s2, pool);
    return UCFP_OK;
}

}  // namespace ucfp

extern "C" {

int ucfp_text_grapheme_covered(uint32_t cp) {
    uint32_t m[8] = {0}, n = 0;
    if (!ucfp_text_utab_lookup(cp, m, &n, nullptr)) return 0;
    for (uint32_t t = 0; t < n; t++)
        if (ucfp::grapheme_excluded(m[t])) return 0;
    return 1;
}

int ucfp_text_tokens_validate(const uint64_t* tok_offsets, const uint64_t* doc_tokens, size_t n) {
    if (n == 0) return UCFP_OK;
    if (!tok_offsets || !doc_tokens) return ucfp::capi_fail(UCFP_E_INVALID, "tok_offsets/doc_tokens is NULL");
    for (size_t i = 0; i < n; i++)
        if (doc_tokens[i + 1] < doc_tokens[i]) return ucfp::capi_fail(UCFP_E_INVALID, "doc_tokens must be non-decreasing");
    for (uint64_t t = doc_tokens[0]; t < doc_tokens[n]; t++)
        if (tok_offsets[t + 1] < tok_offsets[t]) return ucfp::capi_fail(UCFP_E_INVALID, "tok_offsets must be non-decreasing");
    return UCFP_OK;
}

int ucfp_text_minhash_batch_ex_dev(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, int mode, int tokenizer,
                                   uint32_t shingle_k, uint8_t* d_out, int32_t* d_status, void* stream) {
    if (!ctx) return ucfp::capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (int rc = ucfp::tokenizer_check(tokenizer)) return rc;
    if (tokenizer == UCFP_TEXT_TOK_WORD) return ucfp_text_minhash_batch_dev(ctx, d_utf8, d_offsets, n, mode, shingle_k, d_out, d_status, stream);
    return ucfp::grapheme_dev(ctx, false, d_utf8, d_offsets, n, mode, shingle_k, d_out, d_status, (hipStream_t)stream);
}

int ucfp_text_minhash_batch_ex(ucfp_ctx* ctx, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode, int tokenizer,
                               uint32_t shingle_k, uint8_t* out, int32_t* status) {
    if (!ctx) return ucfp::capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (int rc = ucfp::tokenizer_check(tokenizer)) return rc;
    if (tokenizer == UCFP_TEXT_TOK_WORD) return ucfp_text_minhash_batch(ctx, utf8, offsets, n, mode, shingle_k, out, status);
    return ucfp::grapheme_host(ctx, false, utf8, offsets, n, mode, shingle_k, out, status);
}

int ucfp_text_simhash_batch_ex_dev(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, int mode, int tokenizer,
                                   uint8_t* d_out, int32_t* d_status, void* stream) {
    if (!ctx) return ucfp::capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (int rc = ucfp::tokenizer_check(tokenizer)) return rc;
    if (tokenizer == UCFP_TEXT_TOK_WORD) return ucfp_text_simhash_batch_dev(ctx, d_utf8, d_offsets, n, mode, d_out, d_status, stream);
    return ucfp::grapheme_dev(ctx, true, d_utf8, d_offsets, n, mode, 1, d_out, d_status, (hipStream_t)stream);
}

int ucfp_text_simhash_batch_ex(ucfp_ctx* ctx, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode, int tokenizer,
                               uint8_t* out, int32_t* status) {
    if (!ctx) return ucfp::capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (int rc = ucfp::tokenizer_check(tokenizer)) return rc;
    if (tokenizer == UCFP_TEXT_TOK_WORD) return ucfp_text_simhash_batch(ctx, utf8, offsets, n, mode, out, status);
    return ucfp::grapheme_host(ctx, true, utf8, offsets, n, mode, 1, out, status);
}

int ucfp_text_minhash_tokens_batch_dev(ucfp_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_tok_offsets,
                                       const uint64_t* d_doc_tokens, size_t n, uint32_t shingle_k, uint8_t* d_out, int32_t* d_status,
                                       void* stream) {
    return ucfp::tokens_dev(ctx, false, d_bytes, d_tok_offsets, d_doc_tokens, n, shingle_k, d_out, d_status, (hipStream_t)stream);
}

int ucfp_text_minhash_tokens_batch(ucfp_ctx* ctx, const uint8_t* bytes, const uint64_t* tok_offsets, const uint64_t* doc_tokens,
                                   size_t n, uint32_t shingle_k, uint8_t* out, int32_t* status) {
    return ucfp::tokens_host(ctx, false, bytes, tok_offsets, doc_tokens, n, shingle_k, out, status);
}

int ucfp_text_minhash_tokens_h_batch_dev(ucfp_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_tok_offsets,
                                         const uint64_t* d_doc_tokens, size_t n, uint32_t shingle_k, uint32_t h, uint8_t* d_out,
                                         int32_t* d_status, void* stream) {
    if (!ctx) return ucfp::capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (int rc = ucfp::minhash_h_check(h)) return rc;
    return ucfp::tokens_dev(ctx, false, d_bytes, d_tok_offsets, d_doc_tokens, n, shingle_k, d_out, d_status, (hipStream_t)stream, h);
}

int ucfp_text_minhash_tokens_h_batch(ucfp_ctx* ctx, const uint8_t* bytes, const uint64_t* tok_offsets, const uint64_t* doc_tokens,
                                     size_t n, uint32_t shingle_k, uint32_t h, uint8_t* out, int32_t* status) {
    if (!ctx) return ucfp::capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (int rc = ucfp::minhash_h_check(h)) return rc;
    return ucfp::tokens_host(ctx, false, bytes, tok_offsets, doc_tokens, n, shingle_k, out, status, h);
}

int ucfp_text_simhash_tokens_batch_dev(ucfp_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_tok_offsets,
                                       const uint64_t* d_doc_tokens, size_t n, uint8_t* d_out, int32_t* d_status, void* stream) {
    return ucfp::tokens_dev(ctx, true, d_bytes, d_tok_offsets, d_doc_tokens, n, 1, d_out, d_status, (hipStream_t)stream);
}

int ucfp_text_simhash_tokens_batch(ucfp_ctx* ctx, const uint8_t* bytes, const uint64_t* tok_offsets, const uint64_t* doc_tokens,
                                   size_t n, uint8_t* out, int32_t* status) {
    return ucfp::tokens_host(ctx, true, bytes, tok_offsets, doc_tokens, n, 1, out, status);
}

}  // extern "C"
