// bm25_terms.hip -- BM25 text ingest on the GPU: tokenise, hash and count the terms of a batch (gfx950).
//
// Replaces `tokenize` (src/index/embedded/bm25.rs:88-97) and the term counting of the index path (bm25.rs:343) for ASCII
// documents: a token is a maximal run of [0-9A-Za-z], lower-cased; its key is XXH3_64 of its bytes (ucfp_text_token_key).
// The outputs are what ucfp_bm25_index_upsert_dev (COUNTS) and ucfp_bm25_index_query_dev (SEQUENCE) take.
//
//   valid     pmax[i] = max(offsets[0 .. i]) (rocPRIM scan).  Document i is tokenised iff pmax[i] == offsets[i] <=
//             offsets[i + 1] <= n_bytes and it is shorter than 2^31 bytes: such documents do not share bytes, so their
//             lengths add up to at most n_bytes, which is what ucfp_bm25_terms_max_pairs counts on.  The others get -4.
//   tokenise  one wave per document: bm25_step below (the word rule of A23.1 as ballot masks over 64-byte steps) in front
//             of the LDS batch, XXH3 from LDS and the T_KEYS flush of text_core.h.  A document has at most ceil(len / 2)
//             tokens, so document i owns the slots [(offsets[i] + i) / 2, + ceil(len / 2)): disjoint, (n_bytes + n) / 2 + 1
//             in all.  Token t goes to slot t of its document; the wave leaves the token count (0 unless the status is 0).
//             The flush also writes the document's ordinal beside every key (slot_ords: 4 of the 12 bytes of a slot), as
//             the IDF fit needs it; nothing here reads it -- the price of leaving text_flush as it is.
//   scan      exclusive scan of the token counts (rocPRIM): the documents' places in text order.
//   gather    one wave per document copies its slots to its place.  SEQUENCE ends here: the caller's arrays are the target.
//   sort      COUNTS: rocPRIM's segmented radix sort orders each document's keys (postings.h sort_segments),
//   heads     the compaction of postings.h (post_count, post_scan_tiles, post_compact) keeps the first token of every
//             (document, key) run and notes where it stood; tf is the distance to the next head, and pair_offsets[i] is the
//             rank of the head at document i's first token (every document's first token is a head).
// A term on both sides of an LDS flush is two slots with one key: the sort brings them together, the run is one pair.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <new>

#include "ctx.h"
#include "postings.h"
#include "text_core.h"

namespace ucfp {

struct Bm25TermsWs {
    hipEvent_t done = nullptr;   // the previous call's last work: the scratch is free after it
    DevArr slot_keys, slot_ords, pmax, ntok, tok_off, scan_tmp;                  // both forms
    DevArr seq, sorted, tdoc, hpos, rank_at, tile_cnt, tile_off, sort_tmp;       // COUNTS
};

void bm25_terms_ws_free(Bm25TermsWs* w) {
    if (!w) return;
    for (DevArr* a : {&w->slot_keys, &w->slot_ords, &w->pmax, &w->ntok, &w->tok_off, &w->scan_tmp, &w->seq, &w->sorted, &w->tdoc,
                      &w->hpos, &w->rank_at, &w->tile_cnt, &w->tile_off, &w->sort_tmp})
        a->release();
    if (w->done) (void)hipEventDestroy(w->done);
    delete w;
}

namespace {

// One 64-byte step of the BM25 word rule: lane = the byte at `pos`, bytes at or past `end` are not processed.  A word byte
// is a letter or a digit and nothing else, so the mask needs no neighbours; what it does with the mask is text_step's.
__device__ __forceinline__ void bm25_step(WaveLds& L, TextWave& W, int sub, size_t pos, size_t end, int lane) {
    const uint32_t c = L.stage[64 * sub + lane];
    const bool w = pos < end && ((c | 0x20u) - 'a' <= 25u || c - '0' <= 9u);
    const uint64_t inw = __ballot(w);
    const uint64_t prev = (inw << 1) | (W.carry ? 1ull : 0ull);
    const uint64_t starts = inw & ~prev;
    const uint64_t endmark = ~inw & prev;   // first non-word byte after a token
    const uint32_t nin_before = popc_below(inw, lane);
    const uint32_t nst_before = popc_below(starts, lane);
    const bool is_start = (starts >> lane) & 1ull;
    if (w) {
        const uint32_t tok = W.ntok + nst_before + (is_start ? 1u : 0u) - 1u;
        const uint32_t cpos = W.cbase + nin_before + tok;
        L.canon[cpos] = (uint8_t)(c - 'A' <= 25u ? c + 32u : c);
        if (is_start) {
            L.cstart[tok] = (uint16_t)cpos;
            if (cpos > 0) L.canon[cpos - 1] = ' ';
        }
    }
    if ((endmark >> lane) & 1ull) {
        const uint32_t tok = W.ntok + nst_before - 1u;   // starts strictly before this byte
        L.cend[tok] = (uint16_t)(W.cbase + nin_before + tok);
    }
    W.ntok += (uint32_t)__popcll(starts);
    W.cbase += (uint32_t)__popcll(inw);
    W.carry = (inw >> 63) & 1ull;
}

// the byte reader of text_hash_kernel around bm25_step; aux carries the slot arrays (key_out, ord_out)
__global__ __launch_bounds__(64 * kWavesPerBlock) void bm25_terms_kernel(const uint8_t* __restrict__ utf8,
                                                                         const uint64_t* __restrict__ offsets,
                                                                         const uint64_t* __restrict__ pmax, size_t n, uint64_t n_bytes,
                                                                         TextIdfAux aux, uint64_t* __restrict__ ntok,
                                                                         int32_t* __restrict__ status) {
    __shared__ WaveLds lds[kWavesPerBlock];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t doc = (size_t)blockIdx.x * kWavesPerBlock + wave;
    if (doc >= n) return;  // whole wave
    WaveLds& L = lds[wave];
    const uint64_t o0 = offsets[doc], o1 = offsets[doc + 1];
    if (pmax[doc] != o0 || o1 < o0 || o1 > n_bytes || o1 - o0 >= 0x80000000ull) {
        if (lane == 0) {
            status[doc] = UCFP_E_INVALID;
            ntok[doc] = 0;
        }
        return;
    }
    const uint8_t* __restrict__ text = utf8 + o0;
    const size_t len = (size_t)(o1 - o0);
    const bool aligned4 = (reinterpret_cast<uintptr_t>(text) & 3u) == 0;
    aux.slot0 = (o0 + doc) >> 1;
    aux.doc_cap = (uint32_t)((len + 1) >> 1);
    aux.ord = (uint32_t)doc;

    TextWave W;
    bool nonascii = false, too_long = false;
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
    size_t base = 0;
    for (; base < len && !too_long; base += 256) {
        const uint32_t nxt = load_chunk(base + 256);
        wave_sync();
        *reinterpret_cast<uint32_t*>(&L.stage[4 * lane]) = cur;
        wave_sync();
        nonascii |= (cur & 0x80808080u) != 0;
#pragma unroll 1
        for (int sub = 0; sub < 4; sub++) {
            if (base + 64 * sub >= len) break;
            if (text_batch_full(W)) {   // make room
                text_flush<T_KEYS>(L, W, 1u, lane, false, &aux);
                if (text_batch_full(W)) too_long = true;   // one token fills the batch
                if (too_long) break;
            }
            bm25_step(L, W, sub, base + 64 * sub + lane, len, lane);
        }
        cur = nxt;
    }
    // a refused document still says whether the host must take it: NEEDS_HOST wins wherever the byte stands
    for (; base < len; base += 256) nonascii |= (load_chunk(base) & 0x80808080u) != 0;
    // close a token that runs to the end of the document, then the final flush
    if (W.carry && W.ntok > 0 && lane == 0) L.cend[W.ntok - 1] = (uint16_t)(W.cbase + W.ntok - 1);
    if (!too_long) text_flush<T_KEYS>(L, W, 1u, lane, true, &aux);
    const int32_t stv = __ballot(nonascii) != 0 ? UCFP_TEXT_NEEDS_HOST : too_long ? UCFP_E_UNSUPPORTED : 0;
    if (lane == 0) {
        status[doc] = stv;
        ntok[doc] = stv == 0 ? W.total_tok : 0;
    }
}

// one wave per document: its ntok slots to its place in text order (tdoc: the document of every token, COUNTS only)
__global__ __launch_bounds__(256) void bm25_terms_gather_kernel(const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ ntok,
                                                                const uint64_t* __restrict__ tok_off, size_t n,
                                                                const uint64_t* __restrict__ slot_keys, uint64_t* __restrict__ out,
                                                                uint32_t* __restrict__ tdoc) {
    const int lane = threadIdx.x & 63;
    const size_t doc = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (doc >= n) return;
    const uint64_t cnt = ntok[doc];
    if (cnt == 0) return;   // also every document whose offsets were refused: they are not read again
    const uint64_t s0 = (offsets[doc] + doc) >> 1, d0 = tok_off[doc];
    for (uint64_t t = lane; t < cnt; t += 64) {
        out[d0 + t] = slot_keys[s0 + t];
        if (tdoc) tdoc[d0 + t] = (uint32_t)doc;
    }
}

// the first token of a (document, key) run among the sorted tokens
struct TermHead {
    const uint64_t* key;
    const uint32_t* doc;
    __device__ bool operator()(size_t i) const { return i == 0 || key[i] != key[i - 1] || doc[i] != doc[i - 1]; }
};
struct TermEmit {
    const uint64_t* key;
    uint64_t* out_keys;
    uint32_t* hpos;      // where head o stood
    uint32_t* rank_at;   // the rank of the head that stands at i
    __device__ void operator()(size_t i, uint64_t o) const {
        out_keys[o] = key[i];
        hpos[o] = (uint32_t)i;
        rank_at[i] = (uint32_t)o;
    }
};

// tf of pair o = the distance from its head to the next one (T behind the last); *total = the number of heads
__global__ void bm25_terms_tf_kernel(const uint32_t* __restrict__ hpos, const uint64_t* __restrict__ total, uint64_t T,
                                     uint32_t* __restrict__ tfs) {
    const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t u = *total;
    if (o >= u) return;
    tfs[o] = (o + 1 < u ? hpos[o + 1] : (uint32_t)T) - hpos[o];
}

// pair_offsets[d], d in [0, n]: the token at tok_off[d] is a head (the first token of the next document that has one)
__global__ void bm25_terms_pair_off_kernel(const uint64_t* __restrict__ tok_off, const uint32_t* __restrict__ rank_at,
                                           const uint64_t* __restrict__ total, uint64_t T, size_t n, uint64_t* __restrict__ pair_off) {
    const size_t d = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d > n) return;
    const uint64_t t = tok_off[d];
    pair_off[d] = t < T ? (uint64_t)rank_at[t] : *total;
}

int terms_ws(ucfp_ctx* ctx, Bm25TermsWs** out) {   // under ctx->terms_mu
    if (!ctx->terms_ws) {
        Bm25TermsWs* w = new (std::nothrow) Bm25TermsWs();
        if (!w) return capi_fail(UCFP_E_INDEX, "out of host memory");
        hipError_t e = hipEventCreateWithFlags(&w->done, hipEventDisableTiming);
        if (e != hipSuccess) {
            delete w;
            return capi_fail(UCFP_E_INDEX, "hipEventCreate: %s", hipGetErrorString(e));
        }
        ctx->terms_ws = w;
    }
    *out = ctx->terms_ws;
    return UCFP_OK;
}

// what both entries check before anything runs (ctx first)
int terms_check(const ucfp_ctx* ctx, const void* utf8, const void* offsets, size_t n, size_t n_bytes, int form, const void* keys,
                const void* tfs, size_t cap_pairs, const void* pair_offsets, const void* status) {
    if (!ctx) return capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (form != UCFP_BM25_TERMS_COUNTS && form != UCFP_BM25_TERMS_SEQUENCE) return capi_fail(UCFP_E_INVALID, "unknown terms form %d", form);
    if (!offsets || !keys || !pair_offsets || !status || (form == UCFP_BM25_TERMS_COUNTS && !tfs) || (n_bytes && !utf8))
        return capi_fail(UCFP_E_INVALID, "utf8/offsets/keys/tfs/pair_offsets/status is NULL");
    if (n > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "batch of %zu documents exceeds one launch", n);
    if (ucfp_bm25_terms_max_pairs(n_bytes, n) >= ((size_t)1 << 32))   // token positions are 32-bit
        return capi_fail(UCFP_E_INVALID, "a terms batch has n_bytes + n below 2^33");
    if (cap_pairs < ucfp_bm25_terms_max_pairs(n_bytes, n))
        return capi_fail(UCFP_E_INVALID, "cap_pairs %zu is below ucfp_bm25_terms_max_pairs = %zu", cap_pairs, ucfp_bm25_terms_max_pairs(n_bytes, n));
    return UCFP_OK;
}

// the work of a checked call, enqueued on st; the caller holds ctx->terms_mu and has selected the device
int terms_run(Bm25TermsWs* w, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, size_t n_bytes, int form, uint64_t* d_keys,
              uint32_t* d_tfs, uint64_t* d_pair_offsets, int32_t* d_status, hipStream_t st) {
    const bool counts = form == UCFP_BM25_TERMS_COUNTS;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_pair_offsets, 0, 8, st));
        return UCFP_OK;
    }
    const size_t slots = ucfp_bm25_terms_max_pairs(n_bytes, n) + 1;
    int rc;
    if ((rc = w->slot_keys.ensure(slots * 8)) || (rc = w->slot_ords.ensure(slots * 4)) || (rc = w->pmax.ensure(n * 8)) ||
        (rc = w->ntok.ensure((n + 1) * 8)) || (rc = w->tok_off.ensure((n + 1) * 8)))
        return rc;
    uint64_t* tok_off = counts ? w->tok_off.as<uint64_t>() : d_pair_offsets;
    size_t b0 = 0, b1 = 0;
    HIP_TRY(rocprim::inclusive_scan(nullptr, b0, d_offsets, w->pmax.as<uint64_t>(), n, rocprim::maximum<uint64_t>(), st));
    HIP_TRY(rocprim::exclusive_scan(nullptr, b1, w->ntok.as<uint64_t>(), tok_off, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), st));
    size_t sb = b0 > b1 ? b0 : b1;
    if ((rc = w->scan_tmp.ensure(sb))) return rc;
    HIP_TRY(rocprim::inclusive_scan(w->scan_tmp.p, b0, d_offsets, w->pmax.as<uint64_t>(), n, rocprim::maximum<uint64_t>(), st));
    TextIdfAux aux;
    aux.key_out = w->slot_keys.as<uint64_t>();
    aux.ord_out = w->slot_ords.as<uint32_t>();
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    HIP_TRY(hipMemsetAsync(w->ntok.as<uint64_t>() + n, 0, 8, st));
    hipLaunchKernelGGL(bm25_terms_kernel, dim3(grid), dim3(64 * kWavesPerBlock), 0, st, d_utf8, d_offsets, w->pmax.as<uint64_t>(), n,
                       (uint64_t)n_bytes, aux, w->ntok.as<uint64_t>(), d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::exclusive_scan(w->scan_tmp.p, b1, w->ntok.as<uint64_t>(), tok_off, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), st));
    if (!counts) {
        hipLaunchKernelGGL(bm25_terms_gather_kernel, dim3(grid), dim3(256), 0, st, d_offsets, w->ntok.as<uint64_t>(), tok_off, n,
                           w->slot_keys.as<uint64_t>(), d_keys, (uint32_t*)nullptr);
        HIP_TRY(hipGetLastError());
        return UCFP_OK;
    }
    uint64_t T = 0;   // the batch's tokens: sizes the sort and its scratch (the one host synchronisation of this form)
    HIP_TRY(hipMemcpyAsync(&T, tok_off + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (T == 0) {
        HIP_TRY(hipMemsetAsync(d_pair_offsets, 0, (n + 1) * 8, st));
        return UCFP_OK;
    }
    const size_t nb = ((size_t)T + kCompactTile - 1) / kCompactTile;
    if ((rc = w->seq.ensure(T * 8)) || (rc = w->sorted.ensure(T * 8)) || (rc = w->tdoc.ensure(T * 4)) || (rc = w->hpos.ensure(T * 4)) ||
        (rc = w->rank_at.ensure(T * 4)) || (rc = w->tile_cnt.ensure(nb * 4)) || (rc = w->tile_off.ensure((nb + 1) * 8)))
        return rc;
    hipLaunchKernelGGL(bm25_terms_gather_kernel, dim3(grid), dim3(256), 0, st, d_offsets, w->ntok.as<uint64_t>(), tok_off, n,
                       w->slot_keys.as<uint64_t>(), w->seq.as<uint64_t>(), w->tdoc.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    if ((rc = sort_segments(w->sort_tmp, w->seq.as<uint64_t>(), w->sorted.as<uint64_t>(), (size_t)T, n, tok_off, st))) return rc;
    const TermHead head{w->sorted.as<uint64_t>(), w->tdoc.as<uint32_t>()};
    const TermEmit emit{w->sorted.as<uint64_t>(), d_keys, w->hpos.as<uint32_t>(), w->rank_at.as<uint32_t>()};
    hipLaunchKernelGGL(post_count<TermHead>, dim3((unsigned)nb), dim3(kThreads), 0, st, head, (size_t)T, w->tile_cnt.as<uint32_t>());
    hipLaunchKernelGGL(post_scan_tiles, dim3(1), dim3(kThreads), 0, st, w->tile_cnt.as<uint32_t>(), nb, w->tile_off.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    if ((rc = compact_heads(head, emit, (size_t)T, w->tile_off, st))) return rc;
    const uint64_t* total = w->tile_off.as<uint64_t>() + nb;
    hipLaunchKernelGGL(bm25_terms_tf_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, w->hpos.as<uint32_t>(), total, T, d_tfs);
    hipLaunchKernelGGL(bm25_terms_pair_off_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, st, tok_off, w->rank_at.as<uint32_t>(),
                       total, T, n, d_pair_offsets);
    HIP_TRY(hipGetLastError());
    return UCFP_OK;
}

// lock, wait for the scratch, run, leave the event behind
int terms_ordered(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, size_t n_bytes, int form, uint64_t* d_keys,
                  uint32_t* d_tfs, uint64_t* d_pair_offsets, int32_t* d_status, hipStream_t st) {
    std::lock_guard<std::mutex> lk(ctx->terms_mu);
    Bm25TermsWs* w;
    int rc = terms_ws(ctx, &w);
    if (rc) return rc;
    HIP_TRY(hipStreamWaitEvent(st, w->done, 0));
    rc = terms_run(w, d_utf8, d_offsets, n, n_bytes, form, d_keys, d_tfs, d_pair_offsets, d_status, st);
    HIP_TRY(hipEventRecord(w->done, st));
    return rc;
}

}  // namespace

}  // namespace ucfp

extern "C" {

using namespace ucfp;

size_t ucfp_bm25_terms_max_pairs(size_t n_bytes, size_t n) { return (n_bytes + n) / 2; }

int ucfp_bm25_terms_batch_dev(ucfp_ctx* ctx, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, size_t n_bytes, int form,
                              uint64_t* d_keys, uint32_t* d_tfs, size_t cap_pairs, uint64_t* d_pair_offsets, int32_t* d_status,
                              void* stream) {
    if (int rc = terms_check(ctx, d_utf8, d_offsets, n, n_bytes, form, d_keys, d_tfs, cap_pairs, d_pair_offsets, d_status)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return terms_ordered(ctx, d_utf8, d_offsets, n, n_bytes, form, d_keys, d_tfs, d_pair_offsets, d_status, (hipStream_t)stream);
}

int ucfp_bm25_terms_batch(ucfp_ctx* ctx, const uint8_t* utf8, const uint64_t* offsets, size_t n, int form, uint64_t* keys, uint32_t* tfs,
                          size_t cap_pairs, uint64_t* pair_offsets, int32_t* status) {
    if (!ctx) return capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (!offsets) return capi_fail(UCFP_E_INVALID, "offsets is NULL");
    const size_t n_bytes = (size_t)offsets[n];   // the blob ends where the last document does: one that reaches past it is refused
    if (int rc = terms_check(ctx, utf8, offsets, n, n_bytes, form, keys, tfs, cap_pairs, pair_offsets, status)) return rc;
    const bool counts = form == UCFP_BM25_TERMS_COUNTS;
    const size_t cap = ucfp_bm25_terms_max_pairs(n_bytes, n);
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->host_stream;
    // staging in: the bytes, then the offsets as they are; out: keys, pair_offsets, tfs, statuses
    const size_t i_off = (n_bytes + 16 + 255) & ~(size_t)255;
    const size_t o_po = (cap * 8 + 255) & ~(size_t)255, o_tf = o_po + (((n + 1) * 8 + 255) & ~(size_t)255);
    const size_t o_st = o_tf + ((cap * 4 + 255) & ~(size_t)255);
    int rc;
    if ((rc = grow(&ctx->stage_in, &ctx->stage_in_cap, i_off + (n + 1) * 8)) || (rc = grow(&ctx->stage_out, &ctx->stage_out_cap, o_st + n * 4 + 4)))
        return rc;
    if (n_bytes) HIP_TRY(hipMemcpyAsync(ctx->stage_in, utf8, n_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->stage_in + i_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, st));
    uint64_t* d_keys = reinterpret_cast<uint64_t*>(ctx->stage_out);
    uint64_t* d_po = reinterpret_cast<uint64_t*>(ctx->stage_out + o_po);
    uint32_t* d_tf = reinterpret_cast<uint32_t*>(ctx->stage_out + o_tf);
    int32_t* d_st = reinterpret_cast<int32_t*>(ctx->stage_out + o_st);
    if ((rc = terms_ordered(ctx, ctx->stage_in, reinterpret_cast<const uint64_t*>(ctx->stage_in + i_off), n, n_bytes, form, d_keys, d_tf, d_po,
                            d_st, st))) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(pair_offsets, d_po, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (n) HIP_TRY(hipMemcpyAsync(status, d_st, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const size_t total = (size_t)pair_offsets[n];
    if (total) {
        HIP_TRY(hipMemcpyAsync(keys, d_keys, total * 8, hipMemcpyDeviceToHost, st));
        if (counts) HIP_TRY(hipMemcpyAsync(tfs, d_tf, total * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return UCFP_OK;
}

}  // extern "C"
