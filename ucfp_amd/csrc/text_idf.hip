// text_idf.hip -- TF.IDF SimHash: an IDF table fitted and applied on the GPU (gfx950).
//
// Replaces text::fingerprint_simhash_idf(text, opts, &IdfTable, ..) (src/modality/text.rs:344-362) for a caller-supplied or
// a fitted table.  The table is a device-resident open-addressing map from a token's key -- XXH3_64 of its canonical
// bytes, the value T6 hashes anyway -- to a Q16.16 weight; the weighted record comes from the tokeniser kernels in mode
// T_IDF (text_core.h: the lane that hashes a token probes the table, the fold adds weights instead of ones), so every
// token source -- word tokeniser, RAW_UTF8 behind the canon pass, graphemes, the caller's tokens -- serves it.
//
// FIT (ucfp_idf_table_add_*): the same kernels in mode T_KEYS write each token's key and its document's ordinal to
// scratch -- document d of a piece owns the slots [byte offset of d, + bytes of d) (token units for the token form), more
// than it has tokens, the rest stays void -- then
//   sort     rocPRIM's stable radix sort by key (postings.h sort_pairs).  Slots ascend with the document, so inside a run
//            of one key the entries of one document are adjacent;
//   runs     the number of runs bounds the new keys: the table is grown for them first (rehash into twice the size or
//            more, behind a stream synchronisation -- this is a fit step);
//   insert   one thread per entry; the first entry of a (key, document) pair whose document ended with status 0 claims
//            the key's slot with a 64-bit compare-and-swap and adds 1 to its df.  The status is final by then, so a
//            document that turns out too long (-2) contributes nothing, its earlier batches included.
// Counts are integers: the result does not depend on the order of anything.
//
// TABLE: capacity a power of two, keys[i] = 0 means empty and key 0 lives in the extra slot `cap`, so every u64 is a
// legal key.  LOAD BOUND: at most cap / 2 keys (kIdfLoadDen), kept by growing BEFORE a piece's inserts; a probe for an
// absent key therefore meets an empty slot.  Home slot = top bits of key * 2^64/phi, linear probing.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "ctx.h"
#include "idf_math.h"
#include "postings.h"
#include "text_idf.h"

namespace ucfp {

namespace {

constexpr size_t kIdfLoadDen = 2;                 // keys <= cap / 2
constexpr size_t kIdfMinCap = 16;
constexpr size_t kIdfDefaultPiece = (size_t)1 << 22;
constexpr uint32_t kVoid = 0xffffffffu;
enum { C_KEYS = 0, C_ZERO = 1, C_DOCS = 2, C_RUNS = 3, C_WORDS = 4 };   // the table's device counters

enum { SRC_WORD_ASCII = 0, SRC_WORD_PRETOK = 1, SRC_G_ASCII = 2, SRC_G_CANON = 3, SRC_TOKENS = 4 };

struct Source {
    int kind;
    const uint8_t* bytes;
    const uint64_t* offsets;   // documents' byte offsets; SRC_TOKENS: doc_tokens
    const uint64_t* tok_off;   // SRC_TOKENS only
};

void launch_source(bool idf, const TextIdfAux& aux, const Source& s, size_t i0, size_t n, uint8_t* out, int32_t* status,
                   hipStream_t st) {
    if (s.kind == SRC_WORD_ASCII || s.kind == SRC_WORD_PRETOK)
        launch_text_idf_words(idf, aux, s.bytes, s.offsets + i0, n, s.kind == SRC_WORD_PRETOK ? UCFP_TEXT_PRETOKENIZED : UCFP_TEXT_RAW_ASCII,
                              out, status, st);
    else
        launch_text_idf_marked(s.kind - SRC_G_ASCII, idf, aux, s.bytes, s.offsets + i0, s.tok_off, n, out, status, st);
}

// slot of `key` != 0, claimed when absent (*fresh); the load bound keeps an empty slot on every probe path
__device__ __forceinline__ uint32_t idf_claim(uint64_t* keys, uint32_t shift, uint32_t mask, uint64_t key, bool* fresh) {
    uint32_t i = (uint32_t)((key * kIdfMul) >> shift);
    for (;;) {
        const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long*>(&keys[i]), 0ull, (unsigned long long)key);
        if (old == 0ull || old == key) {
            *fresh = old == 0ull;
            return i;
        }
        i = (i + 1) & mask;
    }
}

// runs of equal keys among n sorted slots (void slots included: an upper bound of the keys the piece can add)
__global__ void idf_runs_kernel(const uint64_t* __restrict__ keys, size_t n, uint32_t* __restrict__ cnt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool head = i < n && (i == 0 || keys[i] != keys[i - 1]);
    const uint64_t m = __ballot(head);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[C_RUNS], (uint32_t)__popcll(m));
}

__global__ void idf_docs_kernel(const int32_t* __restrict__ status, size_t n, uint32_t* __restrict__ cnt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t m = __ballot(i < n && status[i] == 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[C_DOCS], (uint32_t)__popcll(m));
}

__global__ void idf_insert_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ ords, size_t n,
                                  const int32_t* __restrict__ status, size_t n_docs, uint64_t* __restrict__ tab_keys,
                                  uint32_t* __restrict__ tab_df, uint32_t shift, uint32_t mask, uint32_t* __restrict__ cnt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = ords[i];
    if (o == kVoid || o >= n_docs || status[o] != 0) return;
    const uint64_t key = keys[i];
    if (i > 0 && keys[i - 1] == key && ords[i - 1] == o) return;   // not the pair's first entry
    if (key == 0) {
        if (atomicCAS(&cnt[C_ZERO], 0u, 1u) == 0u) atomicAdd(&cnt[C_KEYS], 1u);
        atomicAdd(&tab_df[(size_t)mask + 1], 1u);
        return;
    }
    bool fresh;
    const uint32_t s = idf_claim(tab_keys, shift, mask, key, &fresh);
    if (fresh) atomicAdd(&cnt[C_KEYS], 1u);
    atomicAdd(&tab_df[s], 1u);
}

// every entry of the old table into the new one (twice the size or more: the bound holds with room to spare)
__global__ void idf_rehash_kernel(const uint64_t* __restrict__ ok, const uint32_t* __restrict__ odf, const uint32_t* __restrict__ ow,
                                  size_t ocap, uint64_t* __restrict__ nk, uint32_t* __restrict__ ndf, uint32_t* __restrict__ nw,
                                  uint32_t shift, uint32_t mask) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > ocap) return;
    if (i == ocap) {   // the slot of key 0
        ndf[(size_t)mask + 1] = odf[ocap];
        nw[(size_t)mask + 1] = ow[ocap];
        return;
    }
    const uint64_t key = ok[i];
    if (key == 0) return;
    bool fresh;
    const uint32_t s = idf_claim(nk, shift, mask, key, &fresh);
    ndf[s] = odf[i];
    nw[s] = ow[i];
}

// n distinct (key, weight) pairs into an emptied table
__global__ void idf_set_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ w, size_t n, uint64_t* __restrict__ tab_keys,
                               uint32_t* __restrict__ tab_w, uint32_t shift, uint32_t mask, uint32_t* __restrict__ cnt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    if (key == 0) {
        cnt[C_ZERO] = 1u;
        tab_w[(size_t)mask + 1] = w[i];
        return;
    }
    bool fresh;
    tab_w[idf_claim(tab_keys, shift, mask, key, &fresh)] = w[i];
}

__global__ void idf_finalize_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ df, uint32_t* __restrict__ w,
                                    size_t cap, uint64_t n_docs, const uint32_t* __restrict__ cnt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > cap) return;
    if (i == cap) w[cap] = idf_weight_q16(n_docs, cnt[C_ZERO] ? df[cap] : 0);
    else if (keys[i] != 0) w[i] = idf_weight_q16(n_docs, df[i]);
}

size_t pow2_at_least(size_t v) {
    size_t c = kIdfMinCap;
    while (c < v) c <<= 1;
    return c;
}

}  // namespace

}  // namespace ucfp

struct ucfp_idf_table {
    ucfp_ctx* ctx = nullptr;
    int device = 0;
    std::mutex mu;
    uint64_t* keys = nullptr;   // cap + 1 each; slot cap is key 0's
    uint32_t* df = nullptr;
    uint32_t* wts = nullptr;
    uint32_t* cnt = nullptr;    // C_WORDS device counters
    size_t cap = 0;
    size_t n_keys = 0;
    uint64_t n_docs = 0;
    bool is_final = false;
    uint32_t default_w = 0x10000u;
    size_t piece = ucfp::kIdfDefaultPiece;
    ucfp::DevArr k_in, k_out, o_in, o_out, sort_tmp, st_buf, canon_buf;   // fit scratch, grown on demand
    uint8_t* in_buf = nullptr;   // staging of the host add entries
    size_t in_cap = 0;

    uint32_t shift() const { return (uint32_t)(64 - __builtin_ctzll((unsigned long long)cap)); }
    void release() {
        if (keys) (void)hipFree(keys);
        if (df) (void)hipFree(df);
        if (wts) (void)hipFree(wts);
        keys = nullptr, df = nullptr, wts = nullptr;
    }
};

namespace ucfp {

TextIdfAux idf_table_aux(const ucfp_idf_table* t, bool* is_final, int* device) {
    TextIdfAux a;
    a.tab_keys = t->keys;
    a.tab_wts = t->wts;
    a.shift = t->shift();
    a.mask = (uint32_t)(t->cap - 1);
    a.default_w = t->default_w;
    if (is_final) *is_final = t->is_final;
    if (device) *device = t->device;
    return a;
}

namespace {

int idf_alloc(size_t cap, uint64_t** k, uint32_t** d, uint32_t** w) {
    *k = nullptr, *d = nullptr, *w = nullptr;
    hipError_t e = hipMalloc((void**)k, (cap + 1) * 8);
    if (e == hipSuccess) e = hipMalloc((void**)d, (cap + 1) * 4);
    if (e == hipSuccess) e = hipMalloc((void**)w, (cap + 1) * 4);
    if (e == hipSuccess) e = hipMemset(*k, 0, (cap + 1) * 8);
    if (e == hipSuccess) e = hipMemset(*d, 0, (cap + 1) * 4);
    if (e == hipSuccess) e = hipMemset(*w, 0, (cap + 1) * 4);
    if (e != hipSuccess) {
        if (*k) (void)hipFree(*k);
        if (*d) (void)hipFree(*d);
        if (*w) (void)hipFree(*w);
        *k = nullptr, *d = nullptr, *w = nullptr;
        return capi_fail(UCFP_E_INDEX, "IDF table of %zu slots: %s", cap, hipGetErrorString(e));
    }
    return UCFP_OK;
}

// room for `extra` more keys under the load bound; growing drains `st` and the device (a fit step)
int idf_reserve(ucfp_idf_table* t, size_t extra, hipStream_t st) {
    const size_t need = (t->n_keys + extra) * kIdfLoadDen;
    if (need <= t->cap) return UCFP_OK;
    const size_t ncap = pow2_at_least(std::max(need, t->cap * 2));
    if (ncap > ((size_t)1 << 31)) return capi_fail(UCFP_E_INVALID, "an IDF table holds at most 2^30 keys");
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t* nk;
    uint32_t *nd, *nw;
    const int rc = idf_alloc(ncap, &nk, &nd, &nw);
    if (rc) return rc;
    const uint32_t shift = (uint32_t)(64 - __builtin_ctzll((unsigned long long)ncap));
    hipLaunchKernelGGL(idf_rehash_kernel, dim3((unsigned)((t->cap + 256) / 256)), dim3(256), 0, st, t->keys, t->df, t->wts, t->cap, nk,
                       nd, nw, shift, (uint32_t)(ncap - 1));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(nk), (void)hipFree(nd), (void)hipFree(nw);
        return capi_fail(UCFP_E_INDEX, "IDF table growth failed: %s", hipGetErrorString(e));
    }
    t->release();
    t->keys = nk, t->df = nd, t->wts = nw, t->cap = ncap;
    return UCFP_OK;
}

TextIdfAux idf_aux(const ucfp_idf_table* t) { return idf_table_aux(t, nullptr, nullptr); }

int idf_counters(ucfp_idf_table* t, uint32_t* h, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(h, t->cnt, C_WORDS * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return UCFP_OK;
}

// The fit of n documents that are on the device: h_off = the host's copy of s.offsets[0 .. n] (non-decreasing).  Statuses
// go to d_status (device, n words).  Pieces of at most t->piece slots; a larger document is a piece of its own.
int idf_add_core(ucfp_idf_table* t, const Source& s, const uint64_t* h_off, size_t n, int32_t* d_status, hipStream_t st) {
    t->is_final = false;
    uint32_t h[C_WORDS];
    uint64_t docs = 0;
    int rc = UCFP_OK;
    for (size_t i0 = 0; i0 < n && !rc;) {
        size_t i1 = i0 + 1;
        while (i1 < n && h_off[i1 + 1] - h_off[i0] <= t->piece) i1++;
        const size_t P = (size_t)(h_off[i1] - h_off[i0]), nd = i1 - i0;
        if ((rc = t->k_in.ensure(P * 8)) || (rc = t->k_out.ensure(P * 8)) || (rc = t->o_in.ensure(P * 4)) || (rc = t->o_out.ensure(P * 4)))
            break;
        HIP_TRY(hipMemsetAsync(t->cnt + C_DOCS, 0, 8, st));   // C_DOCS, C_RUNS
        if (P) {
            HIP_TRY(hipMemsetAsync(t->k_in.p, 0, P * 8, st));
            HIP_TRY(hipMemsetAsync(t->o_in.p, 0xff, P * 4, st));
        }
        TextIdfAux a;
        a.key_out = t->k_in.as<uint64_t>();
        a.ord_out = t->o_in.as<uint32_t>();
        a.slot_base = h_off[i0];
        a.slot_cap = P;
        launch_source(false, a, s, i0, nd, nullptr, d_status + i0, st);
        hipLaunchKernelGGL(idf_docs_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, d_status + i0, nd, t->cnt);
        HIP_TRY(hipGetLastError());
        if (P) {
            if ((rc = sort_pairs(t->sort_tmp, t->k_in.as<uint64_t>(), t->k_out.as<uint64_t>(), t->o_in.as<uint32_t>(),
                                 t->o_out.as<uint32_t>(), P, 64, st)))
                break;
            hipLaunchKernelGGL(idf_runs_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, t->k_out.as<uint64_t>(), P, t->cnt);
            HIP_TRY(hipGetLastError());
        }
        if ((rc = idf_counters(t, h, st))) break;
        docs += h[C_DOCS];
        if (P) {
            if ((rc = idf_reserve(t, h[C_RUNS], st))) break;
            hipLaunchKernelGGL(idf_insert_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, t->k_out.as<uint64_t>(),
                               t->o_out.as<uint32_t>(), P, d_status + i0, nd, t->keys, t->df, t->shift(), (uint32_t)(t->cap - 1), t->cnt);
            HIP_TRY(hipGetLastError());
            if ((rc = idf_counters(t, h, st))) break;
            t->n_keys = h[C_KEYS];
        }
        i0 = i1;
    }
    t->n_docs += docs;
    return rc;
}

// the canon pass of mode RAW_UTF8 into the table's own scratch: *tokens / *tok_off / *cstatus point into it
int idf_canon(ucfp_idf_table* t, bool grapheme, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, size_t total,
              uint8_t** tokens, uint64_t** tok_off, int32_t** cstatus, hipStream_t st) {
    const size_t o_st = ((n + 1) * 8 + 255) & ~(size_t)255;
    const size_t o_tok = o_st + ((n * 4 + 255) & ~(size_t)255);
    const int rc = t->canon_buf.ensure(o_tok + ucfp_text_canon_bound(total) + 64);
    if (rc) return rc;
    uint8_t* base = t->canon_buf.as<uint8_t>();
    *tok_off = reinterpret_cast<uint64_t*>(base);
    *cstatus = reinterpret_cast<int32_t*>(base + o_st);
    *tokens = base + o_tok;
    if (grapheme) return launch_text_gcanon(t->ctx, d_utf8, d_offsets, n, *tokens, *tok_off, *cstatus, st);
    launch_text_canon(d_utf8, d_offsets, n, *tokens, *tok_off, *cstatus, st);
    return UCFP_OK;
}

int idf_mode_check(int mode, int tokenizer) {
    if (tokenizer != UCFP_TEXT_TOK_WORD && tokenizer != UCFP_TEXT_TOK_GRAPHEME)
        return capi_fail(UCFP_E_INVALID, "unknown tokenizer %d", tokenizer);
    if (mode != UCFP_TEXT_RAW_ASCII && mode != UCFP_TEXT_PRETOKENIZED && mode != UCFP_TEXT_RAW_UTF8)
        return capi_fail(UCFP_E_INVALID, "unknown text mode %d", mode);
    if (tokenizer == UCFP_TEXT_TOK_GRAPHEME && mode == UCFP_TEXT_PRETOKENIZED)
        return capi_fail(UCFP_E_INVALID, "the grapheme tokeniser takes raw text; tokens go to the token entries");
    return UCFP_OK;
}

int src_kind(int mode, int tokenizer) {
    if (tokenizer == UCFP_TEXT_TOK_GRAPHEME) return mode == UCFP_TEXT_RAW_ASCII ? SRC_G_ASCII : SRC_G_CANON;
    return mode == UCFP_TEXT_RAW_ASCII ? SRC_WORD_ASCII : SRC_WORD_PRETOK;
}

// documents on the device, offsets known to the host
int idf_add_docs(ucfp_idf_table* t, const uint8_t* d_utf8, const uint64_t* d_offsets, const uint64_t* h_off, size_t n, int mode,
                 int tokenizer, int32_t* d_status, hipStream_t st) {
    if (mode != UCFP_TEXT_RAW_UTF8) return idf_add_core(t, Source{src_kind(mode, tokenizer), d_utf8, d_offsets, nullptr}, h_off, n, d_status, st);
    uint8_t* tokens;
    uint64_t* tok_off;
    int32_t* cstatus;
    int rc = idf_canon(t, tokenizer == UCFP_TEXT_TOK_GRAPHEME, d_utf8, d_offsets, n, (size_t)(h_off[n] - h_off[0]), &tokens, &tok_off,
                       &cstatus, st);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    std::vector<uint64_t> h_tok(n + 1);
    HIP_TRY(hipMemcpyAsync(h_tok.data(), tok_off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // a handed-back document has no canonical bytes: no keys, status -1 from the key pass, then NEEDS_HOST from the merge
    rc = idf_add_core(t, Source{src_kind(mode, tokenizer), tokens, tok_off, nullptr}, h_tok.data(), n, d_status, st);
    launch_text_canon_merge(cstatus, n, d_status, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

int idf_table_check(const ucfp_idf_table* t) {
    if (!t) return capi_fail(UCFP_E_INVALID, "table is NULL");
    return UCFP_OK;
}

// the weighted record of documents on the device; total = bytes of the batch (mode RAW_UTF8 sizes the context's scratch)
int idf_simhash_docs(ucfp_ctx* ctx, const ucfp_idf_table* t, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, size_t total,
                     int mode, int tokenizer, uint8_t* d_out, int32_t* d_status, hipStream_t st) {
    const TextIdfAux a = idf_aux(t);
    if (mode != UCFP_TEXT_RAW_UTF8) {
        launch_source(true, a, Source{src_kind(mode, tokenizer), d_utf8, d_offsets, nullptr}, 0, n, d_out, d_status, st);
        HIP_TRY(hipGetLastError());
        return UCFP_OK;
    }
    const size_t o_st = ((n + 1) * 8 + 255) & ~(size_t)255;
    const size_t o_tok = o_st + ((n * 4 + 255) & ~(size_t)255);
    const size_t need = o_tok + ucfp_text_canon_bound(total) + 64;
    std::lock_guard<std::mutex> lk(ctx->canon_mu);   // the scratch of the RAW_UTF8 routes, ordered by canon_done
    HIP_TRY(hipStreamWaitEvent(st, ctx->canon_done, 0));
    int rc = grow(&ctx->canon_ws, &ctx->canon_ws_cap, need);
    if (rc) return rc;
    uint64_t* tok_off = reinterpret_cast<uint64_t*>(ctx->canon_ws);
    int32_t* cstatus = reinterpret_cast<int32_t*>(ctx->canon_ws + o_st);
    uint8_t* tokens = ctx->canon_ws + o_tok;
    if (tokenizer == UCFP_TEXT_TOK_GRAPHEME) {
        if ((rc = launch_text_gcanon(ctx, d_utf8, d_offsets, n, tokens, tok_off, cstatus, st))) return rc;
    } else {
        launch_text_canon(d_utf8, d_offsets, n, tokens, tok_off, cstatus, st);
    }
    launch_source(true, a, Source{src_kind(mode, tokenizer), tokens, tok_off, nullptr}, 0, n, d_out, d_status, st);
    if (d_status) launch_text_canon_merge(cstatus, n, d_status, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->canon_done, st));
    return UCFP_OK;
}

int idf_final_check(ucfp_ctx* ctx, const ucfp_idf_table* t) {
    if (!ctx) return capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (int rc = idf_table_check(t)) return rc;
    if (!t->is_final) return capi_fail(UCFP_E_INVALID, "the IDF table is not final: call ucfp_idf_table_finalize or _set_weights");
    if (t->device != ctx->device) return capi_fail(UCFP_E_INVALID, "the IDF table lives on device %d, the context on %d", t->device, ctx->device);
    return UCFP_OK;
}

// a host batch of documents staged into *buf (grown on demand): the bytes, then offsets relative to the first
int stage_docs(uint8_t** buf, size_t* buf_cap, const uint8_t* utf8, const uint64_t* offsets, size_t n, std::vector<uint64_t>& rel, const uint8_t** d_bytes,
               const uint64_t** d_off, hipStream_t st) {
    if (!offsets) return capi_fail(UCFP_E_INVALID, "offsets is NULL");
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return capi_fail(UCFP_E_INVALID, "offsets must be non-decreasing");
    const size_t base = offsets[0], total = offsets[n] - offsets[0];
    if (total && !utf8) return capi_fail(UCFP_E_INVALID, "utf8 is NULL");
    const size_t o_off = (total + 16 + 255) & ~(size_t)255;
    const int rc = grow(buf, buf_cap, o_off + (n + 1) * 8);
    if (rc) return rc;
    rel.resize(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = offsets[i] - base;
    uint8_t* d = *buf;
    if (total) HIP_TRY(hipMemcpyAsync(d, utf8 + base, total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + o_off, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    *d_bytes = d;
    *d_off = reinterpret_cast<const uint64_t*>(d + o_off);
    return UCFP_OK;
}

// the same for the token form (tables checked whole first): bytes, tok_offsets and doc_tokens, all relative
int stage_tokens(uint8_t** buf, size_t* buf_cap, const uint8_t* bytes, const uint64_t* tok_offsets, const uint64_t* doc_tokens, size_t n,
                 std::vector<uint64_t>& rel_tok, std::vector<uint64_t>& rel_doc, const uint8_t** d_bytes, const uint64_t** d_tok,
                 const uint64_t** d_doc, hipStream_t st) {
    int rc = ucfp_text_tokens_validate(tok_offsets, doc_tokens, n);
    if (rc) return rc;
    const uint64_t T0 = doc_tokens[0], nt = doc_tokens[n] - T0;
    const uint64_t base = tok_offsets[T0], total = tok_offsets[T0 + nt] - base;
    if (total && !bytes) return capi_fail(UCFP_E_INVALID, "bytes is NULL");
    const size_t o_tok = ((size_t)total + 16 + 255) & ~(size_t)255;
    const size_t o_doc = o_tok + ((((size_t)nt + 1) * 8 + 255) & ~(size_t)255);
    if ((rc = grow(buf, buf_cap, o_doc + (n + 1) * 8))) return rc;
    rel_tok.resize((size_t)nt + 1);
    rel_doc.resize(n + 1);
    for (size_t k = 0; k <= (size_t)nt; k++) rel_tok[k] = tok_offsets[T0 + k] - base;
    for (size_t i = 0; i <= n; i++) rel_doc[i] = doc_tokens[i] - T0;
    uint8_t* d = *buf;
    if (total) HIP_TRY(hipMemcpyAsync(d, bytes + base, (size_t)total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + o_tok, rel_tok.data(), ((size_t)nt + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + o_doc, rel_doc.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    *d_bytes = d;
    *d_tok = reinterpret_cast<const uint64_t*>(d + o_tok);
    *d_doc = reinterpret_cast<const uint64_t*>(d + o_doc);
    return UCFP_OK;
}

int batch_size_check(size_t n) {
    if (n > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "batch of %zu documents exceeds one launch", n);
    return UCFP_OK;
}

}  // namespace

}  // namespace ucfp

extern "C" {

using namespace ucfp;

int ucfp_idf_table_create(ucfp_ctx* ctx, size_t capacity_hint, size_t piece_tokens, uint32_t flags, ucfp_idf_table** out) {
    if (!ctx || !out) return capi_fail(UCFP_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (flags) return capi_fail(UCFP_E_INVALID, "unknown IDF table flags %u", flags);
    if (capacity_hint > ((size_t)1 << 30)) return capi_fail(UCFP_E_INVALID, "an IDF table holds at most 2^30 keys");
    ucfp_idf_table* t = new (std::nothrow) ucfp_idf_table();
    if (!t) return capi_fail(UCFP_E_INDEX, "out of host memory");
    t->ctx = ctx;
    t->device = ctx->device;
    if (piece_tokens) t->piece = piece_tokens;
    t->cap = pow2_at_least(capacity_hint * kIdfLoadDen);
    hipError_t e = hipSetDevice(t->device);
    int rc = e == hipSuccess ? idf_alloc(t->cap, &t->keys, &t->df, &t->wts) : capi_fail(UCFP_E_INDEX, "hipSetDevice: %s", hipGetErrorString(e));
    if (!rc) {
        e = hipMalloc((void**)&t->cnt, C_WORDS * 4);
        if (e == hipSuccess) e = hipMemset(t->cnt, 0, C_WORDS * 4);
        if (e != hipSuccess) rc = capi_fail(UCFP_E_INDEX, "IDF table counters: %s", hipGetErrorString(e));
    }
    if (rc) {
        ucfp_idf_table_destroy(t);
        return rc;
    }
    *out = t;
    return UCFP_OK;
}

void ucfp_idf_table_destroy(ucfp_idf_table* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();
    t->release();
    if (t->cnt) (void)hipFree(t->cnt);
    for (DevArr* a : {&t->k_in, &t->k_out, &t->o_in, &t->o_out, &t->sort_tmp, &t->st_buf, &t->canon_buf}) a->release();
    if (t->in_buf) (void)hipFree(t->in_buf);
    delete t;
}

int ucfp_idf_table_add_batch_dev(ucfp_idf_table* t, const uint8_t* d_utf8, const uint64_t* d_offsets, size_t n, int mode, int tokenizer,
                                 int32_t* d_status, void* stream) {
    int rc;
    if ((rc = idf_table_check(t)) || (rc = idf_mode_check(mode, tokenizer)) || (rc = batch_size_check(n))) return rc;
    if (n == 0) return UCFP_OK;
    if (!d_offsets) return capi_fail(UCFP_E_INVALID, "offsets is NULL");
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(t->mu);
    HIP_TRY(hipSetDevice(t->device));
    std::vector<uint64_t> h_off(n + 1);   // the pieces are planned on the host: a fit step reads the offsets back
    HIP_TRY(hipMemcpyAsync(h_off.data(), d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; i++)
        if (h_off[i + 1] < h_off[i]) return capi_fail(UCFP_E_INVALID, "offsets must be non-decreasing");
    if (!d_status) {
        if ((rc = t->st_buf.ensure(n * 4))) return rc;
        d_status = t->st_buf.as<int32_t>();
    }
    return idf_add_docs(t, d_utf8, d_offsets, h_off.data(), n, mode, tokenizer, d_status, st);
}

int ucfp_idf_table_add_batch(ucfp_idf_table* t, const uint8_t* utf8, const uint64_t* offsets, size_t n, int mode, int tokenizer,
                             int32_t* status) {
    int rc;
    if ((rc = idf_table_check(t)) || (rc = idf_mode_check(mode, tokenizer)) || (rc = batch_size_check(n))) return rc;
    if (n == 0) return UCFP_OK;
    std::lock_guard<std::mutex> lk(t->mu);
    HIP_TRY(hipSetDevice(t->device));
    hipStream_t st = t->ctx->host_stream;
    std::vector<uint64_t> rel;
    const uint8_t* d_bytes;
    const uint64_t* d_off;
    if ((rc = stage_docs(&t->in_buf, &t->in_cap, utf8, offsets, n, rel, &d_bytes, &d_off, st)) || (rc = t->st_buf.ensure(n * 4))) return rc;
    rc = idf_add_docs(t, d_bytes, d_off, rel.data(), n, mode, tokenizer, t->st_buf.as<int32_t>(), st);
    if (!rc && status) HIP_TRY(hipMemcpyAsync(status, t->st_buf.p, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

int ucfp_idf_table_add_tokens_batch_dev(ucfp_idf_table* t, const uint8_t* d_bytes, const uint64_t* d_tok_offsets,
                                        const uint64_t* d_doc_tokens, size_t n, int32_t* d_status, void* stream) {
    int rc;
    if ((rc = idf_table_check(t)) || (rc = batch_size_check(n))) return rc;
    if (n == 0) return UCFP_OK;
    if (!d_tok_offsets || !d_doc_tokens) return capi_fail(UCFP_E_INVALID, "tok_offsets/doc_tokens is NULL");
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(t->mu);
    HIP_TRY(hipSetDevice(t->device));
    // the pieces are planned from doc_tokens, read back; a table that decreases is refused whole.  tok_offsets stays on the
    // device: the wave of a document checks its own slice, as in the TF entry
    std::vector<uint64_t> h_doc(n + 1);
    HIP_TRY(hipMemcpyAsync(h_doc.data(), d_doc_tokens, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; i++)
        if (h_doc[i + 1] < h_doc[i]) return capi_fail(UCFP_E_INVALID, "doc_tokens must be non-decreasing");
    if (!d_status) {
        if ((rc = t->st_buf.ensure(n * 4))) return rc;
        d_status = t->st_buf.as<int32_t>();
    }
    return idf_add_core(t, Source{SRC_TOKENS, d_bytes, d_doc_tokens, d_tok_offsets}, h_doc.data(), n, d_status, st);
}

int ucfp_idf_table_add_tokens_batch(ucfp_idf_table* t, const uint8_t* bytes, const uint64_t* tok_offsets, const uint64_t* doc_tokens,
                                    size_t n, int32_t* status) {
    int rc;
    if ((rc = idf_table_check(t)) || (rc = batch_size_check(n))) return rc;
    if (n == 0) return UCFP_OK;
    if (!tok_offsets || !doc_tokens) return capi_fail(UCFP_E_INVALID, "tok_offsets/doc_tokens is NULL");
    std::lock_guard<std::mutex> lk(t->mu);
    HIP_TRY(hipSetDevice(t->device));
    hipStream_t st = t->ctx->host_stream;
    std::vector<uint64_t> rel_tok, rel_doc;
    const uint8_t* d_bytes;
    const uint64_t *d_tok, *d_doc;
    if ((rc = stage_tokens(&t->in_buf, &t->in_cap, bytes, tok_offsets, doc_tokens, n, rel_tok, rel_doc, &d_bytes, &d_tok, &d_doc, st)) ||
        (rc = t->st_buf.ensure(n * 4)))
        return rc;
    rc = idf_add_core(t, Source{SRC_TOKENS, d_bytes, d_doc, d_tok}, rel_doc.data(), n, t->st_buf.as<int32_t>(), st);
    if (!rc && status) HIP_TRY(hipMemcpyAsync(status, t->st_buf.p, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

int ucfp_idf_table_set_weights(ucfp_idf_table* t, const uint64_t* keys, const uint32_t* weights_q16, size_t n, uint32_t default_q16) {
    if (int rc = idf_table_check(t)) return rc;
    if (n && (!keys || !weights_q16)) return capi_fail(UCFP_E_INVALID, "keys/weights is NULL");
    if (n > ((size_t)1 << 30)) return capi_fail(UCFP_E_INVALID, "an IDF table holds at most 2^30 keys");
    {
        std::vector<uint64_t> sorted(keys, keys + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return capi_fail(UCFP_E_INVALID, "a key appears twice in the supplied weights");
    }
    std::lock_guard<std::mutex> lk(t->mu);
    HIP_TRY(hipSetDevice(t->device));
    hipStream_t st = t->ctx->host_stream;
    HIP_TRY(hipDeviceSynchronize());   // readers of the old contents are done
    int rc;
    if ((rc = t->k_in.ensure(n * 8)) || (rc = t->o_in.ensure(n * 4))) return rc;
    const size_t need = pow2_at_least(n * kIdfLoadDen);
    if (need > t->cap) {
        uint64_t* nk;
        uint32_t *nd, *nw;
        if ((rc = idf_alloc(need, &nk, &nd, &nw))) return rc;
        t->release();
        t->keys = nk, t->df = nd, t->wts = nw, t->cap = need;
    } else {
        HIP_TRY(hipMemsetAsync(t->keys, 0, (t->cap + 1) * 8, st));
        HIP_TRY(hipMemsetAsync(t->df, 0, (t->cap + 1) * 4, st));
        HIP_TRY(hipMemsetAsync(t->wts, 0, (t->cap + 1) * 4, st));
    }
    HIP_TRY(hipMemsetAsync(t->cnt, 0, C_WORDS * 4, st));
    HIP_TRY(hipMemcpyAsync(t->wts + t->cap, &default_q16, 4, hipMemcpyHostToDevice, st));   // key 0 weighs the default while absent
    if (n) {
        HIP_TRY(hipMemcpyAsync(t->k_in.p, keys, n * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t->o_in.p, weights_q16, n * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(idf_set_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t->k_in.as<uint64_t>(),
                           t->o_in.as<uint32_t>(), n, t->keys, t->wts, t->shift(), (uint32_t)(t->cap - 1), t->cnt);
        HIP_TRY(hipGetLastError());
    }
    const uint32_t nk32 = (uint32_t)n;
    HIP_TRY(hipMemcpyAsync(t->cnt + C_KEYS, &nk32, 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    t->n_keys = n;
    t->n_docs = 0;
    t->default_w = default_q16;
    t->is_final = true;
    return UCFP_OK;
}

int ucfp_idf_table_finalize(ucfp_idf_table* t, void* stream) {
    if (int rc = idf_table_check(t)) return rc;
    std::lock_guard<std::mutex> lk(t->mu);
    HIP_TRY(hipSetDevice(t->device));
    hipLaunchKernelGGL(idf_finalize_kernel, dim3((unsigned)((t->cap + 256) / 256)), dim3(256), 0, (hipStream_t)stream, t->keys, t->df,
                       t->wts, t->cap, t->n_docs, t->cnt);
    HIP_TRY(hipGetLastError());
    t->default_w = idf_weight_q16(t->n_docs, 0);
    t->is_final = true;
    // a final table is read, not fitted: give the fit scratch back (12 bytes per slot of a piece, twice, and the sort's).
    // The weights are written when this returns
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (DevArr* a : {&t->k_in, &t->k_out, &t->o_in, &t->o_out, &t->sort_tmp, &t->canon_buf}) a->release();
    return UCFP_OK;
}

int ucfp_idf_table_size(ucfp_idf_table* t, uint64_t* n_docs, size_t* n_keys, int* is_final) {
    if (int rc = idf_table_check(t)) return rc;
    std::lock_guard<std::mutex> lk(t->mu);
    if (n_docs) *n_docs = t->n_docs;
    if (n_keys) *n_keys = t->n_keys;
    if (is_final) *is_final = t->is_final ? 1 : 0;
    return UCFP_OK;
}

int ucfp_idf_table_export(ucfp_idf_table* t, uint64_t* keys, uint32_t* dfs, uint32_t* weights_q16, size_t cap, size_t* n,
                          uint32_t* default_q16) {
    if (int rc = idf_table_check(t)) return rc;
    std::lock_guard<std::mutex> lk(t->mu);
    if (n) *n = t->n_keys;
    if (default_q16) *default_q16 = t->default_w;
    if (cap < t->n_keys) {
        if (!keys && !dfs && !weights_q16 && cap == 0) return UCFP_OK;   // a size query
        return capi_fail(UCFP_E_INVALID, "the table holds %zu keys, the caller's arrays %zu", t->n_keys, cap);
    }
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint64_t> hk(t->cap + 1);
    std::vector<uint32_t> hd(t->cap + 1), hw(t->cap + 1);
    uint32_t h[C_WORDS];
    HIP_TRY(hipMemcpy(hk.data(), t->keys, (t->cap + 1) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hd.data(), t->df, (t->cap + 1) * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hw.data(), t->wts, (t->cap + 1) * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h, t->cnt, sizeof h, hipMemcpyDeviceToHost));
    size_t o = 0;
    for (size_t i = 0; i <= t->cap && o < cap; i++) {
        if (i < t->cap ? hk[i] == 0 : h[C_ZERO] == 0) continue;
        if (keys) keys[o] = i < t->cap ? hk[i] : 0;
        if (dfs) dfs[o] = hd[i];
        if (weights_q16) weights_q16[o] = hw[i];
        o++;
    }
    if (n) *n = o;
    return UCFP_OK;
}

int ucfp_text_simhash_idf_batch_dev(ucfp_ctx* ctx, const ucfp_idf_table* table, const uint8_t* d_utf8, const uint64_t* d_offsets,
                                    size_t n, int mode, int tokenizer, uint8_t* d_out, int32_t* d_status, void* stream) {
    int rc;
    if ((rc = idf_final_check(ctx, table)) || (rc = idf_mode_check(mode, tokenizer)) || (rc = batch_size_check(n))) return rc;
    if (n == 0) return UCFP_OK;
    if (!d_offsets || !d_out) return capi_fail(UCFP_E_INVALID, "offsets/out is NULL");
    hipStream_t st = (hipStream_t)stream;
    size_t total = 0;
    if (mode == UCFP_TEXT_RAW_UTF8) {   // as the TF entries: the scratch is sized by the batch's bytes, read back once
        uint64_t ends[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(&ends[0], d_offsets, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&ends[1], d_offsets + n, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (ends[1] < ends[0]) return capi_fail(UCFP_E_INVALID, "offsets must be non-decreasing");
        total = (size_t)(ends[1] - ends[0]);
    }
    return idf_simhash_docs(ctx, table, d_utf8, d_offsets, n, total, mode, tokenizer, d_out, d_status, st);
}

int ucfp_text_simhash_idf_batch(ucfp_ctx* ctx, const ucfp_idf_table* table, const uint8_t* utf8, const uint64_t* offsets, size_t n,
                                int mode, int tokenizer, uint8_t* out, int32_t* status) {
    int rc;
    if ((rc = idf_final_check(ctx, table)) || (rc = idf_mode_check(mode, tokenizer)) || (rc = batch_size_check(n))) return rc;
    if (n == 0) return UCFP_OK;
    if (!out) return capi_fail(UCFP_E_INVALID, "out is NULL");
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->host_stream;
    std::vector<uint64_t> rel;
    const uint8_t* d_bytes;
    const uint64_t* d_off;
    if ((rc = stage_docs(&ctx->stage_in, &ctx->stage_in_cap, utf8, offsets, n, rel, &d_bytes, &d_off, st))) return rc;
    const size_t o_st = (n * UCFP_SIMHASH_BYTES + 255) & ~(size_t)255;
    if ((rc = grow(&ctx->stage_out, &ctx->stage_out_cap, o_st + n * 4))) return rc;
    int32_t* d_st = reinterpret_cast<int32_t*>(ctx->stage_out + o_st);
    if ((rc = idf_simhash_docs(ctx, table, d_bytes, d_off, n, (size_t)rel[n], mode, tokenizer, ctx->stage_out, d_st, st))) return rc;
    HIP_TRY(hipMemcpyAsync(out, ctx->stage_out, n * UCFP_SIMHASH_BYTES, hipMemcpyDeviceToHost, st));
    if (status) HIP_TRY(hipMemcpyAsync(status, d_st, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return UCFP_OK;
}

int ucfp_text_simhash_idf_tokens_batch_dev(ucfp_ctx* ctx, const ucfp_idf_table* table, const uint8_t* d_bytes,
                                           const uint64_t* d_tok_offsets, const uint64_t* d_doc_tokens, size_t n, uint8_t* d_out,
                                           int32_t* d_status, void* stream) {
    int rc;
    if ((rc = idf_final_check(ctx, table)) || (rc = batch_size_check(n))) return rc;
    if (n == 0) return UCFP_OK;
    if (!d_tok_offsets || !d_doc_tokens || !d_out) return capi_fail(UCFP_E_INVALID, "tok_offsets/doc_tokens/out is NULL");
    launch_source(true, idf_aux(table), Source{SRC_TOKENS, d_bytes, d_doc_tokens, d_tok_offsets}, 0, n, d_out, d_status, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UCFP_OK;
}

int ucfp_text_simhash_idf_tokens_batch(ucfp_ctx* ctx, const ucfp_idf_table* table, const uint8_t* bytes, const uint64_t* tok_offsets,
                                       const uint64_t* doc_tokens, size_t n, uint8_t* out, int32_t* status) {
    int rc;
    if ((rc = idf_final_check(ctx, table)) || (rc = batch_size_check(n))) return rc;
    if (n == 0) return UCFP_OK;
    if (!tok_offsets || !doc_tokens || !out) return capi_fail(UCFP_E_INVALID, "tok_offsets/doc_tokens/out is NULL");
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->host_stream;
    std::vector<uint64_t> rel_tok, rel_doc;
    const uint8_t* d_bytes;
    const uint64_t *d_tok, *d_doc;
    if ((rc = stage_tokens(&ctx->stage_in, &ctx->stage_in_cap, bytes, tok_offsets, doc_tokens, n, rel_tok, rel_doc, &d_bytes, &d_tok, &d_doc, st)))
        return rc;
    const size_t o_st = (n * UCFP_SIMHASH_BYTES + 255) & ~(size_t)255;
    if ((rc = grow(&ctx->stage_out, &ctx->stage_out_cap, o_st + n * 4))) return rc;
    int32_t* d_st = reinterpret_cast<int32_t*>(ctx->stage_out + o_st);
    launch_source(true, idf_aux(table), Source{SRC_TOKENS, d_bytes, d_doc, d_tok}, 0, n, ctx->stage_out, d_st, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, ctx->stage_out, n * UCFP_SIMHASH_BYTES, hipMemcpyDeviceToHost, st));
    if (status) HIP_TRY(hipMemcpyAsync(status, d_st, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // rel_tok / rel_doc stay alive until here
    return UCFP_OK;
}

}  // extern "C"
