// text_core.h -- the hash stage of the text kernels, once: text_hash_kernel (text.hip, whole documents) and
// text_stream_kernel (text_streams.hip, streams) are this file's bodies around their own byte readers.  Here: the launch
// shape, the LDS batch of one wave and its limits, the ASCII word rule, XXH3 read from LDS, the MinHash second hash, the
// wave state (TextWave), the 64-byte tokeniser step (text_step), the flush of a batch (text_flush) and the record and
// status of a finished document (text_emit).  The canon stage in front of it is text_canon_core.h.  text_marked_kernel
// (text_grapheme.hip: graphemes, caller-segmented tokens) runs the same flush and record behind text_step_marked, the step
// whose token starts are a mask.  Flush and record come in four modes (T_MIN .. T_KEYS below): MinHash, SimHash, and for
// TF.IDF SimHash (text_idf.hip) the weighted SimHash against a table and the emission of the tokens' keys.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ucfp_hip.h"
#include "../../include/ucfp_xxh3.h"
#include "common.h"
#include "text_idf.h"

namespace ucfp {

namespace {

constexpr int kWavesPerBlock = 4;    // one wave per document / stream entry, in every text kernel
constexpr int kTokCap = 256;        // tokens per LDS batch
constexpr int kCanonCap = 1536;     // canonical bytes per LDS batch
constexpr int kStepTok = 33;        // a 64-byte step can open at most 32 (+1 carried) tokens
constexpr int kStepRoom = 130;      // canonical bytes a step may add (64 + 32 separators), with margin
// what survives a flush is a prefix of one k-token window: it must leave room for the next step (derivation in ucfp_hip.h)
static_assert(kCanonCap - kStepRoom - 1 == UCFP_TEXT_MAX_WINDOW_BYTES, "the documented -2 limit follows these constants");

struct WaveLds {
    uint8_t stage[256 + 8];
    uint8_t canon[kCanonCap + 72];
    uint16_t cstart[kTokCap + 8];
    uint16_t cend[kTokCap + 8];
    uint64_t h1[kTokCap];
    uint64_t h2[kTokCap];
};

enum { C_O = 0, C_L = 1, C_N = 2, C_ML = 3, C_MNL = 4, C_MN = 5 };

__device__ __forceinline__ int cls(uint32_t c) {
    const uint32_t lc = c | 0x20u;
    int r = C_O;
    r = (lc - 'a' <= 25u || c == '_') ? C_L : r;
    r = (c - '0' <= 9u) ? C_N : r;
    r = (c == ':') ? C_ML : r;
    r = (c == '.' || c == '\'') ? C_MNL : r;
    r = (c == ',' || c == ';') ? C_MN : r;
    return r;
}

__device__ __forceinline__ bool inword(uint32_t p, uint32_t c, uint32_t q, bool pretok) {
    if (pretok) return c != ' ';   // every other byte, 0x00 included (the caller's `pos < len` guards the padding)
    const int cc = cls(c), pc = cls(p), qc = cls(q);
    const bool mid_l = (cc == C_ML || cc == C_MNL) && pc == C_L && qc == C_L;   // WB6/7
    const bool mid_n = (cc == C_MN || cc == C_MNL) && pc == C_N && qc == C_N;   // WB11/12
    return cc == C_L || cc == C_N || mid_l || mid_n;
}

// XXH3 over the canonical token stream in LDS.  Unaligned 8 / 4-byte words come from ALIGNED dwords and
// v_alignbyte (3 + 2 or 2 + 1 instructions instead of 8 / 4 byte loads and a shift/or ladder); the stream has
// 72 bytes of slack behind it, so the dword past the end is readable.  The hash body is force-inlined, which
// also keeps the pointer in the LDS address space (ds_read, not flat loads).
#define UCFP_RD8_LDS(p, i) ((p)[(i)])
__device__ __forceinline__ uint64_t xxh3_lds_rd64(const uint8_t* src, size_t o) {
    const uint8_t* q = src + o;
    const uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(q) & 3u;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(q - sh);   // pointer arithmetic keeps the LDS address space
    const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
    return (uint64_t)__builtin_amdgcn_alignbyte(d1, d0, sh) | ((uint64_t)__builtin_amdgcn_alignbyte(d2, d1, sh) << 32);
}
__device__ __forceinline__ uint32_t xxh3_lds_rd32(const uint8_t* src, size_t o) {
    const uint8_t* q = src + o;
    const uint32_t sh = (uint32_t)reinterpret_cast<uintptr_t>(q) & 3u;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(q - sh);
    return __builtin_amdgcn_alignbyte(p[1], p[0], sh);
}
UCFP_XXH3_DEFINE_BODY(xxh3_lds, const uint8_t*, UCFP_RD8_LDS)

__device__ __forceinline__ uint64_t mix_h2(uint64_t h1) {
    uint64_t z = h1 + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (z ^ (z >> 31)) | 1ull;
}

__device__ __forceinline__ uint32_t popc_below(uint64_t m, int lane) {  // bits of m below `lane`
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    (void)lane;
}

__device__ __forceinline__ void wave_sync() { wave_lds_sync(); }

// What a kernel makes of a document's tokens.  T_MIN and T_SIM are the records of T5 and T6 (the values of the former
// `bool MODE_SIM`, so text_flush<false> / <true> mean what they meant); T_IDF is the weighted SimHash of DESIGN.md T9.3;
// T_KEYS writes every token's key (T9.1) and the document's ordinal out for the fit of an IDF table (T9.4).
enum { T_MIN = 0, T_SIM = 1, T_IDF = 2, T_KEYS = 3 };

// the table probe of T_IDF (TextIdfAux, text_idf.h): one lane, one probe sequence
__device__ __forceinline__ uint32_t idf_lookup(const TextIdfAux& A, uint64_t key) {
    if (key == 0) return A.tab_wts[(size_t)A.mask + 1];
    uint32_t i = (uint32_t)((key * kIdfMul) >> A.shift);
    for (;;) {
        const uint64_t k = A.tab_keys[i];
        if (k == key) return A.tab_wts[i];
        if (k == 0) return A.default_w;
        i = (i + 1) & A.mask;
    }
}

// T_KEYS: where the tokens of this wave's document go -- its slots begin at its byte offset within the piece and there are
// as many as it has bytes, cut at the end of the piece's arrays whatever the offsets say
__device__ __forceinline__ void text_keys_doc(TextIdfAux& A, uint64_t byte0, size_t len, size_t doc) {
    const bool in = byte0 >= A.slot_base && byte0 - A.slot_base <= A.slot_cap;
    A.slot0 = in ? byte0 - A.slot_base : 0;
    uint64_t room = in ? A.slot_cap - A.slot0 : 0;
    room = room < (uint64_t)len ? room : (uint64_t)len;
    A.doc_cap = (uint32_t)(room < 0x7fffffffull ? room : 0x7fffffffull);
    A.ord = (uint32_t)doc;
}

// what one wave carries through a document: between two steps offline, from one push to the next in a stream
struct TextWave {
    uint64_t m0 = ~0ull, m1 = ~0ull;  // MinHash running minima: slots lane, lane + 64
    uint32_t ones = 0;                // SimHash: count of bit `lane`
    uint64_t pos = 0, tot = 0;        // T_IDF: weight of the tokens with bit `lane` set, weight of all tokens (Q16.16 sums)
    uint32_t total_tok = 0;           // complete tokens consumed by flushes (net of carried ones)
    bool any_shingle = false;
    // wave-uniform tokenizer state of the current LDS batch
    uint32_t ntok = 0;        // tokens opened in this batch (the last one may be unfinished)
    uint32_t cbase = 0;       // word bytes written in this batch
    bool carry = false;       // the byte just before the current step was a word byte
    uint32_t prev_last = 0;   // that byte
};

// no room for another step: it opens at most 32 tokens and writes at most 64 + 32 bytes
__device__ __forceinline__ bool text_batch_full(const TextWave& W) {
    return W.ntok + kStepTok > (uint32_t)kTokCap || W.cbase + W.ntok + kStepRoom > (uint32_t)kCanonCap;
}

// MinHash with H slots: a lane keeps NR = ceil(H / 64) running minima, slots lane + 64 r.  The first two
// are TextWave's m0 and m1 (what a stream saves and restores); the others live in an array of the kernel's, `mx`, that
// only constant indices touch, so it stays in registers.  NR = 1 leaves m1 alone.
constexpr int text_mx_len(int NR) { return NR > 2 ? NR - 2 : 1; }

// consume the batch: hash complete items, fold them in, carry the tail to the front
template <int MODE, int NR = 2>
__device__ __forceinline__ void text_flush(WaveLds& L, TextWave& W, uint32_t k, int lane, bool final,
                                           const TextIdfAux* A = nullptr, uint64_t* mx = nullptr) {
    constexpr bool MODE_SIM = MODE != T_MIN;   // the items are single tokens
    wave_sync();
    const uint32_t ncomplete = W.ntok - (W.carry && !final ? 1u : 0u);
    uint32_t nitems, keep_from;
    if (MODE_SIM) {
        nitems = ncomplete;
        keep_from = ncomplete;
    } else if (ncomplete >= k) {
        nitems = ncomplete - k + 1;
        keep_from = ncomplete - (k - 1);
    } else if (final && !W.any_shingle && ncomplete > 0) {
        nitems = 1;  // fewer than k tokens in the whole document: one shingle of all of them
        keep_from = ncomplete;
    } else {
        nitems = 0;
        keep_from = 0;
    }
    for (uint32_t s0 = 0; s0 < nitems; s0 += 64) {
        const uint32_t s = s0 + lane;
        if (s < nitems) {
            uint32_t e;
            if (MODE_SIM) e = s;
            else e = ncomplete >= k ? s + k - 1 : ncomplete - 1;
            const uint32_t a = L.cstart[s], b = L.cend[e];
            const uint64_t h = xxh3_lds(L.canon + a, (size_t)(b - a));
            if (MODE != T_KEYS) L.h1[s] = h;
            if (MODE == T_MIN) L.h2[s] = mix_h2(h);
            if (MODE == T_IDF) L.h2[s] = idf_lookup(*A, h);   // one probe sequence per lane: 64 independent gathers
            if (MODE == T_KEYS) {
                const uint32_t t = W.total_tok + s;
                if (t < A->doc_cap) {
                    A->key_out[A->slot0 + t] = h;
                    A->ord_out[A->slot0 + t] = A->ord;
                }
            }
        }
    }
    wave_sync();
    if (MODE == T_SIM) {
        for (uint32_t s = 0; s < nitems; s++) W.ones += (uint32_t)((L.h1[s] >> lane) & 1ull);
    } else if (MODE == T_IDF) {
        for (uint32_t s = 0; s < nitems; s++) {
            const uint64_t w = L.h2[s];   // < 2^32; at most 2^31 tokens, so neither sum wraps
            W.pos += ((L.h1[s] >> lane) & 1ull) ? w : 0ull;
            W.tot += w;
        }
    } else if (MODE == T_MIN) {
        constexpr int kUnroll = NR <= 2 ? 4 : NR <= 4 ? 2 : 1;
#pragma unroll kUnroll
        for (uint32_t s = 0; s < nitems; s++) {
            const uint64_t h = L.h1[s], g = L.h2[s];
            const uint64_t v0 = h + (uint64_t)lane * g;
            const uint64_t v1 = v0 + (g << 6);
            W.m0 = v0 < W.m0 ? v0 : W.m0;
            if (NR >= 2) W.m1 = v1 < W.m1 ? v1 : W.m1;
            uint64_t v = v1;
#pragma unroll
            for (int r = 2; r < NR; r++) {
                v += g << 6;
                mx[r - 2] = v < mx[r - 2] ? v : mx[r - 2];
            }
        }
    }
    if (nitems) W.any_shingle = true;
    W.total_tok += keep_from;
    if (final) return;
    // carry tokens [keep_from, ntok) to the front
    if (keep_from == 0) return;  // nothing consumed (fewer than k complete tokens): the caller re-checks room
    const uint32_t src0 = keep_from < W.ntok ? L.cstart[keep_from] : W.cbase + W.ntok - 1 + (W.carry ? 1u : 0u);
    const uint32_t used = W.cbase + (W.ntok ? W.ntok - 1 : 0);   // bytes of canon in use
    const uint32_t nkeep = W.ntok - keep_from;
    wave_sync();
    uint16_t ks = 0, ke = 0;
    if ((uint32_t)lane < nkeep) {   // nkeep <= k <= 64
        ks = (uint16_t)(L.cstart[keep_from + lane] - src0);
        ke = (uint16_t)(L.cend[keep_from + lane] - src0);
    }
    for (uint32_t o = 0; src0 + o < used; o += 64) {
        const uint32_t i = src0 + o + lane;
        const uint8_t v = i < used ? L.canon[i] : 0;
        wave_sync();
        if (i < used) L.canon[o + lane] = v;
        wave_sync();
    }
    if ((uint32_t)lane < nkeep) {
        L.cstart[lane] = ks;
        L.cend[lane] = ke;
    }
    // word bytes kept = total kept bytes minus the separators between kept tokens
    const uint32_t kept_bytes = used > src0 ? used - src0 : 0;
    W.ntok = nkeep;
    W.cbase = kept_bytes - (nkeep ? nkeep - 1 : 0);
    wave_sync();
}

// One 64-byte step over L.stage[64 sub ..]: lane = byte at `pos`, bytes at or past `end` are not processed.  Writes the
// word bytes and token bounds into the batch (the caller made room) and returns the step's word mask.  carry and
// prev_last come out as after a FULL step: a caller whose range can end inside a step (a stream's push) corrects them.
__device__ __forceinline__ uint64_t text_step(WaveLds& L, TextWave& W, int sub, size_t pos, size_t end, bool pretok, int lane) {
    const uint32_t c = L.stage[64 * sub + lane];
    const uint32_t q = L.stage[64 * sub + lane + 1];
    uint32_t p = __shfl_up(c, 1, 64);
    if (lane == 0) p = W.prev_last;
    const bool w = pos < end && inword(p, c, q, pretok);
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
        uint32_t ch = c;
        if (!pretok && ch - 'A' <= 25u) ch += 32;
        L.canon[cpos] = (uint8_t)ch;
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
    W.prev_last = __shfl(c, 63, 64);
    return inw;
}

// ---- the marked step (text_grapheme.hip): token starts come from a mask, not from the word rule ----
// Every byte of the document is a token byte and tokens abut, so a 64-byte step can open 64 tokens and add 64 bytes plus
// 64 separators.  The byte room of the word step already covers that; the token cap is checked against 64.  After a
// flush at most k <= 64 tokens remain (k - 1 complete ones and the unfinished one), so, as for the word step, the token
// cap cannot fail right after a flush and UCFP_TEXT_MAX_WINDOW_BYTES holds unchanged: the kept bytes are a prefix of one
// k-token window, refused exactly when prefix + 1 + kStepRoom > kCanonCap.
constexpr int kMarkedStepTok = 64;
static_assert(64 + kMarkedStepTok <= kStepRoom, "a marked step's bytes and separators fit the room every step demands");
static_assert(64 + kMarkedStepTok <= kTokCap, "the k <= 64 tokens a flush keeps leave room for a marked step's tokens");

__device__ __forceinline__ bool text_batch_full_marked(const TextWave& W) {
    return W.ntok + kMarkedStepTok > (uint32_t)kTokCap || W.cbase + W.ntok + kStepRoom > (uint32_t)kCanonCap;
}

// One 64-byte step: lane = the byte `ch` (already canonical) at `pos`, bytes at or past `end` are not processed; bit i of
// `starts` says that lane i's byte begins a token; the document's first byte always does.  The last token of a step
// stays open (W.carry): the next start, or the caller at the document's end, closes it.
__device__ __forceinline__ void text_step_marked(WaveLds& L, TextWave& W, uint32_t ch, uint64_t starts, size_t pos, size_t end,
                                                 int lane) {
    const bool w = pos < end;
    const uint64_t inw = __ballot(w);
    if (W.ntok == 0) starts |= 1ull;   // a document's first byte begins its first token, whatever the mask says
    starts &= inw;
    const uint32_t nin_before = popc_below(inw, lane);
    const uint32_t nst_before = popc_below(starts, lane);
    const bool is_start = (starts >> lane) & 1ull;
    if (w) {
        const uint32_t tok = W.ntok + nst_before + (is_start ? 1u : 0u) - 1u;
        const uint32_t cpos = W.cbase + nin_before + tok;
        L.canon[cpos] = (uint8_t)ch;
        if (is_start) {
            L.cstart[tok] = (uint16_t)cpos;
            if (tok > 0) {   // the separator in front of it, and the end of the token before it
                L.canon[cpos - 1] = ' ';
                L.cend[tok - 1] = (uint16_t)(cpos - 1);
            }
        }
    }
    W.ntok += (uint32_t)__popcll(starts);
    W.cbase += (uint32_t)__popcll(inw);
    W.carry = W.carry || inw != 0;
}

// The end of a document: its status, and its record at `rec` (MinHash: 8 + 8 h bytes; SimHash: 8), zero unless the status
// is 0.  h <= 64 NR; a lane whose slot lane + 64 r is not below h stores nothing.
template <int MODE, int NR = 2>
__device__ __forceinline__ int32_t text_emit(uint8_t* rec, const TextWave& W, bool nonascii, bool too_long, int lane,
                                             uint32_t h = 128, const uint64_t* mx = nullptr) {
    constexpr bool MODE_SIM = MODE != T_MIN;
    int32_t stv = 0;
    if (nonascii) stv = 1;                    // non-ASCII in raw mode: host must pre-tokenise
    else if (too_long) stv = -2;              // UCFP_E_UNSUPPORTED: a token / k-token run exceeds the LDS batch
    else if (W.total_tok == 0 || (!MODE_SIM && !W.any_shingle)) stv = -1;   // UCFP_E_MODALITY: no tokens
    else if (MODE == T_IDF && W.tot == 0) stv = -1;   // every token weighs 0 (T9.3)
    if (MODE == T_KEYS) return stv;   // no record: the keys went out in the flushes
    if (MODE_SIM) {
        const uint64_t bits = MODE == T_IDF ? __ballot(2ull * W.pos > W.tot) : __ballot(2u * W.ones > W.total_tok);
        if (lane == 0) {
            const uint64_t v = stv == 0 ? bits : 0ull;
            for (int b = 0; b < 8; b++) rec[b] = (uint8_t)(v >> (8 * b));
        }
    } else {
        // the records are only 8-byte aligned when the base is: write dwords
        const uint64_t a = stv == 0 ? W.m0 : 0ull, b = stv == 0 ? W.m1 : 0ull;
        uint32_t* o0 = reinterpret_cast<uint32_t*>(rec + 8 + 8 * lane);
        uint32_t* o1 = reinterpret_cast<uint32_t*>(rec + 8 + 8 * (lane + 64));
        if ((uint32_t)lane < h) {
            o0[0] = (uint32_t)a;
            o0[1] = (uint32_t)(a >> 32);
        }
        if (NR >= 2 && (uint32_t)lane + 64u < h) {
            o1[0] = (uint32_t)b;
            o1[1] = (uint32_t)(b >> 32);
        }
#pragma unroll
        for (int r = 2; r < NR; r++) {
            const uint64_t c = stv == 0 ? mx[r - 2] : 0ull;
            if ((uint32_t)lane + 64u * (uint32_t)r < h) {
                uint32_t* o = reinterpret_cast<uint32_t*>(rec + 8 + 8 * (lane + 64 * r));
                o[0] = (uint32_t)c;
                o[1] = (uint32_t)(c >> 32);
            }
        }
        if (lane == 0) {
            uint32_t* o32 = reinterpret_cast<uint32_t*>(rec);
            o32[0] = stv == 0 ? 1u : 0u;  // schema: u16 = 1, pad
            o32[1] = 0;
        }
    }
    return stv;
}
}  // namespace

}  // namespace ucfp
