// text_html.hip -- HTML pages -> text on the GPU (gfx950): the `preprocess = html` stage of the text route
// (src/modality/text.rs:751-767 behind POST .../preprocess/html, src/server/handlers.rs:628-699).
//
// A total function from bytes to bytes: markup is dropped, character references are decoded, white space is folded.
// Spec: DESIGN.md T12, rules M1..M8; plain-Python restatement: tests/text_html_ref.py; named references:
// include/ucfp_text_html_tab.h (tools/gen_text_html_tab.py).  txtfp::html_to_text is not in the tree: parity unpinned.
//
// ONE WAVE PER DOCUMENT, 64 source bytes per step, no workgroup barrier (the launch shape of text_canon.hip).  A step:
//   A  lane = byte.  The step's bytes go to the LDS stage with the first 9 bytes of the next step behind them (the next
//      step's bytes are loaded one step early, so the look-ahead costs no second load).  A lane at `<` reads its
//      look-ahead and says what starts there (M1, M2) and, for a tag, its class (M4).  Ballots turn this into one 64-bit
//      mask per byte class.
//   B  the markup automaton -- text, TAG / EQ / DQ / SQ (M3), comment, declaration, raw text (M5) -- is resolved by a
//      wave-uniform loop on those masks: from one state change to the next with find-first-set on the mask the current
//      state cares about.  It runs once per state change in the step, not once per byte (`="value"` with both quotes in
//      the step is one turn: the loop is scalar code, and a CU's SIMDs share one scalar unit), and leaves two masks: the lanes
//      in text, and the lanes whose `>` ends markup that leaves a space (M6).  The state, the tag's class, the comment's
//      earliest end and the last two `-` bits are carried from step to step as wave-uniform values.
//   C  a lane at a `&` in text matches its reference (M7) against the wave's LDS copy of the name table, filled at the
//      document's first `&` in text.  A reference
//      covers the lanes up to its `;` (its body holds neither `&` nor `<`, so references never overlap and
//      never change state): a lane finds the nearest reference start at or below it and asks whether a `;` lies between.
//      A reference that runs into the next step carries the count of bytes it still covers.
//   D  every lane now emits 0 .. 4 bytes that are white space or not.  M8 from the two ballots and two carried bits
//      ("white space pending", "something emitted"): a lane that emits text puts one space before it when white space lies
//      between it and the text before it.  A wave scan gives the positions.
//
// SIZING: count -> scan -> emit (template <bool EMIT>), as text_canon.hip: one compact blob under one n + 1 offsets array,
// the shape every text entry takes.  The output is never longer than the input, so the caller's buffer
// needs ucfp_text_html_bound = n_bytes; the emit pass never writes past the length the count pass found.
//
// Output writes are plain byte stores of vector lanes; nothing is written twice.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "../../include/ucfp_text_html_tab.h"
#include "ctx.h"
#include "text_core.h"

namespace ucfp {

namespace {

__device__ const uint64_t d_ent_keys[UCFP_TEXT_HTML_TAB_N] = UCFP_TEXT_HTML_TAB_KEYS;
__device__ const uint16_t d_ent_cps[UCFP_TEXT_HTML_TAB_N] = UCFP_TEXT_HTML_TAB_CPS;
const uint64_t h_ent_keys[UCFP_TEXT_HTML_TAB_N] = UCFP_TEXT_HTML_TAB_KEYS;
const uint16_t h_ent_cps[UCFP_TEXT_HTML_TAB_N] = UCFP_TEXT_HTML_TAB_CPS;
static_assert(UCFP_TEXT_HTML_TAB_MAX_CP <= 0xFFFFu, "the code points of the named references fit 16 bits");
static_assert(UCFP_TEXT_HTML_TAB_MAX_NAME == 8, "a name packs into one uint64_t");

constexpr int kLookAhead = 9;   // `</script` or `</strong` and the delimiter; `&thetasym;`

constexpr int kEntSlots = 256;   // the table of named references, padded to a power of two for a bisection of fixed depth
static_assert(UCFP_TEXT_HTML_TAB_N <= kEntSlots, "the bisection below runs over 256 slots");

// one wave's LDS: the byte stage, and the wave's own copy of the named references -- a `&` in text costs eight dependent
// look-ups, which from LDS are eight short ones.  The copy is made at a document's first `&` in text, so a page without
// one, or a short document, does not pay for it
struct HtmlLds {
    uint64_t ent_keys[kEntSlots];         // ascending; ~0 behind the last name
    uint16_t ent_cps[kEntSlots];
    uint8_t bytes[64 + kLookAhead + 7];   // [0, 64): this step; [64, 73): the next step's first bytes (0 past the end)
};

// M7, named, on the device: lower bound over the padded copy.  No name packs to ~0, and the padding's code point is 0.
__device__ __forceinline__ uint32_t entity_lookup_lds(const HtmlLds& L, uint64_t key) {
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t step = kEntSlots / 2; step; step >>= 1)
        if (L.ent_keys[lo + step - 1] < key) lo += step;
    return L.ent_keys[lo] == key ? (uint32_t)L.ent_cps[lo] : 0u;
}

// the automaton's states (M2, M3, M5)
enum : uint32_t { H_TEXT = 0, H_TAG, H_EQ, H_DQ, H_SQ, H_COMMENT, H_DECL, H_RAW };
// what a `<` starts (M1, M2) and a tag's class (M4)
enum : uint32_t { K_NONE = 0, K_TAG, K_COMMENT, K_DECL };
enum : uint32_t { C_BREAK = 0, C_INLINE, C_SCRIPT, C_STYLE };

constexpr uint64_t pack_name(const char* s) {
    uint64_t v = 0;
    for (int t = 0; s[t]; t++) v |= (uint64_t)(uint8_t)s[t] << (8 * t);
    return v;
}

// M4: the inline set
constexpr uint64_t kInline[] = {
    pack_name("a"),     pack_name("abbr"),  pack_name("b"),      pack_name("bdi"),    pack_name("bdo"),  pack_name("big"),
    pack_name("cite"),  pack_name("code"),  pack_name("data"),   pack_name("del"),    pack_name("dfn"),  pack_name("em"),
    pack_name("font"),  pack_name("i"),     pack_name("ins"),    pack_name("kbd"),    pack_name("label"), pack_name("mark"),
    pack_name("q"),     pack_name("s"),     pack_name("samp"),   pack_name("small"),  pack_name("span"), pack_name("strike"),
    pack_name("strong"), pack_name("sub"),  pack_name("sup"),    pack_name("time"),   pack_name("tt"),   pack_name("u"),
    pack_name("var"),   pack_name("wbr")};
static_assert(sizeof(kInline) / sizeof(kInline[0]) == 32, "DESIGN.md T12 M4 lists 32 inline names");

__host__ __device__ __forceinline__ bool is_ws(uint32_t c) { return c == 9u || c == 10u || c == 12u || c == 13u || c == 32u; }
__host__ __device__ __forceinline__ bool is_letter(uint32_t c) { return (c | 32u) - 97u < 26u; }
__host__ __device__ __forceinline__ bool is_delim(uint32_t c) { return is_ws(c) || c == '/' || c == '>'; }

// M7, named: the code point of the name packed in `key`, or 0 (no name has code point 0)
__host__ __device__ __forceinline__ uint32_t entity_lookup(const uint64_t* keys, const uint16_t* cps, uint64_t key) {
    int lo = 0, hi = UCFP_TEXT_HTML_TAB_N;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < UCFP_TEXT_HTML_TAB_N && keys[lo] == key ? (uint32_t)cps[lo] : 0u;
}

// M4 for the tag name that starts `at` (0 or 1) bytes into the 8 bytes of `w` (byte t of w = the byte t + 1 after `<`):
// the name ends at the first ws, `/` or `>`; a name of more than 6 bytes, or one the document's end cuts off (a zero
// byte is no delimiter), is a break tag.
__device__ __forceinline__ uint32_t classify_tag(uint64_t w, uint32_t at) {
    uint64_t name = 0;
    bool closed = false;
#pragma unroll
    for (uint32_t t = 0; t < 7; t++) {
        const uint32_t b = (uint32_t)(w >> (8 * (at + t))) & 255u;   // at + t <= 7
        if (!closed) {
            if (is_delim(b)) closed = true;
            else if (t < 6 && b != 0u) name |= (uint64_t)(b - 65u < 26u ? b | 32u : b) << (8 * t);
            else name = ~0ull;   // a seventh name byte, or a 0x00 in the name (it would pack as nothing): no member
        }
    }
    if (!closed) return C_BREAK;
    if (name == pack_name("script")) return C_SCRIPT;
    if (name == pack_name("style")) return C_STYLE;
    bool in = false;
#pragma unroll
    for (uint64_t m : kInline) in |= name == m;
    return in ? C_INLINE : C_BREAK;
}

struct HtmlRef {
    uint32_t len;   // bytes of the reference, `&` and `;` included: 0 when there is none, else 4 .. 10
    uint32_t cp;
};

// M7 for the `&` whose 9 following bytes are w (8) and b9
__device__ __forceinline__ HtmlRef match_ref(const HtmlLds& L, uint64_t w, uint32_t b9) {
    uint32_t semi = 0;   // index of the first `;` among the 9 bytes, 9 = none
    {
        bool found = false;
        semi = 9;
#pragma unroll
        for (uint32_t t = 0; t < 9; t++) {
            const uint32_t b = t < 8 ? (uint32_t)(w >> (8 * t)) & 255u : b9;
            if (!found && b == ';') {
                found = true;
                semi = t;
            }
        }
    }
    if (semi == 9 || semi == 0) return {0u, 0u};
    const uint32_t b0 = (uint32_t)w & 255u, b1 = (uint32_t)(w >> 8) & 255u;
    if (b0 == '#') {
        const bool hex = (b1 | 32u) == 'x';
        const uint32_t first = hex ? 2u : 1u, digits = semi - first;
        if (semi <= first || digits > (hex ? 6u : 7u)) return {0u, 0u};
        uint32_t v = 0;
        bool ok = true;
#pragma unroll
        for (uint32_t t = 1; t < 8; t++) {
            if (t >= first && t < semi) {
                const uint32_t b = (uint32_t)(w >> (8 * t)) & 255u;
                const uint32_t d = b - '0' < 10u ? b - '0' : hex && ((b | 32u) - 'a' < 6u) ? (b | 32u) - 'a' + 10u : 99u;
                ok &= d != 99u;
                v = v * (hex ? 16u : 10u) + (d & 15u);   // 7 decimal or 6 hex digits stay below 2^32
            }
        }
        if (!ok) return {0u, 0u};
        if (v == 0u || v - 0xD800u < 0x800u || v > 0x10FFFFu) v = 0xFFFDu;
        return {semi + 2u, v};
    }
    const uint64_t key = semi == 8 ? w : w & ((1ull << (8 * semi)) - 1ull);
    // a 0x00 in the body would pack as nothing (`lt\0` as `lt`): no name holds one
    const uint64_t body = semi == 8 ? w : w | ~0ull << (8 * semi);
    if ((body - 0x0101010101010101ull) & ~body & 0x8080808080808080ull) return {0u, 0u};
    const uint32_t cp = entity_lookup_lds(L, key);
    return {cp ? semi + 2u : 0u, cp};
}

__device__ __forceinline__ uint64_t bits_from(uint32_t p) { return p < 64u ? ~0ull << p : 0ull; }   // lanes >= p

}  // namespace

// EMIT = false: text_off[doc + 1] = the document's text bytes, flags[doc] (when not NULL) its two flag bits.
// EMIT = true (after the scan): the text bytes go to text + text_off[doc].
template <bool EMIT>
__global__ __launch_bounds__(64 * kWavesPerBlock) void text_html_kernel(
    const uint8_t* __restrict__ html, const uint64_t* __restrict__ offsets, size_t n, uint64_t* __restrict__ text_off,
    uint8_t* __restrict__ text, uint32_t* __restrict__ flags) {
    __shared__ HtmlLds lds[kWavesPerBlock];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t doc = (size_t)blockIdx.x * kWavesPerBlock + wave;
    if (doc >= n) return;  // whole wave
    HtmlLds& L = lds[wave];
    const uint8_t* __restrict__ src = html + offsets[doc];
    const size_t len = (size_t)(offsets[doc + 1] - offsets[doc]);
    uint8_t* out = nullptr;
    uint64_t final_len = 0;
    if (EMIT) {
        out = text + text_off[doc];
        final_len = text_off[doc + 1] - text_off[doc];
        if (final_len == 0) return;
    }

    // wave-uniform state, carried from step to step
    uint32_t state = H_TEXT;
    bool tag_space = false;      // the open tag leaves a space (every class but inline)
    uint32_t tag_raw = 0;        // C_SCRIPT / C_STYLE: the open tag is a start tag that raw text follows (M5)
    uint32_t raw_kind = 0;       // H_RAW: whose end tag ends it
    uint32_t cmin = 0;           // H_COMMENT: the first lane whose `>` may end it (M2: `-->` begins after `<!--`)
    uint64_t dash_carry = 0;     // bit 0: the byte two before this step is `-`; bit 1: the byte before it is
    uint32_t ref_skip = 0;       // leading bytes of this step a reference of the last one covers
    bool ws_pending = false, emitted = false, high = false;   // M8's two bits; flag bit 0
    uint64_t out_pos = 0;

    bool tab_ready = false;      // the wave's LDS copy of the name table is filled: at the first `&` in text, if any
    uint32_t c_next = (size_t)lane < len ? src[lane] : 0u;
    for (size_t base = 0; base < len; base += 64) {
        const size_t pos = base + lane;
        const bool valid = pos < len;
        const uint32_t c = c_next;
        c_next = pos + 64 < len ? src[pos + 64] : 0u;
        // ---- A: stage, classify ----
        wave_lds_sync();
        L.bytes[lane] = (uint8_t)c;
        if (lane < kLookAhead) L.bytes[64 + lane] = (uint8_t)c_next;
        wave_lds_sync();
        uint32_t kind = K_NONE, cls = C_BREAK;
        bool is_end = false;
        if (c == '<') {
            uint64_t w = 0;
#pragma unroll
            for (int t = 0; t < 8; t++) w |= (uint64_t)L.bytes[lane + 1 + t] << (8 * t);
            const uint32_t b1 = (uint32_t)w & 255u, b2 = (uint32_t)(w >> 8) & 255u, b3 = (uint32_t)(w >> 16) & 255u;
            if (is_letter(b1)) {
                kind = K_TAG;
                cls = classify_tag(w, 0);
            } else if (b1 == '/' && is_letter(b2)) {
                kind = K_TAG;
                is_end = true;
                cls = classify_tag(w, 1);
            } else if (b1 == '!') {
                kind = b2 == '-' && b3 == '-' ? K_COMMENT : K_DECL;
            } else if (b1 == '?') {
                kind = K_DECL;
            }
        }
        const uint64_t VALID = __ballot(valid);
        const uint64_t MK = __ballot(kind != K_NONE), CM = __ballot(kind == K_COMMENT), DC = __ballot(kind == K_DECL);
        const uint64_t IN = __ballot(cls == C_INLINE), SC = __ballot(cls == C_SCRIPT), ST = __ballot(cls == C_STYLE);
        const uint64_t EN = __ballot(is_end);
        const uint64_t GT = __ballot(c == '>'), EQ = __ballot(c == '='), DQ = __ballot(c == '"'), SQ = __ballot(c == '\'');
        const uint64_t WS = __ballot(valid && is_ws(c)), DASH = __ballot(c == '-'), SEMI = __ballot(c == ';');
        const uint64_t CEND = GT & (DASH << 1 | dash_carry >> 1) & (DASH << 2 | (dash_carry & 2ull) | (dash_carry & 1ull));
        dash_carry = DASH >> 62;

        // ---- B: the automaton, one turn per state change (a quoted attribute value is one turn, not three) ----
        // The loop runs on the scalar unit, which the CU's four SIMDs share: every instruction in it counts.
        const uint64_t NWE = VALID & ~(WS | EQ);   // EQ state: what ends the wait for a value
        uint64_t T = 0, SP = 0;
        uint32_t p = 0;
        while (p < 64u) {
            const uint64_t ge = ~0ull << p;
            if (state == H_TEXT) {
                const uint64_t m = MK & ge;
                if (!m) {
                    T |= ge;
                    break;
                }
                const uint32_t q = (uint32_t)__builtin_ctzll(m);
                const uint64_t bit = 1ull << q;
                T |= ge & (bit - 1ull);
                if (CM & bit) {
                    state = H_COMMENT;
                    cmin = q + 6;
                } else if (DC & bit) {
                    state = H_DECL;
                } else {
                    state = H_TAG;
                    tag_space = !(IN & bit);
                    tag_raw = (EN & bit) ? 0u : (SC & bit) ? (uint32_t)C_SCRIPT : (ST & bit) ? (uint32_t)C_STYLE : 0u;
                }
                p = q + 1;
            } else if (state == H_TAG || state == H_EQ) {
                const uint64_t m = (state == H_TAG ? GT | EQ : NWE) & ge;
                if (!m) break;
                const uint32_t q = (uint32_t)__builtin_ctzll(m);
                const uint64_t bit = 1ull << q;
                p = q + 1;
                if (GT & bit) {            // the tag ends
                    if (tag_space) SP |= bit;
                    state = tag_raw ? H_RAW : H_TEXT;
                    raw_kind = tag_raw;
                } else if (state == H_EQ) {
                    state = (DQ & bit) ? H_DQ : (SQ & bit) ? H_SQ : H_TAG;
                } else {
                    state = H_EQ;
                    // the common case `="value"` in one turn: the quote right behind `=`, its partner in this step
                    const uint64_t nb = p < 64u ? 1ull << p : 0ull;
                    const uint64_t QM = (DQ & nb) ? DQ : (SQ & nb) ? SQ : 0ull;
                    if (QM) {
                        const uint64_t m2 = p + 1u < 64u ? QM & (~0ull << (p + 1u)) : 0ull;
                        if (!m2) {
                            state = (DQ & nb) ? H_DQ : H_SQ;
                            break;
                        }
                        state = H_TAG;
                        p = (uint32_t)__builtin_ctzll(m2) + 1u;
                    }
                }
            } else {                       // the states that wait for one byte class
                const uint64_t m = (state == H_DQ        ? DQ
                                    : state == H_SQ      ? SQ
                                    : state == H_COMMENT ? CEND & bits_from(cmin)
                                    : state == H_DECL    ? GT
                                                         : EN & (raw_kind == C_SCRIPT ? SC : ST)) &
                                   ge;
                if (!m) break;
                const uint32_t q = (uint32_t)__builtin_ctzll(m);
                if (state == H_DQ || state == H_SQ) {
                    state = H_TAG;
                } else if (state == H_RAW) {   // the end tag runs by M3 and leaves a space
                    state = H_TAG;
                    tag_space = true;
                    tag_raw = 0;
                } else {                       // a comment or a declaration ends
                    state = H_TEXT;
                    SP |= 1ull << q;
                }
                p = q + 1;
            }
        }
        T &= VALID;
        cmin = cmin > 64u ? cmin - 64u : 0u;

        // ---- C: references ----
        const bool in_text = (T >> lane) & 1ull;
        HtmlRef ref = {0u, 0u};
        if (!tab_ready && __ballot(in_text && c == '&')) {   // a page without a reference never pays for the table
            for (int t = lane; t < kEntSlots; t += 64) {
                L.ent_keys[t] = t < UCFP_TEXT_HTML_TAB_N ? d_ent_keys[t] : ~0ull;
                L.ent_cps[t] = t < UCFP_TEXT_HTML_TAB_N ? d_ent_cps[t] : (uint16_t)0;
            }
            wave_lds_sync();
            tab_ready = true;
        }
        if (in_text && c == '&') {   // only a `&` in text is matched: attribute values are full of them
            uint64_t w = 0;
#pragma unroll
            for (int t = 0; t < 8; t++) w |= (uint64_t)L.bytes[lane + 1 + t] << (8 * t);
            ref = match_ref(L, w, L.bytes[lane + 9]);
        }
        const bool is_ref = ref.len != 0u;
        const uint64_t R = __ballot(is_ref);
        bool covered = (uint32_t)lane < ref_skip;
        {
            const uint64_t r = R & (lane == 63 ? ~0ull : (2ull << lane) - 1ull);
            if (r) {
                const uint32_t i = 63u - (uint32_t)__builtin_clzll(r);
                if ((uint32_t)lane > i) {
                    const uint32_t gap = (uint32_t)lane - i - 1u;   // bytes strictly between the `&` and this lane
                    covered |= ((SEMI >> (i + 1u)) & ((1ull << gap) - 1ull)) == 0ull;
                }
            }
        }
        {   // the last reference of the step may run into the next one
            const uint64_t over = __ballot(is_ref && (uint32_t)lane + ref.len > 64u);
            ref_skip = over ? (uint32_t)__shfl((int)((uint32_t)lane + ref.len - 64u), (int)__builtin_ctzll(over), 64) : 0u;
        }

        // ---- D: what every lane emits, M8, positions ----
        uint32_t nb = 0, enc = 0;
        bool ws_out = (SP >> lane) & 1ull;
        if (is_ref) {
            const uint32_t cp = ref.cp;
            if (is_ws(cp)) {
                ws_out = true;
            } else if (cp < 0x80u) {
                nb = 1, enc = cp;
            } else if (cp < 0x800u) {
                nb = 2, enc = (0xC0u | cp >> 6) | (0x80u | (cp & 0x3Fu)) << 8;
            } else if (cp < 0x10000u) {
                nb = 3, enc = (0xE0u | cp >> 12) | (0x80u | (cp >> 6 & 0x3Fu)) << 8 | (0x80u | (cp & 0x3Fu)) << 16;
            } else {
                nb = 4, enc = (0xF0u | cp >> 18) | (0x80u | (cp >> 12 & 0x3Fu)) << 8 | (0x80u | (cp >> 6 & 0x3Fu)) << 16 |
                              (0x80u | (cp & 0x3Fu)) << 24;
            }
        } else if (in_text && !covered) {
            if (is_ws(c)) ws_out = true;
            else nb = 1, enc = c;
        }
        const uint64_t W = __ballot(ws_out), N = __ballot(nb != 0u);
        high |= __ballot(nb != 0u && (enc & 0x80u)) != 0ull;   // a reference's first byte is >= 0x80 when any of them is
        uint32_t space = 0;
        if (nb) {
            const uint64_t below = (1ull << lane) - 1ull;
            const uint64_t nprev = N & below;
            if (nprev) {
                const uint32_t j = 63u - (uint32_t)__builtin_clzll(nprev);
                space = (W & below & (~0ull << j)) != 0ull;
            } else {
                space = emitted && (ws_pending || (W & below) != 0ull);
            }
        }
        const uint32_t contrib = nb + space;
        const uint32_t incl = wave_incl_scan(contrib, lane);
        if (EMIT && contrib) {
            uint64_t at = out_pos + (incl - contrib);
            if (space) {
                if (at < final_len) out[at] = (uint8_t)' ';
                at++;
            }
            for (uint32_t t = 0; t < nb; t++, at++)
                if (at < final_len) out[at] = (uint8_t)(enc >> (8 * t));
        }
        out_pos += (uint32_t)__shfl((int)incl, 63, 64);
        if (N) {
            emitted = true;
            ws_pending = (W & (~0ull << (63 - __builtin_clzll(N)))) != 0ull;
        } else {
            ws_pending |= W != 0ull;
        }
    }
    if (EMIT) return;
    if (lane == 0) {
        text_off[doc + 1] = out_pos;
        if (flags) flags[doc] = (high ? 1u : 0u) | (state != H_TEXT ? 2u : 0u);
    }
}

int launch_text_html(const uint8_t* html, const uint64_t* offsets, size_t n, uint8_t* text, uint64_t* text_off, uint32_t* flags,
                     hipStream_t stream) {
    const unsigned grid = (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock);
    if (n)
        hipLaunchKernelGGL(text_html_kernel<false>, dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, html, offsets, n, text_off, text,
                           flags);
    launch_text_canon_scan(text_off, n, stream);   // lengths -> offsets, text_off[0] = 0 (n = 0 included)
    if (n)
        hipLaunchKernelGGL(text_html_kernel<true>, dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, html, offsets, n, text_off, text,
                           flags);
    return 0;
}

}  // namespace ucfp

extern "C" {

size_t ucfp_text_html_bound(size_t n_bytes) { return n_bytes; }

int ucfp_text_html_entity(const char* name, size_t len, uint32_t* cp) {
    if (cp) *cp = 0;
    if (!name || len == 0 || len > UCFP_TEXT_HTML_TAB_MAX_NAME) return 0;
    uint64_t key = 0;
    for (size_t t = 0; t < len; t++) {
        if (!name[t]) return 0;
        key |= (uint64_t)(uint8_t)name[t] << (8 * t);
    }
    const uint32_t v = ucfp::entity_lookup(ucfp::h_ent_keys, ucfp::h_ent_cps, key);
    if (!v) return 0;
    if (cp) *cp = v;
    return 1;
}

int ucfp_text_html_batch_dev(ucfp_ctx* ctx, const uint8_t* d_html, const uint64_t* d_offsets, size_t n, uint8_t* d_text,
                             uint64_t* d_text_offsets, uint32_t* d_flags, void* stream) {
    if (!ctx) return ucfp::capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (n > 0x7fffffffu) return ucfp::capi_fail(UCFP_E_INVALID, "batch of %zu documents exceeds one launch", n);
    if (!d_text_offsets) return ucfp::capi_fail(UCFP_E_INVALID, "text_offsets is NULL");
    if (n && (!d_offsets || !d_text)) return ucfp::capi_fail(UCFP_E_INVALID, "offsets/text is NULL");
    ucfp::launch_text_html(d_html, d_offsets, n, d_text, d_text_offsets, d_flags, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return UCFP_OK;
}

int ucfp_text_html_batch(ucfp_ctx* ctx, const uint8_t* html, const uint64_t* offsets, size_t n, uint8_t* text, size_t text_cap,
                         uint64_t* text_offsets, uint32_t* flags) {
    if (!ctx) return ucfp::capi_fail(UCFP_E_INVALID, "ctx is NULL");
    if (n > 0x7fffffffu) return ucfp::capi_fail(UCFP_E_INVALID, "batch of %zu documents exceeds one launch", n);
    if (n == 0) {
        if (text_offsets) text_offsets[0] = 0;
        return UCFP_OK;
    }
    if (!offsets || !text_offsets) return ucfp::capi_fail(UCFP_E_INVALID, "offsets/text_offsets is NULL");
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return ucfp::capi_fail(UCFP_E_INVALID, "offsets must be non-decreasing");
    const size_t base = offsets[0], total = offsets[n] - offsets[0];
    if (total && !html) return ucfp::capi_fail(UCFP_E_INVALID, "html is NULL");
    const size_t o_off = (total + 16 + 255) & ~(size_t)255;
    const size_t in_bytes = o_off + (n + 1) * 8;
    const size_t o_fl = ((n + 1) * 8 + 255) & ~(size_t)255;
    const size_t o_txt = o_fl + ((n * 4 + 255) & ~(size_t)255);
    const size_t out_bytes = o_txt + ucfp_text_html_bound(total) + 64;
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = ucfp::grow(&ctx->stage_in, &ctx->stage_in_cap, in_bytes);
    if (rc) return rc;
    rc = ucfp::grow(&ctx->stage_out, &ctx->stage_out_cap, out_bytes);
    if (rc) return rc;
    hipStream_t st = ctx->host_stream;
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = offsets[i] - base;
    if (total) HIP_TRY(hipMemcpyAsync(ctx->stage_in, html + base, total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->stage_in + o_off, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    uint64_t* d_toff = reinterpret_cast<uint64_t*>(ctx->stage_out);
    uint32_t* d_fl = reinterpret_cast<uint32_t*>(ctx->stage_out + o_fl);
    ucfp::launch_text_html(ctx->stage_in, reinterpret_cast<const uint64_t*>(ctx->stage_in + o_off), n, ctx->stage_out + o_txt, d_toff,
                           d_fl, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(text_offsets, d_toff, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (flags) HIP_TRY(hipMemcpyAsync(flags, d_fl, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const size_t made = (size_t)text_offsets[n];
    if (made > text_cap || (made && !text))
        return ucfp::capi_fail(UCFP_E_INVALID, "the text has %zu bytes, the caller's buffer %zu (ucfp_text_html_bound)", made, text_cap);
    if (made) {
        HIP_TRY(hipMemcpyAsync(text, ctx->stage_out + o_txt, made, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return UCFP_OK;
}

}  // extern "C"
