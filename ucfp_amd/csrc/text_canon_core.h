// text_canon_core.h -- the canon stage of the text kernels, once: the step body of the UTF-8 canonicaliser (DESIGN.md
// U1..U5) as text_canon_kernel (text_canon.hip, whole documents, count and emit passes) and the canon stage of
// text_stream_kernel<true> (text_streams.hip, held || chunk of a push) run it.  Here: the flag words of a canonical code
// point, the LDS stage of one wave, the UAX#29 boundary table, step parts A + B (canon_place: decode, validate, look up,
// place) and C + D (canon_decide: boundaries, segments, the provisional keep and its rewind, the UTF-8 re-encode, the
// context for the next step), and canon_whole, which the grapheme tokeniser (text_grapheme.hip) runs in place
// of C + D: the whole canonical stream, no boundaries.  The kernels keep what differs between them: where a byte comes from, which step is the
// last, where a byte goes (the store functor), and the load and store of their state.
// A header of its own, not a part of text_core.h: the hash stage needs nothing of the code-point table and the canon
// stage nothing of the LDS batch; what the two share is the launch shape, which this header takes from text_core.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ucfp_text_gtab.h"
#include "../../include/ucfp_text_utab.h"
#include "common.h"
#include "text_core.h"

namespace ucfp {

namespace {

constexpr uint32_t kCpMask = 0x1FFFFu, kAlnum = 1u << 28, kVowel = 1u << 27, kFlagMask = 0xFu << 23 | kAlnum | kVowel;
constexpr uint32_t kNone = kCpMask | 15u << 23;   // "no code point": class 15 is in no class set, the value no apostrophe
// Canonical code points a step can add: a code point whose lead byte lies in the step has at most 3x its own bytes of
// canonical UTF-8 (U1), and those code points span at most 64 + 3 bytes.
constexpr int kStepCps = 3 * 67;
constexpr int kXCap = 2 + 1 + kStepCps + 4;

struct CanonLds {
    uint8_t bytes[3 + 64 + 3 + 2];   // [0, 3): the previous step's last bytes; [3, 67): this step; [67, 70): the next step's first
    uint32_t x[kXCap];               // [0, 2): context; then the undecided code point of the last step, then this step's
};

// wave-uniform state of the decision.  Positions (P: uint64_t in a document, uint32_t in a stream's slice) count the
// stream (' ' token)*.
template <class P>
struct CanonSeg {
    uint32_t pend = 0;            // 1: x[2] holds a code point whose boundary waits for its right neighbour
    P out_pos = 0;                // stream bytes so far, the open segment included
    P seg_start = 0;              // where the open segment began
    bool seg_alnum = false;       // the open segment has an alphanumeric: it is a token
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

struct CanonPlaced {
    bool err;         // malformed UTF-8 or a code point outside the covered set (wave-uniform; nothing was placed)
    uint32_t added;   // canonical code points the step made
};

// Step parts A + B.  Lane = the byte `c` at `pos` of `len`; L.bytes holds the step's bytes and their neighbours.  Places
// the step's canonical code points in L.x behind the `pend` undecided one.
__device__ __forceinline__ CanonPlaced canon_place(CanonLds& L, uint32_t c, size_t pos, size_t len, int lane, uint32_t pend,
                                                   const uint16_t* stage1, const uint32_t* stage2, const uint32_t* pool) {
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
            err = c < 0xC2u || c > 0xF4u || pos + need >= len || (c1 & 0xC0u) != 0x80u;   // cut by the end (a stream: of a final push only)
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
            e = stage2[((uint32_t)stage1[cp >> UCFP_TEXT_UTAB_SHIFT] << UCFP_TEXT_UTAB_SHIFT) |
                       (cp & ((1u << UCFP_TEXT_UTAB_SHIFT) - 1u))];
            if (!(e >> 31)) err = true;
            else nout = ((e >> 29) & 3u) == 2u ? (e >> 17) & 7u : 1u;
        }
    }
    if (__ballot(err)) return {true, 0u};
    const uint32_t incl = wave_incl_scan(nout, lane);
    const uint32_t added = __shfl(incl, 63, 64);
    if (nout) {
        const uint32_t at = 2u + pend + incl - nout;   // < 2 + 1 + kStepCps
        const uint32_t kind = (e >> 29) & 3u;
        if (kind == 0) L.x[at] = cp | (e & kFlagMask);
        else if (kind == 1) L.x[at] = (e & kCpMask) | (e & kFlagMask);
        else
            for (uint32_t t = 0; t < nout; t++) L.x[at + t] = pool[(e & kCpMask) + t];
    }
    wave_lds_sync();
    return {false, added};
}

// Step parts C + D over the S.pend + added code points in L.x (`final`: the last step, which decides them all), then the
// context for the next step (`c`: the lane's source byte).  store(p, byte) writes the byte at stream position p, bounds
// included; a Store with kEmit = false only counts (no stores, no fence, no byte assembly).
template <class P, class Store>
__device__ __forceinline__ void canon_decide(CanonLds& L, CanonSeg<P>& S, uint32_t c, uint32_t added, bool final, int lane,
                                             const Store& store) {
    const uint32_t m = S.pend + added;
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
        const bool carried_has = S.seg_alnum || (amask & (fb == 64 ? ~0ull : (1ull << fb) - 1ull)) != 0;
        const bool drop0 = bmask != 0 && !carried_has;
        // this lane's segment: [its last boundary at or before the lane, the next boundary)
        const uint64_t le = bmask & (~0ull >> (63 - lane));
        const int sb = le ? 63 - __builtin_clzll(le) : -1;
        const uint64_t gt = lane == 63 ? 0ull : bmask & (~0ull << (lane + 1));
        const int eb = gt ? __builtin_ctzll(gt) : 64;
        const uint64_t range = (eb == 64 ? ~0ull : (1ull << eb) - 1ull) & (sb <= 0 ? ~0ull : ~((1ull << sb) - 1ull));
        const bool seg_has = (amask & range) != 0 || (sb < 0 && S.seg_alnum);
        const bool keep = has && (eb == 64 || seg_has);   // the open segment is kept provisionally
        const uint32_t cpw = w & kCpMask;
        const uint32_t nb = cpw < 0x80u ? 1u : cpw < 0x800u ? 2u : cpw < 0x10000u ? 3u : 4u;
        const uint32_t contrib = keep ? nb + (bnd ? 1u : 0u) : 0u;
        const uint32_t cincl = wave_incl_scan(contrib, lane);
        const uint32_t excl = cincl - contrib;
        const P base_pos = drop0 ? S.seg_start : S.out_pos;
        if (Store::kEmit) {
            // A rewind: other lanes are about to store where the provisional bytes went.  One wave's stores are issued in
            // program order, so a fence at WAVEFRONT scope is all the ordering the two generations of stores need.
            if (drop0) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            if (keep) {
                P p = base_pos + excl;
                uint32_t bytes;
                if (nb == 1) bytes = cpw;
                else if (nb == 2) bytes = (0xC0u | cpw >> 6) | (0x80u | (cpw & 0x3Fu)) << 8;
                else if (nb == 3) bytes = (0xE0u | cpw >> 12) | (0x80u | (cpw >> 6 & 0x3Fu)) << 8 | (0x80u | (cpw & 0x3Fu)) << 16;
                else
                    bytes = (0xF0u | cpw >> 18) | (0x80u | (cpw >> 12 & 0x3Fu)) << 8 | (0x80u | (cpw >> 6 & 0x3Fu)) << 16 |
                            (0x80u | (cpw & 0x3Fu)) << 24;
                if (bnd) {
                    store(p, (uint8_t)' ');
                    p++;
                }
                for (uint32_t t = 0; t < nb; t++, p++) store(p, (uint8_t)(bytes >> (8 * t)));
            }
        }
        if (bmask) {
            const int hb = 63 - __builtin_clzll(bmask);
            S.seg_start = base_pos + __shfl(excl, hb, 64);
            S.seg_alnum = (amask >> hb) != 0;
        } else {
            S.seg_alnum = S.seg_alnum || amask != 0;
        }
        S.out_pos = base_pos + __shfl(cincl, 63, 64);
    }
    // context for the next step: the last two decided code points and the undecided one
    wave_lds_sync();
    const uint32_t keep3 = lane < 3 ? L.x[ndec + lane] : 0u;
    wave_lds_sync();
    if (lane < 3) L.x[lane] = keep3;
    if (lane >= 61) L.bytes[lane - 61] = (uint8_t)c;
    S.pend = m - ndec;
}

// a canonical code point whose Grapheme_Cluster_Break is Prepend, L, V or T (include/ucfp_text_gtab.h)
__device__ __host__ __forceinline__ bool grapheme_excluded(uint32_t cp) {
    constexpr uint32_t r[UCFP_TEXT_GTAB_N][2] = UCFP_TEXT_GTAB_RANGES;
    if (cp < UCFP_TEXT_GTAB_MIN || cp > UCFP_TEXT_GTAB_MAX) return false;
    bool in = false;
#pragma unroll
    for (int i = 0; i < UCFP_TEXT_GTAB_N; i++) in = in || (cp >= r[i][0] && cp <= r[i][1]);
    return in;
}

// The store mode of the grapheme tokeniser in place of parts C + D: the whole U3 stream, every one of
// the `added` code points canon_place put in L.x (there is no undecided one: pend = 0), re-encoded at stream position
// out_pos on; no boundaries, no segments, nothing dropped.  Returns false (wave-uniform) when a code point is outside
// the grapheme set.  Leaves the byte context for the next step, as canon_decide does.
template <class P, class Store>
__device__ __forceinline__ bool canon_whole(CanonLds& L, P& out_pos, uint32_t c, uint32_t added, int lane, const Store& store) {
    bool excl_any = false;
    for (uint32_t j0 = 0; j0 < added; j0 += 64) {
        const uint32_t j = j0 + lane;
        const bool has = j < added;
        const uint32_t cpw = has ? L.x[2u + j] & kCpMask : 0u;
        excl_any |= has && grapheme_excluded(cpw);
        const uint32_t nb = cpw < 0x80u ? 1u : cpw < 0x800u ? 2u : cpw < 0x10000u ? 3u : 4u;
        const uint32_t contrib = has ? nb : 0u;
        const uint32_t cincl = wave_incl_scan(contrib, lane);
        if (Store::kEmit && has) {
            P p = out_pos + (cincl - contrib);
            uint32_t bytes;
            if (nb == 1) bytes = cpw;
            else if (nb == 2) bytes = (0xC0u | cpw >> 6) | (0x80u | (cpw & 0x3Fu)) << 8;
            else if (nb == 3) bytes = (0xE0u | cpw >> 12) | (0x80u | (cpw >> 6 & 0x3Fu)) << 8 | (0x80u | (cpw & 0x3Fu)) << 16;
            else
                bytes = (0xF0u | cpw >> 18) | (0x80u | (cpw >> 12 & 0x3Fu)) << 8 | (0x80u | (cpw >> 6 & 0x3Fu)) << 16 |
                        (0x80u | (cpw & 0x3Fu)) << 24;
            for (uint32_t t = 0; t < nb; t++, p++) store(p, (uint8_t)(bytes >> (8 * t)));
        }
        out_pos += __shfl(cincl, 63, 64);
    }
    wave_lds_sync();
    if (lane >= 61) L.bytes[lane - 61] = (uint8_t)c;
    return __ballot(excl_any) == 0;
}

}  // namespace

}  // namespace ucfp
