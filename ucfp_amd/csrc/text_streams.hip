// text_streams.hip -- streaming MinHash-128 and streaming SimHash, TF and TF.IDF:
// device-resident text sessions, batched pushes, for gfx950.
//
// Counterpart of text::StreamingMinHashSession::new / push / finalize (src/modality/text.rs:645-730) behind the stream
// ingest route (src/server/handlers.rs:590-626).  The reference buffers the whole document and hashes it at the end; a
// MinHash record is 128 minima over the document's shingles and a shingle is final as soon as its k-th token closes, so
// here a stream is the offline kernel (text.hip) with its wave state loaded at the start of a push and stored at the
// end.  What text_hash_kernel carries over a flush of its LDS batch -- the last k - 1 complete tokens and the unfinished
// one, a prefix of one k-token window -- is exactly what a stream carries from one push to the next.
//
// ONE WAVE PER (stream, chunk) ENTRY of a push, four waves per block, no workgroup barrier: the shape of
// text_hash_kernel<false>.  A long chunk is therefore serial on one wave.
//   load   the slot's state (TextStreamState): minima to registers, the kept canonical bytes and token bounds to LDS
//   bytes  the wave reads pending || chunk, where `pending` is the one raw byte the previous push held back: whether a
//          byte is inside a word depends on the byte after it, and a stream must not guess that byte.  A non-final push
//          processes all but the last byte, which becomes the new `pending`; a final push processes every byte and the
//          byte past the end reads as 0, as offline
//   steps  tokenise / write canonical / room check / flush: the offline kernel's, the same code (text_step and text_flush
//          of text_core.h); only a push's last step, which may be partial, corrects `carry` and `prev_last` afterwards
//   end    non-final: flush(false), then the state goes back; final: close an open token, flush(true), emit the record
//
// UTF-8 STREAMS (sets made with UCFP_TEXT_STREAMS_UTF8; DESIGN.md T7 "UTF-8 streams", restated in plain Python in
// tests/text_canon_stream_ref.py).  ONE FUSED LAUNCH: text_stream_kernel<true> is the kernel above with a streaming form
// of text_canon_kernel (text_canon.hip) in front for the entries whose slot is RAW_UTF8.  The wave canonicalises
// held || chunk into its slice of the set's scratch as (' ' token)*, then hashes that slice as the next piece of a
// PRETOKENIZED stream: a leading or a doubled space means nothing there, and a piece that ends inside a token continues
// it.  The canon stage's wave state (CanonStreamState) is loaded and stored the same way:
//   held   the bytes of a UTF-8 sequence a non-final chunk ends in (at most 3) wait, raw, for the next chunk
//   pend   the last canonical code point stays undecided, as between two 64-byte steps offline; a final push decides it
//   prov   an open segment that has an alphanumeric is a token and its bytes go out; one that has none is written, then
//          taken back into the state (at most UCFP_TEXT_STREAM_OPEN_SEGMENT_BYTES, more is NEEDS_HOST) and restored to
//          the front of the next push's slice
// The step body is text_canon_kernel's, the same code (canon_place and canon_decide of text_canon_core.h), as the hash
// stage's is text_hash_kernel's.  text_stream_kernel<false, ..> is what sets without the flag launch.
//
// SIMHASH STREAMS (sets made by ucfp_text_streams_create_sim).  The kernel's second template parameter is
// the MODE of text_core.h: T_MIN above, T_SIM (text.rs:328-343) and T_IDF (text.rs:344-362; the table of text_idf.hip).
// A SimHash item is one token and is final as soon as the token closes, so what survives flush(false) is at most the
// unfinished token, at canon[0]: a slot (SimStreamState) keeps 64 counters -- `ones` of bit `lane`, or T_IDF's `pos` --
// the total weight, that token's bytes, and the tokeniser words a MinHash slot keeps.  Bytes, steps, the held-back byte,
// the canon stage and the statuses are the ones above, the same code; the record is text_emit<MODE>'s 8 bytes.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "ctx.h"
#include "text_canon_core.h"
#include "text_core.h"

#define fail ucfp::capi_fail

namespace ucfp {

namespace {

constexpr int kKeepTok = 64 + 2;   // tokens a stored state can hold: k - 1 complete ones and an unfinished one, k <= 64

// one slot of a set on the device; what the wave of text_hash_kernel holds in registers and LDS between two steps
struct TextStreamState {
    uint64_t m0[64], m1[64];        // running minima of slots lane, lane + 64
    uint64_t total_bytes;           // bytes pushed so far
    uint32_t ntok, cbase;           // kept tokens (the last may be unfinished), their word bytes
    uint32_t carry, prev_last;      // the last processed byte was a word byte; that byte
    uint32_t total_tok;
    uint32_t flags;                 // kAnyShingle | kNonAscii | kTooLong
    uint32_t pending;               // kPendValid | the held-back byte
    uint32_t mode;
    uint16_t cstart[kKeepTok], cend[kKeepTok];
    uint8_t canon[kCanonCap];       // tok ' ' tok ' ' ...: cbase + ntok - 1 bytes in use
};
static_assert(sizeof(TextStreamState) <= 4096 && sizeof(TextStreamState) % 8 == 0, "about 3 KiB per stream");
static_assert(offsetof(TextStreamState, canon) % 4 == 0 && offsetof(WaveLds, canon) % 4 == 0, "canon moves as dwords");

// one slot of a SimHash set: CNT = uint32_t for T_SIM (`ones`), uint64_t for T_IDF (`pos`)
template <typename CNT>
struct SimStreamState {
    CNT cnt[64];                    // lane b: tokens (T_SIM) or weight of the tokens (T_IDF) with bit b set
    uint64_t tot;                   // T_IDF: weight of all tokens
    uint64_t total_bytes;
    uint32_t ntok, cbase;           // 0 or 1 kept token, the unfinished one, which begins at canon[0]; its bytes
    uint32_t carry, prev_last;
    uint32_t total_tok;
    uint32_t flags;
    uint32_t pending;
    uint32_t mode;
    uint8_t canon[kCanonCap];
};
static_assert(sizeof(SimStreamState<uint32_t>) == 1840 && sizeof(SimStreamState<uint64_t>) == 2096, "about 2 KiB per stream");
static_assert(offsetof(SimStreamState<uint32_t>, canon) % 4 == 0 && offsetof(SimStreamState<uint64_t>, canon) % 4 == 0,
              "canon moves as dwords");

template <int MODE> struct StreamStateOf { using type = TextStreamState; };
template <> struct StreamStateOf<T_SIM> { using type = SimStreamState<uint32_t>; };
template <> struct StreamStateOf<T_IDF> { using type = SimStreamState<uint64_t>; };

enum : uint32_t { kAnyShingle = 1, kNonAscii = 2, kTooLong = 4, kPendValid = 0x100 };
enum : uint32_t { kEntFinal = 1, kEntFresh = 2, kEntModeShift = 2 };

// one entry of a push, planned on the host
struct TextStreamEntry {
    uint64_t off, len;   // the chunk: bytes[off, off + len)
    uint32_t slot, flags;
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// ---------------------------------------- the streaming canonicaliser ----------------------------------------

constexpr uint32_t kProvCap = UCFP_TEXT_STREAM_OPEN_SEGMENT_BYTES;
// a slice holds the restored provisional bytes, 4 x (held + chunk) (ucfp_text_canon_bound) and the code point the last
// push left undecided with its separator; slices begin on 128-byte lines so that no two waves share one
constexpr uint64_t kSliceSlack = kProvCap + 4 * 3 + 8;
constexpr uint64_t kSliceAlign = 128;

// one slot's canon stage between two pushes (wave-uniform in text_canon_kernel)
struct CanonStreamState {
    uint32_t x[3];              // two context code points and the undecided one (valid when pend)
    uint32_t pend, seg_alnum;   // seg_alnum: the open segment has an alphanumeric, its bytes went out
    uint32_t bad;               // sticky NEEDS_HOST
    uint32_t nheld, held;       // raw bytes of an incomplete UTF-8 sequence, byte i in bits [8i, 8i + 8)
    uint32_t nprov, pad_;
    uint8_t prov[kProvCap];     // the open segment's canonical bytes, separator included, while it has no alphanumeric
};
static_assert(sizeof(CanonStreamState) == 40 + kProvCap && sizeof(CanonStreamState) % 8 == 0, "about 300 bytes per stream");

struct CanonSlice {
    uint64_t off;   // into the set's scratch
    uint32_t cap, pad_;
};

struct CanonArgs {
    CanonStreamState* cstates;
    const CanonSlice* slices;   // per entry of the push
    uint8_t* scratch;
    const uint16_t* stage1;     // the code-point table of text_canon.hip
    const uint32_t* stage2;
    const uint32_t* pool;
};

static_assert(sizeof(CanonLds) <= sizeof(WaveLds::h1) && offsetof(WaveLds, h1) % 8 == 0, "the canon stage borrows h1");

// where a byte of the piece goes: position p of the slice
struct SliceStore {
    static constexpr bool kEmit = true;
    uint8_t* out;
    uint32_t cap;
    __device__ __forceinline__ void operator()(uint32_t p, uint8_t v) const {
        if (p < cap) out[p] = v;
    }
};

// One push of one RAW_UTF8 stream through the canon stage: V = held || chunk, of which a non-final push processes all
// but an incomplete sequence at the end.  Writes the piece -- the part of the stream (' ' token)* this push settles --
// to out[0, cap) and returns its length; *bad_out: the stream is handed back (now or by an earlier push).  Steps A..D
// are text_canon_kernel<true>'s (text_canon_core.h); positions are relative to the slice, which begins with the restored
// provisional bytes.
__device__ __forceinline__ uint32_t canon_stream_push(CanonLds& L, const CanonArgs& ca, CanonStreamState& C,
                                                      const uint8_t* __restrict__ chunk, size_t clen, bool fin, bool fresh,
                                                      uint8_t* out, uint32_t cap, int lane, bool* bad_out) {
    CanonSeg<uint32_t> S;
    uint32_t nheld = 0, held = 0, nprov = 0;
    bool bad = false;
    uint32_t xin = kNone;
    if (!fresh) {
        S.pend = uni(C.pend) & 1u;
        S.seg_alnum = uni(C.seg_alnum) != 0;
        bad = uni(C.bad) != 0;
        nheld = uni(C.nheld);
        held = uni(C.held);
        nprov = uni(C.nprov);
        if (nheld > 3u) nheld = 0;                 // a stored state never has more: keeps every index in range
        if (nprov > kProvCap) nprov = 0;
        if (lane < 3) xin = C.x[lane];
    }
    if (bad) {
        *bad_out = true;
        return 0;
    }
    if (nprov > cap) nprov = 0;                    // (the host sizes every slice above kProvCap)
    for (uint32_t i = lane; i < nprov; i += 64) out[i] = C.prov[i];
    wave_lds_sync();                               // the LDS behind L was the hash stage's of the block's last entry
    if (lane < 3) {
        L.x[lane] = xin;
        L.bytes[lane] = 0;   // V begins where a sequence begins: a continuation byte there is claimed by nobody
    }

    const size_t vlen = (size_t)nheld + clen;
    auto V = [&](size_t i) -> uint32_t { return i < nheld ? (held >> (8u * (uint32_t)i)) & 0xffu : (uint32_t)chunk[i - nheld]; };
    // the incomplete sequence a non-final push ends in: the last lead byte among the last three, reaching past the end
    uint32_t nh = 0;
    if (!fin) {
        for (uint32_t back = 1; back <= 3u && back <= vlen; back++) {
            const uint32_t b = V(vlen - back);
            if (b < 0x80u) break;
            if (b >= 0xC0u) {
                const uint32_t seq = b >= 0xF0u ? 4u : b >= 0xE0u ? 3u : 2u;
                nh = back < seq ? back : 0u;
                break;
            }
        }
    }
    const size_t len = vlen - nh;
    uint32_t new_held = 0;
    for (uint32_t t = 0; t < nh; t++) new_held |= V(len + t) << (8u * t);

    S.out_pos = nprov;            // slice bytes so far, the open segment included
    S.seg_start = 0;              // where the open segment began (a provisional one: at the slice's front)
    const SliceStore store{out, cap};

    for (size_t base = 0; base < len || (fin && base == 0); base += 64) {   // a final push decides `pend` even without bytes
        const size_t pos = base + lane;
        const uint32_t c = pos < len ? V(pos) : 0u;
        wave_lds_sync();
        L.bytes[3 + lane] = (uint8_t)c;
        if (lane < 3) L.bytes[67 + lane] = base + 64 + lane < len ? (uint8_t)V(base + 64 + lane) : (uint8_t)0;
        wave_lds_sync();
        const CanonPlaced pl = canon_place(L, c, pos, len, lane, S.pend, ca.stage1, ca.stage2, ca.pool);   // A, B
        if (pl.err) {
            bad = true;
            break;
        }
        canon_decide(L, S, c, pl.added, fin && base + 64 >= len, lane, store);                             // C, D
    }
    if (S.out_pos > cap) bad = true;   // cannot happen (the slice holds 4 x the bytes): refuse rather than hash a cut piece

    // ---- what this push settles, and what goes back into the state ----
    uint32_t plen = 0, np = 0;
    if (!bad) {
        if (fin) {
            plen = S.seg_alnum ? S.out_pos : S.seg_start;   // the last segment closes at the stream's end
        } else if (S.seg_alnum) {
            plen = S.out_pos;                           // an open token: its bytes so far go out, the next piece continues it
        } else {
            plen = S.seg_start;
            np = S.out_pos - S.seg_start;
            if (np > kProvCap) bad = true, plen = 0, np = 0;   // the documented open-segment condition
        }
    }
    if (!fin) {
        if (np) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the bytes were stored by other lanes of this wave
            for (uint32_t i = lane; i < np; i += 64) C.prov[i] = out[S.seg_start + i];
        }
        wave_lds_sync();
        if (lane < 3) C.x[lane] = L.x[lane];
        if (lane == 0) {
            C.pend = S.pend;
            C.seg_alnum = S.seg_alnum ? 1u : 0u;
            C.bad = bad ? 1u : 0u;
            C.nheld = bad ? 0u : nh;
            C.held = new_held;
            C.nprov = np;
        }
    }
    *bad_out = bad;
    return plen;
}

}  // namespace

// MODE: T_MIN, T_SIM or T_IDF (never T_KEYS); `k` is 1 and `aux` the table of this push for the SimHash modes
template <bool UTF8, int MODE>
__global__ __launch_bounds__(64 * kWavesPerBlock) void text_stream_kernel(
    typename StreamStateOf<MODE>::type* __restrict__ states, const TextStreamEntry* __restrict__ ents, size_t n,
    const uint8_t* __restrict__ bytes, uint32_t k, uint8_t* __restrict__ out, int32_t* __restrict__ status, CanonArgs ca,
    TextIdfAux aux) {
    static_assert(MODE == T_MIN || MODE == T_SIM || MODE == T_IDF, "T_KEYS is never a stream mode");
    constexpr size_t kRecBytes = MODE == T_MIN ? UCFP_MINHASH_BYTES : UCFP_SIMHASH_BYTES;
    const TextIdfAux* A = MODE == T_IDF ? &aux : nullptr;
    __shared__ WaveLds lds[kWavesPerBlock];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t ei = (size_t)blockIdx.x * kWavesPerBlock + wave;
    if (ei >= n) return;  // whole wave
    WaveLds& L = lds[wave];
    const TextStreamEntry ent = ents[ei];
    const uint32_t eflags = uni(ent.flags);
    const bool fin = eflags & kEntFinal, fresh = eflags & kEntFresh;
    typename StreamStateOf<MODE>::type& S = states[uni(ent.slot)];

    TextWave W;
    bool nonascii = false, too_long = false;
    uint32_t pend = 0;
    uint32_t mode = eflags >> kEntModeShift;
    uint64_t total_bytes = 0;
    bool dead = false;   // a sticky status was stored by an earlier push: nothing is processed any more

    // ---- load ----
    if (!fresh) {
        if constexpr (MODE == T_MIN) {
            W.m0 = S.m0[lane];
            W.m1 = S.m1[lane];
        } else if constexpr (MODE == T_SIM) {
            W.ones = S.cnt[lane];
        } else {
            W.pos = S.cnt[lane];
            W.tot = S.tot;
        }
        total_bytes = S.total_bytes;
        W.ntok = uni(S.ntok);
        W.cbase = uni(S.cbase);
        W.carry = uni(S.carry) != 0;
        W.prev_last = uni(S.prev_last);
        W.total_tok = uni(S.total_tok);
        const uint32_t f = uni(S.flags);
        W.any_shingle = f & kAnyShingle;
        nonascii = f & kNonAscii;
        too_long = f & kTooLong;
        dead = nonascii || too_long;
        pend = uni(S.pending);
        mode = uni(S.mode);
        if (W.ntok > (MODE == T_MIN ? 64u : 1u)) W.ntok = MODE == T_MIN ? 64u : 0u;   // a stored state never has more: keeps every index in range
        if (W.cbase + W.ntok > (uint32_t)kCanonCap) W.cbase = 0, W.ntok = 0;
        const uint32_t used = W.cbase + (W.ntok ? W.ntok - 1 : 0);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(S.canon);
        uint32_t* dst = reinterpret_cast<uint32_t*>(L.canon);
        for (uint32_t i = lane; 4 * i < used; i += 64) dst[i] = src[i];
        if constexpr (MODE == T_MIN) {
            if ((uint32_t)lane < W.ntok) {
                L.cstart[lane] = S.cstart[lane];
                L.cend[lane] = S.cend[lane];
            }
        } else {
            if (lane == 0 && W.ntok) L.cstart[0] = 0;   // the unfinished token: a flush left it at the front, its end is not known yet
        }
    }
    const bool pretok = UTF8 ? mode != UCFP_TEXT_RAW_ASCII : mode == UCFP_TEXT_PRETOKENIZED;   // a canon piece is pre-tokenised

    // ---- RAW_UTF8: canonicalise held || chunk into the entry's scratch slice; the hash stage below reads the piece ----
    const uint8_t* src_bytes = bytes + ent.off;
    size_t src_len = (size_t)ent.len;
    bool canon_bad = false;
    if (UTF8 && (eflags >> kEntModeShift) == (uint32_t)UCFP_TEXT_RAW_UTF8) {
        const CanonSlice sl = ca.slices[ei];
        uint8_t* piece = ca.scratch + sl.off;
        // the hash stage's h1 is idle until the first flush: the canon stage's LDS lives there
        CanonLds& CL = *reinterpret_cast<CanonLds*>(L.h1);
        src_len = canon_stream_push(CL, ca, ca.cstates[uni(ent.slot)], src_bytes, src_len, fin, fresh, piece, uni(sl.cap), lane,
                                    &canon_bad);
        src_bytes = piece;
        // the piece was stored by this wave's lanes and is loaded by others of them: the stores complete before the loads issue
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        wave_sync();
    }

    // ---- the bytes of this push: V = pending || chunk; V[0, proc) is processed, V[proc] is the byte after it ----
    const uint32_t npend = dead ? 0u : (pend >> 8) & 1u;
    const uint32_t pbyte = pend & 0xffu;
    const size_t clen = src_len;
    const uint8_t* __restrict__ chunk = src_bytes;            // V[i] = chunk[i - npend] for i >= npend
    const size_t vlen = dead ? 0 : npend + clen;
    const size_t proc = fin ? vlen : (vlen ? vlen - 1 : 0);
    const bool aligned4 = ((reinterpret_cast<uintptr_t>(chunk) - npend) & 3u) == 0;
    auto load_chunk = [&](size_t base) -> uint32_t {  // this lane's 4 bytes of V[base, base + 256)
        const size_t o = base + 4 * (size_t)lane;
        if (o >= vlen) return 0u;
        if (aligned4 && o >= npend && o + 4 <= vlen) return *reinterpret_cast<const uint32_t*>(chunk + (o - npend));
        uint32_t v = 0;
        for (int j = 0; j < 4; j++) {
            const size_t i = o + j;
            if (i < vlen) v |= (i < npend ? pbyte : (uint32_t)chunk[i - npend]) << (8 * j);
        }
        return v;
    };
    uint32_t cur = load_chunk(0);
    for (size_t base = 0; base < proc && !too_long; base += 256) {
        const uint32_t nxt = load_chunk(base + 256);
        wave_sync();
        *reinterpret_cast<uint32_t*>(&L.stage[4 * lane]) = cur;
        if (lane == 0) *reinterpret_cast<uint32_t*>(&L.stage[256]) = __builtin_amdgcn_readfirstlane(nxt);
        wave_sync();
        if (!pretok) nonascii |= (cur & 0x80808080u) != 0;
#pragma unroll 1
        for (int sub = 0; sub < 4; sub++) {
            const size_t pos = base + 64 * sub + lane;
            if (base + 64 * sub >= proc) break;
            if (text_batch_full(W)) {   // make room
                text_flush<MODE>(L, W, k, lane, false, A);
                if (text_batch_full(W)) too_long = true;
                if (too_long) break;
            }
            const uint64_t inw = text_step(L, W, sub, pos, proc, pretok, lane);
            // the last PROCESSED byte: a step that ends the push may be partial, text_step's carry and prev_last are a full one's
            const size_t left = proc - (base + 64 * sub);
            if (left < 64) W.carry = (inw >> (left - 1)) & 1ull;
            W.prev_last = __shfl((uint32_t)L.stage[64 * sub + lane], left < 64 ? (int)left - 1 : 63, 64);
        }
        cur = nxt;
    }
    // the held-back byte of a non-final push: seen (it counts for NEEDS_HOST), not processed
    if (!fin && vlen) {
        const size_t i = vlen - 1;
        const uint32_t b = i < npend ? pbyte : (uint32_t)chunk[i - npend];
        pend = kPendValid | b;
        if (!pretok && b >= 0x80u) nonascii = true;
    }
    if (UTF8 && canon_bad) nonascii = true;   // the canon stage's NEEDS_HOST: sticky, and it wins over the hash stage's status
    const bool na = __ballot(nonascii) != 0;
    total_bytes += clen;

    if (!fin) {
        // ---- store: what survives flush(false) is a prefix of one k-token window (SimHash: of the unfinished token) ----
        if (!too_long && !dead) text_flush<MODE>(L, W, k, lane, false, A);
        if (too_long) W.ntok = 0, W.cbase = 0, W.carry = false;
        wave_sync();
        if constexpr (MODE == T_MIN) {
            S.m0[lane] = W.m0;
            S.m1[lane] = W.m1;
        } else if constexpr (MODE == T_SIM) {
            S.cnt[lane] = W.ones;
        } else {
            S.cnt[lane] = W.pos;
            if (lane == 0) S.tot = W.tot;
        }
        const uint32_t used = W.cbase + (W.ntok ? W.ntok - 1 : 0);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(L.canon);
        uint32_t* dst = reinterpret_cast<uint32_t*>(S.canon);
        for (uint32_t i = lane; 4 * i < used; i += 64) dst[i] = src[i];
        if constexpr (MODE == T_MIN) {
            if ((uint32_t)lane < W.ntok) {   // ntok <= k <= 64 after the flush
                S.cstart[lane] = L.cstart[lane];
                S.cend[lane] = L.cend[lane];
            }
        }
        if (lane == 0) {
            S.total_bytes = total_bytes;
            S.ntok = W.ntok;
            S.cbase = W.cbase;
            S.carry = W.carry ? 1u : 0u;
            S.prev_last = W.prev_last;
            S.total_tok = W.total_tok;
            S.flags = (W.any_shingle ? kAnyShingle : 0u) | (na ? kNonAscii : 0u) | (too_long ? kTooLong : 0u);
            S.pending = pend;
            S.mode = mode;
            status[ei] = na ? 1 : (too_long ? -2 : 0);
        }
        return;
    }

    // ---- final: close a token that runs to the end of the stream, the final flush, emit as text_hash_kernel does ----
    if (W.carry && W.ntok > 0 && lane == 0) L.cend[W.ntok - 1] = (uint16_t)(W.cbase + W.ntok - 1);
    if (!too_long && !dead) text_flush<MODE>(L, W, k, lane, true, A);
    const int32_t stv = text_emit<MODE>(out + ei * kRecBytes, W, na, too_long, lane);
    if (lane == 0) status[ei] = stv;
}

}  // namespace ucfp

// ================================================ host ================================================

#include "stream_set.h"

// the slot table counts bytes; the pinned tables hold a push
struct ucfp_text_streams : ucfp::streams::Slots, ucfp::streams::Tables {
    ucfp_ctx* ctx = nullptr;
    uint32_t k = 0;
    int kind = ucfp::T_MIN;               // the kernel's MODE: T_MIN, or T_SIM / T_IDF for a set of create_sim
    const ucfp_idf_table* table = nullptr;   // T_IDF: read at every push, not owned
    std::vector<uint8_t> fresh;           // opened, not pushed yet: the device state is not read
    std::vector<uint8_t> mode;
    void* states = nullptr;               // TextStreamState or SimStreamState<..> per slot, by `kind`
    ucfp::TextStreamEntry* tab_d = nullptr;           // the push table on the device; the next push waits for `done`
    // UTF-8 sets (UCFP_TEXT_STREAMS_UTF8); the push tables then carry a CanonSlice per entry behind the entries
    bool utf8 = false;
    uint64_t max_push_bytes = 0;          // RAW_UTF8 chunk bytes one push may carry: the scratch is sized for them
    ucfp::CanonArgs ca = {};              // canon states, scratch, the code-point table
};

namespace {

constexpr uint64_t kMaxStreamBytes = (uint64_t)1 << 63;
// A SimHash stream carries FEWER than this many bytes, so that no counter of any mode wraps.  text_emit<T_SIM> compares
// 2u * ones with total_tok in 32 bits and ones <= total_tok; T_IDF adds weights below 2^32 into 64-bit sums, which hold
// 2^31 of them (pos <= tot < 2^63, and 2 pos is compared).  Both are safe while total_tok < 2^31.  A token costs at least
// two canonical bytes, its separator included, and only the last token has none: c canonical bytes hold at most
// (c + 1) / 2 tokens.  A RAW_UTF8 stream of n bytes makes at most ucfp_text_canon_bound(n) = 4 n canonical bytes (the
// other modes at most n), so total_tok <= (4 n + 1) / 2 <= 2 n, and n < 2^30 gives total_tok <= 2^31 - 2.
constexpr uint64_t kSimStreamLimit = UCFP_TEXT_SIMHASH_STREAM_LIMIT_BYTES;
static_assert(2 * (kSimStreamLimit - 1) < ((uint64_t)1 << 31), "total_tok stays below 2^31 in a SimHash stream");
constexpr uint64_t kMaxPushBytes = (uint64_t)1 << 28;   // 4 x this, and a slice's cap, stay below 2^32

// the scratch slice of a RAW_UTF8 entry with a chunk of `len` bytes
uint64_t slice_bytes(uint64_t len) {
    return (ucfp_text_canon_bound((size_t)len) + ucfp::kSliceSlack + ucfp::kSliceAlign - 1) & ~(ucfp::kSliceAlign - 1);
}

// validates the push; nothing changes
int check_push(ucfp_text_streams* s, const uint32_t* slots, const uint64_t* n_bytes, size_t n) {
    if (n && (!slots || !n_bytes)) return fail(UCFP_E_INVALID, "slots / n_bytes is NULL");
    int rc = s->fits(n, "entries", "push");
    if (rc) return rc;
    const bool sim = s->kind != ucfp::T_MIN;
    for (size_t i = 0; i < n && rc == UCFP_OK; i++) {
        const uint32_t slot = slots[i];
        rc = s->mark(slot, "push");
        if (rc) break;
        if (sim) {   // s->n[slot] < kSimStreamLimit
            if (n_bytes[i] >= kSimStreamLimit - s->n[slot])
                rc = fail(UCFP_E_INVALID, "slot %u would reach 2^30 bytes: a SimHash stream carries fewer (UCFP_TEXT_SIMHASH_STREAM_LIMIT_BYTES)", slot);
        } else if (n_bytes[i] > kMaxStreamBytes - s->n[slot]) {
            rc = fail(UCFP_E_INVALID, "slot %u would pass 2^63 bytes", slot);
        }
    }
    s->unmark(slots, n);
    if (rc == UCFP_OK && s->table) {
        bool is_final = false;
        (void)ucfp::idf_table_aux(s->table, &is_final, nullptr);
        if (!is_final) rc = fail(UCFP_E_INVALID, "the IDF table is not final: call ucfp_idf_table_finalize or _set_weights");
    }
    if (rc == UCFP_OK && s->utf8) {
        uint64_t total = 0;
        for (size_t i = 0; i < n; i++)
            if (s->mode[slots[i]] == UCFP_TEXT_RAW_UTF8) total += n_bytes[i] < kMaxPushBytes ? n_bytes[i] : kMaxPushBytes + 1;
        if (total > s->max_push_bytes)
            rc = fail(UCFP_E_INVALID, "the RAW_UTF8 chunks of this push have %llu bytes, the set was created for %llu (max_push_bytes)",
                      (unsigned long long)total, (unsigned long long)s->max_push_bytes);
    }
    return rc;
}

// the set's lock is held; the push is valid
int push_impl(ucfp_text_streams* s, const uint32_t* slots, const uint64_t* n_bytes, const uint8_t* fin, size_t n,
              const uint8_t* d_bytes, uint8_t* d_out, int32_t* d_status, hipStream_t st) {
    if (n == 0) return UCFP_OK;
    HIP_TRY(hipSetDevice(s->ctx->device));
    // the pinned table this push fills was last copied two pushes ago
    int t = 0;
    int rc = s->next(&t);
    if (rc) return rc;
    ucfp::TextStreamEntry* tab = reinterpret_cast<ucfp::TextStreamEntry*>(s->tab_h[t]);
    ucfp::CanonSlice* slices = reinterpret_cast<ucfp::CanonSlice*>(tab + n);   // UTF-8 sets: behind the n entries
    uint64_t off = 0, soff = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t slot = slots[i];
        tab[i].off = off;
        tab[i].len = n_bytes[i];
        tab[i].slot = slot;
        tab[i].flags = ((fin && fin[i]) ? ucfp::kEntFinal : 0u) | (s->fresh[slot] ? ucfp::kEntFresh : 0u) |
                       ((uint32_t)s->mode[slot] << ucfp::kEntModeShift);
        off += n_bytes[i];
        if (s->utf8) {
            const uint64_t sb = s->mode[slot] == UCFP_TEXT_RAW_UTF8 ? slice_bytes(n_bytes[i]) : 0;   // check_push bounds the sum
            slices[i].off = soff;
            slices[i].cap = (uint32_t)sb;
            slices[i].pad_ = 0;
            soff += sb;
        }
    }
    const size_t tab_bytes = n * (sizeof(ucfp::TextStreamEntry) + (s->utf8 ? sizeof(ucfp::CanonSlice) : 0));
    HIP_TRY(hipStreamWaitEvent(st, s->done, 0));
    HIP_TRY(hipMemcpyAsync(s->tab_d, tab, tab_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->tab_copied[t], st));
    const unsigned grid = (unsigned)((n + ucfp::kWavesPerBlock - 1) / ucfp::kWavesPerBlock);
    ucfp::CanonArgs ca = s->utf8 ? s->ca : ucfp::CanonArgs{};
    if (s->utf8) ca.slices = reinterpret_cast<const ucfp::CanonSlice*>(s->tab_d + n);
    const ucfp::TextIdfAux aux = s->table ? ucfp::idf_table_aux(s->table, nullptr, nullptr) : ucfp::TextIdfAux{};   // check_push saw it final
#define UCFP_STREAM_LAUNCH(UTF8, MODE)                                                                                              \
    hipLaunchKernelGGL((ucfp::text_stream_kernel<UTF8, ucfp::MODE>), dim3(grid), dim3(64 * ucfp::kWavesPerBlock), 0, st,            \
                       static_cast<ucfp::StreamStateOf<ucfp::MODE>::type*>(s->states), s->tab_d, n, d_bytes, s->k, d_out, d_status, \
                       ca, aux)
    switch (s->kind * 2 + (s->utf8 ? 1 : 0)) {
        case ucfp::T_MIN * 2: UCFP_STREAM_LAUNCH(false, T_MIN); break;
        case ucfp::T_MIN * 2 + 1: UCFP_STREAM_LAUNCH(true, T_MIN); break;
        case ucfp::T_SIM * 2: UCFP_STREAM_LAUNCH(false, T_SIM); break;
        case ucfp::T_SIM * 2 + 1: UCFP_STREAM_LAUNCH(true, T_SIM); break;
        case ucfp::T_IDF * 2: UCFP_STREAM_LAUNCH(false, T_IDF); break;
        case ucfp::T_IDF * 2 + 1: UCFP_STREAM_LAUNCH(true, T_IDF); break;
        default: return fail(UCFP_E_INVALID, "stream set of unknown kind %d", s->kind);   // a missing kernel is an error
    }
#undef UCFP_STREAM_LAUNCH
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->done, st));
    for (size_t i = 0; i < n; i++) {
        const uint32_t slot = slots[i];
        s->fresh[slot] = 0;
        s->n[slot] += n_bytes[i];
        if (fin && fin[i]) s->open[slot] = 0;
    }
    return UCFP_OK;
}

size_t hash_state_bytes(int kind) {
    return kind == ucfp::T_MIN ? sizeof(ucfp::TextStreamState)
           : kind == ucfp::T_SIM ? sizeof(ucfp::SimStreamState<uint32_t>)
                                 : sizeof(ucfp::SimStreamState<uint64_t>);
}

size_t record_bytes(int kind) { return kind == ucfp::T_MIN ? (size_t)UCFP_MINHASH_BYTES : (size_t)UCFP_SIMHASH_BYTES; }

// a set of `kind` (shingle_k: 1 for the SimHash kinds); `table` only for T_IDF
int create_set(ucfp_ctx* ctx, int kind, const ucfp_idf_table* table, uint32_t shingle_k, uint32_t max_streams, uint32_t flags,
               uint64_t max_push_bytes, ucfp_text_streams** out);

}  // namespace

extern "C" {

size_t ucfp_text_streams_state_bytes(void) { return sizeof(ucfp::TextStreamState); }

size_t ucfp_text_streams_state_bytes_ex(uint32_t flags) {
    return sizeof(ucfp::TextStreamState) + ((flags & UCFP_TEXT_STREAMS_UTF8) ? sizeof(ucfp::CanonStreamState) : 0);
}

size_t ucfp_text_streams_state_bytes_sim(uint32_t flags, int weighted) {
    return hash_state_bytes(weighted ? ucfp::T_IDF : ucfp::T_SIM) + ((flags & UCFP_TEXT_STREAMS_UTF8) ? sizeof(ucfp::CanonStreamState) : 0);
}

size_t ucfp_text_streams_record_bytes(const ucfp_text_streams* s) { return s ? record_bytes(s->kind) : 0; }

int ucfp_text_streams_create(ucfp_ctx* ctx, uint32_t shingle_k, uint32_t max_streams, ucfp_text_streams** out) {
    return ucfp_text_streams_create_ex(ctx, shingle_k, max_streams, 0, 0, out);
}

int ucfp_text_streams_create_ex(ucfp_ctx* ctx, uint32_t shingle_k, uint32_t max_streams, uint32_t flags, uint64_t max_push_bytes,
                                ucfp_text_streams** out) {
    if (shingle_k == 0 || shingle_k > 64) return fail(UCFP_E_MODALITY, "shingle k must be in [1, 64] (got %u)", shingle_k);
    return create_set(ctx, ucfp::T_MIN, nullptr, shingle_k, max_streams, flags, max_push_bytes, out);
}

int ucfp_text_streams_create_sim(ucfp_ctx* ctx, uint32_t max_streams, uint32_t flags, uint64_t max_push_bytes,
                                 const ucfp_idf_table* table, ucfp_text_streams** out) {
    return create_set(ctx, table ? ucfp::T_IDF : ucfp::T_SIM, table, 1, max_streams, flags, max_push_bytes, out);
}

}  // extern "C"

namespace {

int create_set(ucfp_ctx* ctx, int kind, const ucfp_idf_table* table, uint32_t shingle_k, uint32_t max_streams, uint32_t flags,
               uint64_t max_push_bytes, ucfp_text_streams** out) {
    if (!out) return fail(UCFP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (flags & ~(uint32_t)UCFP_TEXT_STREAMS_UTF8) return fail(UCFP_E_INVALID, "unknown flags 0x%x", flags);
    const bool utf8 = (flags & UCFP_TEXT_STREAMS_UTF8) != 0;
    if (utf8 && (max_push_bytes == 0 || max_push_bytes > kMaxPushBytes))
        return fail(UCFP_E_INVALID, "max_push_bytes %llu outside [1, 2^28]", (unsigned long long)max_push_bytes);
    if (!ctx) {
        if (!ucfp::have_gfx950()) return fail(UCFP_E_INDEX, "no gfx950 device available; this library has no CPU path");
        return fail(UCFP_E_INVALID, "ctx is NULL");
    }
    if (max_streams == 0 || max_streams > (1u << 20)) return fail(UCFP_E_INVALID, "max_streams %u outside [1, 2^20]", max_streams);
    if (table) {
        int tdev = 0;
        (void)ucfp::idf_table_aux(table, nullptr, &tdev);
        if (tdev != ctx->device) return fail(UCFP_E_INVALID, "the IDF table lives on device %d, the context on %d", tdev, ctx->device);
    }
    HIP_TRY(hipSetDevice(ctx->device));
    ucfp_text_streams* s = new (std::nothrow) ucfp_text_streams();
    if (!s) return fail(UCFP_E_INDEX, "out of host memory");
    s->ctx = ctx;
    s->k = shingle_k;
    s->kind = kind;
    s->table = table;
    s->init(max_streams);
    s->fresh.assign(max_streams, 0);
    s->mode.assign(max_streams, 0);
    s->utf8 = utf8;
    s->max_push_bytes = utf8 ? max_push_bytes : 0;
    const size_t tab_bytes = (size_t)max_streams * (sizeof(ucfp::TextStreamEntry) + (utf8 ? sizeof(ucfp::CanonSlice) : 0));
    hipError_t e = hipMalloc(&s->states, (size_t)max_streams * hash_state_bytes(kind));
    if (utf8) {
        // every slice of a push at once: 4 x the chunk bytes, and per entry the slack and the rounding to a line
        const size_t scratch = (size_t)ucfp_text_canon_bound((size_t)max_push_bytes) +
                               (size_t)max_streams * (size_t)(ucfp::kSliceSlack + ucfp::kSliceAlign) + 64;   // the hash stage reads whole dwords
        if (e == hipSuccess) e = hipMalloc((void**)&s->ca.cstates, (size_t)max_streams * sizeof(ucfp::CanonStreamState));
        if (e == hipSuccess) e = hipMalloc((void**)&s->ca.scratch, scratch);
        if (e == hipSuccess && ucfp::text_canon_tables(ctx->device, &s->ca.stage1, &s->ca.stage2, &s->ca.pool) != UCFP_OK) e = hipErrorNotFound;
    }
    if (e == hipSuccess) e = hipMalloc((void**)&s->tab_d, tab_bytes);
    if (e == hipSuccess) e = s->setup(tab_bytes);
    if (e != hipSuccess) {
        ucfp_text_streams_destroy(s);
        return fail(UCFP_E_INDEX, "stream set allocation failed: %s", hipGetErrorString(e));
    }
    *out = s;
    return UCFP_OK;
}

}  // namespace

extern "C" {

void ucfp_text_streams_destroy(ucfp_text_streams* s) {
    if (!s) return;
    s->teardown();
    if (s->states) (void)hipFree(s->states);
    if (s->ca.cstates) (void)hipFree(s->ca.cstates);
    if (s->ca.scratch) (void)hipFree(s->ca.scratch);
    if (s->tab_d) (void)hipFree(s->tab_d);
    delete s;
}

int ucfp_text_streams_open(ucfp_text_streams* s, int mode, uint32_t* slot) {
    if (!s || !slot) return fail(UCFP_E_INVALID, "set / slot is NULL");
    if (mode == UCFP_TEXT_RAW_UTF8 && !s->utf8)
        return fail(UCFP_E_UNSUPPORTED, "RAW_UTF8 streams are not built: canonicalise on the host and open a PRETOKENIZED stream");
    if (mode != UCFP_TEXT_RAW_ASCII && mode != UCFP_TEXT_PRETOKENIZED && mode != UCFP_TEXT_RAW_UTF8) return fail(UCFP_E_INVALID, "unknown text mode %d", mode);
    std::lock_guard<std::mutex> lk(s->mu);
    const int rc = s->acquire(slot);
    if (rc) return rc;
    s->fresh[*slot] = 1;
    s->mode[*slot] = (uint8_t)mode;
    return UCFP_OK;
}

int ucfp_text_streams_close(ucfp_text_streams* s, uint32_t slot) {
    if (!s) return fail(UCFP_E_INVALID, "set is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    return s->release(slot);   // `fresh` stays as it is: the next open sets it
}

int ucfp_text_streams_push_dev(ucfp_text_streams* s, const uint32_t* slots, const uint64_t* n_bytes, const uint8_t* final,
                               size_t n, const uint8_t* d_bytes, uint8_t* d_out, int32_t* d_status, void* stream) {
    if (!s) return fail(UCFP_E_INVALID, "set is NULL");
    if (n && !d_status) return fail(UCFP_E_INVALID, "d_status is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    int rc = check_push(s, slots, n_bytes, n);
    if (rc) return rc;
    uint64_t total = 0;
    bool any_final = false;
    for (size_t i = 0; i < n; i++) {
        total += n_bytes[i];
        any_final |= final && final[i];
    }
    if (total && !d_bytes) return fail(UCFP_E_INVALID, "d_bytes is NULL");
    if (any_final && !d_out) return fail(UCFP_E_INVALID, "d_out is NULL and an entry is final");
    return push_impl(s, slots, n_bytes, final, n, d_bytes, d_out, d_status, (hipStream_t)stream);
}

int ucfp_text_streams_push(ucfp_text_streams* s, uint32_t slot, const uint8_t* bytes, size_t n, int final, uint8_t* out,
                           int32_t* status) {
    if (!s) return fail(UCFP_E_INVALID, "set is NULL");
    if ((n && !bytes) || (final && !out)) return fail(UCFP_E_INVALID, "NULL buffer");
    std::lock_guard<std::mutex> lk(s->mu);
    const uint64_t m = n;
    const uint8_t fin = final ? 1 : 0;
    int rc = check_push(s, &slot, &m, 1);
    if (rc) return rc;
    ucfp_ctx* ctx = s->ctx;
    std::lock_guard<std::mutex> lk2(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    rc = ucfp::grow(&ctx->stage_in, &ctx->stage_in_cap, n ? n : 1);
    const size_t rec = record_bytes(s->kind);
    if (!rc) rc = ucfp::grow(&ctx->stage_out, &ctx->stage_out_cap, 256 + rec);
    if (rc) return rc;
    hipStream_t st = ctx->host_stream;
    int32_t* d_st = reinterpret_cast<int32_t*>(ctx->stage_out);
    uint8_t* d_out = ctx->stage_out + 256;
    if (n) HIP_TRY(hipMemcpyAsync(ctx->stage_in, bytes, n, hipMemcpyHostToDevice, st));
    rc = push_impl(s, &slot, &m, &fin, 1, ctx->stage_in, d_out, d_st, st);
    if (rc) return rc;
    int32_t stv = 0;
    HIP_TRY(hipMemcpyAsync(&stv, d_st, 4, hipMemcpyDeviceToHost, st));
    if (final) HIP_TRY(hipMemcpyAsync(out, d_out, rec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (status) *status = stv;
    return UCFP_OK;
}

}  // extern "C"
