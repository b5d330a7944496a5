// text_streams.hip -- streaming MinHash-128: device-resident text sessions, batched pushes, for gfx950.
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
//   steps  tokenise / write canonical / room check / flush: the offline kernel's, unchanged (own copy of its two
//          lambdas, so that text_hash_kernel's text and registers stay as they are)
//   end    non-final: flush(false), then the state goes back; final: close an open token, flush(true), emit the record
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "ctx.h"
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

enum : uint32_t { kAnyShingle = 1, kNonAscii = 2, kTooLong = 4, kPendValid = 0x100 };
enum : uint32_t { kEntFinal = 1, kEntFresh = 2, kEntModeShift = 2 };

// one entry of a push, planned on the host
struct TextStreamEntry {
    uint64_t off, len;   // the chunk: bytes[off, off + len)
    uint32_t slot, flags;
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

}  // namespace

__global__ __launch_bounds__(64 * kWavesPerBlock) void text_stream_kernel(
    TextStreamState* __restrict__ states, const TextStreamEntry* __restrict__ ents, size_t n,
    const uint8_t* __restrict__ bytes, uint32_t k, uint8_t* __restrict__ out, int32_t* __restrict__ status) {
    __shared__ WaveLds lds[kWavesPerBlock];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t ei = (size_t)blockIdx.x * kWavesPerBlock + wave;
    if (ei >= n) return;  // whole wave
    WaveLds& L = lds[wave];
    const TextStreamEntry ent = ents[ei];
    const uint32_t eflags = uni(ent.flags);
    const bool fin = eflags & kEntFinal, fresh = eflags & kEntFresh;
    TextStreamState& S = states[uni(ent.slot)];

    uint64_t m0 = ~0ull, m1 = ~0ull;
    uint32_t total_tok = 0;
    bool any_shingle = false, nonascii = false, too_long = false;
    uint32_t ntok = 0, cbase = 0;
    bool carry = false;
    uint32_t prev_last = 0;
    uint32_t pend = 0;
    uint32_t mode = eflags >> kEntModeShift;
    uint64_t total_bytes = 0;
    bool dead = false;   // a sticky status was stored by an earlier push: nothing is processed any more

    // ---- load ----
    if (!fresh) {
        m0 = S.m0[lane];
        m1 = S.m1[lane];
        total_bytes = S.total_bytes;
        ntok = uni(S.ntok);
        cbase = uni(S.cbase);
        carry = uni(S.carry) != 0;
        prev_last = uni(S.prev_last);
        total_tok = uni(S.total_tok);
        const uint32_t f = uni(S.flags);
        any_shingle = f & kAnyShingle;
        nonascii = f & kNonAscii;
        too_long = f & kTooLong;
        dead = nonascii || too_long;
        pend = uni(S.pending);
        mode = uni(S.mode);
        if (ntok > 64u) ntok = 64u;                                   // a stored state never has more: keeps every index in range
        if (cbase + ntok > (uint32_t)kCanonCap) cbase = 0, ntok = 0;
        const uint32_t used = cbase + (ntok ? ntok - 1 : 0);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(S.canon);
        uint32_t* dst = reinterpret_cast<uint32_t*>(L.canon);
        for (uint32_t i = lane; 4 * i < used; i += 64) dst[i] = src[i];
        if ((uint32_t)lane < ntok) {
            L.cstart[lane] = S.cstart[lane];
            L.cend[lane] = S.cend[lane];
        }
    }
    const bool pretok = mode == UCFP_TEXT_PRETOKENIZED;

    // consume the batch: hash complete shingles, fold them in, carry the tail to the front (text_hash_kernel's flush)
    auto flush = [&](bool final) {
        wave_sync();
        const uint32_t ncomplete = ntok - (carry && !final ? 1u : 0u);
        uint32_t nitems, keep_from;
        if (ncomplete >= k) {
            nitems = ncomplete - k + 1;
            keep_from = ncomplete - (k - 1);
        } else if (final && !any_shingle && ncomplete > 0) {
            nitems = 1;  // fewer than k tokens in the whole stream: one shingle of all of them
            keep_from = ncomplete;
        } else {
            nitems = 0;
            keep_from = 0;
        }
        for (uint32_t s0 = 0; s0 < nitems; s0 += 64) {
            const uint32_t s = s0 + lane;
            if (s < nitems) {
                const uint32_t e = ncomplete >= k ? s + k - 1 : ncomplete - 1;
                const uint32_t a = L.cstart[s], b = L.cend[e];
                const uint64_t h = xxh3_lds(L.canon + a, (size_t)(b - a));
                L.h1[s] = h;
                L.h2[s] = mix_h2(h);
            }
        }
        wave_sync();
#pragma unroll 4
        for (uint32_t s = 0; s < nitems; s++) {
            const uint64_t h = L.h1[s], g = L.h2[s];
            const uint64_t v0 = h + (uint64_t)lane * g;
            const uint64_t v1 = v0 + (g << 6);
            m0 = v0 < m0 ? v0 : m0;
            m1 = v1 < m1 ? v1 : m1;
        }
        if (nitems) any_shingle = true;
        total_tok += keep_from;
        if (final) return;
        // carry tokens [keep_from, ntok) to the front
        if (keep_from == 0) return;  // nothing consumed (fewer than k complete tokens): the caller re-checks room
        const uint32_t src0 = keep_from < ntok ? L.cstart[keep_from] : cbase + ntok - 1 + (carry ? 1u : 0u);
        const uint32_t used = cbase + (ntok ? ntok - 1 : 0);   // bytes of canon in use
        const uint32_t nkeep = ntok - keep_from;
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
        ntok = nkeep;
        cbase = kept_bytes - (nkeep ? nkeep - 1 : 0);
        wave_sync();
    };

    // ---- the bytes of this push: V = pending || chunk; V[0, proc) is processed, V[proc] is the byte after it ----
    const uint32_t npend = dead ? 0u : (pend >> 8) & 1u;
    const uint32_t pbyte = pend & 0xffu;
    const size_t clen = (size_t)ent.len;
    const uint8_t* __restrict__ chunk = bytes + ent.off;      // V[i] = chunk[i - npend] for i >= npend
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
            // make room: a step opens at most 32 tokens and writes at most 64 + 32 bytes
            if (ntok + kStepTok > (uint32_t)kTokCap || cbase + ntok + kStepRoom > (uint32_t)kCanonCap) {
                flush(false);
                if (ntok + kStepTok > (uint32_t)kTokCap || cbase + ntok + kStepRoom > (uint32_t)kCanonCap) too_long = true;
                if (too_long) break;
            }
            const uint32_t c = L.stage[64 * sub + lane];
            const uint32_t q = L.stage[64 * sub + lane + 1];
            uint32_t p = __shfl_up(c, 1, 64);
            if (lane == 0) p = prev_last;
            const bool w = pos < proc && inword(p, c, q, pretok);
            const uint64_t inw = __ballot(w);
            const uint64_t prev = (inw << 1) | (carry ? 1ull : 0ull);
            const uint64_t starts = inw & ~prev;
            const uint64_t endmark = ~inw & prev;   // first non-word byte after a token
            const uint32_t nin_before = popc_below(inw, lane);
            const uint32_t nst_before = popc_below(starts, lane);
            const bool is_start = (starts >> lane) & 1ull;
            if (w) {
                const uint32_t tok = ntok + nst_before + (is_start ? 1u : 0u) - 1u;
                const uint32_t cpos = cbase + nin_before + tok;
                uint32_t ch = c;
                if (!pretok && ch - 'A' <= 25u) ch += 32;
                L.canon[cpos] = (uint8_t)ch;
                if (is_start) {
                    L.cstart[tok] = (uint16_t)cpos;
                    if (cpos > 0) L.canon[cpos - 1] = ' ';
                }
            }
            if ((endmark >> lane) & 1ull) {
                const uint32_t tok = ntok + nst_before - 1u;   // starts strictly before this byte
                L.cend[tok] = (uint16_t)(cbase + nin_before + tok);
            }
            ntok += (uint32_t)__popcll(starts);
            cbase += (uint32_t)__popcll(inw);
            carry = (inw >> 63) & 1ull;
            // the last PROCESSED byte: a step that ends the push may be partial
            const size_t left = proc - (base + 64 * sub);
            if (left < 64) carry = (inw >> (left - 1)) & 1ull;
            prev_last = __shfl(c, left < 64 ? (int)left - 1 : 63, 64);
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
    const bool na = __ballot(nonascii) != 0;
    total_bytes += clen;

    if (!fin) {
        // ---- store: what survives flush(false) is a prefix of one k-token window ----
        if (!too_long && !dead) flush(false);
        if (too_long) ntok = 0, cbase = 0, carry = false;
        wave_sync();
        S.m0[lane] = m0;
        S.m1[lane] = m1;
        const uint32_t used = cbase + (ntok ? ntok - 1 : 0);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(L.canon);
        uint32_t* dst = reinterpret_cast<uint32_t*>(S.canon);
        for (uint32_t i = lane; 4 * i < used; i += 64) dst[i] = src[i];
        if ((uint32_t)lane < ntok) {   // ntok <= k <= 64 after the flush
            S.cstart[lane] = L.cstart[lane];
            S.cend[lane] = L.cend[lane];
        }
        if (lane == 0) {
            S.total_bytes = total_bytes;
            S.ntok = ntok;
            S.cbase = cbase;
            S.carry = carry ? 1u : 0u;
            S.prev_last = prev_last;
            S.total_tok = total_tok;
            S.flags = (any_shingle ? kAnyShingle : 0u) | (na ? kNonAscii : 0u) | (too_long ? kTooLong : 0u);
            S.pending = pend;
            S.mode = mode;
            status[ei] = na ? 1 : (too_long ? -2 : 0);
        }
        return;
    }

    // ---- final: close a token that runs to the end of the stream, the final flush, emit as text_hash_kernel does ----
    if (carry && ntok > 0 && lane == 0) L.cend[ntok - 1] = (uint16_t)(cbase + ntok - 1);
    if (!too_long && !dead) flush(true);
    int32_t stv = 0;
    if (na) stv = 1;                          // non-ASCII in raw mode: host must pre-tokenise
    else if (too_long) stv = -2;              // UCFP_E_UNSUPPORTED: a token / k-token run exceeds the LDS batch
    else if (total_tok == 0 || !any_shingle) stv = -1;   // UCFP_E_MODALITY: no tokens
    uint8_t* rec = out + ei * 1032;
    const uint64_t a = stv == 0 ? m0 : 0ull, b = stv == 0 ? m1 : 0ull;
    // 1032-byte records are only 8-byte aligned when the base is: write dwords
    uint32_t* o0 = reinterpret_cast<uint32_t*>(rec + 8 + 8 * lane);
    uint32_t* o1 = reinterpret_cast<uint32_t*>(rec + 8 + 8 * (lane + 64));
    o0[0] = (uint32_t)a;
    o0[1] = (uint32_t)(a >> 32);
    o1[0] = (uint32_t)b;
    o1[1] = (uint32_t)(b >> 32);
    if (lane == 0) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(rec);
        o32[0] = stv == 0 ? 1u : 0u;  // schema: u16 = 1, pad
        o32[1] = 0;
        status[ei] = stv;
    }
}

}  // namespace ucfp

// ================================================ host ================================================

struct ucfp_text_streams {
    ucfp_ctx* ctx = nullptr;
    uint32_t k = 0;
    uint32_t max_streams = 0;
    std::mutex mu;                        // serialises the set's calls
    std::vector<uint64_t> n;              // bytes seen per slot
    std::vector<uint8_t> open;
    std::vector<uint8_t> fresh;           // opened, not pushed yet: the device state is not read
    std::vector<uint8_t> mode;
    std::vector<uint8_t> seen;            // duplicate-slot check of one push
    ucfp::TextStreamState* states = nullptr;
    ucfp::TextStreamEntry* tab_d = nullptr;           // the push table on the device; the next push waits for `done`
    ucfp::TextStreamEntry* tab_h[2] = {nullptr, nullptr};   // pinned push tables, used in turn
    hipEvent_t tab_copied[2] = {nullptr, nullptr};
    int tab_next = 0;
    hipEvent_t done = nullptr;            // behind the last push: the next one waits for it
};

namespace {

constexpr uint64_t kMaxStreamBytes = (uint64_t)1 << 63;

// validates the push; nothing changes
int check_push(ucfp_text_streams* s, const uint32_t* slots, const uint64_t* n_bytes, size_t n) {
    if (n && (!slots || !n_bytes)) return fail(UCFP_E_INVALID, "slots / n_bytes is NULL");
    if (n > s->max_streams) return fail(UCFP_E_INVALID, "%zu entries in one push, the set has %u slots", n, s->max_streams);
    int rc = UCFP_OK;
    size_t marked = 0;
    for (size_t i = 0; i < n && rc == UCFP_OK; i++) {
        const uint32_t slot = slots[i];
        if (slot >= s->max_streams) rc = fail(UCFP_E_INVALID, "slot %u out of range [0, %u)", slot, s->max_streams);
        else if (!s->open[slot]) rc = fail(UCFP_E_INVALID, "slot %u is not open", slot);
        else if (s->seen[slot]) rc = fail(UCFP_E_INVALID, "slot %u appears twice in one push", slot);
        else if (n_bytes[i] > kMaxStreamBytes - s->n[slot]) rc = fail(UCFP_E_INVALID, "slot %u would pass 2^63 bytes", slot);
        if (rc) break;
        s->seen[slot] = 1;
        marked = i + 1;
    }
    for (size_t i = 0; i < marked; i++) s->seen[slots[i]] = 0;
    return rc;
}

// the set's lock is held; the push is valid
int push_impl(ucfp_text_streams* s, const uint32_t* slots, const uint64_t* n_bytes, const uint8_t* fin, size_t n,
              const uint8_t* d_bytes, uint8_t* d_out, int32_t* d_status, hipStream_t st) {
    if (n == 0) return UCFP_OK;
    HIP_TRY(hipSetDevice(s->ctx->device));
    // the pinned table this push fills was last copied two pushes ago
    const int t = s->tab_next;
    s->tab_next ^= 1;
    HIP_TRY(hipEventSynchronize(s->tab_copied[t]));
    ucfp::TextStreamEntry* tab = s->tab_h[t];
    uint64_t off = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t slot = slots[i];
        tab[i].off = off;
        tab[i].len = n_bytes[i];
        tab[i].slot = slot;
        tab[i].flags = ((fin && fin[i]) ? ucfp::kEntFinal : 0u) | (s->fresh[slot] ? ucfp::kEntFresh : 0u) |
                       ((uint32_t)s->mode[slot] << ucfp::kEntModeShift);
        off += n_bytes[i];
    }
    HIP_TRY(hipStreamWaitEvent(st, s->done, 0));
    HIP_TRY(hipMemcpyAsync(s->tab_d, tab, n * sizeof(ucfp::TextStreamEntry), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->tab_copied[t], st));
    const unsigned grid = (unsigned)((n + ucfp::kWavesPerBlock - 1) / ucfp::kWavesPerBlock);
    hipLaunchKernelGGL(ucfp::text_stream_kernel, dim3(grid), dim3(64 * ucfp::kWavesPerBlock), 0, st, s->states, s->tab_d, n,
                       d_bytes, s->k, d_out, d_status);
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

// a set needs a gfx950 device; a NULL context on a host without one is "no device", not a caller bug
bool have_gfx950() {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return false;
    for (int d = 0; d < count; d++) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) return true;
    }
    return false;
}

}  // namespace

extern "C" {

size_t ucfp_text_streams_state_bytes(void) { return sizeof(ucfp::TextStreamState); }

int ucfp_text_streams_create(ucfp_ctx* ctx, uint32_t shingle_k, uint32_t max_streams, ucfp_text_streams** out) {
    if (shingle_k == 0 || shingle_k > 64) return fail(UCFP_E_MODALITY, "shingle k must be in [1, 64] (got %u)", shingle_k);
    if (!out) return fail(UCFP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!ctx) {
        if (!have_gfx950()) return fail(UCFP_E_INDEX, "no gfx950 device available; this library has no CPU path");
        return fail(UCFP_E_INVALID, "ctx is NULL");
    }
    if (max_streams == 0 || max_streams > (1u << 20)) return fail(UCFP_E_INVALID, "max_streams %u outside [1, 2^20]", max_streams);
    HIP_TRY(hipSetDevice(ctx->device));
    ucfp_text_streams* s = new (std::nothrow) ucfp_text_streams();
    if (!s) return fail(UCFP_E_INDEX, "out of host memory");
    s->ctx = ctx;
    s->k = shingle_k;
    s->max_streams = max_streams;
    s->n.assign(max_streams, 0);
    s->open.assign(max_streams, 0);
    s->fresh.assign(max_streams, 0);
    s->mode.assign(max_streams, 0);
    s->seen.assign(max_streams, 0);
    const size_t tab_bytes = (size_t)max_streams * sizeof(ucfp::TextStreamEntry);
    hipError_t e = hipMalloc((void**)&s->states, (size_t)max_streams * sizeof(ucfp::TextStreamState));
    if (e == hipSuccess) e = hipMalloc((void**)&s->tab_d, tab_bytes);
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipHostMalloc((void**)&s->tab_h[i], tab_bytes, 0);
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreateWithFlags(&s->tab_copied[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->done, hipEventDisableTiming);
    if (e != hipSuccess) {
        ucfp_text_streams_destroy(s);
        return fail(UCFP_E_INDEX, "stream set allocation failed: %s", hipGetErrorString(e));
    }
    *out = s;
    return UCFP_OK;
}

void ucfp_text_streams_destroy(ucfp_text_streams* s) {
    if (!s) return;
    if (s->done) (void)hipEventSynchronize(s->done);
    if (s->states) (void)hipFree(s->states);
    if (s->tab_d) (void)hipFree(s->tab_d);
    for (int i = 0; i < 2; i++) {
        if (s->tab_h[i]) (void)hipHostFree(s->tab_h[i]);
        if (s->tab_copied[i]) (void)hipEventDestroy(s->tab_copied[i]);
    }
    if (s->done) (void)hipEventDestroy(s->done);
    delete s;
}

int ucfp_text_streams_open(ucfp_text_streams* s, int mode, uint32_t* slot) {
    if (!s || !slot) return fail(UCFP_E_INVALID, "set / slot is NULL");
    if (mode == UCFP_TEXT_RAW_UTF8)
        return fail(UCFP_E_UNSUPPORTED, "RAW_UTF8 streams are not built: canonicalise on the host and open a PRETOKENIZED stream");
    if (mode != UCFP_TEXT_RAW_ASCII && mode != UCFP_TEXT_PRETOKENIZED) return fail(UCFP_E_INVALID, "unknown text mode %d", mode);
    std::lock_guard<std::mutex> lk(s->mu);
    for (uint32_t i = 0; i < s->max_streams; i++) {
        if (!s->open[i]) {
            s->open[i] = 1;
            s->fresh[i] = 1;
            s->mode[i] = (uint8_t)mode;
            s->n[i] = 0;
            *slot = i;
            return UCFP_OK;
        }
    }
    return fail(UCFP_E_INVALID, "all %u slots are open", s->max_streams);
}

int ucfp_text_streams_close(ucfp_text_streams* s, uint32_t slot) {
    if (!s) return fail(UCFP_E_INVALID, "set is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    if (slot >= s->max_streams || !s->open[slot]) return fail(UCFP_E_INVALID, "slot %u is not open", slot);
    s->open[slot] = 0;
    s->n[slot] = 0;
    return UCFP_OK;
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
    if (!rc) rc = ucfp::grow(&ctx->stage_out, &ctx->stage_out_cap, 256 + UCFP_MINHASH_BYTES);
    if (rc) return rc;
    hipStream_t st = ctx->host_stream;
    int32_t* d_st = reinterpret_cast<int32_t*>(ctx->stage_out);
    uint8_t* d_out = ctx->stage_out + 256;
    if (n) HIP_TRY(hipMemcpyAsync(ctx->stage_in, bytes, n, hipMemcpyHostToDevice, st));
    rc = push_impl(s, &slot, &m, &fin, 1, ctx->stage_in, d_out, d_st, st);
    if (rc) return rc;
    int32_t stv = 0;
    HIP_TRY(hipMemcpyAsync(&stv, d_st, 4, hipMemcpyDeviceToHost, st));
    if (final) HIP_TRY(hipMemcpyAsync(out, d_out, UCFP_MINHASH_BYTES, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (status) *status = stv;
    return UCFP_OK;
}

}  // extern "C"
