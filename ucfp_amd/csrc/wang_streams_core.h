// wang_streams_core.h -- the host side of a stream set over Wang's front end, shared by the two planners
// built on it: wang_streams.hip (pairs, A9) and panako_streams.hip (triplets, A19).  The host tracks how many samples
// each stream has seen, which fixes every frame range of a push: the host plans, the device keeps the data (carried
// samples, the open second's candidates, the retained peaks).  What an anchor emits is the including file's business.
// Either set may keep a live window per stream (A19, A20): the rings and the windows call are here too.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/ucfp_hip.h"
#include "common.h"
#include "ctx.h"
#include "stream_resample.h"
#include "stream_set.h"

namespace ucfp {
namespace wstreams {

constexpr uint64_t kMaxChunk = (uint64_t)1 << 29;     // samples of one stream in one push (18.6 h): t << 9 | k stays packable
constexpr uint64_t kMaxPushSamples = (uint64_t)1 << 31;   // carried + new samples of one push (32-bit sample offsets)
constexpr uint64_t kMaxFrames = ((uint64_t)1 << 32) - 1024;   // frames of a stream (u32 t_anchor, ~795 days)
constexpr uint32_t kMaxWindowFrames = 8192;           // W of a live window (131 s)
constexpr size_t kRingHeader = 8;                     // head and count
static_assert(kMaxWindowFrames == UCFP_WANG_STREAM_MAX_WINDOW_FRAMES &&
              kMaxWindowFrames == UCFP_PANAKO_STREAM_MAX_WINDOW_FRAMES, "");

// ucfp_wang_config and ucfp_panako_config carry the same five fields with the same ranges
struct Cfg {
    uint32_t fan_out, target_zone_t, target_zone_f, peaks_per_sec;
    float min_anchor_mag_db;
};
template <class C>
inline Cfg cfg_of(const C& c) {
    return Cfg{c.fan_out, c.target_zone_t, c.target_zone_f, c.peaks_per_sec, c.min_anchor_mag_db};
}

inline bool cfg_ok(const Cfg& c) {
    return c.fan_out >= 1 && c.fan_out <= 64 && c.target_zone_t >= 1 && c.target_zone_t <= 512 && c.target_zone_f >= 1 &&
           c.target_zone_f <= 1024 && c.peaks_per_sec >= 1 && c.peaks_per_sec <= 256;
}

// A9, all in frames / samples since the stream was opened
inline uint64_t frames_of(uint64_t n) { return n < 1024 ? 0 : (n - 1024) / 128 + 1; }
inline uint64_t judged_of(uint64_t n) { const uint64_t f = frames_of(n); return f > 7 ? f - 7 : 0; }   // J(n)
inline uint64_t sec_of(uint64_t t) { return (t * 128) / 8000; }
inline uint64_t f0_of(uint64_t s) { return (125 * s + 1) / 2; }                                        // ceil(125 s / 2)
inline uint64_t closed_of(uint64_t j) { return f0_of(sec_of(j)); }     // C = f0(S), S = the second holding frame J
inline uint64_t frontier_of(uint64_t j, uint32_t zone_t) { const uint64_t c = closed_of(j); return c > zone_t ? c - zone_t : 0; }

// A21 (stream_resample.h): a set takes its feed at `sr`, 1 .. 384 kHz; every quantity of A9 above is then taken at
// S(n) = samples_of(n, sr, final), the 8 kHz samples that are final after n input samples.

// retained peaks: the selected peaks of [F, C), zone_t frames wide
inline uint32_t ret_cap_of(const Cfg& c) { return c.peaks_per_sec * ((c.target_zone_t * 2 + 124) / 125 + 2); }

// one entry of a push, planned on the host
struct Plan {
    uint32_t slot;
    uint64_t m, n0, n1;                   // 8 kHz samples: S before and after the push, m = n1 - n0
    RsSpan rs;                            // the same in input samples, and the carried inputs (A21)
    bool fin;
    uint64_t vbase, o, j0, j1, s0, n_closed, f_lo, f_hi, cap, bound;
};

// the slot table counts samples; the pinned tables hold a push or the items of a windows call
struct Set : streams::Slots, streams::Tables {
    ucfp_ctx* ctx = nullptr;
    Cfg cfg{};
    float floor_p = 0.0f;
    std::vector<Plan> plan;
    WangStreamsDev dev{};
    WangStreamsRsDev rs{nullptr, 0, kSr8k};   // A21: the input rate and the carried inputs
    uint8_t* dev_mem = nullptr;
    uint32_t window = 0;                  // W in frames (0: the set keeps no windows)
    uint8_t* ring_mem = nullptr;          // the rings of the including file's record type
};

// records a window of W frames can hold (A19, A20): the emitted anchors of [w0, F) lie in at most ceil(2 W / 125) + 1
// seconds, a second holds at most peaks_per_sec anchors and an anchor emits at most fan_out records
inline size_t window_cap_of(const Cfg& c, uint32_t w) {
    return w ? ((size_t)(2 * w + 124) / 125 + 1) * c.peaks_per_sec * c.fan_out : 0;
}

inline size_t state_bytes_per_stream(uint32_t ret_cap) {
    return (size_t)kWangCarry * 4 + 4 + (size_t)kWangCandCap * 12 + 4 + (size_t)ret_cap * 12;
}

inline size_t tab_bytes_max(uint32_t max_streams, bool resample) {
    return (size_t)max_streams * (sizeof(WangStreamClip) + sizeof(WangStreamEntry) +
                                  (resample ? sizeof(WangStreamRsEntry) : 0)) +
           3 * ((size_t)max_streams + 1) * 4 + 4 + 256;
}

// host state, device state and the pinned tables of a set; on failure the caller releases what exists
inline hipError_t set_init(Set* s, ucfp_ctx* ctx, const Cfg& c, uint32_t max_streams, uint32_t sr) {
    s->ctx = ctx;
    s->rs.sr = sr;
    s->rs.carry_cap = carry_cap_of(sr);
    s->cfg = c;
    s->floor_p = (float)(65536.0 * pow(10.0, (double)c.min_anchor_mag_db / 10.0));
    s->init(max_streams);
    const uint32_t rc = ret_cap_of(c);
    const size_t ms = max_streams;
    const size_t bytes = ms * (state_bytes_per_stream(rc) + (size_t)s->rs.carry_cap * 4) + 17 * 256;
    hipError_t e = hipMalloc((void**)&s->dev_mem, bytes);
    if (e == hipSuccess) {
        size_t off = 0;
        auto take = [&](size_t b) { uint8_t* p = s->dev_mem + off; off = (off + b + 255) & ~(size_t)255; return p; };
        s->dev.smp = reinterpret_cast<float*>(take(ms * kWangCarry * 4));
        s->dev.cand_n = reinterpret_cast<uint32_t*>(take(ms * 4));
        s->dev.cand_t = reinterpret_cast<uint32_t*>(take(ms * kWangCandCap * 4));
        s->dev.cand_k = reinterpret_cast<uint32_t*>(take(ms * kWangCandCap * 4));
        s->dev.cand_p = reinterpret_cast<float*>(take(ms * kWangCandCap * 4));
        s->dev.ret_n = reinterpret_cast<uint32_t*>(take(ms * 4));
        s->dev.ret_t = reinterpret_cast<uint32_t*>(take(ms * rc * 4));
        s->dev.ret_k = reinterpret_cast<uint32_t*>(take(ms * rc * 4));
        s->dev.ret_p = reinterpret_cast<float*>(take(ms * rc * 4));
        s->dev.ret_cap = rc;
        if (s->rs.carry_cap) s->rs.carry = reinterpret_cast<float*>(take(ms * s->rs.carry_cap * 4));
    }
    return e == hipSuccess ? s->setup(tab_bytes_max(max_streams, sr != kSr8k)) : e;
}

// one ring of window_cap records per slot behind set_init (window_frames != 0)
template <class Rec>
inline hipError_t rings_init(Set* s, uint32_t window_frames, StreamRingsDev<Rec>* rg) {
    const size_t ms = s->max_streams, cap = window_cap_of(s->cfg, window_frames);
    const size_t rec_bytes = (ms * cap * sizeof(Rec) + 255) & ~(size_t)255, idx_bytes = (ms * 4 + 255) & ~(size_t)255;
    const hipError_t e = hipMalloc((void**)&s->ring_mem, rec_bytes + 2 * idx_bytes);
    if (e != hipSuccess) return e;
    rg->rec = reinterpret_cast<Rec*>(s->ring_mem);
    rg->head = reinterpret_cast<uint32_t*>(s->ring_mem + rec_bytes);
    rg->count = reinterpret_cast<uint32_t*>(s->ring_mem + rec_bytes + idx_bytes);
    rg->cap = (uint32_t)cap;
    rg->window = window_frames;
    return hipSuccess;
}

inline void set_release(Set* s) {
    s->teardown();
    if (s->dev_mem) (void)hipFree(s->dev_mem);
    if (s->ring_mem) (void)hipFree(s->ring_mem);
}

inline int set_open(Set* s, uint32_t* slot) {
    std::lock_guard<std::mutex> lk(s->mu);
    return s->acquire(slot);
}

inline int set_close(Set* s, uint32_t slot) {
    std::lock_guard<std::mutex> lk(s->mu);
    return s->release(slot);
}

// validates the push and plans every entry; nothing changes.  *bound: hashes / records the push can emit (either back
// end emits at most fan_out per anchor)
inline int plan_push(Set* s, const uint32_t* slots, const uint64_t* n_samples, const uint8_t* fin, size_t n, size_t* bound) {
    if (n && (!slots || !n_samples)) return capi_fail(UCFP_E_INVALID, "slots / n_samples is NULL");
    int rc = s->fits(n, "entries", "push");
    if (rc) return rc;
    const Cfg& c = s->cfg;
    const uint32_t sr = s->rs.sr;
    s->plan.resize(n);
    size_t total = 0;
    uint64_t total_v = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t slot = slots[i];
        rc = s->mark(slot, "push");
        if (rc) break;
        if (n_samples[i] > kMaxChunk) {
            rc = capi_fail(UCFP_E_INVALID, "a chunk of %llu samples exceeds 2^29: split it", (unsigned long long)n_samples[i]);
            break;
        }
        // the slot table counts input samples; A9 runs on the final 8 kHz samples (A21)
        Plan& p = s->plan[i];
        p.slot = slot;
        p.fin = fin && fin[i];
        p.rs = rs_span(s->n[slot], n_samples[i], sr, p.fin);
        p.n0 = p.rs.s0;
        p.n1 = p.rs.s1;
        p.m = p.n1 - p.n0;
        if (p.m > kMaxChunk)
            rc = capi_fail(UCFP_E_INVALID, "a chunk of %llu samples at 8 kHz exceeds 2^29: split it", (unsigned long long)p.m);
        else if (frames_of(p.n1) > kMaxFrames)
            rc = capi_fail(UCFP_E_INVALID, "slot %u would pass 2^32 frames", slot);
        if (rc) break;
        p.j0 = judged_of(p.n0);
        p.s0 = sec_of(p.j0);
        p.f_lo = frontier_of(p.j0, c.target_zone_t);
        p.vbase = p.j0 > 7 ? p.j0 - 7 : 0;
        p.o = p.vbase < p.f_lo ? p.vbase : p.f_lo;
        const uint64_t fr1 = frames_of(p.n1);
        uint64_t emit_hi;                                  // anchors emitted: [f_lo, emit_hi)
        if (p.fin) {
            p.j1 = fr1;
            const uint64_t last = fr1 ? sec_of(fr1 - 1) + 1 : 0;     // seconds below `last` hold frames
            p.n_closed = last > p.s0 ? last - p.s0 : 0;
            p.f_hi = fr1;
            emit_hi = fr1;
        } else {
            p.j1 = judged_of(p.n1);
            p.n_closed = sec_of(p.j1) - p.s0;
            p.f_hi = frontier_of(p.j1, c.target_zone_t);
            emit_hi = p.f_hi;
        }
        p.cap = ret_cap_of(c) + p.n_closed * c.peaks_per_sec;
        p.bound = emit_hi > p.f_lo ? (sec_of(emit_hi - 1) - sec_of(p.f_lo) + 1) * c.peaks_per_sec * c.fan_out : 0;
        total += p.bound;
        total_v += p.n0 - 128 * p.vbase + p.m;
    }
    s->unmark(slots, n);
    if (rc) return rc;
    if (total_v >= kMaxPushSamples)
        return capi_fail(UCFP_E_INVALID, "push of %llu samples exceeds 2^31: split it", (unsigned long long)total_v);
    *bound = total;
    return UCFP_OK;
}

// The set's and the context's locks are held; the plan is current.  Lays the push out in the context's workspace, fills
// the host-built table and enqueues its copy behind the previous audio call and the set's previous push.  The caller
// launches its kernels on `st` next and then calls push_end.
inline int push_begin(Set* s, size_t n, hipStream_t st, WangPushWs* out_w) {
    ucfp_ctx* ctx = s->ctx;
    const Cfg& c = s->cfg;
    size_t n_closed = 0, n_open = 0, total_v = 0, total_cap = 0, judged = 0;
    for (size_t i = 0; i < n; i++) {
        const Plan& p = s->plan[i];
        n_closed += p.n_closed;
        n_open += p.fin ? 0 : 1;
        total_v += p.n0 - 128 * p.vbase + p.m;
        total_cap += p.cap;
        judged += p.j1 - p.j0;
    }
    const bool resample = s->rs.sr != kSr8k;
    WangPushWs w = wang_push_layout(n, n_closed + n_open, n_closed, total_v, total_cap, judged, c.peaks_per_sec, resample);
    if (total_cap >= 0x7fffffffu || (n_closed + n_open) * kWangCandCap >= ((size_t)1 << 30))
        return capi_fail(UCFP_E_INVALID, "push too large for one call: split it");
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = grow(&ctx->audio_ws, &ctx->audio_ws_cap, w.total);
    if (rc) return rc;
    // the pinned table this push fills was last copied two pushes ago
    int k = 0;
    rc = s->next(&k);
    if (rc) return rc;
    uint8_t* tab = s->tab_h[k];
    auto* clips = reinterpret_cast<WangStreamClip*>(tab + w.clips);
    auto* ents = reinterpret_cast<WangStreamEntry*>(tab + w.ents);
    auto* v_base = reinterpret_cast<uint32_t*>(tab + w.v_base);
    auto* seg_base = reinterpret_cast<uint32_t*>(tab + w.seg_base);
    auto* pk_base = reinterpret_cast<uint32_t*>(tab + w.pk_base);
    auto* rs_ents = reinterpret_cast<WangStreamRsEntry*>(tab + w.rs);     // filled on a resampling set only
    uint32_t vb = 0, sb = 0, pb = 0, closed_base = 0, open_slot = (uint32_t)n_closed;
    for (size_t i = 0; i < n; i++) {
        const Plan& p = s->plan[i];
        const uint64_t carry_in = p.n0 - 128 * p.vbase, vlen = carry_in + p.m;
        WangStreamClip& cl = clips[i];
        cl.src_off = vb;
        cl.src_n = cl.n8k = vlen;
        cl.frames = (uint32_t)frames_of(vlen);
        cl.j_lo = (uint32_t)(p.j0 - p.vbase);
        cl.j_hi = (uint32_t)(p.j1 - p.vbase);
        cl.t_shift = (uint32_t)(p.vbase - p.o);
        cl.t_org = (uint32_t)p.o;
        cl.sec_org = (uint32_t)p.s0;
        cl.n_closed = (uint32_t)p.n_closed;
        cl.closed_base = closed_base;
        cl.open_slot = p.fin ? 0xffffffffu : open_slot;
        cl.pad = 0;
        WangStreamEntry& e = ents[i];
        e.slot = p.slot;
        e.carry_in = (uint32_t)carry_in;
        const uint64_t keep = p.j1 > 7 ? p.j1 - 7 : 0;           // the next push starts at frame J - 7
        e.keep_rel = p.fin ? 0 : (uint32_t)(128 * (keep - p.vbase));
        e.carry_out = p.fin ? 0 : (uint32_t)(p.n1 - 128 * keep);
        e.chunk_off = 0;
        e.o = (uint32_t)p.o;
        e.f_lo = (uint32_t)p.f_lo;
        e.f_hi = (uint32_t)p.f_hi;
        e.fin = p.fin ? 1u : 0u;
        e.ret_from = (uint32_t)p.f_hi;
        e.fresh = p.n0 == 0 ? 1u : 0u;
        v_base[i] = vb;
        seg_base[i] = sb;
        pk_base[i] = pb;
        vb += (uint32_t)vlen;
        sb += (uint32_t)((p.j1 - p.j0 + w.seg - 1) / w.seg);
        pb += (uint32_t)p.cap;
        closed_base += (uint32_t)p.n_closed;
        if (!p.fin) open_slot++;
    }
    uint64_t chunk = 0;
    for (size_t i = 0; i < n; i++) {
        const Plan& p = s->plan[i];
        ents[i].chunk_off = chunk;
        if (resample) {
            // between pushes the state holds the inputs from floor(S sr / 8000) on, S the non-final count: the final
            // push of a stream carries nothing out
            WangStreamRsEntry& r = rs_ents[i];
            r.s0 = p.rs.s0;
            r.n0 = p.rs.n0;
            r.n1 = p.rs.n1;
            r.c_in = p.rs.c_in;
            r.c_out = p.rs.c_out;
            r.chunk_off = chunk;
            r.slot = p.slot;
            r.fin = p.fin ? 1u : 0u;
        }
        chunk += p.rs.n1 - p.rs.n0;
    }
    v_base[n] = vb;
    seg_base[n] = sb;
    pk_base[n] = pb;
    *reinterpret_cast<uint32_t*>(tab + w.n_closed_w) = (uint32_t)n_closed;
    w.n_seg = sb;
    HIP_TRY(hipStreamWaitEvent(st, ctx->audio_done, 0));
    HIP_TRY(hipStreamWaitEvent(st, s->done, 0));
    HIP_TRY(hipMemcpyAsync(ctx->audio_ws + w.clips, tab, w.tab_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->tab_copied[k], st));
    *out_w = w;
    return UCFP_OK;
}

// behind the push's launches: orders the next audio call and the set's next push after them, then advances the host
// state (a final push closes its slot)
inline int push_end(Set* s, size_t n, hipStream_t st) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ctx->audio_done, st));
    HIP_TRY(hipEventRecord(s->done, st));
    for (size_t i = 0; i < n; i++) {
        const Plan& p = s->plan[i];
        s->n[p.slot] = p.fin ? 0 : p.rs.n1;
        if (p.fin) s->open[p.slot] = 0;
    }
    return UCFP_OK;
}

// ---- the entries both back ends export: max_hashes, push_dev and the staged single-stream push.  A back end K names
// its set type `set`, the bytes of a record `rec_bytes`, the alignment asked of the caller's record buffer `align`
// with the refusal `align_msg`, its name in the C ABI `abi`, whether a push must emit fewer than 2^32 - 1 records
// `bound32`, and `launch`, its kernels behind push_begin. ----

// the set's and the context's locks are held; the plan is current
template <class K>
int push_impl(typename K::set* s, size_t n, const float* d_pcm, uint8_t* d_out, size_t cap_hashes, uint64_t* d_out_offsets,
              hipStream_t st) {
    WangPushWs w;
    int rc = push_begin(s, n, st, &w);
    if (rc) return rc;
    K::launch(s, d_pcm, w, d_out, cap_hashes, d_out_offsets, st);
    return push_end(s, n, st);
}

// the set's lock is held; the plan is current and bounds the push by `bound` records
template <class K>
int check_cap(size_t cap_hashes, size_t bound) {
    if (cap_hashes < bound)
        return capi_fail(UCFP_E_INVALID, "cap_hashes %zu below ucfp_%s_streams_max_hashes = %zu", cap_hashes, K::abi, bound);
    if (K::bound32 && bound >= 0xffffffffu) return capi_fail(UCFP_E_INVALID, "push too large for one call: split it");
    return UCFP_OK;
}

template <class K>
size_t entry_max_hashes(typename K::set* s, const uint32_t* slots, const uint64_t* n_samples, const uint8_t* fin, size_t n) {
    if (!s) return 0;
    std::lock_guard<std::mutex> lk(s->mu);
    size_t bound = 0;
    return plan_push(s, slots, n_samples, fin, n, &bound) == UCFP_OK ? bound : 0;
}

template <class K>
int entry_push_dev(typename K::set* s, const uint32_t* slots, const uint64_t* n_samples, const uint8_t* fin, size_t n,
                   const float* d_pcm, uint8_t* d_out, size_t cap_hashes, uint64_t* d_out_offsets, void* stream) {
    if (!s) return capi_fail(UCFP_E_INVALID, "set is NULL");
    if (!d_out_offsets || (cap_hashes && !d_out)) return capi_fail(UCFP_E_INVALID, "NULL buffer");
    if (cap_hashes && ((uintptr_t)d_out & (K::align - 1))) return capi_fail(UCFP_E_INVALID, "%s", K::align_msg);
    std::lock_guard<std::mutex> lk(s->mu);
    size_t bound = 0;
    int rc = plan_push(s, slots, n_samples, fin, n, &bound);
    if (rc) return rc;
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) total += n_samples[i];
    if (total && !d_pcm) return capi_fail(UCFP_E_INVALID, "d_pcm is NULL");
    rc = check_cap<K>(cap_hashes, bound);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk2(s->ctx->mu);
    return push_impl<K>(s, n, d_pcm, d_out, cap_hashes, d_out_offsets, (hipStream_t)stream);
}

template <class K>
int entry_push(typename K::set* s, uint32_t slot, const float* pcm, size_t n, int fin_flag, uint8_t* out, size_t cap_hashes,
               size_t* n_hashes) {
    if (!s || !n_hashes) return capi_fail(UCFP_E_INVALID, "set / n_hashes is NULL");
    *n_hashes = 0;
    if ((n && !pcm) || (cap_hashes && !out)) return capi_fail(UCFP_E_INVALID, "NULL buffer");
    std::lock_guard<std::mutex> lk(s->mu);
    const uint64_t m = n;
    const uint8_t fin = fin_flag ? 1 : 0;
    size_t bound = 0;
    int rc = plan_push(s, &slot, &m, &fin, 1, &bound);
    if (!rc) rc = check_cap<K>(cap_hashes, bound);
    if (rc) return rc;
    ucfp_ctx* ctx = s->ctx;
    std::lock_guard<std::mutex> lk2(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    rc = grow(&ctx->stage_in, &ctx->stage_in_cap, (n ? n : 1) * 4);
    if (!rc) rc = grow(&ctx->stage_out, &ctx->stage_out_cap, 256 + (bound ? bound : 1) * K::rec_bytes);
    if (rc) return rc;
    hipStream_t st = ctx->host_stream;
    uint64_t* d_off = reinterpret_cast<uint64_t*>(ctx->stage_out);
    uint8_t* d_out = ctx->stage_out + 256;          // hipMalloc'ed, so 256 on keeps a record's alignment
    if (n) HIP_TRY(hipMemcpyAsync(ctx->stage_in, pcm, n * 4, hipMemcpyHostToDevice, st));
    rc = push_impl<K>(s, 1, reinterpret_cast<const float*>(ctx->stage_in), d_out, bound, d_off, st);
    if (rc) return rc;
    uint64_t off[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(off, d_off, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const size_t h = (size_t)(off[1] - off[0]);
    if (h) HIP_TRY(hipMemcpy(out, d_out + off[0] * K::rec_bytes, h * K::rec_bytes, hipMemcpyDeviceToHost));
    *n_hashes = h;
    return UCFP_OK;
}

// Creation, for either back end: K also names the algorithm `name`, its default config `defaults()` and the set's rings
// `rings(s)`.  The rate and the config are judged first (UCFP_E_MODALITY), whatever else is wrong.
// `any_rate` (the _sr entries, A21): the set resamples its feed on the device; otherwise only 8 kHz is taken, as the
// reference does.
template <class K, class C>
int entry_create(ucfp_ctx* ctx, uint32_t sample_rate, const C* cfg, uint32_t max_streams, uint32_t window_frames,
                 typename K::set** out, bool any_rate = false) {
    if (any_rate && !sr_ok(sample_rate))
        return capi_fail(UCFP_E_MODALITY, "%s streams: sample rate %u Hz outside [%u, %u]", K::name, sample_rate, kMinSr,
                         kMaxSr);
    if (!any_rate && sample_rate != kSr8k)
        return capi_fail(UCFP_E_MODALITY, "%s requires 8 kHz mono input (got %u Hz); resample upstream", K::name, sample_rate);
    const Cfg c = cfg ? cfg_of(*cfg) : K::defaults();
    if (!cfg_ok(c)) return capi_fail(UCFP_E_MODALITY, "%sConfig outside the ranges of /v1/algorithms", K::name);
    if (!ctx || !out) return capi_fail(UCFP_E_INVALID, "ctx / out is NULL");
    *out = nullptr;
    if (max_streams == 0 || max_streams > (1u << 20))
        return capi_fail(UCFP_E_INVALID, "max_streams %u outside [1, 2^20]", max_streams);
    if (window_frames > kMaxWindowFrames)
        return capi_fail(UCFP_E_INVALID, "window_frames %u above %u", window_frames, kMaxWindowFrames);
    HIP_TRY(hipSetDevice(ctx->device));
    typename K::set* s = new (std::nothrow) typename K::set();
    if (!s) return capi_fail(UCFP_E_INDEX, "out of host memory");
    hipError_t e = set_init(s, ctx, c, max_streams, sample_rate);
    s->window = window_frames;
    if (e == hipSuccess && window_frames) e = rings_init(s, window_frames, &K::rings(s));
    if (e != hipSuccess) {
        set_release(s);
        delete s;
        return capi_fail(UCFP_E_INDEX, "stream set allocation failed: %s", hipGetErrorString(e));
    }
    *out = s;
    return UCFP_OK;
}

// host-only: records of a window, device bytes per stream (0 for out-of-range arguments)
template <class K, class C>
size_t entry_window_cap(const C* cfg, uint32_t window_frames) {
    const Cfg c = cfg ? cfg_of(*cfg) : K::defaults();
    return cfg_ok(c) && window_frames <= kMaxWindowFrames ? window_cap_of(c, window_frames) : 0;
}

template <class K, class C>
size_t entry_state_bytes(const C* cfg, uint32_t window_frames, uint32_t sample_rate = kSr8k) {
    const Cfg c = cfg ? cfg_of(*cfg) : K::defaults();
    if (!cfg_ok(c) || window_frames > kMaxWindowFrames || !sr_ok(sample_rate)) return 0;
    const size_t ring = window_frames ? kRingHeader + K::rec_bytes * window_cap_of(c, window_frames) : 0;
    return state_bytes_per_stream(ret_cap_of(c)) + ring + (size_t)carry_cap_of(sample_rate) * 4;
}

// The live windows of n distinct open slots in the ragged shape of the back end's index, rebased to their origins; K
// also names the set's rings `rings(s)`, the argument that counts the caller's records `cap_arg` and its buffer
// `buf_name`.  The items go through the set's pinned tables, in turn with the pushes'; no host synchronisation.
template <class K>
int entry_windows_dev(typename K::set* s, const uint32_t* slots, size_t n, uint8_t* d_out, size_t cap, uint64_t* d_offsets,
                      uint32_t* d_origins, void* stream) {
    if (!s) return capi_fail(UCFP_E_INVALID, "set is NULL");
    if (!d_offsets || (n && !slots) || (cap && !d_out)) return capi_fail(UCFP_E_INVALID, "NULL buffer");
    if (cap && ((uintptr_t)d_out & (K::align - 1))) return capi_fail(UCFP_E_INVALID, "%s", K::align_msg);
    std::lock_guard<std::mutex> lk(s->mu);
    if (!s->window) return capi_fail(UCFP_E_INVALID, "the set was created with window_frames = 0: it keeps no windows");
    int rc = s->check(slots, n, "items", "call");
    if (rc) return rc;
    const auto& rg = K::rings(s);
    const size_t need = n * (size_t)rg.cap;
    if (cap < need)
        return capi_fail(UCFP_E_INVALID, "%s %zu below n * ucfp_%s_streams_window_cap = %zu", K::cap_arg, cap, K::abi, need);
    if (need >= 0xffffffffu) return capi_fail(UCFP_E_INVALID, "too many windows for one call: split it");
    ucfp_ctx* ctx = s->ctx;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk2(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    const StreamWindowsWs w = stream_windows_layout(n);
    rc = grow(&ctx->audio_ws, &ctx->audio_ws_cap, w.total);
    if (rc) return rc;
    int k = 0;
    rc = s->next(&k);
    if (rc) return rc;
    auto* items = reinterpret_cast<StreamWindowItem*>(s->tab_h[k]);
    for (size_t i = 0; i < n; i++) {
        const uint64_t ns = s->n[slots[i]];
        const uint64_t f = frontier_of(judged_of(samples_of(ns, s->rs.sr, false)), s->cfg.target_zone_t);
        items[i].slot = slots[i];
        items[i].w0 = (uint32_t)(f > s->window ? f - s->window : 0);
        items[i].live = ns ? 1u : 0u;
        items[i].pad = 0;
    }
    HIP_TRY(hipStreamWaitEvent(st, ctx->audio_done, 0));
    HIP_TRY(hipStreamWaitEvent(st, s->done, 0));
    if (n) HIP_TRY(hipMemcpyAsync(ctx->audio_ws + w.items, items, w.tab_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->tab_copied[k], st));
    launch_streams_windows(rg, ctx->audio_ws, w, d_out, cap, d_offsets, d_origins, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->audio_done, st));
    HIP_TRY(hipEventRecord(s->done, st));
    return UCFP_OK;
}

}  // namespace wstreams
}  // namespace ucfp
