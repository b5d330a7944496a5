// haitsma_streams.hip -- streaming Haitsma-Kalker sub-fingerprints: device-resident sessions, batched
// pushes, live blocks for ucfp_haitsma_index_query_dev.
//
// A set holds up to max_streams live streams at one sample rate; one push advances any subset of them by one chunk each
// with one launch sequence (audio.hip, launch_haitsma_streams_push).  The host tracks how many samples each stream has
// seen, which fixes every count and offset of the push in integers (A18): the host plans, the device keeps the data (the
// 5 kHz tail of the next frame, the input samples the next output still needs, the last frame's band energies, a ring
// of the latest sub-fingerprints).
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/ucfp_hip.h"
#include "common.h"
#include "ctx.h"
#include "stream_set.h"

#define fail ucfp::capi_fail

namespace {

constexpr uint64_t kMaxChunk = (uint64_t)1 << 29;         // samples of one stream in one push
constexpr uint64_t kMaxPushSamples = (uint64_t)1 << 31;   // carried + new 5 kHz samples of one push (32-bit run offsets)
constexpr uint64_t kMaxFrames = ((uint64_t)1 << 32) - 1024;   // frames of a stream (~636 days)
constexpr uint32_t kSr = 5000, kN = 2048, kHop = 64;

bool rate_ok(uint32_t sr) { return sr >= 1000 && sr <= 384000; }
bool edges_ok(float fmin, float fmax) { return fmin >= 1.0f && fmax > fmin && fmax <= 2500.0f; }

// A18, all since the stream was opened
uint64_t final_len(uint64_t n, uint32_t sr) {                 // the offline resampler's length
    return sr == kSr ? n : (uint64_t)(((unsigned __int128)n * kSr) / sr);
}
uint64_t samples_of(uint64_t n, uint32_t sr, bool fin) {      // S(n): final 5 kHz samples
    if (sr == kSr || fin || n == 0) return final_len(n, sr);
    const uint64_t a = (uint64_t)((((unsigned __int128)(n - 1) * kSr) + sr - 1) / sr);   // right neighbour arrived
    const uint64_t b = final_len(n, sr);
    return a < b ? a : b;
}
uint64_t frames_of(uint64_t s5) { return s5 < kN ? 0 : (s5 - kN) / kHop + 1; }   // Fr
uint64_t input_of(uint64_t s5, uint32_t sr) {                 // the input sample output s5 starts from
    return sr == kSr ? s5 : (uint64_t)(((unsigned __int128)s5 * sr) / kSr);
}
uint32_t carry_cap_of(uint32_t sr) { return (sr + kSr - 1) / kSr + 1; }

size_t state_bytes_per_stream(uint32_t sr, uint32_t block) {
    return ((size_t)ucfp::kHkTailCap + carry_cap_of(sr) + ucfp::kHkEnergies + block) * 4;
}

// one entry of a push, planned on the host
struct Plan {
    uint32_t slot;
    uint64_t m, n0, n1, s0, s1, f0, f1;
    bool fin;
};

}  // namespace

// the slot table counts samples; the pinned tables hold a push or the entries of a blocks call
struct ucfp_haitsma_streams : ucfp::streams::Slots, ucfp::streams::Tables {
    ucfp_ctx* ctx = nullptr;
    uint32_t sr = 0, block = 0;
    std::vector<Plan> plan;
    ucfp::HaitsmaStreamsDev dev{};
    uint8_t* dev_mem = nullptr;
    ucfp::HaitsmaBlockEntry* blk_d = nullptr;   // the table of the last blocks call
};

namespace {

size_t tab_bytes_max(uint32_t max_streams) {
    return (size_t)max_streams * sizeof(ucfp::HaitsmaStreamEntry) + 2 * ((size_t)max_streams + 1) * 4 + 256;
}

// validates the push and plans every entry; nothing changes.  *frames: what the push emits, *run: its 5 kHz samples
int plan_push(ucfp_haitsma_streams* s, const uint32_t* slots, const uint64_t* n_samples, const uint8_t* fin, size_t n,
              size_t* frames, uint64_t* run) {
    if (n && !n_samples) return fail(UCFP_E_INVALID, "n_samples is NULL");
    if (n && !slots) return fail(UCFP_E_INVALID, "slots is NULL");
    int rc = s->check(slots, n, "entries", "call");   // every slot is judged before anything else
    if (rc) return rc;
    s->plan.resize(n);
    uint64_t total_f = 0, total_r = 0;
    for (size_t i = 0; i < n; i++) {
        Plan& p = s->plan[i];
        p.slot = slots[i];
        p.m = n_samples[i];
        if (p.m > kMaxChunk)
            return fail(UCFP_E_INVALID, "a chunk of %llu samples exceeds 2^29: split it", (unsigned long long)p.m);
        p.n0 = s->n[p.slot];
        p.n1 = p.n0 + p.m;
        p.fin = fin && fin[i];
        p.s0 = samples_of(p.n0, s->sr, false);
        p.s1 = samples_of(p.n1, s->sr, p.fin);
        p.f0 = frames_of(p.s0);
        p.f1 = frames_of(p.s1);
        if (p.f1 > kMaxFrames) return fail(UCFP_E_INVALID, "slot %u would pass 2^32 frames", p.slot);
        // what A18 bounds, checked where a miss would write past the slot's state
        if (!p.fin && (p.s1 - kHop * p.f1 >= ucfp::kHkTailCap || p.n1 - input_of(p.s1, s->sr) > s->dev.carry_cap))
            return fail(UCFP_E_INVALID, "slot %u would carry more than its state holds", p.slot);
        total_f += p.f1 - p.f0;
        total_r += p.s1 - kHop * p.f0;
        if (total_r >= kMaxPushSamples)
            return fail(UCFP_E_INVALID, "push of %llu samples at 5 kHz reaches 2^31: split it", (unsigned long long)total_r);
    }
    *frames = (size_t)total_f;
    *run = total_r;
    return UCFP_OK;
}

// the set's and the context's locks are held; the plan is current
int push_impl(ucfp_haitsma_streams* s, size_t n, size_t frames, uint64_t run, const float* d_pcm, uint32_t* d_out,
              uint64_t* d_out_offsets, hipStream_t st) {
    ucfp_ctx* ctx = s->ctx;
    const ucfp::HaitsmaPushWs w = ucfp::haitsma_push_layout(n, (size_t)run, frames);
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = ucfp::grow(&ctx->audio_ws, &ctx->audio_ws_cap, w.total);
    if (rc) return rc;
    int k = 0;
    rc = s->next(&k);
    if (rc) return rc;
    uint8_t* tab = s->tab_h[k];
    auto* ents = reinterpret_cast<ucfp::HaitsmaStreamEntry*>(tab + w.ents);
    auto* run_base = reinterpret_cast<uint32_t*>(tab + w.run_base);
    auto* fr_base = reinterpret_cast<uint32_t*>(tab + w.fr_base);
    uint32_t rb = 0, fb = 0;
    uint64_t chunk = 0;
    for (size_t i = 0; i < n; i++) {
        const Plan& p = s->plan[i];
        ucfp::HaitsmaStreamEntry& e = ents[i];
        e.s0 = p.s0;
        e.n0 = p.n0;
        e.n1 = p.n1;
        e.c_in = input_of(p.s0, s->sr);
        e.c_out = input_of(p.s1, s->sr);
        e.f0 = p.f0;
        e.chunk_off = chunk;
        e.slot = p.slot;
        e.tail_in = (uint32_t)(p.s0 - kHop * p.f0);
        e.tail_out = p.fin ? 0 : (uint32_t)(p.s1 - kHop * p.f1);
        e.fin = p.fin ? 1u : 0u;
        run_base[i] = rb;
        fr_base[i] = fb;
        rb += (uint32_t)(p.s1 - kHop * p.f0);
        fb += (uint32_t)(p.f1 - p.f0);
        chunk += p.m;
    }
    run_base[n] = rb;
    fr_base[n] = fb;
    HIP_TRY(hipStreamWaitEvent(st, ctx->audio_done, 0));
    HIP_TRY(hipStreamWaitEvent(st, s->done, 0));
    HIP_TRY(hipMemcpyAsync(ctx->audio_ws + w.ents, tab, w.tab_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->tab_copied[k], st));
    ucfp::launch_haitsma_streams_push(d_pcm, s->dev, s->sr, ctx->audio_ws, w, d_out, d_out_offsets, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->audio_done, st));
    HIP_TRY(hipEventRecord(s->done, st));
    for (size_t i = 0; i < n; i++) {
        const Plan& p = s->plan[i];
        s->n[p.slot] = p.fin ? 0 : p.n1;
        if (p.fin) s->open[p.slot] = 0;
    }
    return UCFP_OK;
}

}  // namespace

extern "C" {

uint64_t ucfp_haitsma_stream_frames(uint64_t n_samples, uint32_t sample_rate, int final) {
    return rate_ok(sample_rate) ? frames_of(samples_of(n_samples, sample_rate, final != 0)) : 0;
}

size_t ucfp_haitsma_streams_state_bytes(uint32_t sample_rate, uint32_t block_frames) {
    if (!rate_ok(sample_rate) || block_frames > UCFP_HAITSMA_MAX_QUERY_FRAMES) return 0;
    return state_bytes_per_stream(sample_rate, block_frames);
}

int ucfp_haitsma_streams_create(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_haitsma_config* cfg, uint32_t max_streams,
                                uint32_t block_frames, ucfp_haitsma_streams** out) {
    if (!rate_ok(sample_rate))
        return fail(UCFP_E_MODALITY, "invalid sample rate %u (1 000 .. 384 000 Hz)", sample_rate);
    const float fmin = cfg ? cfg->fmin : 300.0f, fmax = cfg ? cfg->fmax : 2000.0f;
    if (!edges_ok(fmin, fmax)) return fail(UCFP_E_MODALITY, "Haitsma band edges must satisfy 1 <= fmin < fmax <= 2500 Hz");
    if (out) *out = nullptr;
    if (block_frames > UCFP_HAITSMA_MAX_QUERY_FRAMES)
        return fail(UCFP_E_INVALID, "block_frames %u above UCFP_HAITSMA_MAX_QUERY_FRAMES = %u", block_frames,
                    UCFP_HAITSMA_MAX_QUERY_FRAMES);
    if (!ctx) {
        if (!ucfp::have_gfx950()) return fail(UCFP_E_INDEX, "no gfx950 device available; this library has no CPU path");
        return fail(UCFP_E_INVALID, "ctx is NULL");
    }
    if (!out) return fail(UCFP_E_INVALID, "out is NULL");
    if (max_streams == 0 || max_streams > (1u << 20)) return fail(UCFP_E_INVALID, "max_streams %u outside [1, 2^20]", max_streams);
    HIP_TRY(hipSetDevice(ctx->device));
    ucfp_haitsma_streams* s = new (std::nothrow) ucfp_haitsma_streams();
    if (!s) return fail(UCFP_E_INDEX, "out of host memory");
    s->ctx = ctx;
    s->sr = sample_rate;
    s->block = block_frames;
    s->init(max_streams);
    const uint32_t cc = carry_cap_of(sample_rate);
    const size_t ms = max_streams;
    const size_t bytes = ms * (state_bytes_per_stream(sample_rate, block_frames) + sizeof(ucfp::HaitsmaBlockEntry)) + 8 * 256;
    uint32_t edges[34];
    ucfp::haitsma_band_edges(fmin, fmax, edges);
    hipError_t e = hipMalloc((void**)&s->dev_mem, bytes);
    if (e == hipSuccess) {
        size_t off = 0;
        auto take = [&](size_t b) { uint8_t* p = s->dev_mem + off; off = (off + b + 255) & ~(size_t)255; return p; };
        s->dev.tail = reinterpret_cast<float*>(take(ms * ucfp::kHkTailCap * 4));
        s->dev.carry = reinterpret_cast<float*>(take(ms * cc * 4));
        s->dev.energy = reinterpret_cast<float*>(take(ms * ucfp::kHkEnergies * 4));
        s->dev.ring = reinterpret_cast<uint32_t*>(take(ms * block_frames * 4));
        s->dev.edges = reinterpret_cast<uint32_t*>(take(sizeof edges));
        s->blk_d = reinterpret_cast<ucfp::HaitsmaBlockEntry*>(take(ms * sizeof(ucfp::HaitsmaBlockEntry)));
        s->dev.carry_cap = cc;
        s->dev.block = block_frames;
        e = hipMemcpy(s->dev.edges, edges, sizeof edges, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = s->setup(tab_bytes_max(max_streams));
    if (e != hipSuccess) {
        ucfp_haitsma_streams_destroy(s);
        return fail(UCFP_E_INDEX, "stream set allocation failed: %s", hipGetErrorString(e));
    }
    *out = s;
    return UCFP_OK;
}

void ucfp_haitsma_streams_destroy(ucfp_haitsma_streams* s) {
    if (!s) return;
    s->teardown();
    if (s->dev_mem) (void)hipFree(s->dev_mem);
    delete s;
}

int ucfp_haitsma_streams_open(ucfp_haitsma_streams* s, uint32_t* slot) {
    if (!s || !slot) return fail(UCFP_E_INVALID, "set / slot is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    return s->acquire(slot);
}

int ucfp_haitsma_streams_close(ucfp_haitsma_streams* s, uint32_t slot) {
    if (!s) return fail(UCFP_E_INVALID, "set is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    return s->release(slot);
}

size_t ucfp_haitsma_streams_max_frames(ucfp_haitsma_streams* s, const uint32_t* slots, const uint64_t* n_samples,
                                       const uint8_t* final, size_t n) {
    if (!s) return 0;
    std::lock_guard<std::mutex> lk(s->mu);
    size_t frames = 0;
    uint64_t run = 0;
    return plan_push(s, slots, n_samples, final, n, &frames, &run) == UCFP_OK ? frames : 0;
}

int ucfp_haitsma_streams_push_dev(ucfp_haitsma_streams* s, const uint32_t* slots, const uint64_t* n_samples,
                                  const uint8_t* final, size_t n, const float* d_pcm, uint32_t* d_out, size_t cap_frames,
                                  uint64_t* d_out_offsets, void* stream) {
    if (!s) return fail(UCFP_E_INVALID, "set is NULL");
    if (!d_out_offsets || (cap_frames && !d_out)) return fail(UCFP_E_INVALID, "NULL buffer");
    std::lock_guard<std::mutex> lk(s->mu);
    size_t frames = 0;
    uint64_t run = 0;
    int rc = plan_push(s, slots, n_samples, final, n, &frames, &run);
    if (rc) return rc;
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) total += n_samples[i];
    if (total && !d_pcm) return fail(UCFP_E_INVALID, "d_pcm is NULL");
    if (cap_frames < frames)
        return fail(UCFP_E_INVALID, "cap_frames %zu below ucfp_haitsma_streams_max_frames = %zu", cap_frames, frames);
    std::lock_guard<std::mutex> lk2(s->ctx->mu);
    return push_impl(s, n, frames, run, d_pcm, d_out, d_out_offsets, (hipStream_t)stream);
}

int ucfp_haitsma_streams_push(ucfp_haitsma_streams* s, uint32_t slot, const float* pcm, size_t n, int final, uint32_t* out,
                              size_t cap_frames, size_t* n_frames) {
    if (!s || !n_frames) return fail(UCFP_E_INVALID, "set / n_frames is NULL");
    *n_frames = 0;
    if ((n && !pcm) || (cap_frames && !out)) return fail(UCFP_E_INVALID, "NULL buffer");
    std::lock_guard<std::mutex> lk(s->mu);
    const uint64_t m = n;
    const uint8_t fin = final ? 1 : 0;
    size_t frames = 0;
    uint64_t run = 0;
    int rc = plan_push(s, &slot, &m, &fin, 1, &frames, &run);
    if (rc) return rc;
    if (cap_frames < frames)
        return fail(UCFP_E_INVALID, "cap_frames %zu below ucfp_haitsma_streams_max_frames = %zu", cap_frames, frames);
    ucfp_ctx* ctx = s->ctx;
    std::lock_guard<std::mutex> lk2(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    rc = ucfp::grow(&ctx->stage_in, &ctx->stage_in_cap, (n ? n : 1) * 4);
    if (!rc) rc = ucfp::grow(&ctx->stage_out, &ctx->stage_out_cap, 256 + (frames ? frames : 1) * 4);
    if (rc) return rc;
    hipStream_t st = ctx->host_stream;
    uint64_t* d_off = reinterpret_cast<uint64_t*>(ctx->stage_out);
    uint32_t* d_out = reinterpret_cast<uint32_t*>(ctx->stage_out + 256);
    if (n) HIP_TRY(hipMemcpyAsync(ctx->stage_in, pcm, n * 4, hipMemcpyHostToDevice, st));
    rc = push_impl(s, 1, frames, run, reinterpret_cast<const float*>(ctx->stage_in), d_out, d_off, st);
    if (rc) return rc;
    if (frames) HIP_TRY(hipMemcpyAsync(out, d_out, frames * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_frames = frames;
    return UCFP_OK;
}

int ucfp_haitsma_streams_blocks_dev(ucfp_haitsma_streams* s, const uint32_t* slots, size_t n, uint32_t* d_frames,
                                    size_t cap_frames, uint64_t* d_offsets, void* stream) {
    if (!s) return fail(UCFP_E_INVALID, "set is NULL");
    if (!d_offsets || (cap_frames && !d_frames)) return fail(UCFP_E_INVALID, "NULL buffer");
    std::lock_guard<std::mutex> lk(s->mu);
    if (n && !slots) return fail(UCFP_E_INVALID, "slots is NULL");
    int rc = s->check(slots, n, "entries", "call");   // every slot is judged before anything else
    if (rc) return rc;
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t fr = frames_of(samples_of(s->n[slots[i]], s->sr, false));
        total += fr < s->block ? fr : s->block;
    }
    if (cap_frames < total) return fail(UCFP_E_INVALID, "cap_frames %zu below the %llu frames of the blocks", cap_frames,
                                        (unsigned long long)total);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(s->ctx->device));
    int k = 0;
    rc = s->next(&k);
    if (rc) return rc;
    auto* tab = reinterpret_cast<ucfp::HaitsmaBlockEntry*>(s->tab_h[k]);
    uint64_t off = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t fr = frames_of(samples_of(s->n[slots[i]], s->sr, false));
        const uint32_t m = (uint32_t)(fr < s->block ? fr : s->block);
        tab[i] = ucfp::HaitsmaBlockEntry{off, slots[i], m ? (uint32_t)((fr - m) % s->block) : 0u, m, 0u};
        off += m;
    }
    HIP_TRY(hipStreamWaitEvent(st, s->done, 0));
    if (n) HIP_TRY(hipMemcpyAsync(s->blk_d, tab, n * sizeof(ucfp::HaitsmaBlockEntry), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->tab_copied[k], st));
    ucfp::launch_haitsma_streams_blocks(s->blk_d, n, s->dev, d_frames, d_offsets, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->done, st));
    return UCFP_OK;
}

}  // extern "C"
