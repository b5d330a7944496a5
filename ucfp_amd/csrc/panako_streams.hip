// panako_streams.hip -- streaming Panako fingerprints: device-resident sessions, batched pushes, and a
// live window per stream for the tempo-tolerant matcher (panako_index.hip, A14).
//
// Panako runs on Wang's front end unchanged (A13 P1), so a set is a Wang stream set (wang_streams_core.h: the plan of a
// push, the carried state) sized with the Panako config; a push ends in triplets instead of pairs (audio.hip,
// launch_panako_streams_push).  On top comes one ring of records per stream: the emitted records with t_a >= w0 =
// max(0, F(n) - W), which ucfp_panako_streams_windows_dev hands out rebased to w0 in the ragged shape
// ucfp_panako_index_query_dev takes.
#include "wang_streams_core.h"

#define fail ucfp::capi_fail

using namespace ucfp::wstreams;

struct ucfp_panako_streams : Set {
    uint32_t window = 0;                  // W in frames
    ucfp::PanakoRingsDev rings{};
    uint8_t* ring_mem = nullptr;
};

namespace {

constexpr size_t kRingHeader = 8;         // head and count

Cfg defaults() { return Cfg{5u, 96u, 96u, 30u, -50.0f}; }

// records a window of W frames can hold (A19): the emitted anchors of [w0, F) lie in at most ceil(2 W / 125) + 1 seconds
size_t window_cap_of(const Cfg& c, uint32_t w) {
    return w ? ((size_t)(2 * w + 124) / 125 + 1) * c.peaks_per_sec * c.fan_out : 0;
}

// what Panako's entries put into the shared ones (wang_streams_core.h): 16-byte aligned records, fewer than 2^32 - 1 of
// them per push, its name, its launch
struct Panako {
    using set = ucfp_panako_streams;
    static constexpr size_t rec_bytes = 16, align = 16;
    static constexpr const char* align_msg = "the record buffer must be 16-byte aligned";
    static constexpr const char* abi = "panako";
    static constexpr bool bound32 = true;
    static void launch(set* s, const float* d_pcm, const ucfp::WangPushWs& w, uint8_t* d_out, size_t cap_hashes,
                       uint64_t* d_out_offsets, hipStream_t st) {
        const Cfg& c = s->cfg;
        ucfp::launch_panako_streams_push(d_pcm, s->dev, s->rings, c.fan_out, c.target_zone_t, c.target_zone_f,
                                         c.peaks_per_sec, s->floor_p, s->ctx->audio_ws, w,
                                         reinterpret_cast<uint32_t*>(d_out), cap_hashes, d_out_offsets, st);
    }
};

}  // namespace

extern "C" {

uint64_t ucfp_panako_stream_frontier(uint64_t n_samples, const ucfp_panako_config* cfg) {
    const Cfg c = cfg ? cfg_of(*cfg) : defaults();
    return frontier_of(judged_of(n_samples), c.target_zone_t);
}

size_t ucfp_panako_streams_window_cap(const ucfp_panako_config* cfg, uint32_t window_frames) {
    const Cfg c = cfg ? cfg_of(*cfg) : defaults();
    return cfg_ok(c) && window_frames <= UCFP_PANAKO_STREAM_MAX_WINDOW_FRAMES ? window_cap_of(c, window_frames) : 0;
}

size_t ucfp_panako_streams_state_bytes(const ucfp_panako_config* cfg, uint32_t window_frames) {
    const Cfg c = cfg ? cfg_of(*cfg) : defaults();
    if (!cfg_ok(c) || window_frames > UCFP_PANAKO_STREAM_MAX_WINDOW_FRAMES) return 0;
    const size_t ring = window_frames ? kRingHeader + 16 * window_cap_of(c, window_frames) : 0;
    return state_bytes_per_stream(ret_cap_of(c)) + ring;
}

int ucfp_panako_streams_create(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_panako_config* cfg, uint32_t max_streams,
                               uint32_t window_frames, ucfp_panako_streams** out) {
    if (sample_rate != 8000)
        return fail(UCFP_E_MODALITY, "Panako requires 8 kHz mono input (got %u Hz); resample upstream", sample_rate);
    const Cfg c = cfg ? cfg_of(*cfg) : defaults();
    if (!cfg_ok(c)) return fail(UCFP_E_MODALITY, "PanakoConfig outside the ranges of /v1/algorithms");
    if (!ctx || !out) return fail(UCFP_E_INVALID, "ctx / out is NULL");
    *out = nullptr;
    if (max_streams == 0 || max_streams > (1u << 20)) return fail(UCFP_E_INVALID, "max_streams %u outside [1, 2^20]", max_streams);
    if (window_frames > UCFP_PANAKO_STREAM_MAX_WINDOW_FRAMES)
        return fail(UCFP_E_INVALID, "window_frames %u above %u", window_frames, UCFP_PANAKO_STREAM_MAX_WINDOW_FRAMES);
    HIP_TRY(hipSetDevice(ctx->device));
    ucfp_panako_streams* s = new (std::nothrow) ucfp_panako_streams();
    if (!s) return fail(UCFP_E_INDEX, "out of host memory");
    hipError_t e = set_init(s, ctx, c, max_streams);
    s->window = window_frames;
    if (e == hipSuccess && window_frames) {
        const size_t ms = max_streams, cap = window_cap_of(c, window_frames);
        const size_t rec_bytes = (ms * cap * 16 + 255) & ~(size_t)255;
        e = hipMalloc((void**)&s->ring_mem, rec_bytes + 2 * ((ms * 4 + 255) & ~(size_t)255));
        if (e == hipSuccess) {
            s->rings.rec = reinterpret_cast<uint4*>(s->ring_mem);
            s->rings.head = reinterpret_cast<uint32_t*>(s->ring_mem + rec_bytes);
            s->rings.count = reinterpret_cast<uint32_t*>(s->ring_mem + rec_bytes + ((ms * 4 + 255) & ~(size_t)255));
            s->rings.cap = (uint32_t)cap;
            s->rings.window = window_frames;
        }
    }
    if (e != hipSuccess) {
        ucfp_panako_streams_destroy(s);
        return fail(UCFP_E_INDEX, "stream set allocation failed: %s", hipGetErrorString(e));
    }
    *out = s;
    return UCFP_OK;
}

void ucfp_panako_streams_destroy(ucfp_panako_streams* s) {
    if (!s) return;
    set_release(s);
    if (s->ring_mem) (void)hipFree(s->ring_mem);
    delete s;
}

int ucfp_panako_streams_open(ucfp_panako_streams* s, uint32_t* slot) {
    if (!s || !slot) return fail(UCFP_E_INVALID, "set / slot is NULL");
    return set_open(s, slot);
}

// the ring needs no device work: a slot that has seen no sample since it was opened has an empty window (windows_dev),
// and its first push starts the ring afresh
int ucfp_panako_streams_close(ucfp_panako_streams* s, uint32_t slot) {
    if (!s) return fail(UCFP_E_INVALID, "set is NULL");
    return set_close(s, slot);
}

size_t ucfp_panako_streams_max_hashes(ucfp_panako_streams* s, const uint32_t* slots, const uint64_t* n_samples,
                                      const uint8_t* final, size_t n) {
    return entry_max_hashes<Panako>(s, slots, n_samples, final, n);
}

int ucfp_panako_streams_push_dev(ucfp_panako_streams* s, const uint32_t* slots, const uint64_t* n_samples,
                                 const uint8_t* final, size_t n, const float* d_pcm, uint8_t* d_out, size_t cap_hashes,
                                 uint64_t* d_out_offsets, void* stream) {
    return entry_push_dev<Panako>(s, slots, n_samples, final, n, d_pcm, d_out, cap_hashes, d_out_offsets, stream);
}

int ucfp_panako_streams_push(ucfp_panako_streams* s, uint32_t slot, const float* pcm, size_t n, int final, uint8_t* out,
                             size_t cap_hashes, size_t* n_hashes) {
    return entry_push<Panako>(s, slot, pcm, n, final, out, cap_hashes, n_hashes);
}

int ucfp_panako_streams_windows_dev(ucfp_panako_streams* s, const uint32_t* slots, size_t n, uint8_t* d_records,
                                    size_t cap_records, uint64_t* d_offsets, uint32_t* d_origins, void* stream) {
    if (!s) return fail(UCFP_E_INVALID, "set is NULL");
    if (!d_offsets || (n && !slots) || (cap_records && !d_records)) return fail(UCFP_E_INVALID, "NULL buffer");
    if (cap_records && ((uintptr_t)d_records & 15u)) return fail(UCFP_E_INVALID, "the record buffer must be 16-byte aligned");
    std::lock_guard<std::mutex> lk(s->mu);
    if (!s->window) return fail(UCFP_E_INVALID, "the set was created with window_frames = 0: it keeps no windows");
    int rc = s->check(slots, n, "items", "call");
    if (rc) return rc;
    const size_t need = n * (size_t)s->rings.cap;
    if (cap_records < need)
        return fail(UCFP_E_INVALID, "cap_records %zu below n * ucfp_panako_streams_window_cap = %zu", cap_records, need);
    if (need >= 0xffffffffu) return fail(UCFP_E_INVALID, "too many windows for one call: split it");
    ucfp_ctx* ctx = s->ctx;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk2(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    const ucfp::PanakoWindowsWs w = ucfp::panako_windows_layout(n);
    rc = ucfp::grow(&ctx->audio_ws, &ctx->audio_ws_cap, w.total);
    if (rc) return rc;
    // the items go through the set's pinned tables, in turn with the pushes'
    int k = 0;
    rc = s->next(&k);
    if (rc) return rc;
    auto* items = reinterpret_cast<ucfp::PanakoWindowItem*>(s->tab_h[k]);
    for (size_t i = 0; i < n; i++) {
        const uint64_t ns = s->n[slots[i]], f = frontier_of(judged_of(ns), s->cfg.target_zone_t);
        items[i].slot = slots[i];
        items[i].w0 = (uint32_t)(f > s->window ? f - s->window : 0);
        items[i].live = ns ? 1u : 0u;
        items[i].pad = 0;
    }
    HIP_TRY(hipStreamWaitEvent(st, ctx->audio_done, 0));
    HIP_TRY(hipStreamWaitEvent(st, s->done, 0));
    if (n) HIP_TRY(hipMemcpyAsync(ctx->audio_ws + w.items, items, w.tab_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s->tab_copied[k], st));
    ucfp::launch_panako_streams_windows(s->rings, ctx->audio_ws, w, d_records, cap_records, d_offsets, d_origins, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->audio_done, st));
    HIP_TRY(hipEventRecord(s->done, st));
    return UCFP_OK;
}

}  // extern "C"
