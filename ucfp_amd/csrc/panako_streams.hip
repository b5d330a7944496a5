// panako_streams.hip -- streaming Panako fingerprints: device-resident sessions, batched pushes, and a
// live window per stream for the tempo-tolerant matcher (panako_index.hip, A14).
//
// Panako runs on Wang's front end unchanged (A13 P1), so a set is a Wang stream set (wang_streams_core.h: the plan of a
// push, the carried state) sized with the Panako config; a push ends in triplets instead of pairs (audio.hip,
// launch_panako_streams_push).  On top comes one ring of records per stream: the emitted records with t_a >= w0 =
// max(0, F(n) - W), which ucfp_panako_streams_windows_dev hands out rebased to w0 in the ragged shape
// ucfp_panako_index_query_dev takes.  A set from ucfp_panako_streams_create_sr resamples its feed on the device (A21).
#include "wang_streams_core.h"

#define fail ucfp::capi_fail

using namespace ucfp::wstreams;

struct ucfp_panako_streams : Set {
    ucfp::PanakoRingsDev rings{};         // the latest window_cap records per stream (window != 0)
};

namespace {

// what Panako's entries put into the shared ones (wang_streams_core.h): 16-byte aligned records, fewer than 2^32 - 1 of
// them per push, its names, its launch
struct Panako {
    using set = ucfp_panako_streams;
    static constexpr size_t rec_bytes = 16, align = 16;
    static constexpr const char* align_msg = "the record buffer must be 16-byte aligned";
    static constexpr const char* abi = "panako";
    static constexpr const char* name = "Panako";
    static constexpr const char* cap_arg = "cap_records";
    static constexpr bool bound32 = true;
    static Cfg defaults() { return Cfg{5u, 96u, 96u, 30u, -50.0f}; }
    static ucfp::PanakoRingsDev& rings(set* s) { return s->rings; }
    static void launch(set* s, const float* d_pcm, const ucfp::WangPushWs& w, uint8_t* d_out, size_t cap_hashes,
                       uint64_t* d_out_offsets, hipStream_t st) {
        const Cfg& c = s->cfg;
        ucfp::launch_panako_streams_push(d_pcm, s->dev, s->rs, s->rings, c.fan_out, c.target_zone_t, c.target_zone_f,
                                         c.peaks_per_sec, s->floor_p, s->ctx->audio_ws, w,
                                         reinterpret_cast<uint32_t*>(d_out), cap_hashes, d_out_offsets, st);
    }
};

}  // namespace

extern "C" {

uint64_t ucfp_panako_stream_frontier(uint64_t n_samples, const ucfp_panako_config* cfg) {
    const Cfg c = cfg ? cfg_of(*cfg) : Panako::defaults();
    return frontier_of(judged_of(n_samples), c.target_zone_t);
}

size_t ucfp_panako_streams_window_cap(const ucfp_panako_config* cfg, uint32_t window_frames) {
    return entry_window_cap<Panako>(cfg, window_frames);
}

size_t ucfp_panako_streams_state_bytes(const ucfp_panako_config* cfg, uint32_t window_frames) {
    return entry_state_bytes<Panako>(cfg, window_frames);
}

size_t ucfp_panako_streams_state_bytes_sr(const ucfp_panako_config* cfg, uint32_t window_frames, uint32_t sample_rate) {
    return entry_state_bytes<Panako>(cfg, window_frames, sample_rate);
}

int ucfp_panako_streams_create(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_panako_config* cfg, uint32_t max_streams,
                               uint32_t window_frames, ucfp_panako_streams** out) {
    return entry_create<Panako>(ctx, sample_rate, cfg, max_streams, window_frames, out);
}

int ucfp_panako_streams_create_sr(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_panako_config* cfg,
                                  uint32_t max_streams, uint32_t window_frames, ucfp_panako_streams** out) {
    return entry_create<Panako>(ctx, sample_rate, cfg, max_streams, window_frames, out, true);
}

void ucfp_panako_streams_destroy(ucfp_panako_streams* s) {
    if (!s) return;
    set_release(s);
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
    return entry_windows_dev<Panako>(s, slots, n, d_records, cap_records, d_offsets, d_origins, stream);
}

}  // extern "C"
