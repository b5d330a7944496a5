// wang_streams.hip -- streaming Wang fingerprints: device-resident sessions, batched pushes.
//
// Counterpart of audio::StreamingWangSession::new / push / finalize (src/modality/audio.rs:413-480) behind the stream
// ingest route (src/server/handlers.rs:957-1010).  A set holds up to max_streams live streams; one push advances any
// subset of them by one chunk each with one launch sequence (audio.hip, launch_wang_streams_push).  The host tracks
// how many samples each stream has seen, which fixes every frame range of the push (A9): the host plans, the device
// keeps the data (carried samples, the open second's candidates, the retained peaks).  A set created with window_frames
// = W > 0 also keeps one ring of hashes per stream (A20): the emitted hashes with t_anchor >= w0 = max(0, F(n) - W),
// which ucfp_wang_streams_windows_dev hands out rebased to w0 in the ragged shape ucfp_landmark_index_query_dev takes.
// A set from ucfp_wang_streams_create_sr takes its feed at any rate from 1 to 384 kHz (A21): the slot also carries the
// few input samples the next 8 kHz sample needs, and n above becomes S(n), the 8 kHz samples that are final.
#include "wang_streams_core.h"

#define fail ucfp::capi_fail

using namespace ucfp::wstreams;   // the plan of a push, shared with panako_streams.hip

struct ucfp_wang_streams : Set {
    ucfp::WangRingsDev rings{};           // A20: the latest window_cap hashes per stream (window != 0)
};

namespace {

// what Wang's entries put into the shared ones (wang_streams_core.h): 8-byte hashes, its names, its launch
struct Wang {
    using set = ucfp_wang_streams;
    static constexpr size_t rec_bytes = 8, align = 8;
    static constexpr const char* align_msg = "the hash buffer must be 8-byte aligned";
    static constexpr const char* abi = "wang";
    static constexpr const char* name = "Wang";
    static constexpr const char* cap_arg = "cap_landmarks";
    static constexpr bool bound32 = false;
    static Cfg defaults() { return Cfg{10u, 63u, 64u, 30u, -50.0f}; }
    static ucfp::WangRingsDev& rings(set* s) { return s->rings; }
    static void launch(set* s, const float* d_pcm, const ucfp::WangPushWs& w, uint8_t* d_out, size_t cap_hashes,
                       uint64_t* d_out_offsets, hipStream_t st) {
        const Cfg& c = s->cfg;
        ucfp::launch_wang_streams_push(d_pcm, s->dev, s->rs, s->rings, c.fan_out, c.target_zone_t, c.target_zone_f,
                                       c.peaks_per_sec, s->floor_p, s->ctx->audio_ws, w,
                                       reinterpret_cast<uint32_t*>(d_out), cap_hashes, d_out_offsets, st);
    }
};

}  // namespace

extern "C" {

uint64_t ucfp_wang_stream_frontier(uint64_t n_samples, const ucfp_wang_config* cfg) {
    const Cfg c = cfg ? cfg_of(*cfg) : Wang::defaults();
    return frontier_of(judged_of(n_samples), c.target_zone_t);
}

uint64_t ucfp_wang_stream_samples(uint64_t n_samples, uint32_t sample_rate, int final) {
    return sr_ok(sample_rate) ? samples_of(n_samples, sample_rate, final != 0) : 0;
}

size_t ucfp_wang_streams_state_bytes(const ucfp_wang_config* cfg) { return entry_state_bytes<Wang>(cfg, 0); }

size_t ucfp_wang_streams_state_bytes_ex(const ucfp_wang_config* cfg, uint32_t window_frames) {
    return entry_state_bytes<Wang>(cfg, window_frames);
}

size_t ucfp_wang_streams_state_bytes_sr(const ucfp_wang_config* cfg, uint32_t window_frames, uint32_t sample_rate) {
    return entry_state_bytes<Wang>(cfg, window_frames, sample_rate);
}

size_t ucfp_wang_streams_window_cap(const ucfp_wang_config* cfg, uint32_t window_frames) {
    return entry_window_cap<Wang>(cfg, window_frames);
}

int ucfp_wang_streams_create(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_wang_config* cfg, uint32_t max_streams,
                             ucfp_wang_streams** out) {
    return entry_create<Wang>(ctx, sample_rate, cfg, max_streams, 0, out);
}

int ucfp_wang_streams_create_ex(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_wang_config* cfg, uint32_t max_streams,
                                uint32_t window_frames, ucfp_wang_streams** out) {
    return entry_create<Wang>(ctx, sample_rate, cfg, max_streams, window_frames, out);
}

int ucfp_wang_streams_create_sr(ucfp_ctx* ctx, uint32_t sample_rate, const ucfp_wang_config* cfg, uint32_t max_streams,
                                uint32_t window_frames, ucfp_wang_streams** out) {
    return entry_create<Wang>(ctx, sample_rate, cfg, max_streams, window_frames, out, true);
}

void ucfp_wang_streams_destroy(ucfp_wang_streams* s) {
    if (!s) return;
    set_release(s);
    delete s;
}

int ucfp_wang_streams_open(ucfp_wang_streams* s, uint32_t* slot) {
    if (!s || !slot) return fail(UCFP_E_INVALID, "set / slot is NULL");
    return set_open(s, slot);
}

// the ring needs no device work: a slot that has seen no sample since it was opened has an empty window (windows_dev),
// and its first push starts the ring afresh
int ucfp_wang_streams_close(ucfp_wang_streams* s, uint32_t slot) {
    if (!s) return fail(UCFP_E_INVALID, "set is NULL");
    return set_close(s, slot);
}

size_t ucfp_wang_streams_max_hashes(ucfp_wang_streams* s, const uint32_t* slots, const uint64_t* n_samples,
                                    const uint8_t* final, size_t n) {
    return entry_max_hashes<Wang>(s, slots, n_samples, final, n);
}

int ucfp_wang_streams_push_dev(ucfp_wang_streams* s, const uint32_t* slots, const uint64_t* n_samples,
                               const uint8_t* final, size_t n, const float* d_pcm, uint8_t* d_out, size_t cap_hashes,
                               uint64_t* d_out_offsets, void* stream) {
    return entry_push_dev<Wang>(s, slots, n_samples, final, n, d_pcm, d_out, cap_hashes, d_out_offsets, stream);
}

int ucfp_wang_streams_push(ucfp_wang_streams* s, uint32_t slot, const float* pcm, size_t n, int final, uint8_t* out,
                           size_t cap_hashes, size_t* n_hashes) {
    return entry_push<Wang>(s, slot, pcm, n, final, out, cap_hashes, n_hashes);
}

int ucfp_wang_streams_windows_dev(ucfp_wang_streams* s, const uint32_t* slots, size_t n, uint8_t* d_landmarks,
                                  size_t cap_landmarks, uint64_t* d_offsets, uint32_t* d_origins, void* stream) {
    return entry_windows_dev<Wang>(s, slots, n, d_landmarks, cap_landmarks, d_offsets, d_origins, stream);
}

}  // extern "C"
